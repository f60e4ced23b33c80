'use strict'
// DocBackend.materializeAt(n) / GpuEngine.materialize on the GPU drop-in against the JS restatement:
// materialize(Backend.applyChanges(Backend.init(), history.slice(0, n))[0]) of oracle/js/backend.js.
//   1. the reference's tests/repo.test.ts:129-164 document (foo = bar0, bar1, bar2, bar3) at every n
//   2. the documents given on stdin ({docs: [[chunk of changes, ...], ...], mode}): fed in rounds, then
//      every history length of every document in one batched call, and one clock request each
// Prints {scenario, mismatches, checked, docs}: mismatches lists the first differing requests.
const path = require('path')
const G = require(path.join(__dirname, '..', '..', 'hypermerge_amd', 'js', 'GpuDocBackend.js'))
const J = require(path.join(__dirname, '..', '..', 'oracle', 'js', 'backend.js'))
const ROOT = '00000000-0000-0000-0000-000000000000'
const tick = () => new Promise((r) => setImmediate(r))

function canon(v) {
  if (v === null || typeof v !== 'object') return JSON.stringify(v)
  if (Array.isArray(v)) return '[' + v.map(canon).join(',') + ']'
  return '{' + Object.keys(v).sort().map((k) => JSON.stringify(k) + ':' + canon(v[k])).join(',') + '}'
}
const replay = (changes) => J.Backend.applyChanges(J.Backend.init(), changes)[0]

;(async () => {
  const input = JSON.parse(require('fs').readFileSync(0, 'utf8'))
  const mode = input.mode || 'batched'
  const engine = new G.GpuEngine({ mode, aStride: 8 })
  const idle = async () => { if (mode === 'async') await engine.idle(); else { await tick(); await tick() } }

  // 1. the reference scenario
  const actor = 'aaaaaaaa'
  const change = (seq, v) => ({ actor, seq, deps: {}, ops: [{ action: 'set', obj: ROOT, key: 'foo', value: v }] })
  const doc = new G.DocBackend('scenario', () => {}, undefined, engine)
  const before = doc.materializeAt(1)
  doc.init([change(1, 'bar0')], actor)
  await idle()
  for (let s = 2; s <= 4; s++) { doc.applyLocalChange(change(s, 'bar' + (s - 1))); await idle() }
  const scenario = { before: before === undefined }
  for (let n = 0; n <= 5; n++) {
    const m = doc.materializeAt(n)
    scenario[n] = { doc: m.doc, history: m.history, clock: m.clock }
  }

  // 2. seeded documents against the JS restatement
  const docs = input.docs.map((chunks, i) => ({ d: new G.DocBackend('doc' + i, () => {}, undefined, engine), chunks }))
  const rounds = Math.max(0, ...input.docs.map((c) => c.length))
  for (let r = 0; r < rounds; r++) {
    for (const x of docs) {
      if (r >= x.chunks.length) continue
      if (r === 0) x.d.init(x.chunks[0], 'local')
      else if (x.chunks[r].length) x.d.applyRemoteChanges(x.chunks[r])
    }
    await idle()
  }
  const reqs = [], want = []
  docs.forEach((x, i) => {
    const h = x.d.back.getIn(['opSet', 'history'])
    const hist = h.slice(0, h.size).toArray()
    for (let n = 0; n <= hist.length + 1; n++) {
      reqs.push(n % 2 ? { id: 'doc' + i, history: n } : { state: x.d.back, history: n })
      want.push(replay(hist.slice(0, n)))
    }
    // each actor's changes up to about half of its seqs: loadDocument's cursor
    const clock = {}
    for (const c of hist) clock[c.actor] = Math.max(clock[c.actor] || 0, c.seq)
    for (const a of Object.keys(clock)) clock[a] = Math.floor(clock[a] / 2)
    reqs.push({ state: x.d.back, clock })
    want.push(replay(hist.filter((c) => c.seq <= clock[c.actor])))
  })
  const got = engine.materialize(reqs)
  const mismatches = []
  got.forEach((g, k) => {
    const w = want[k]
    const wc = {}
    for (const [a, q] of w.clock) wc[a] = q
    const ok = canon(g.doc) === canon(J.materialize(w)) && g.history === w.history.length && canon(g.clock) === canon(wc)
    if (!ok && mismatches.length < 5) mismatches.push({ k, req: { history: reqs[k].history, clock: reqs[k].clock }, got: g, want: J.materialize(w) })
  })
  // one document at a time gives the same as the batched call
  let single = 0
  docs.slice(0, 8).forEach((x) => {
    const n = Math.floor(x.d.back.histLen / 2)
    const a = x.d.materializeAt(n), b = engine.materialize([{ state: x.d.back, history: n }])[0]
    if (canon(a) === canon(b) && canon(a.doc) === canon(J.materialize(replay(x.d.back.getIn(['opSet', 'history']).slice(0, n).toArray())))) single++
  })
  process.stdout.write(JSON.stringify({ scenario, mismatches, checked: got.length, docs: docs.length, single }) + '\n', () => process.exit(0))
})().catch((e) => { console.error(e && e.stack || e); process.exit(1) })
