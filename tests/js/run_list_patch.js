'use strict'
// DocBackend.materializePatchAt(n, { lists: true }) / GpuEngine.materializePatch(reqs, { lists: true })
// on the GPU drop-in against the JS restatement: Backend.applyChanges(Backend.init(),
// history.slice(0, n))[1] of oracle/js/backend.js, compared for deep equality of clock, deps and
// diffs, the list / text element diffs included: no prefix may come back with patch: null.  The
// documents come on stdin ({docs: [[chunk of changes, ...], ...], mode}), are fed in rounds, then
// every history length of every document is asked in one batched call, with the option and without
// it (where a prefix that assigns list / text elements still comes back with patch: null).
// Prints {mismatches, checked, nulls, elementDiffs, plainNulls, plainMismatches, docs, single}.
const path = require('path')
const G = require(path.join(__dirname, '..', '..', 'hypermerge_amd', 'js', 'GpuDocBackend.js'))
const J = require(path.join(__dirname, '..', '..', 'oracle', 'js', 'backend.js'))
const tick = () => new Promise((r) => setImmediate(r))

function canon(v) {
  if (v === null || typeof v !== 'object') return JSON.stringify(v)
  if (Array.isArray(v)) return '[' + v.map(canon).join(',') + ']'
  return '{' + Object.keys(v).sort().map((k) => JSON.stringify(k) + ':' + canon(v[k])).join(',') + '}'
}
const patchOf = (changes) => J.Backend.applyChanges(J.Backend.init(), changes)[1]
const elementDiff = (d) => (d.type === 'list' || d.type === 'text') && d.action !== 'create'
const equal = (g, w) => g.patch !== null && g.history === w.history && canon(g.patch.clock) === canon(w.patch.clock) &&
  canon(g.patch.deps) === canon(w.patch.deps) && canon(g.patch.diffs) === canon(w.patch.diffs) &&
  g.patch.canUndo === false && g.patch.canRedo === false

;(async () => {
  const input = JSON.parse(require('fs').readFileSync(0, 'utf8'))
  const mode = input.mode || 'batched'
  const engine = new G.GpuEngine({ mode, aStride: 8 })
  const idle = async () => { if (mode === 'async') await engine.idle(); else { await tick(); await tick() } }
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
      want.push({ patch: patchOf(hist.slice(0, n)), history: Math.min(n, hist.length) })
    }
  })
  const got = engine.materializePatch(reqs, { lists: true })
  const mismatches = []
  let nulls = 0, elementDiffs = 0
  got.forEach((g, k) => {
    if (g.patch === null) nulls++
    elementDiffs += want[k].patch.diffs.filter(elementDiff).length
    if (!equal(g, want[k]) && mismatches.length < 5) mismatches.push({ k, history: reqs[k].history, got: g, want: want[k] })
  })
  // without the option: null exactly where the restatement's patch holds an element diff
  const plain = engine.materializePatch(reqs)
  let plainNulls = 0, plainMismatches = 0
  plain.forEach((g, k) => {
    const w = want[k]
    if (g.patch === null) { plainNulls++; if (!w.patch.diffs.some(elementDiff)) plainMismatches++ } else if (w.patch.diffs.some(elementDiff) || !equal(g, w)) plainMismatches++
  })
  // one document at a time gives the same as the batched call
  let single = 0
  docs.slice(0, 8).forEach((x) => {
    const n = Math.floor(x.d.back.histLen / 2)
    const a = x.d.materializePatchAt(n, { lists: true }), b = engine.materializePatch([{ state: x.d.back, history: n }], { lists: true })[0]
    if (canon(a) === canon(b) && a.patch !== null) single++
  })
  process.stdout.write(JSON.stringify({ mismatches, checked: got.length, nulls, elementDiffs, plainNulls, plainMismatches, docs: docs.length, single }) + '\n', () => process.exit(0))
})().catch((e) => { console.error(e && e.stack || e); process.exit(1) })
