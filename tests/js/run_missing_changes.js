'use strict'
// Feeds documents through GpuDocBackend in rounds (chunk 0 via init(), the rest via
// applyRemoteChanges()) and a fork of each document that stops after chunk 0.  After every round it
// compares, per document, with Automerge 0.12's rules restated here over the CPU restatement's
// OpSet (oracle/js/backend.js: s.states, s.history) fed the same chunks:
//   Backend.getMissingChanges(back, clock) for the empty clock, the clock before this round, and
//     that clock with its keys reversed and every second seq lowered (not causally closed: the
//     fold's order matters)
//   Backend.getChangesForActor(back, actor, afterSeq) for every actor, afterSeq 0 and half its seq
//   GpuEngine.missingChanges(states, clocks) for all documents in one call
// and at the end Backend.getChanges(fork.back, doc.back).
// Prints {rounds: [{compared, nonEmpty}], mismatches, nMismatches}; exits 1 on any mismatch.
const path = require('path')
const { GpuEngine, DocBackend, makeBackend } = require(path.join(__dirname, '..', '..', 'hypermerge_amd', 'js', 'GpuDocBackend.js'))
const Oracle = require(path.join(__dirname, '..', '..', 'oracle', 'js', 'backend.js')).Backend

const input = JSON.parse(require('fs').readFileSync(0, 'utf8'))
const engine = new GpuEngine({ mode: input.mode || 'sync' })
const Backend = makeBackend(engine)
const tick = () => new Promise((r) => setImmediate(r))

// op_set.js transitiveDeps / getMissingChanges / getChangesForActor restated
function transitiveDeps(s, have) {
  const deps = new Map()
  for (const a of Object.keys(have)) {
    const q = have[a]
    if (q <= 0) continue
    const st = s.states.get(a)
    const t = st && st[q - 1] ? st[q - 1].allDeps : null
    if (t) for (const [x, v] of t) if (v > (deps.get(x) || 0)) deps.set(x, v)
    deps.set(a, q)
  }
  return deps
}
function missingOf(s, have) {
  const deps = transitiveDeps(s, have)
  return s.history.filter((c) => c.seq > (deps.get(c.actor) || 0))
}
const forActor = (s, a, n) => (s.states.get(a) || []).slice(n).map((st) => st.change)
const ids = (cs) => JSON.stringify(cs.map((c) => [c.actor, c.seq]))
const clockOf = (s) => { const o = {}; for (const [a, q] of s.clock) o[a] = q; return o }
function skewed(clock) {
  const o = {}
  Object.keys(clock).reverse().forEach((a, k) => { o[a] = k % 2 ? Math.max(clock[a] - 1 - (k % 3), 0) : clock[a] })
  return o
}

;(async () => {
  const docs = input.docs.map((chunks, i) => ({
    d: new DocBackend('doc' + i, () => {}, undefined, engine),
    fork: new DocBackend('fork' + i, () => {}, undefined, engine),
    chunks, s: Oracle.init(), fs: Oracle.init(), prev: {},
  }))
  const settle = async () => { if (engine.mode === 'async') await engine.idle(); else { await tick(); await tick() } }
  const nRounds = Math.max(...input.docs.map((c) => c.length))
  const rounds = [], mismatches = []
  const cmp = (r, id, what, got, want) => { if (ids(got) !== ids(want)) mismatches.push({ r, id, what, got: ids(got), want: ids(want) }) }
  for (let r = 0; r < nRounds; r++) {
    for (const x of docs) {
      if (r >= x.chunks.length) continue
      x.prev = clockOf(x.s)
      if (r === 0) {
        x.d.init(x.chunks[0], 'local')
        x.fork.init(x.chunks[0], 'local')
        Oracle.applyChanges(x.fs, JSON.parse(JSON.stringify(x.chunks[0])))
      } else if (x.chunks[r].length) x.d.applyRemoteChanges(x.chunks[r])
      Oracle.applyChanges(x.s, JSON.parse(JSON.stringify(x.chunks[r])))
    }
    await settle()
    let compared = 0, nonEmpty = 0
    for (const x of docs) {
      for (const have of [{}, x.prev, skewed(x.prev), skewed(clockOf(x.s)), { nobody: 3 }]) {
        const want = missingOf(x.s, have)
        cmp(r, x.d.id, 'getMissingChanges ' + JSON.stringify(have), Backend.getMissingChanges(x.d.back, have), want)
        compared++
        if (want.length) nonEmpty++
      }
      for (const [a, q] of x.s.clock) {
        for (const n of [0, q >> 1]) cmp(r, x.d.id, `getChangesForActor ${a} ${n}`, Backend.getChangesForActor(x.d.back, a, n), forActor(x.s, a, n))
      }
      cmp(r, x.d.id, 'getChangesForActor default', Backend.getChangesForActor(x.d.back, 'nobody'), [])
    }
    const all = engine.missingChanges(docs.map((x) => x.d.back), docs.map((x) => x.prev))
    docs.forEach((x, i) => cmp(r, x.d.id, 'engine.missingChanges', all[i], missingOf(x.s, x.prev)))
    rounds.push({ compared, nonEmpty })
  }
  let forks = 0
  for (const x of docs) {
    const want = missingOf(x.s, clockOf(x.fs))
    cmp('end', x.d.id, 'getChanges(fork, doc)', Backend.getChanges(x.fork.back, x.d.back), want)
    cmp('end', x.d.id, 'getChanges(doc, doc)', Backend.getChanges(x.d.back, x.d.back), [])
    if (want.length) forks++
  }
  process.stdout.write(JSON.stringify({ rounds, forks, mismatches: mismatches.slice(0, 10), nMismatches: mismatches.length }) + '\n')
  if (mismatches.length) process.exit(1)
})().catch((e) => { console.error(e); process.exit(1) })
