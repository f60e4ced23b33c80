'use strict'
// Feeds documents through GpuDocBackend in rounds (chunk 0 via init(), the rest via
// applyRemoteChanges()) and, after every round, compares with values restated from the CPU
// restatement's state (oracle/js/backend.js: s.queue, s.clock) fed the same chunks:
//   Backend.getMissingDeps(doc.back), getIn(['opSet','queue']).toArray() as (actor, seq) pairs,
//   DocBackend.missingDeps() and engine.blocked().
// Prints {rounds: [{blocked, nonEmpty}], mismatches: [...]}; exits 1 on any mismatch.
const path = require('path')
const { GpuEngine, DocBackend, makeBackend } = require(path.join(__dirname, '..', '..', 'hypermerge_amd', 'js', 'GpuDocBackend.js'))
const Oracle = require(path.join(__dirname, '..', '..', 'oracle', 'js', 'backend.js')).Backend

const input = JSON.parse(require('fs').readFileSync(0, 'utf8'))
const engine = new GpuEngine({ mode: input.mode || 'sync' })
const Backend = makeBackend(engine)
const tick = () => new Promise((r) => setImmediate(r))

// getMissingDeps restated: a queued change needs deps.set(actor, seq - 1); per actor the largest
// need that the clock of applied changes has not reached
function missingOf(s) {
  const missing = {}
  for (const c of s.queue) {
    const need = Object.assign({}, c.deps || {})
    need[c.actor] = c.seq - 1
    for (const a of Object.keys(need)) {
      if ((s.clock.get(a) || 0) < need[a]) missing[a] = Math.max(missing[a] || 0, need[a])
    }
  }
  return missing
}
const sorted = (o) => JSON.stringify(Object.keys(o).sort().map((k) => [k, o[k]]))

;(async () => {
  const docs = input.docs.map((chunks, i) => {
    const d = new DocBackend('doc' + i, () => {}, undefined, engine)
    return { d, chunks, s: Oracle.init() }
  })
  const nRounds = Math.max(...input.docs.map((c) => c.length))
  const rounds = [], mismatches = []
  for (let r = 0; r < nRounds; r++) {
    for (const x of docs) {
      if (r >= x.chunks.length) continue
      if (r === 0) x.d.init(x.chunks[0], 'local')
      else if (x.chunks[r].length) x.d.applyRemoteChanges(x.chunks[r])
      Oracle.applyChanges(x.s, JSON.parse(JSON.stringify(x.chunks[r])))
    }
    // the queries reflect the rounds already applied: an async engine is idle first
    if (engine.mode === 'async') await engine.idle()
    else { await tick(); await tick() }
    let nonEmpty = 0
    const wantBlocked = {}
    for (const x of docs) {
      const want = missingOf(x.s)
      const wantQ = x.s.queue.map((c) => [c.actor, c.seq])
      const got = Backend.getMissingDeps(x.d.back)
      const q = x.d.back.getIn(['opSet', 'queue'])
      const gotQ = q.toArray().map((c) => [c.actor, c.seq])
      if (sorted(got) !== sorted(want)) mismatches.push({ r, id: x.d.id, what: 'missing', got, want })
      if (sorted(x.d.missingDeps()) !== sorted(want)) mismatches.push({ r, id: x.d.id, what: 'DocBackend.missingDeps' })
      if (JSON.stringify(gotQ) !== JSON.stringify(wantQ) || q.size !== wantQ.length) mismatches.push({ r, id: x.d.id, what: 'queue', gotQ, wantQ })
      if (wantQ.length) { nonEmpty++; wantBlocked[x.d.id] = want }
    }
    const b = engine.blocked()
    const gotIds = b.map((e) => e.id).sort(), wantIds = Object.keys(wantBlocked).sort()
    if (JSON.stringify(gotIds) !== JSON.stringify(wantIds)) mismatches.push({ r, what: 'blocked ids', got: gotIds.length, want: wantIds.length })
    for (const e of b) {
      if (wantBlocked[e.id] && sorted(e.missing) !== sorted(wantBlocked[e.id])) mismatches.push({ r, id: e.id, what: 'blocked missing' })
    }
    rounds.push({ blocked: b.length, nonEmpty })
  }
  process.stdout.write(JSON.stringify({ rounds, mismatches: mismatches.slice(0, 10), nMismatches: mismatches.length }) + '\n')
  if (mismatches.length) process.exit(1)
})().catch((e) => { console.error(e); process.exit(1) })
