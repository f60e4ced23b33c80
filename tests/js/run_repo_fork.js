'use strict'
// The fork scenario of tests/golden/repo_scenarios.json (tests/repo.test.ts:103-127: fork = create() +
// merge(fork, url), src/RepoFrontend.ts:95-100) through the GPU drop-in with the fork made on the device:
// the merge into the still empty document is DocBackend.mergeFrom (GpuEngine.fork), not a re-feed of the
// parent's blocks.  The host logic around it is the part of tests/js/run_repo_scenarios.js the scenario
// uses (create, watch, merge, change; renders follow DocFrontend: minimumClockSatisfied && diffs.length).
// argv[2] = mode ('sync' | 'batched' | 'async'), argv[3] = diffs ('ops' | 'device').
// Prints {renders: {"repo/doc": [renders...]}, messages: {"repo/doc": [types...]}, forks, submits}.
const path = require('path')
const fs = require('fs')
const G = require(path.join(__dirname, '..', '..', 'hypermerge_amd', 'js', 'GpuDocBackend.js'))

const gold = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'golden', 'repo_scenarios.json'), 'utf8'))
const INF = gold.INF
const ROOT = '00000000-0000-0000-0000-000000000000'
const mode = process.argv[2] || 'sync'
const engine = new G.GpuEngine({ mode, diffs: process.argv[3] || 'ops' })
const tick = () => new Promise((r) => setImmediate(r))
const idle = async () => { if (mode === 'async') await engine.idle(); for (let k = 0; k < 4; k++) await tick() }

function plain(view, uuid) {
  const ov = view.get(uuid)
  if (!ov) return {}
  const val = (e) => (e.link ? plain(view, e.value) : e.value)
  if (ov.type === 'list' || ov.type === 'text') return ov.elems.filter(Boolean).map(([, e]) => val(e))
  const o = {}
  for (const [k, e] of ov.keys) o[k] = val(e)
  return o
}
const render = (doc) => plain(G.materialize(doc.back), ROOT)

;(async () => {
  const docs = new Map(), cursors = new Map(), watched = new Map(), messages = new Map()
  let forks = 0
  const cursorUpdate = (doc, clock) => {
    const cur = cursors.get(doc) || {}
    for (const [a, s0] of Object.entries(clock)) { const s = Math.min(s0, INF); if (!(a in cur) || s > cur[a]) cur[a] = s }
    cursors.set(doc, cur)
  }
  const notify = (m) => {
    const d = docs.get(m.id)
    messages.get(m.id).push(m.type)
    if (watched.has(m.id) && m.patch && m.type !== 'ReadyMsg' && m.minimumClockSatisfied && m.patch.diffs.length > 0)
      watched.get(m.id).push(render(d))
  }
  for (const st of gold.scenarios.fork.steps) {
    const [op, , id] = st
    if (op === 'create') {
      messages.set(id, [])
      const d = new G.DocBackend(id, notify, engine.init(id), engine)
      docs.set(id, d)
      cursorUpdate(id, { [id]: INF })
      for (const c of st[3]) d.applyLocalChange(c)
    } else if (op === 'watch') {
      const d = docs.get(id)
      watched.set(id, [])
      if (d.back && d.minimumClockSatisfied) watched.get(id).push(render(d))
    } else if (op === 'merge') {
      // cursors.update + syncReadyActors: the listed actors' changes 1 .. clock[actor] go to the document;
      // here every listed actor is another document's root actor and the target is still empty: a fork
      const d = docs.get(id), clock = st[3]
      cursorUpdate(id, clock)
      const from = Object.keys(clock).map((a) => docs.get(a))
      if (from.length !== 1 || !from[0] || d.back.histLen !== 0) throw new Error('not a fork: ' + JSON.stringify(st))
      d.mergeFrom(from[0], clock)
      for (const a of Object.keys(clock)) d.changes.set(a, Math.min(clock[a], from[0].back.clock[a] || 0))
      forks++
    } else if (op === 'change') {
      docs.get(id).applyLocalChange(st[3])
    } else throw new Error(op)
    await idle()
  }
  const renders = {}, msgs = {}
  for (const [d, v] of watched) renders['R/' + d] = v
  for (const [d, v] of messages) msgs['R/' + d] = v
  const f = docs.get('F')
  process.stdout.write(JSON.stringify({ renders, messages: msgs, forks, submits: engine.submits, forkClock: f.clock,
    forkHistory: f.back.histLen, forkLog: f.back.log.length }) + '\n', () => process.exit(0))
})().catch((e) => { console.error(e && e.stack || e); process.exit(1) })
