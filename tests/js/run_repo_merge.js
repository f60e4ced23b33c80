'use strict'
// Repo.merge into a document that already holds changes, through DocBackend.mergeFrom on the GPU drop-in.
//  1. The "merge" scenario of tests/golden/repo_scenarios.json (tests/repo.test.ts "Test document merging"):
//     D1 holds {foo: 'bar'}, D2 {baz: 'bah'}; merge(D1, D2 at {D2: 1}); a later change of D2 must not reach D1.
//  2. A conflicting key on both sides, and a repeated merge, against the JS restatement (oracle/js/backend.js):
//     the control DocBackend receives the same changes through applyRemoteChanges; message sequences, clocks
//     and histories must be equal.  With argv[4] = '2' the engine has two docsets on one device and the
//     documents are named so that source and destination hash to different shards: the host hand-over.
// argv[2] = mode ('sync' | 'batched' | 'async'), argv[3] = diffs ('ops' | 'device'), argv[4] = docsets.
// Prints {renders, messages, submits, d1Clock, d1History, mismatches, crossShard}.
const path = require('path')
const fs = require('fs')
const G = require(path.join(__dirname, '..', '..', 'hypermerge_amd', 'js', 'GpuDocBackend.js'))
const J = require(path.join(__dirname, '..', '..', 'oracle', 'js', 'backend.js'))

const gold = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'golden', 'repo_scenarios.json'), 'utf8'))
const ROOT = '00000000-0000-0000-0000-000000000000'
const mode = process.argv[2] || 'sync'
const shards = Number(process.argv[4] || 1)
const engine = new G.GpuEngine({ mode, diffs: process.argv[3] || 'ops', devices: new Array(shards).fill(0) })
const tick = () => new Promise((r) => setImmediate(r))
const idle = async () => { if (mode === 'async') await engine.idle(); for (let k = 0; k < 4; k++) await tick() }

function canon(v) {
  if (v === undefined) return 'undefined'
  if (v === null || typeof v !== 'object') return JSON.stringify(v)
  if (v instanceof Map) return canon(Object.fromEntries(v))
  if (Array.isArray(v)) return '[' + v.map(canon).join(',') + ']'
  return '{' + Object.keys(v).sort().map((k) => JSON.stringify(k) + ':' + canon(v[k])).join(',') + '}'
}
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
const set = (key, value) => ({ action: 'set', obj: ROOT, key, value })

;(async () => {
  // ---- 1. the reference's scenario
  const docs = new Map(), watched = new Map(), messages = new Map()
  const submits0 = engine.submits
  const notify = (m) => {
    messages.get(m.id).push(m.type)
    if (watched.has(m.id) && m.patch && m.type !== 'ReadyMsg' && m.minimumClockSatisfied && m.patch.diffs.length > 0)
      watched.get(m.id).push(render(docs.get(m.id)))
  }
  for (const st of gold.scenarios.merge.steps) {
    const [op, , id] = st
    if (op === 'create') {
      messages.set(id, [])
      const d = new G.DocBackend(id, notify, engine.init(id), engine)
      docs.set(id, d)
      for (const c of st[3]) d.applyLocalChange(c)
    } else if (op === 'watch') {
      const d = docs.get(id)
      watched.set(id, [])
      if (d.back && d.minimumClockSatisfied) watched.get(id).push(render(d))
    } else if (op === 'merge') {
      const d = docs.get(id), clock = st[3]
      for (const a of Object.keys(clock)) d.mergeFrom(docs.get(a), { [a]: clock[a] })
    } else if (op === 'change') {
      docs.get(id).applyLocalChange(st[3])
    } else if (op !== 'expect_cursor') throw new Error(op)
    await idle()
  }
  const renders = {}, msgs = {}
  for (const [d, v] of watched) renders['R/' + d] = v
  for (const [d, v] of messages) msgs['R/' + d] = v
  const d1 = docs.get('D1')
  const out = { renders, messages: msgs, submits: engine.submits - submits0, d1Clock: d1.clock, d1History: d1.back.histLen,
    d1Log: d1.back.log.length, mismatches: [], crossShard: 0 }
  const bad = (what, got, want) => { if (out.mismatches.length < 5) out.mismatches.push({ what, got, want }) }

  // ---- 2. a conflicting key on both sides, then the same merge again (nothing left to hand), then a wider clock
  let dstId = 'conflict-into', srcId = 'conflict-from'
  if (shards > 1) for (let k = 0; engine.shardOf(dstId) === engine.shardOf(srcId); k++) srcId = 'conflict-from-' + k
  const mine = [{ actor: 'mmmm', seq: 1, deps: {}, ops: [set('k', 'mine'), set('only-mine', 1)] }]
  const theirs = [{ actor: 'aaaa', seq: 1, deps: {}, ops: [set('k', 'theirs'), set('only-theirs', 2)] },
    { actor: 'aaaa', seq: 2, deps: {}, ops: [set('k', 'theirs again')] },
    { actor: 'zzzz', seq: 1, deps: { aaaa: 1 }, ops: [set('k', 'third'), set('z', true)] }]
  const gm = [], jm = []
  const into = new G.DocBackend(dstId, (m) => gm.push(m), undefined, engine)
  const from = new G.DocBackend(srcId, () => {}, undefined, engine)
  const ctl = new J.DocBackend(dstId, (m) => jm.push(m))
  into.init(mine, 'me'); from.init(theirs, 'them'); ctl.init(mine, 'me')
  await idle()
  if (into.back.shard !== from.back.shard) out.crossShard++
  const rounds = [[{ aaaa: 1 }, [theirs[0]]], [{ aaaa: 1 }, []], [{ zzzz: 1, aaaa: 5, nobody: 2 }, [theirs[2], theirs[1]]]]
  for (const [clock, handed] of rounds) {
    into.mergeFrom(from, clock)
    if (handed.length) ctl.applyRemoteChanges(handed)
    await idle()
  }
  if (canon(gm) !== canon(jm)) bad('messages', gm, jm)
  if (canon(into.clock) !== canon(ctl.clock)) bad('clock', into.clock, ctl.clock)
  if (into.back.histLen !== ctl.back.history.length) bad('history', into.back.histLen, ctl.back.history.length)
  if (into.back.log.length !== 4) bad('log', into.back.log.length, 4)
  if (canon(render(into)) !== canon({ k: 'third', 'only-mine': 1, 'only-theirs': 2, z: true })) bad('render', render(into), null)
  if (from.back.log.length !== 3) bad('the source is only read', from.back.log.length, 3)
  process.stdout.write(JSON.stringify(out) + '\n', () => process.exit(0))
})().catch((e) => { console.error(e && e.stack || e); process.exit(1) })
