'use strict'
// Local changes with undo / redo on the GPU drop-in with undo: 'fields' (the undo ops built from the
// device's answer for the fields a request touches) and on the JS restatement, side by side, on feeds
// that reach what the default route gets wrong:
//   race       a remote set is applied after the frontend built its request (the request's deps do
//              not name it) and before the request is applied, on a field the request touches twice,
//              or a concurrent counter set under an inc that a later set of the request follows
//   not ready  a request whose deps name a remote change that arrives one step later
// Printed per document: every message's type, history, canUndo / canRedo, the local patches' actor /
// seq, each request's thrown error (if any), and after every step the materialized document and the
// undo / redo stacks; counts: {retouchedUncovered, notReady} = local requests whose re-touched field
// held an op they do not cover / that were not causally ready (asked through engine.fields).
// argv[2]: engine mode (sync | batched | async), argv[3]: documents, argv[4]: the undo route
// ('fields'; 'view' shows what the default route makes of the same feed).
const path = require('path')
const G = require(path.join(__dirname, '..', '..', 'hypermerge_amd', 'js', 'GpuDocBackend.js'))
const J = require(path.join(__dirname, '..', '..', 'oracle', 'js', 'backend.js'))
const ROOT = '00000000-0000-0000-0000-000000000000'
const mode = process.argv[2] || 'sync'
const nDocs = parseInt(process.argv[3] || '24', 10)
const route = process.argv[4] || 'fields'

function rng(seed) {
  let x = seed >>> 0 || 1
  return () => { x ^= x << 13; x >>>= 0; x ^= x >>> 17; x ^= x << 5; x >>>= 0; return x / 4294967296 }
}

function canon(v) {
  if (v === null || typeof v !== 'object') return JSON.stringify(v)
  if (Array.isArray(v)) return '[' + v.map(canon).join(',') + ']'
  return '{' + Object.keys(v).sort().map((k) => JSON.stringify(k) + ':' + canon(v[k])).join(',') + '}'
}

function plain(view, uuid) {
  const ov = view.get(uuid)
  if (!ov) return {}
  const val = (e) => (e.link ? plain(view, e.value) : e.value)
  if (ov.type === 'list' || ov.type === 'text') return ov.elems.map(([, e]) => val(e))
  const o = {}
  for (const [k, e] of ov.keys) o[k] = val(e)
  return o
}

// one document's script: steps of ['init' | 'remote', changes] | ['local' | 'request', request]
function script(seed) {
  const r = rng(seed)
  const LOCAL = 'mmmm', REMOTES = ['aaaa', 'zzzz']
  const LIST = 'list-' + seed
  const seq = { mmmm: 0, aaaa: 0, zzzz: 0 }
  const heads = {}                                      // the remote changes delivered so far
  const steps = []
  const elems = []
  let nextElem = 1
  const keys = ['k0', 'k1', 'k2']
  const pick = (a) => a[Math.floor(r() * a.length)]
  const mk = (actor, deps, ops) => { seq[actor]++; return { actor, seq: seq[actor], deps, ops } }
  const remoteDeps = (a) => { const d = Object.assign({}, heads); delete d[a]; return d }
  const local = (deps, ops) => {
    const req = mk(LOCAL, Object.assign({}, deps), ops)
    req.requestType = 'change'
    steps.push(['local', req])
  }
  steps.push(['init', [mk('aaaa', {}, [{ action: 'set', obj: ROOT, key: 'c', value: 10, datatype: 'counter' },
    { action: 'makeList', obj: LIST }, { action: 'link', obj: ROOT, key: 'l', value: LIST }])]])
  heads.aaaa = 1
  for (let s = 0; s < 16; s++) {
    const p = r()
    if (p < 0.15) {
      const a = pick(REMOTES)
      const c = mk(a, remoteDeps(a), [{ action: 'set', obj: ROOT, key: pick(keys), value: 'r' + s }])
      heads[a] = c.seq
      steps.push(['remote', [c]])
    } else if (p < 0.4) {
      // race: the frontend built its request on `seen`; the remote change lands first
      const seen = Object.assign({}, heads)
      const a = pick(REMOTES)
      const q = r()
      if (q < 0.6) {
        const k = pick(keys)
        const c = mk(a, remoteDeps(a), [{ action: 'set', obj: ROOT, key: k, value: 'race' + s }])
        heads[a] = c.seq
        steps.push(['remote', [c]])
        const ops = [{ action: 'set', obj: ROOT, key: k, value: s * 10 }]
        if (r() < 0.4) ops.push({ action: 'del', obj: ROOT, key: k })
        ops.push({ action: 'set', obj: ROOT, key: k, value: s * 10 + 1 })
        if (r() < 0.3) ops.push({ action: 'set', obj: ROOT, key: k, value: s * 10 + 2 })
        local(seen, ops)
      } else {
        const c = mk(a, remoteDeps(a), [{ action: 'set', obj: ROOT, key: 'c', value: 100 + s, datatype: 'counter' }])
        heads[a] = c.seq
        steps.push(['remote', [c]])
        local(seen, [{ action: 'inc', obj: ROOT, key: 'c', value: 1 + Math.floor(r() * 5) },
          { action: 'set', obj: ROOT, key: 'c', value: 1000 + s, datatype: 'counter' },
          { action: 'inc', obj: ROOT, key: 'c', value: 2 }, { action: 'set', obj: ROOT, key: 'c', value: 7, datatype: 'counter' }])
      }
    } else if (p < 0.5) {
      // not ready: the request names a remote change that arrives one step later
      const a = pick(REMOTES)
      const c = mk(a, remoteDeps(a), [{ action: 'set', obj: ROOT, key: pick(keys), value: 'late' + s }])
      local(Object.assign({}, heads, { [a]: c.seq }), [{ action: 'set', obj: ROOT, key: pick(keys), value: 'early' + s },
        { action: 'inc', obj: ROOT, key: 'c', value: 1 }])
      heads[a] = c.seq
      steps.push(['remote', [c]])
    } else if (p < 0.75) {
      // a local change over the whole document
      const ops = []
      const n = 1 + Math.floor(r() * 3)
      for (let k = 0; k < n; k++) {
        const q = r()
        if (q < 0.4) ops.push({ action: 'set', obj: ROOT, key: pick(keys), value: s * 10 + k })
        else if (q < 0.55) ops.push({ action: 'del', obj: ROOT, key: pick(keys) })
        else if (q < 0.7) ops.push({ action: 'inc', obj: ROOT, key: 'c', value: 1 + Math.floor(r() * 5) })
        else if (q < 0.85 || !elems.length) {
          const e = nextElem++
          ops.push({ action: 'ins', obj: LIST, key: elems.length && r() < 0.5 ? elems[elems.length - 1] : '_head', elem: e })
          ops.push({ action: 'set', obj: LIST, key: LOCAL + ':' + e, value: 'v' + e })
          elems.push(LOCAL + ':' + e)
        } else {
          const e = pick(elems)
          ops.push(r() < 0.5 ? { action: 'del', obj: LIST, key: e } : { action: 'set', obj: LIST, key: e, value: 'w' + s })
        }
      }
      local(heads, ops)
      if (r() < 0.15) steps[steps.length - 1][1].undoable = false
    } else {
      const kind = r() < 0.6 ? 'undo' : 'redo'
      steps.push(['request', { requestType: kind, actor: LOCAL, deps: Object.assign({}, heads) }])
    }
  }
  return steps
}

const counts = { retouchedUncovered: 0, notReady: 0 }

// what the device says of a local change request before it is applied
function census(engine, state, req) {
  const touched = new Map()
  for (const op of req.ops) {
    if (!['set', 'del', 'link', 'inc'].includes(op.action)) continue
    const k = op.obj + '\u0000' + op.key
    touched.set(k, { obj: op.obj, key: op.key, n: (touched.get(k) || { n: 0 }).n + 1 })
  }
  const fields = Array.from(touched.values())
  const got = engine.fields([{ state, change: req, fields: fields.map((f) => [f.obj, f.key]) }])[0]
  if (!got.ready) { counts.notReady++; return }
  if (fields.some((f, i) => f.n > 1 && got.fields[i].some((o) => !o.covered))) counts.retouchedUncovered++
}

async function run(which) {
  let lastErr = null
  const engine = which === 'gpu' ? new G.GpuEngine({ mode, aStride: 8, undo: route, onError: (e) => { lastErr = e.message } }) : null
  const out = []
  for (let d = 0; d < nDocs; d++) {
    const msgs = []
    const doc = which === 'gpu' ? new G.DocBackend('doc' + d, (m) => msgs.push(m), undefined, engine)
      : new J.DocBackend('doc' + d, (m) => msgs.push(m))
    const trace = []
    let localSeq = 0
    for (const [kind, x] of script(2000 + d)) {
      let err = null
      if (kind === 'init') doc.init(x, 'mmmm')
      else if (kind === 'remote') doc.applyRemoteChanges(x)
      else {
        const req = Object.assign({}, x, { seq: localSeq + 1 })
        if (engine && kind === 'local') { await engine.idle(); census(engine, doc.back, req) }
        lastErr = null
        try { doc.applyLocalChange(req) } catch (e) { err = e.message }
        if (engine) await engine.idle()
        if (!err && lastErr) err = lastErr
        if (!err) localSeq++
      }
      if (engine) await engine.idle()
      const st = which === 'gpu' ? plain(G.materialize(doc.back), ROOT) : J.materialize(doc.back)
      const b = doc.back
      trace.push([kind, err, canon(st), canon([b.undoStack, b.undoPos, b.redoStack])])
    }
    out.push({ trace, msgs: msgs.map((m) => [m.type, m.history, m.patch ? !!m.patch.canUndo : null,
      m.patch ? !!m.patch.canRedo : null, m.patch && m.patch.actor, m.patch && m.patch.seq]) })
  }
  return out
}

(async () => {
  const gpu = await run('gpu')
  const cpu = await run('cpu')
  // (exit once the line is flushed: a pipe takes stdout asynchronously)
  process.stdout.write(JSON.stringify({ gpu, cpu, counts }) + '\n', () => process.exit(0))
})().catch((e) => { console.error(e && e.stack || e); process.exit(1) })
