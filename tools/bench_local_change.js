'use strict'
// Local changes through GpuDocBackend, once per undo route, from one build: stdin {docs: {name:
// {changes, text?: uuid, last?: elemId}}, inserts, deletes, undos}.  Per document two engines
// ('view': the whole merged document read and parsed per undoable request; 'fields': one device
// query for the fields the request touches) each hold a copy; every request is issued to both,
// alternating which goes first, and timed from applyLocalChange to engine.idle() (sync mode: the
// round's device work has finished and its patch is rendered).  Printed: {name: {route: {kind:
// [microseconds ...]}}}.  Driven by tools/bench_local_change.py.
const path = require('path')
const G = require(path.join(__dirname, '..', 'hypermerge_amd', 'js', 'GpuDocBackend.js'))
const ROOT = '00000000-0000-0000-0000-000000000000'
const ROUTES = ['view', 'fields']

async function timed(engine, doc, req) {
  const t0 = process.hrtime.bigint()
  doc.applyLocalChange(req)
  await engine.idle()
  return Number(process.hrtime.bigint() - t0) / 1e3
}

async function bench(name, spec, cfg) {
  const side = {}
  for (const route of ROUTES) {
    let err = null
    const engine = new G.GpuEngine({ mode: 'sync', aStride: 8, undo: route, onError: (e) => { err = e } })
    const doc = new G.DocBackend(name, () => {}, undefined, engine)
    doc.init(spec.changes, 'mmmm')
    await engine.idle()
    side[route] = { engine, doc, seq: 0, times: { insert: [], delete: [], undo: [], redo: [] }, fail: () => err }
  }
  const heads = {}
  for (const c of spec.changes) heads[c.actor] = Math.max(heads[c.actor] || 0, c.seq)
  let flip = 0
  const both = async (kind, make, keep) => {
    const order = flip++ % 2 ? ROUTES : ROUTES.slice().reverse()
    for (const route of order) {
      const s = side[route]
      const t = await timed(s.engine, s.doc, make(++s.seq))
      if (s.fail()) throw s.fail()
      if (keep) s.times[kind].push(t)
    }
  }
  const change = (seq, ops) => ({ requestType: 'change', actor: 'mmmm', seq, deps: Object.assign({}, heads), ops })
  let elem = 1000000, prev = spec.last || '_head'
  const typed = []
  const insert = (e) => (seq) => {
    const ops = spec.text ? [{ action: 'ins', obj: spec.text, key: prev, elem: e }, { action: 'set', obj: spec.text, key: 'mmmm:' + e, value: 'x' }]
      : [{ action: 'set', obj: ROOT, key: 'k' + (e % 8), value: e }]
    return change(seq, ops)
  }
  const warm = 10
  for (let i = 0; i < cfg.inserts + warm; i++) {
    await both('insert', insert(++elem), i >= warm)
    if (spec.text) { prev = 'mmmm:' + elem; typed.push(prev) }
  }
  for (let i = 0; i < cfg.deletes + warm; i++) {
    const key = spec.text ? typed[i % typed.length] : 'k' + (i % 8)
    await both('delete', (seq) => change(seq, [{ action: 'del', obj: spec.text || ROOT, key }]), i >= warm)
  }
  for (let i = 0; i < cfg.undos + 2; i++) {
    await both('undo', (seq) => ({ requestType: 'undo', actor: 'mmmm', seq, deps: Object.assign({}, heads) }), i >= 2)
    await both('redo', (seq) => ({ requestType: 'redo', actor: 'mmmm', seq, deps: Object.assign({}, heads) }), i >= 2)
  }
  const out = {}
  for (const route of ROUTES) out[route] = side[route].times
  return out
}

let text = ''
process.stdin.on('data', (d) => { text += d })
process.stdin.on('end', async () => {
  try {
    const cfg = JSON.parse(text)
    const out = {}
    for (const name of Object.keys(cfg.docs)) out[name] = await bench(name, cfg.docs[name], cfg)
    process.stdout.write(JSON.stringify(out) + '\n', () => process.exit(0))
  } catch (e) { console.error(e && e.stack || e); process.exit(1) }
})
