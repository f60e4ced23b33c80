'use strict'
// Backend.getPatch(state) / GpuEngine.getPatches(states) / GpuEngine.views(states) of the GPU drop-in
// (docsetGetPatch / docsetViews under them) against the route they replace, restated here: the
// document read with addon.docsetView and turned into diffs (a create per object but ROOT, then per
// object its sets in key order and its inserts in element order).  argv[2] = JSON list of device
// ordinals (one shard each); stdin = JSON {docs: [[chunk of changes, ...], ...]}, fed in rounds.
// A frontend (applyDiffs below) that applies a patch to an empty document must arrive at the plain
// document of materializeAt(history).
// Prints {docs, shards, mismatches, manyMismatches, viewMismatches, frontendMismatches, diffs, inserts, conflicts, counters, tables}.
const path = require('path')
const assert = require('assert')
const G = require(path.join(__dirname, '..', '..', 'hypermerge_amd', 'js', 'GpuDocBackend.js'))
const ROOT = '00000000-0000-0000-0000-000000000000'

// the old route: Backend.getPatch as it was built from one docsetView read per document
function oldPatch(state) {
  const v = JSON.parse(G.addon.docsetView(state.ds, state.id))
  const diffs = []
  for (const [uuid, ov] of Object.entries(v)) if (uuid !== ROOT) diffs.push({ action: 'create', obj: uuid, type: ov.type })
  for (const [uuid, ov] of Object.entries(v)) {
    for (const [key, e] of ov.keys) diffs.push(Object.assign({ action: 'set', type: ov.type, obj: uuid, key }, e))
    ov.elems.forEach(([elemId, e], index) => diffs.push(Object.assign({ action: 'insert', type: ov.type, obj: uuid, index, elemId }, e)))
  }
  return { clock: Object.assign({}, state.clock), deps: Object.assign({}, state.deps), canUndo: state.canUndo, canRedo: state.canRedo, diffs }
}

// Frontend.applyPatch's effect on an empty document, then the plain document
function applyDiffs(diffs) {
  const objs = { [ROOT]: { type: 'map', keys: new Map(), elems: [] } }
  for (const d of diffs) {
    if (d.action === 'create') { objs[d.obj] = { type: d.type, keys: new Map(), elems: [] }; continue }
    const o = objs[d.obj]
    const e = { value: d.value, link: !!d.link }
    if (d.type === 'list' || d.type === 'text') {
      if (d.action === 'insert') o.elems.splice(d.index, 0, e)
      else if (d.action === 'set') o.elems[d.index] = e
      else o.elems.splice(d.index, 1)
    } else if (d.action === 'set') o.keys.set(d.key, e)
    else o.keys.delete(d.key)
  }
  const plain = (uuid) => {
    const o = objs[uuid]
    if (!o) return {}
    const val = (e) => (e.link ? plain(e.value) : e.value)
    if (o.type === 'list' || o.type === 'text') return o.elems.map(val)
    const out = {}
    for (const [k, e] of o.keys) out[k] = val(e)
    return out
  }
  return plain(ROOT)
}

const same = (a, b) => { try { assert.deepStrictEqual(a, b); return true } catch (e) { return false } }

const devices = JSON.parse(process.argv[2] || '[0]')
const input = JSON.parse(require('fs').readFileSync(0, 'utf8'))
const engine = new G.GpuEngine({ devices, mode: 'sync', aStride: 8 })
const Backend = G.makeBackend(engine)
const states = input.docs.map((_, i) => engine.init('doc' + i))
const rounds = Math.max(0, ...input.docs.map((c) => c.length))
for (let r = 0; r < rounds; r++) {
  input.docs.forEach((chunks, i) => { if (r < chunks.length && chunks[r].length) engine.applyChanges(states[i], chunks[r]) })
}
states.push(engine.init('never-written'))                       // (not placed in any stride class yet)

const out = { docs: states.length, shards: new Set(states.map((s) => s.shard)).size, mismatches: [], manyMismatches: [],
  viewMismatches: [], frontendMismatches: [], diffs: 0, inserts: 0, conflicts: 0, counters: 0, tables: 0 }
const many = engine.getPatches(states)
const views = engine.views(states)
states.forEach((st, i) => {
  const want = oldPatch(st)
  const got = Backend.getPatch(st)
  if (!same(got, want)) out.mismatches.push(i)
  const m = Object.assign({}, many[i].patch, { canUndo: st.canUndo, canRedo: st.canRedo })
  if (!same(m, want) || many[i].history !== st.histLen) out.manyMismatches.push(i)
  if (!same(views[i], JSON.parse(G.addon.docsetView(st.ds, st.id)))) out.viewMismatches.push(i)
  const at = engine.materialize([{ state: st, history: many[i].history }])[0]
  if (!same(applyDiffs(got.diffs), at.doc)) out.frontendMismatches.push(i)
  out.diffs += got.diffs.length
  for (const d of got.diffs) {
    if (d.action === 'insert') out.inserts++
    if (d.conflicts) out.conflicts++
    if (d.datatype === 'counter') out.counters++
    if (d.type === 'table') out.tables++
  }
})
process.stdout.write(JSON.stringify(out) + '\n')
