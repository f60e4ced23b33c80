'use strict'
// Patch sequences of GpuDocBackend with the device-diffs route (GpuEngine({ diffs: 'device' }):
// every round's per-op diffs rendered from the device's op-diff rows) against the JS restatement
// (test driver for tests/test_round_diffs_node_gpu.py).  Input {feeds: [[document chunks]], mode}:
// each feed runs through an engine of its own, its documents fed in the same chunks (init, then
// applyRemoteChanges one event-loop turn apart) through the reference DocBackend API of both;
// every delivered message's patch is collected per document.  Output: {feeds: [{docs: [{gpu,
// cpu}], stats}]}.
const path = require('path')
const G = require(path.join(__dirname, '..', '..', 'hypermerge_amd', 'js', 'GpuDocBackend.js'))
const C = require(path.join(__dirname, '..', '..', 'oracle', 'js', 'backend.js'))

const input = JSON.parse(require('fs').readFileSync(0, 'utf8'))
const tick = () => new Promise((r) => setImmediate(r))
const keep = (m) => (m.patch ? { type: m.type, history: m.history, patch: m.patch } : { type: m.type, history: m.history })

async function run (feed, f) {
  const engine = new G.GpuEngine({ mode: input.mode || 'sync', diffs: 'device' })
  const docs = feed.map((chunks, i) => {
    const gpu = [], cpu = []
    return {
      g: new G.DocBackend('feed' + f + 'doc' + i, (m) => gpu.push(keep(m)), undefined, engine),
      c: new C.DocBackend('feed' + f + 'doc' + i, (m) => cpu.push(keep(m))),
      chunks, gpu, cpu,
    }
  })
  const rounds = Math.max(...feed.map((c) => c.length))
  for (let r = 0; r < rounds; r++) {
    for (const x of docs) {
      if (r >= x.chunks.length) continue
      if (r === 0) { x.g.init(x.chunks[0], 'local'); x.c.init(x.chunks[0], 'local') }
      else if (x.chunks[r].length) { x.g.applyRemoteChanges(x.chunks[r]); x.c.applyRemoteChanges(x.chunks[r]) }
    }
    if (engine.mode === 'async') await engine.idle()
    else { await tick(); await tick() }
  }
  return { docs: docs.map((x) => ({ gpu: x.gpu, cpu: x.cpu })), stats: engine.stats(), diffs: engine.diffs }
}

;(async () => {
  const feeds = []
  for (let f = 0; f < input.feeds.length; f++) feeds.push(await run(input.feeds[f], f))
  process.stdout.write(JSON.stringify({ feeds }) + '\n')
})().catch((e) => { console.error(e); process.exit(1) })
