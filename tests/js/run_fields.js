'use strict'
// The fields a proposed change touches, answered by the JS restatement (oracle/js/backend.js) itself:
// stdin {docs: [{changes: [...], reqs: [{actor, seq, deps, fields: [[obj, key], ...]}]}]}.  Per request
// the document is rebuilt from its changes; each field's current ops are read (what fieldOps copies:
// obj.keys.get(key), winner first), the document's queue is emptied (a would-be change that is not
// ready is then the queue's only entry), then the would-be change is applied with one `del` per field: a
// del keeps exactly the ops that isConcurrent with it, so an op that is gone afterwards is covered.
// ready = the change was applied, not queued (causallyReady).  The fields of a request are distinct.
// Printed: {docs: [[{ready, fields: [[{action, value, datatype?, actor, seq, covered}]]}]]}
const path = require('path')
const J = require(path.join(__dirname, '..', '..', 'oracle', 'js', 'backend.js'))

let text = ''
process.stdin.on('data', (d) => { text += d })
process.stdin.on('end', () => {
  const input = JSON.parse(text)
  const docs = input.docs.map((doc) => doc.reqs.map((req) => {
    const s = J.Backend.init()
    J.Backend.applyChanges(s, doc.changes)
    const cur = (obj, key) => { const o = s.objs.get(obj); return o ? o.keys.get(key) || [] : [] }
    const before = req.fields.map(([obj, key]) => cur(obj, key).slice())
    const ops = req.fields.filter(([obj]) => s.objs.has(obj)).map(([obj, key]) => ({ action: 'del', obj, key }))
    // the answer is about the would-be change alone: changes of the document that wait for its
    // (actor, seq) must not apply behind it (they would rewrite the fields, or name what its real ops make)
    s.queue = []
    J.Backend.applyChanges(s, [{ actor: req.actor, seq: req.seq, deps: req.deps, ops }])
    const ready = (s.clock.get(req.actor) || 0) === req.seq
    const fields = req.fields.map(([obj, key], f) => {
      if (!ready) return []
      const left = cur(obj, key)
      return before[f].map((o) => {
        const r = { action: o.action, value: o.value, actor: o.actor, seq: o.seq,
          covered: !left.some((x) => x.actor === o.actor && x.seq === o.seq) }
        if (o.datatype) r.datatype = o.datatype
        return r
      })
    })
    return { ready, fields }
  }))
  process.stdout.write(JSON.stringify({ docs }) + '\n', () => process.exit(0))
})
