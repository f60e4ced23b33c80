'use strict'
// Opens documents the way loadDocument does at a cursor: per request one Backend.applyChanges call on
// Backend.init() with the changes a clock selects (handed over by the caller, in the order it wants
// them applied).  Prints per request the history length, the changes left queued and the patch.
const path = require('path')
const { Backend } = require(path.join(__dirname, '..', '..', 'oracle', 'js', 'backend.js'))

const input = JSON.parse(require('fs').readFileSync(0, 'utf8'))
const out = input.docs.map((changes) => {
  const s = Backend.init()
  try {
    const patch = Backend.applyChanges(s, changes)[1]
    return { err: null, history: s.history.length, queued: s.queue.length, patch }
  } catch (e) { return { err: e.message, history: 0, queued: 0, patch: null } }
})
process.stdout.write(JSON.stringify({ docs: out }) + '\n')
