'use strict'
// Feeds documents one change at a time through the JS restatement (oracle/js/backend.js
// Backend.applyChanges) and prints, per document, per call: the history length after it and the
// diffs the call returned (per applied op, in application order).
const path = require('path')
const { Backend } = require(path.join(__dirname, '..', '..', 'oracle', 'js', 'backend.js'))

const input = JSON.parse(require('fs').readFileSync(0, 'utf8'))
const out = input.docs.map((changes) => {
  const s = Backend.init()
  const calls = []
  let err = null
  try {
    for (const c of changes) {
      const patch = Backend.applyChanges(s, [c])[1]
      calls.push([s.history.length, patch.diffs])
    }
  } catch (e) { err = e.message }
  return { err, calls }
})
process.stdout.write(JSON.stringify({ docs: out }) + '\n')
