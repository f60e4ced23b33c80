"""The fields a proposed local change touches, restated sequentially over a merge's tables (test
reference only): oracle/js/backend.js applyChange / transitiveDeps / isConcurrent / fieldOps.

    request = (ordered entries (rank, seq), registers); the entries are the would-be change's
              base = {...deps}; base[actor] = seq - 1 in key order
    ready   = every entry has seq <= opSet.clock[actor]            (causallyReady)
    closure = transitiveDeps(entries)                               (missing_changes_ref.closure)
    per register, in request order: its survivors, winner first (fieldOps); per survivor
        (op, action, datatype, vtag, value, actor rank, seq, covered = closure[actor] >= seq)
    covered <=> not isConcurrent(survivor, would-be op): the would-be change's allDeps is the
    closure, and an applied change's allDeps never reaches a change that does not exist yet.
A request that is not ready has no rows and a zero closure; a register at or past n_regs, or one
never touched, has none either.  Expected values in the tests come from here applied to
``oracle.merge`` of the same log (or are written out by hand), never from the engine."""
from missing_changes_ref import closure

NONE = 0xFFFFFFFF


def js_key_order(obj):
    """The (key, value) pairs of a dict in the order Object.keys lists a JS object's: the keys that
    are canonical array indices (an actor id written in decimal digits only, such as "19613698", is
    one) ascending by number, then the others in insertion order."""
    index = lambda k: k.isdigit() and str(int(k)) == k and int(k) < 0xFFFFFFFF
    return sorted(((k, v) for k, v in obj.items() if index(k)), key=lambda kv: int(kv[0])) + \
        [(k, v) for k, v in obj.items() if not index(k)]


def base_entries(rank, actor, seq, deps):
    """The entries of the would-be change (actor, seq, deps {actorId: seq}): base = {...deps};
    base[actor] = seq - 1 in JS key order, over the ranks in ``rank`` ({actorId: rank}).  Returns
    (entries, unknown): unknown = an id the document has never seen has a seq above 0."""
    base = dict(deps)
    base[actor] = seq - 1                      # (keeps its place when deps names it, else goes last)
    ents, unknown = [], False
    for a, q in js_key_order(base):
        if a in rank:
            ents.append((rank[a], int(q)))
        elif q > 0:
            unknown = True
    return ents, unknown


def fields(changes, hist, all_deps, clock, regs, surv, ops, S, entries, field_regs, op_base=0):
    """(ready, closure row, per register its rows) of one document: changes / hist / all_deps its
    change rows (op_first counted from op_base), regs / surv / ops its own segments."""
    if any(q > int(clock[a]) for a, q in entries):
        return False, [0] * S, [[] for _ in field_regs]
    deps = closure(changes, hist, all_deps, S, entries)
    owner = {}
    for i, c in enumerate(changes):
        for k in range(int(c["n_ops"])):
            owner[int(c["op_first"]) - op_base + k] = i
    out = []
    for reg in field_regs:
        rows = []
        if reg < len(regs) and int(regs[reg]["obj"]) != NONE:
            r = regs[reg]
            for k in range(int(r["n_surv"])):
                sv = surv[int(r["surv_off"]) + k]
                op = int(sv["op"])
                c = changes[owner[op]]
                a, q = int(c["actor"]), int(c["seq"])
                rows.append((op, int(ops[op]["action"]), int(ops[op]["datatype"]), int(sv["vtag"]), int(sv["value"]),
                             a, q, deps[a] >= q))
        out.append(rows)
    return True, deps, out


def doc_ref(b, o, d, entries, field_regs):
    """The same for document d of batch b with oracle results o (a document whose merge threw offers
    nothing: no rows, and a clock of zeros)."""
    S = b.a_stride
    row = b.docs[d]
    c0, n = int(row["change_off"]), int(row["n_changes"])
    o0, no = int(row["op_off"]), int(row["n_ops"])
    r0, nr = int(row["reg_off"]), int(row["n_regs"])
    clock = o.clock[d * S:(d + 1) * S]
    if int(o.docs["status"][d]) != 0:
        n, nr, clock = 0, 0, [0] * S
    return fields(b.changes[c0:c0 + n], o.hist[c0:c0 + n], o.all_deps[c0 * S:(c0 + n) * S], clock, o.regs[r0:r0 + nr],
                  o.surv[o0:o0 + no], b.ops[o0:o0 + no], S, entries, field_regs, op_base=o0)


def rows_of(table):
    """FIELD_OP_DT rows (engine.py) as the tuples ``fields`` returns."""
    return [(int(r["op"]), int(r["action"]), int(r["datatype"]), int(r["vtag"]), int(r["value"]), int(r["actor"]),
             int(r["seq"]), bool(r["covered"])) for r in table]
