"""The resident store at its arena-full edge (store.cpp compact / seg_cap, store_kernels.hip
plan_kernel / alloc_kernel): submits whose growing segments just fit the free rows of an arena,
fit them exactly, or miss them by one segment.

The store keeps its rows in four bump-allocated arenas (changes, deps, ops, registers).  A
submit's growth either fits the free rows of every arena (the segments are allocated in place) or
the store compacts into larger arenas and plans again; the verdict is one per submit.  When the
free rows lie in [need, 2 need) a verdict taken from the advancing bump pointers would differ
between the threads of one launch, so that window is where most cases here sit.

`Fill` keeps a host restatement of the segment policy beside the store, only to size the
submits: every case reads hm_store_arena_info before the submit under test, asserts its
precondition from what the store itself reports, and afterwards asserts that the bump pointers
moved by exactly the rows the submit needed (no document skipped, none counted twice) and whether
the capacities changed (a compaction).  Each case runs once; every document of the submit under
test is compared bit-exactly with the oracle's cold merge of its whole log."""
import json

import pytest

from hypermerge_amd.render import canonical_json
from hypermerge_amd.store import DocStore

from kat_cases import ch, s
from test_store_gpu import assert_doc_matches_oracle

pytestmark = pytest.mark.gpu

SPACES = ("changes", "deps", "ops", "regs")
TOTALS = ("n_changes", "n_deps", "n_ops", "n_regs", "n_objs", "n_actors", "hist_len", "n_queued", "n_surv", "status")


def seg(n):
    """Rows of a segment made for n rows: n and a quarter as many again, to a power of two, at
    least 16 (store.cpp seg_cap, plan_kernel grow_rows / pow2c)."""
    x = max(n + n // 4, 16)
    return 1 << (x - 1).bit_length()


def rows_of(changes):
    """(changes, deps, ops, ROOT keys) that changes of set ops on ROOT add to a log."""
    return (len(changes), sum(len(c["deps"]) for c in changes), sum(len(c["ops"]) for c in changes),
            {o["key"] for c in changes for o in c["ops"]})


def new_doc_need(changes):
    """Rows per space a new document with this log takes (nothing for a space it has no row in)."""
    c, d, o, keys = rows_of(changes)
    return [seg(x) if x else 0 for x in (c, d, o, len(keys))]


class Submit:
    """What Fill.apply saw: the result, the arenas before and after, the rows the plan that
    allocated needed, whether the store compacted, and the bump pointers expected after."""

    def __init__(self, res, before, after, need, compacted, expect_used):
        self.res, self.before, self.after, self.need = res, before, after, need
        self.compacted, self.expect_used = compacted, expect_used


class Fill:
    """A DocStore and, per handle, what the segment policy gives it: rows and segment capacity
    per space, the ROOT keys (registers) and the log applied so far."""

    def __init__(self, engine, incremental=None):
        self.store = DocStore(engine, a_stride=8)
        if incremental is not None:
            self.store.set_incremental(incremental)
        self.n, self.cap, self.keys, self.logs = [], [], [], []

    def open(self, k):
        hs = [self.store.open() for _ in range(k)]
        for _ in hs:
            self.n.append([0, 0, 0, 0])
            self.cap.append([0, 0, 0, 0])
            self.keys.append(set())
            self.logs.append([])
        return hs

    def new(self, make, k, base=0):
        return [(h, make(base + j)) for j, h in enumerate(self.open(k))]

    def free(self):
        a = self.store.arena()
        return [c - u for c, u in zip(a["cap"], a["used"])]

    def _after(self, h, changes):
        c, d, o, keys = rows_of(changes)
        n = self.n[h]
        return [n[0] + c, n[1] + d, n[2] + o, len(self.keys[h] | keys)]

    def need(self, items, compacted=False):
        """Rows per space the submit's growing segments take: a segment that the new total outgrows
        is replaced by one made for that total.  compacted: as planned again after a compaction,
        which gave every open handle segments made for its rows."""
        tot = [0, 0, 0, 0]
        for h, changes in items:
            cap = [seg(x) for x in self.n[h]] if compacted else self.cap[h]
            for k, x in enumerate(self._after(h, changes)):
                if x > cap[k]:
                    tot[k] += seg(x)
        return tot

    def apply(self, items, undo=False):
        """One submit (undo: followed by hm_batch_undo of it)."""
        st = self.store
        a0 = st.arena()
        after = {h: self._after(h, changes) for h, changes in items}
        need0, need1 = self.need(items), self.need(items, compacted=True)
        packed = [sum(seg(n[k]) for n in self.n) for k in range(4)]      # every handle's segments after a compaction
        snaps = [st.enc[h].snapshot() for h, _ in items] if undo else None
        st.submit(items)
        bid = st._pending[0]
        r = st.wait()
        if undo:
            st._check(st._L.hm_batch_undo(st._h, bid), "hm_batch_undo")
            for (h, _), sn in zip(items, snaps):
                st.enc[h].restore(sn)
        a1 = st.arena()
        compacted = a1["cap"] != a0["cap"]
        if compacted:
            self.cap = [[seg(x) for x in n] for n in self.n]
        for j, (h, changes) in enumerate(items):
            for k, x in enumerate(after[h]):
                if x > self.cap[h][k]:
                    self.cap[h][k] = seg(x)                   # (a rolled-back document keeps its new segment)
            if not undo and int(r.docs["status"][j]) == 0:
                self.n[h] = after[h]
                self.keys[h] |= rows_of(changes)[3]
                self.logs[h] = self.logs[h] + list(changes)
        need = need1 if compacted else need0
        base = packed if compacted else a0["used"]
        return Submit(r, a0, a1, need, compacted, [b + x for b, x in zip(base, need)])

    def reset(self, hs):
        self.store.reset(hs)
        for h in hs:
            self.n[h], self.cap[h], self.keys[h], self.logs[h] = [0, 0, 0, 0], [0, 0, 0, 0], set(), []

    def check(self, hs):
        for h in hs:
            b, _ = assert_doc_matches_oracle(self.store, h)
            assert len(b.changes) == len(self.logs[h]), h

    def totals(self, h):
        i = self.store.info(h)
        return [i[f] for f in TOTALS]


def fitted(sub):
    """The submit was allocated in place: no compaction, and the bump pointers moved by its need."""
    assert not sub.compacted and sub.after["cap"] == sub.before["cap"], (sub.before, sub.after)
    assert sub.after["used"] == sub.expect_used, (sub.before, sub.after, sub.need)


def compacted(sub):
    """The store compacted for the submit: larger arenas, every handle's segments packed, then the
    submit's growth as planned again on the packed segments."""
    assert sub.compacted, (sub.before, sub.after, sub.need)
    assert sub.after["used"] == sub.expect_used, (sub.before, sub.after, sub.need)
    assert all(u <= c for u, c in zip(sub.after["used"], sub.after["cap"]))


# ---- the documents: each kind makes another arena run out first ----
def tiny(i):
    """One change with one set: 16 change, 16 op and 16 register rows, no dep row."""
    return [ch(f"t{i % 7}", 1, {}, s("x", i))]


def many_ops(i):
    """One change of 24 sets on 12 keys: 32 op rows to 16 change and 16 register rows."""
    return [ch(f"o{i % 5}", 1, {}, *[s(f"k{j % 12}", i + j) for j in range(24)])]


def many_keys(i):
    """One change of 20 sets on 20 keys: 32 register (and op) rows to 16 change rows."""
    return [ch(f"r{i % 3}", 1, {}, *[s(f"k{j}", i + j) for j in range(20)])]


def many_deps(i):
    """Seven actors' first changes, then six changes of an eighth that each list all seven: 42 dep
    rows (a 64-row segment) to 13 change and 13 op rows (16-row segments)."""
    others = [f"d{j}" for j in range(1, 8)]
    first = [ch(a, 1, {}, s(f"k{j}", i + j)) for j, a in enumerate(others)]
    seen = {a: 1 for a in others}
    return first + [ch("d0", q, dict(seen), s("x", i + q)) for q in range(1, 7)]


def heavy_ops(i):
    """One change of 200 sets on two keys: a 256-row op segment."""
    return [ch("h0", 1, {}, *[s(f"k{j % 2}", i + j) for j in range(200)])]


KINDS = {"changes": tiny, "deps": many_deps, "ops": many_ops, "regs": many_keys}


def _alone(space, need, free):
    """`space` is in the window need <= free < 2 need and every other arena has room for twice its
    need (with the tiny documents the op and register arenas fill in step with the change arena)."""
    k = SPACES.index(space)
    assert 0 < need[k] <= free[k] < 2 * need[k], (space, need, free)
    for j in range(4):
        if j != k and not (space == "changes" and (need[j], free[j]) == (need[k], free[k])):
            assert 2 * need[j] <= free[j], (SPACES[j], need, free)


def _to_window(engine, space, fill=None, window=None):
    """A store in which `space` is the arena that runs out first, filled, and the window submit
    made on it: returns (Fill, the documents' maker, the space's rows per new document).  All of
    the window's conditions are asserted here."""
    f, make, k = Fill(engine), KINDS[space], SPACES.index(space)
    if space == "regs":
        # a register has an op, so on a fresh store the op arena runs out no later than the
        # register arena: one submit of op-heavy documents first compacts into a larger op arena
        sub = f.apply(f.new(heavy_ops, 300))
        assert (sub.res.docs["status"] == 0).all()
        compacted(sub)
        assert sub.after["cap"][2] > sub.after["cap"][3]
    per = new_doc_need(make(0))[k]
    free = f.free()
    assert per and free[k] % per == 0, (free, per)
    total = free[k] // per                                     # new documents that fill the arena exactly
    if window is None:
        window = total // 4 + (37 if (total // 4) % 64 == 0 else 0)
        fill = total - window - 96
    # several workgroups of alloc_kernel, the last one and its last wave partly filled
    assert window > 256 and window % 256 and window % 64
    sub = f.apply(f.new(make, fill))
    assert (sub.res.docs["status"] == 0).all()
    fitted(sub)
    items = f.new(make, window, fill)
    _alone(space, f.need(items), f.free())                     # the precondition, from the store's own figures
    sub = f.apply(items)
    assert (sub.res.docs["status"] == 0).all()
    fitted(sub)
    assert sum(f.store.last_routing().values()) == len(items)
    f.check(range(len(f.n)) if space == "changes" else [h for h, _ in items])
    return f, make, per


def test_arena_info_of_a_fresh_store_and_with_a_batch_pending(engine):
    """hm_store_arena_info: four arenas of 65,536 rows with nothing handed out, then the segments
    of one submit; refused like the other reads while a batch is in flight."""
    from hypermerge_amd.engine import EngineError
    f = Fill(engine)
    assert f.store.arena() == {"cap": [65536] * 4, "used": [0] * 4}
    items = f.new(many_deps, 3)
    f.store.submit(items)
    with pytest.raises(EngineError):
        f.store.arena()
    assert (f.store.wait().docs["status"] == 0).all()
    assert f.store.arena() == {"cap": [65536] * 4, "used": [3 * x for x in new_doc_need(many_deps(0))]}


@pytest.mark.parametrize("tail", ["exact", "short"])
@pytest.mark.parametrize("space", SPACES)
def test_window_then_exact_fit_or_one_segment_short(engine, space, tail):
    """Each arena in turn runs out first (the other three have room to spare).  The window: a
    submit of several workgroups, the last partly filled, whose need lies in (free / 2, free] — it
    fits, so the capacities stay, the bump pointers move by exactly its need and every document
    is there.  Then either the submit that fills the arena to its last row (still no compaction),
    or the one that needs one segment more than is free (compaction, every document kept).
    `changes`: the base case, 3,000 one-set documents then 1,000 in the window."""
    f, make, per = _to_window(engine, space, *((3000, 1000) if space == "changes" else ()))
    k = SPACES.index(space)
    free = f.free()
    assert free[k] % per == 0 and 0 < free[k] // per < 256
    items = f.new(make, free[k] // per + (tail == "short"), 10 ** 6)
    need = f.need(items)
    # (the other arenas take it either way; the one-set documents' op and register arenas are in step)
    assert all(need[j] <= free[j] or (need[j], free[j]) == (need[k], free[k]) for j in range(4) if j != k)
    if tail == "exact":
        assert need[k] == free[k]
        sub = f.apply(items)
        fitted(sub)
        assert sub.after["used"][k] == sub.after["cap"][k]
    else:
        assert need[k] == free[k] + per
        sub = f.apply(items)
        compacted(sub)
        assert sub.after["cap"][k] > sub.before["cap"][k]
    assert (sub.res.docs["status"] == 0).all()
    f.check(range(len(f.n)))                                   # every document, old and new


@pytest.mark.parametrize("mode", [1, 2, 0])
def test_growing_segments_in_the_window(engine, mode):
    """The need comes from segments that move (16 rows to 32 in the change and op arenas), not from
    new documents; documents that grow, documents that take a change without growing and documents
    that receive nothing alternate within every wave, so the re-merge list, the append list and the
    lanes with no work interleave in alloc_kernel's list offsets.  Under the incremental modes the
    documents hold incremental state and the submit is routed to the incremental kernels."""
    f = Fill(engine, incremental=mode)
    hs = f.open(600)
    kind = [0 if i % 6 < 3 else 1 if i % 6 < 5 else 2 for i in range(600)]      # grows / fits / receives nothing
    first = {0: 13, 1: 10, 2: 1}

    def more(h, k):
        q = len(f.logs[h])
        return [ch("g", q + 1 + j, {}, s(f"k{(q + j) % 3}", h * 100 + q + j)) for j in range(k)]
    sub = f.apply([(h, more(h, first[kind[i]])) for i, h in enumerate(hs)])
    assert (sub.res.docs["status"] == 0).all()
    sub = f.apply([(h, more(h, 3)) for i, h in enumerate(hs) if kind[i] < 2])        # 16 of 16 rows / 13 of 16
    assert (sub.res.docs["status"] == 0).all()
    fitted(sub)
    items = [(h, more(h, 1) if kind[i] < 2 else []) for i, h in enumerate(hs)]
    need = f.need(items)
    assert need == [300 * 32, 0, 300 * 32, 0]
    # one-set documents (not part of the submit) up to the window
    free = f.free()
    sub = f.apply(f.new(tiny, (free[0] - need[0] - need[0] // 4) // 16))
    fitted(sub)
    free = f.free()
    assert need[0] <= free[0] < 2 * need[0] and need[2] <= free[2] < 2 * need[2], (need, free)
    if mode:
        assert f.store.inc_states() > 0
    sub = f.apply(items)
    assert (sub.res.docs["status"] == 0).all()
    fitted(sub)
    r = f.store.last_routing()
    assert sum(r.values()) == 600, r
    if mode:
        # every document with a new change was planned incremental; those without re-merge
        assert r["incremental"] > 0 and r["incremental"] + r["handed_back"] == 500 and r["remerged"] == 100, r
    else:
        assert r == {"incremental": 0, "remerged": 600, "handed_back": 0}, r
    f.check(hs)


@pytest.mark.parametrize("tail", ["window", "short"])
def test_rollback_next_to_the_boundary(engine, tail):
    """A window submit, and one that needs one segment more than is free, each with a few documents
    that throw (a sequence number reused with other content): those keep their state and totals,
    the rest are as the oracle has them, and the rolled-back documents take a later submit."""
    f = Fill(engine)
    sub = f.apply(f.new(tiny, 3000))
    fitted(sub)
    old = list(range(3000))
    bad = old[5::431]                                          # 7 documents
    assert len(bad) == 7
    free = f.free()
    n_new = 993 if tail == "window" else free[0] // 16 + 1
    new = f.new(tiny, n_new, 5000)
    throws = {h: [ch("zz", 1, {}, s("z", 5)), ch(f.logs[h][0]["actor"], 1, {}, s("x", -1))] for h in bad}
    # the throwing documents spread over the submit's workgroups
    items = list(new)
    for j, h in enumerate(bad):
        items.insert(j * (len(items) // 7) + 3, (h, throws[h]))
    need = f.need(items)
    if tail == "window":
        assert len(items) == 1000 and all(0 < need[k] <= free[k] < 2 * need[k] for k in (0, 2, 3)), (need, free)
    else:
        assert need[0] == free[0] + 16, (need, free)
    before = {h: (canonical_json(*f.store.read(h), 0), f.totals(h)) for h in bad}
    sub = f.apply(items)
    st = sub.res.docs["status"]
    for j, (h, _) in enumerate(items):
        assert int(st[j]) == (1 if h in throws else 0), (j, h, st[j])
    (fitted if tail == "window" else compacted)(sub)
    for h in bad:
        assert (canonical_json(*f.store.read(h), 0), f.totals(h)) == before[h], h
    f.check([h for h, _ in items])
    f.check(old[::50])
    sub = f.apply([(h, throws[h][:1]) for h in bad])
    assert (sub.res.docs["status"] == 0).all()
    f.check(bad)


def test_undo_across_a_compaction(engine):
    """hm_batch_undo of the submit that compacted the store: every document of it (new ones and
    ones that had a state) is back at its rendering and totals from before the submit, in the new
    arenas; the same changes applied again give the oracle's state."""
    f = Fill(engine)
    sub = f.apply(f.new(tiny, 3000))
    fitted(sub)
    free = f.free()
    grown = list(range(0, 3000, 60))                           # 50 documents with a state
    items = [(h, [ch(f.logs[h][0]["actor"], 2, {}, s("y", h))]) for h in grown] + f.new(tiny, free[0] // 16 + 1, 5000)
    assert f.need(items)[0] == free[0] + 16
    before = {h: (canonical_json(*f.store.read(h), 0), f.totals(h)) for h, _ in items}
    sub = f.apply(items, undo=True)
    assert (sub.res.docs["status"] == 0).all()
    assert sub.compacted and sub.after["cap"][0] > sub.before["cap"][0]
    for h, _ in items:
        assert (canonical_json(*f.store.read(h), 0), f.totals(h)) == before[h], h
    f.check(range(1, 3000, 60))                                # bystanders of the compaction
    sub = f.apply(items)
    assert (sub.res.docs["status"] == 0).all()
    fitted(sub)
    f.check([h for h, _ in items])


def test_dead_space_and_reset_through_a_compaction(engine):
    """Half the documents reset: their rows are dead until the store compacts.  A submit of new
    documents that no longer fits compacts; the reset handles are empty documents after it, the
    survivors are as the oracle has them, and the reset handles then take new logs."""
    f = Fill(engine)
    sub = f.apply(f.new(tiny, 3000))
    fitted(sub)
    a0 = f.store.arena()
    gone, kept = list(range(0, 3000, 2)), list(range(1, 3000, 2))
    f.reset(gone)
    assert f.store.arena() == a0                               # dead rows stay allocated
    free = f.free()
    items = f.new(tiny, free[0] // 16 + 1, 5000)
    assert f.need(items)[0] == free[0] + 16
    sub = f.apply(items)
    assert (sub.res.docs["status"] == 0).all()
    compacted(sub)
    for h in gone:
        i = f.store.info(h)
        assert (i["n_changes"], i["n_ops"], i["n_regs"], i["hist_len"], i["status"]) == (0, 0, 0, 0, 0), (h, i)
    f.check(kept)
    f.check([h for h, _ in items])
    again = [(h, tiny(7000 + h) + [ch(f"t{(7000 + h) % 7}", 2, {}, s("y", h))]) for h in gone]
    sub = f.apply(again)
    assert (sub.res.docs["status"] == 0).all()
    fitted(sub)
    f.check(gone)
    f.check(kept[::25])


def test_docset_store_crosses_the_window_and_a_compaction():
    """The docset's stride-8 store over the same edge: 3,000 one-set documents, 1,000 more (its
    change, op and register arenas of 65,536 rows then hold 64,000: the window), then 1,100 that
    no longer fit (a compaction), each group followed by a second round.  Results, clocks and
    patches round by round, and every document's view, history and rebuilt patches at the end,
    equal the oracle's."""
    from hypermerge_amd.columnar import ROOT_ID as R
    from hypermerge_amd.docset import DocSet, render_objects, view_objects
    from hypermerge_amd.engine import Engine
    from test_docset_gpu import _oracle, _run

    def doc(i):
        a = f"a{i % 5}"
        return [[{"actor": a, "seq": 1, "deps": {}, "ops": [{"action": "set", "obj": R, "key": "x", "value": i}]}],
                [{"actor": a, "seq": 2, "deps": {}, "ops": [{"action": "set", "obj": R, "key": "y", "value": -i}]}]]
    ds = DocSet(Engine(0))
    runs = [_run(ds, [doc(i) for i in range(lo, hi)]) for lo, hi in ((0, 3000), (3000, 4000), (4000, 5100))]
    for ids, objects, logs, last in runs:
        for i, d in enumerate(ids):
            sm = _oracle(logs[i])
            assert sm["status"] == "OK"
            state = json.loads(json.dumps(sm["state"]))
            assert render_objects(objects[i]) == state, d
            assert render_objects(view_objects(ds.view(d))) == state, d
            order = ds.history_prefix(d, 1 << 20)
            assert [[logs[i][k]["actor"], logs[i][k]["seq"]] for k in order] == sm["history"], d
            assert last[i][1]["clock"] == sm["clock"] and last[i][2] == sm["backend_clock"]
    assert ds.stats()["calls"] == 6
