"""hm_docset_missing_changes over documents in two stride classes: have-clocks by actor id string,
in an insertion order that is not the rank order; a document that moved to a wider stride class;
an actor id a document has never seen.  Expected values: tests/missing_changes_ref.py on the CPU
oracle's merge of the same log, and answers written out by hand."""
import json

import pytest

from hypermerge_amd.columnar import encode
from hypermerge_amd.docset import DocSet
from hypermerge_amd.engine import EngineError
import oracle.oracle as O

from kat_cases import ch, s
from missing_changes_ref import ONLY_LISTED, RAW, doc_ref
from test_missing_changes_host import CHAIN, ranked

pytestmark = pytest.mark.gpu

A, B, Cc = "aaaa", "bbbb", "cccc"


def _blocks(changes):
    return [json.dumps(c, separators=(",", ":")).encode() for c in changes]


def _want(log, clock, flags=0):
    b = encode([log])
    return doc_ref(b, O.merge(b), 0, ranked(b.doc_actors[0], clock), flags)[0]


def test_docset_missing_changes(engine):
    ds = DocSet(engine)
    first = ds.open(4)
    chain, wide, mover, unplaced = range(first, first + 4)
    writers = [f"w{i:02d}" for i in range(11)]
    logs = {
        chain: list(CHAIN),
        wide: [ch(w, 1, {}, s("k", i)) for i, w in enumerate(writers)]
              + [ch("zzzz", 1, {w: 1 for w in writers[:6]}, s("six", 1)), ch(writers[8], 2, {"zzzz": 1}, s("k", 99))],
        mover: [ch(B, 2, {}, s("y", 2)), ch(B, 1, {}, s("y", 1)), ch(A, 1, {B: 2}, s("x", 1))],
    }
    ids = [chain, wide, mover]
    res, _ = ds.apply(ids, [_blocks(logs[d]) for d in ids])
    assert (res["status"] == 0).all()
    assert ds.info(chain)["a_stride"] == 8 and ds.info(wide)["a_stride"] == 16
    # written out: the order-dependent pair of test_missing_changes_host.py, by actor id
    got = ds.missing_changes([chain, chain, unplaced, mover, chain],
                             [{A: 2, B: 1}, {B: 1, A: 2}, {A: 1}, {A: 1}, {"nobody": 4, B: 2}])
    assert got == [[1, 2], [], [], [], [2, 3, 4]]
    assert ds.missing_changes([mover], [{}]) == [[1, 0, 2]]                  # history order, not log order
    assert ds.missing_changes([chain, mover], [{B: 1}, {B: 0}], RAW | ONLY_LISTED) == [[1, 2], [1, 0]]
    assert ds.missing_changes([chain], [{"nobody": 0}], RAW | ONLY_LISTED) == [[]]
    assert ds.missing_changes([], []) == []
    # the wide class, clocks in orders that are not the rank order
    clocks = [{"zzzz": 1, "w09": 1}, {"w09": 1, "w08": 2, "w00": 0}, {"w08": 2, "zzzz": 0, "w03": 1}, {}, {"w10": 7, "zzzz": 1.9}]
    got = ds.missing_changes([wide] * len(clocks), clocks)
    assert got[:4] == [_want(logs[wide], c) for c in clocks[:4]]
    assert got[0] == [6, 7, 8, 10, 12] and got[1] == [6, 7, 10]
    assert got[4] == _want(logs[wide], {"w10": 7, "zzzz": 1})               # seqs are JS numbers: truncated
    # the mover outgrows its class and keeps answering, by the same actor ids
    r2 = [ch(w, 1, {B: 1}, s("m", i)) for i, w in enumerate(writers[:8])] + [ch(A, 2, {writers[7]: 1}, s("x", 2))]
    res, _ = ds.apply([mover], [_blocks(r2)])
    assert (res["status"] == 0).all() and ds.info(mover)["a_stride"] == 16
    log = logs[mover] + r2
    clocks = [{A: 1}, {A: 2}, {writers[7]: 1, B: 2}, {B: 2, writers[7]: 1}, {writers[3]: 1, "nobody": 1}]
    got = ds.missing_changes([mover] * len(clocks) + [chain], clocks + [{B: 3}])
    assert got[:-1] == [_want(log, c) for c in clocks]
    assert got[0] == list(range(3, 12)) and got[1] == list(range(3, 10))
    assert got[-1] == [3, 4]
    with pytest.raises(EngineError):
        ds.missing_changes([mover, 9999], [{}, {}])
