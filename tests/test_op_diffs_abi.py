"""The op-diff part of the C-ABI (no compute: there may be no GPU here): the row and summary
layouts, and the library exports the new entry points."""
import ctypes

from hypermerge_amd import engine


def test_row_and_summary_layouts():
    assert engine.OP_DIFF_DT.itemsize == 16                       # sizeof(hm_op_diff)
    assert [engine.OP_DIFF_DT.fields[f][1] for f in ("op", "kind", "n_surv", "surv_off")] == [0, 4, 8, 12]
    assert ctypes.sizeof(engine.COpDiffSummary) == 64
    assert engine.COpDiffSummary.flags.offset == 52 and engine.COpDiffSummary.bad.offset == 56
    assert ctypes.sizeof(engine.COpDiffOut) == 8 + 4 * 8


def test_library_exports_the_op_diff_calls():
    L = engine.lib()
    for name in ("hm_store_op_diff_sizes", "hm_store_op_diffs", "hm_op_diffs_work_bytes", "hm_op_diffs_device", "hm_op_diffs_host"):
        assert name in engine.EXPORTS and hasattr(L, name), name
    assert L.hm_op_diffs_work_bytes(None, 0) == 0
    assert L.hm_abi_version() == 4
