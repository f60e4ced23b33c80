"""The state part of the C-ABI (no compute: there may be no GPU here): the row and summary layouts,
the library exports the new entry points, and NULL arguments are refused before anything runs."""
import ctypes
import os
import re

from hypermerge_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("hm_store_state_sizes", "hm_store_state", "hm_state_work_bytes", "hm_state_device", "hm_state_host",
         "hm_docset_views", "hm_docset_get_patch")
INVALID = 32


def test_row_and_summary_layouts():
    assert engine.STATE_ROW_DT.itemsize == 20                     # sizeof(hm_state_row): five 32-bit words
    assert [engine.STATE_ROW_DT.fields[f][1] for f in ("reg", "obj", "index", "n_surv", "surv_off")] == [0, 4, 8, 12, 16]
    assert engine.STATE_ROW_DT.fields["index"][0].kind == "i"
    assert ctypes.sizeof(engine.CStateSummary) == 64              # sizeof(hm_state_summary)
    S = engine.CStateSummary
    assert (S.totals.offset, S.max_rows.offset, S.max_surv.offset, S.flags.offset, S.bad.offset) == (0, 32, 48, 52, 56)
    assert ctypes.sizeof(engine.CStateOut) == 8 + 4 * 8
    assert engine.ST_BAD_ROWS == 1
    # the header says the same
    h = open(os.path.join(ROOT, "include", "hypermerge_amd.h")).read()
    assert re.search(r"#define HM_ST_BAD_ROWS 1u", h) and re.search(r"#define HM_ABI_VERSION 4u\b", h)
    body = re.search(r"typedef struct \{([^}]*)\} hm_state_row;", h).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == ["reg", "obj", "index", "n_surv", "surv_off"]


def test_library_exports_the_state_calls():
    L = engine.lib()
    for name in CALLS:
        assert name in engine.EXPORTS and hasattr(L, name), name
    assert L.hm_abi_version() == 4
    assert L.hm_state_work_bytes(0) == 0
    # [counts 4n][offsets 4n][flags 2n] u32 rounded to 256 bytes, then a scan chunk's ten 64-bit words per 4096 requests
    assert L.hm_state_work_bytes(1) == 256 + 80
    assert L.hm_state_work_bytes(4097) == ((4097 * 40 + 255) & ~255) + 2 * 80


def test_null_arguments_are_invalid():
    L = engine.lib()
    out = engine.CStateOut()
    t = ctypes.c_void_p()
    assert L.hm_store_state_sizes(None, 0, None, None, None, None) == INVALID
    assert L.hm_store_state(None, 0, None, ctypes.byref(out), None, None, None) == INVALID
    assert L.hm_state_device(None, None, None, 0, None, ctypes.byref(out), None, None, None, None, None) == INVALID
    assert L.hm_state_host(None, None, None, 0, None, ctypes.byref(out), None, None, None) == INVALID
    assert L.hm_docset_views(None, 0, None, ctypes.byref(t)) == INVALID
    assert L.hm_docset_get_patch(None, 0, None, ctypes.byref(t)) == INVALID
