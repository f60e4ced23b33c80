"""The ABI of the one-walk op-diff call and of the docset's device-diffs route: the values of the
new option bit and creation flag in the public header and in the Python face, the new export, and
the ABI version, which they leave alone."""
import os
import re

from hypermerge_amd import docset, engine

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hypermerge_amd.h")


def defines():
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (HM_\w+) (\d+)u\b", open(HEADER).read())}


def test_the_flags_values():
    d = defines()
    assert d["HM_ODF_LISTS"] == 1 and d["HM_ODF_ONCE"] == 2
    assert (d["HM_DOCSET_NO_PATCHES"], d["HM_DOCSET_BINARY"], d["HM_DOCSET_NET_DIFFS"], d["HM_DOCSET_DEVICE_DIFFS"]) == (1, 2, 4, 8)
    assert engine.ODF_ONCE == d["HM_ODF_ONCE"] and engine.ODF_LISTS == d["HM_ODF_LISTS"]
    assert docset.DEVICE_DIFFS == d["HM_DOCSET_DEVICE_DIFFS"]


def test_the_new_export_and_the_abi_version():
    assert "hm_docset_diff_stats" in engine.EXPORTS
    L = engine.lib()
    assert hasattr(L, "hm_docset_diff_stats")
    assert L.hm_abi_version() == 4
    assert re.search(r"int hm_docset_diff_stats\(const hm_docset \*ds, uint64_t \*out4\);", open(HEADER).read())
