"""The hand-built documents of tests/small_diet_docs.py against the oracle alone (no GPU): the ones
meant to merge do (status 0), the others throw what they were built to throw, and each group has
the shape it was built for (register / object / op / dep-row counts at the size classes' bounds)."""
import numpy as np

import oracle.oracle as O
from hypermerge_amd.columnar import encode
from small_diet_docs import groups


def test_statuses_and_shapes():
    seen = {}
    for gname, g in groups().items():
        b = encode([d for _, d, _ in g["docs"]], 8)
        o = O.merge(b, threads=2)
        for i, (name, _, status) in enumerate(g["docs"]):
            assert int(o.docs["status"][i]) == status, (gname, name, int(o.docs["status"][i]))
            seen[name] = b.docs[i]
        assert int(b.docs["n_actors"].max()) <= min(g["strides"]), gname
    for r in (0, 1, 31, 32, 33, 64, 65, 128, 129):
        assert int(seen[f"regs{r}"]["n_regs"]) == r
    for n, f, v in (("objs1", "n_objs", 1), ("objs2", "n_objs", 2), ("objs16", "n_objs", 16), ("ops64", "n_ops", 64),
                    ("ops65", "n_ops", 65), ("ops128", "n_ops", 128), ("deps0", "n_deps", 0), ("deps64", "n_deps", 64),
                    ("deps65", "n_deps", 65), ("deps128", "n_deps", 128)):
        assert int(seen[n][f]) == v, (n, f, int(seen[n][f]))
    # class 0 holds 32 registers, 16 objects, 128 dep rows and (two op rows per lane) 128 ops
    for gname in ("class0_4actors", "class0_8actors", "nolist", "counter"):
        b = encode([d for _, d, _ in groups()[gname]["docs"]], 8)
        assert int(b.docs["n_regs"].max()) <= 32 and int(b.docs["n_objs"].max()) <= 16, gname
        assert int(b.docs["n_deps"].max()) <= 128 and int(b.docs["n_ops"].max()) <= 128 and int(b.docs["n_changes"].max()) <= 64, gname


def test_fold_documents_differ_where_built_to():
    """The literal transitiveDeps fold against the closure: all_deps of the author's change knows the
    later change of the lowered actor only in the closure."""
    g = {n: d for n, d, _ in groups()["class0_8actors"]["docs"]}
    for name, lowered in (("fold_equal2", False), ("fold_differ2", True), ("fold_differ5", True), ("fold_top_equal", False),
                          ("fold_top_differ", True), ("fold_mid_differ", True)):
        b = encode([g[name]], 8)
        o = O.merge(b, threads=1)
        z = len(g[name]) - 1                                    # the author's change arrives last
        row = o.all_deps[z * 8: z * 8 + 8]
        clock = o.clock[:8]
        assert np.all(row <= clock)
        f = int(b.docs["n_actors"][0]) - 1                      # the foreign actors (the author `z` ranks last)
        assert bool(np.any(row[:f] < clock[:f])) == lowered, (name, row, clock)
