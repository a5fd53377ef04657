"""Writes tests/golden/workspace_sizes.json: what the three operator workspace-size exports return over a table that crosses
every boundary of their rules (TEST INFRASTRUCTURE; needs no device -- these exports only compute; run ONCE, at the commit whose
sizes must be kept: the parent of the change that carves the operators' scratch with Carver):

    python tools/make_golden_workspace_sizes.py [--out tests/golden/workspace_sizes.json]

tests/test_workspace_sizes_host.py compares the built library with the file.  Per export: "args" names the arguments, "product"
lists the values the leading ones take (the table is their cross product, in itertools.product's order; where "pairs" is given,
each product tuple is followed by every one of these tuples of the trailing arguments), "extra" lists further argument tuples
(the degenerate ones that return 256 among them) and "bytes" the results: the product's first, then the extras'.

geoadv_knn_workspace_bytes (b, n, m, k): clouds at the batch limits; n, m either side of the wave (64), the grid search's lower
bound (512), its grid sizes (4096) and the row limit (16384); k either side of every list length (3, 5, 9, 10, 11, 13, 17 slots)
and of the generic kernel (k > 16).
geoadv_group_point_grad_workspace_bytes (b, n, c, m, nsample): n at the pass counts' edges (6 bits per pass), m * nsample either
side of 1024, 2048 (one, two segments) and 65536 (the 64 segment cap).
geoadv_knn_outlier_loss_workspace_bytes (b, n, k): k at its limits (15; 16 is refused), n from k + 2 to the limit 32767, either
side of the search's 16384.
"""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BATCHES = [0, 1, 2, 32, 256, 65535]
POINTS = [1, 2, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 16384]

TABLES = {
    "geoadv_knn_workspace_bytes": dict(
        args=["b", "n", "m", "k"],
        product=[BATCHES, POINTS, POINTS, [1, 2, 4, 8, 9, 16, 17, 20]],
        extra=[[-1, 64, 64, 4], [2, 0, 64, 4], [2, -5, 64, 4], [2, 64, 0, 4], [2, 64, -1, 4], [2, 64, 64, 0], [2, 64, 64, -3], [0, 0, 0, 0]]),
    "geoadv_group_point_grad_workspace_bytes": dict(
        args=["b", "n", "c", "m", "nsample"],
        # m * nsample = 1, 165, 1023, 1024, 1025, 2047, 2048, 2049, 2400, 65535, 65536, 65537
        product=[BATCHES, [0, 1, 63, 64, 4095, 4096], [3]],
        pairs=[[1, 1], [33, 5], [341, 3], [32, 32], [205, 5], [89, 23], [64, 32], [683, 3], [300, 8], [4369, 15], [2048, 32], [65537, 1]],
        extra=[[-1, 64, 3, 33, 5], [2, -1, 3, 33, 5], [2, 64, 3, 0, 5], [2, 64, 3, -2, 5], [2, 64, 3, 33, 0], [2, 64, 3, 33, -1], [2, 64, 0, 33, 5],
               [2, 64, 64, 33, 5], [0, 0, 0, 0, 0]]),
    "geoadv_knn_outlier_loss_workspace_bytes": dict(
        args=["b", "n", "k"],
        product=None,                                          # n depends on k: every tuple is listed
        extra=[[b, n, k] for b in BATCHES for k in (1, 5, 15, 16) for n in (k + 2, 300, 16384, 16385, 32767)]
        + [[-1, 300, 5], [65536, 300, 5], [2, 300, 0], [2, 300, -1], [2, 6, 5], [2, 16, 15], [2, 32768, 5], [2, 0, 1]]),
}


def cases(table):
    """-> the argument tuples of one table, in the order of its "bytes"."""
    out = []
    if table.get("product"):
        for head in itertools.product(*table["product"]):
            out += [list(head) + list(p) for p in table.get("pairs", [[]])]
    return out + [list(e) for e in table["extra"]]


def main():
    from geometric_adv_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "workspace_sizes.json"))
    a = ap.parse_args()
    lib = _lib.lib()
    doc = {}
    for name, table in TABLES.items():
        got = [int(getattr(lib, name)(*args)) for args in cases(table)]
        assert min(got) == 256 and max(got) > 256, name
        doc[name] = dict(table, bytes=got)
        print("%s: %d cases, %d of them 256 bytes, largest %d" % (name, len(got), got.count(256), max(got)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
