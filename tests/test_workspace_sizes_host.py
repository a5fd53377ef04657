"""CPU: the operators' workspace sizes (geoadv_knn_workspace_bytes, geoadv_group_point_grad_workspace_bytes,
geoadv_knn_outlier_loss_workspace_bytes) are byte for byte those recorded in tests/golden/workspace_sizes.json, over a table that
crosses every boundary of their rules and the degenerate arguments that return 256 (tools/make_golden_workspace_sizes.py wrote the
file at the commit before the scratch layouts were carved with Carver) -- no device is touched: these exports only compute."""
import ctypes
import itertools
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("geoadv_knn_workspace_bytes", "geoadv_group_point_grad_workspace_bytes", "geoadv_knn_outlier_loss_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  -- before the library, so that both bind to one HIP runtime if GPU tests share the process
    from geometric_adv_amd import _lib
    import __graft_entry__
    if not os.path.exists(_lib.LIB_PATH):
        __graft_entry__.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in EXPORTS:
        getattr(so, name).restype = ctypes.c_size_t
    return so


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")) as f:
        return json.load(f)


def _cases(table):
    out = []
    if table.get("product"):
        for head in itertools.product(*table["product"]):
            out += [list(head) + list(p) for p in table.get("pairs", [[]])]
    return out + table["extra"]


@pytest.mark.parametrize("name", EXPORTS)
def test_sizes_are_the_recorded_ones(lib, golden, name):
    table = golden[name]
    cases = _cases(table)
    assert len(cases) == len(table["bytes"]) and len(cases) >= 100
    assert 256 in table["bytes"] and max(table["bytes"]) > 1 << 32
    fn = getattr(lib, name)
    wrong = [(args, want, got) for args, want in zip(cases, table["bytes"]) for got in [int(fn(*[ctypes.c_int(v) for v in args]))] if got != want]
    assert not wrong, "%s: %d of %d sizes differ, the first (%s) = %s: recorded %d, now %d" % (
        name, len(wrong), len(cases), ", ".join(table["args"]), wrong[0][0], wrong[0][1], wrong[0][2])


def test_the_table_holds_what_it_is_there_for(golden):
    """The rule boundaries and the degenerate arguments are in the file."""
    knn = {tuple(a) for a in _cases(golden["geoadv_knn_workspace_bytes"])}
    for b in (0, 1, 2, 32, 256, 65535):
        for n in (1, 2, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 16384):
            for k in (1, 2, 4, 8, 9, 16, 17, 20):
                assert (b, n, 513, k) in knn and (b, 64, n, k) in knn
    gpg = _cases(golden["geoadv_group_point_grad_workspace_bytes"])
    assert {a[1] for a in gpg} >= {0, 1, 63, 64, 4095, 4096}
    assert {a[3] * a[4] for a in gpg} >= {1023, 1024, 1025, 2047, 2048, 2049, 65535, 65536, 65537}
    loss = _cases(golden["geoadv_knn_outlier_loss_workspace_bytes"])
    for k in (1, 5, 15, 16):
        for n in (k + 2, 300, 16384, 16385, 32767):
            assert [2, n, k] in loss and [65535, n, k] in loss
