"""The f16x2 encoder forward keeps the bits it had before its epilogue was shortened (second fp16 piece by a mixed-precision FMA,
ring addresses on the scalar unit): every case of tools/make_golden_encoder_epilogue.py -- latent, adversarial cloud, gradient and
perturbation after three attack steps, in every form of the forward, with the masked and the recomputing backward -- is rebuilt
from the same seeds and compared with tests/golden/encoder_epilogue_parent.npz, which that tool wrote on an MI355X at the commit
before the change: raw arrays where a case is small, SHA-256 of the bytes otherwise.  A case that is missing from the fixture
fails."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_encoder_epilogue as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "encoder_epilogue_parent.npz"))


def test_every_case_is_in_the_fixture(golden):
    assert {k.split("/")[0] for k in golden.files} == set(G.CASES)
    assert {(n, b) for n, b in G.SHAPES} >= {(2048, 2), (2048, 8), (2048, 9), (160, 3)}


@pytest.mark.parametrize("case", G.CASES)
def test_same_bits_as_parent(golden, case):
    got = G.compute(case)
    keys = [k for k in golden.files if k.startswith(case + "/")]
    assert keys, "%s is not in the fixture" % case
    assert {k.split("/")[1].replace(".sha256", "") for k in keys} == set(got) == set(G.ARRAYS)
    for k in keys:
        name = k.split("/")[1]
        if name.endswith(".sha256"):
            a = got[name[:-len(".sha256")]]
            assert G.sha256(a) == str(golden[k]), "%s differs from the parent's bytes" % k
        else:
            a, want = got[name], golden[k]
            assert a.dtype == want.dtype and a.shape == want.shape, k
            same = a.view(np.uint32) == want.view(np.uint32)
            assert same.all(), "%s: %d of %d words differ from the parent, first at %s" % (
                k, same.size - int(same.sum()), same.size, np.argwhere(~same)[0].tolist())
