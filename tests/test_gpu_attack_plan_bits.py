"""The attack loop keeps its bits and its launch decisions now that the symmetric scan's launch is planned before it is launched:
every case of tools/make_golden_attack_plan.py -- one per branch of the forward -- is rebuilt from the same seeds and compared
with tests/golden/attack_plan_parent.npz, which that tool wrote on an MI355X at the commit before the change: the nine plan
entries and the search state after every forward, and pert / adv / recon / latent / grad / the four index arrays / the history
rows after three iterations -- raw arrays where a case is small, SHA-256 of the bytes otherwise.  compute() itself asserts the
form each case exists for.  A case that is missing from the fixture fails."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_attack_plan as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "attack_plan_parent.npz"))


def test_every_case_is_in_the_fixture(golden):
    cases = {k.split("/")[0] for k in golden.files}
    assert cases == set(G.CASES)


@pytest.mark.parametrize("case", list(G.CASES))
def test_same_plan_and_bits_as_parent(golden, case):
    got = G.compute(case)
    keys = [k for k in golden.files if k.startswith(case + "/")]
    assert keys, "%s is not in the fixture" % case
    assert {k.split("/")[1].replace(".sha256", "") for k in keys} == set(got)
    for k in sorted(keys, key=lambda k: k.split("/")[1] not in ("plan", "search")):      # the read-outs first: they explain the rest
        name = k.split("/")[1]
        if name.endswith(".sha256"):
            a = got[name[:-len(".sha256")]]
            assert G.sha256(a) == str(golden[k]), "%s differs from the parent's bytes" % k
        else:
            a, want = got[name], golden[k]
            assert a.dtype == want.dtype and a.shape == want.shape, k
            same = a.view(np.uint32) == want.view(np.uint32)
            assert same.all(), "%s: %d of %d words differ from the parent, first at %s (got %s, parent %s)" % (
                k, same.size - int(same.sum()), same.size, np.argwhere(~same)[0].tolist(), a[~same][:4].tolist(), want[~same][:4].tolist())
