"""bfm_conv3x3x3_wgrad_ex gives the bits stored in tests/golden/wgrad_bits.json (made by
tests/golden/make_golden_wgrad_bits.py from the library as it stood before the route plan, when the launcher chose its
kernels through nested flags), on every route a process can be put on, and reports the route that
tests/wgrad_cases.py expects.  Digest and value equality: no tolerance.  BFM_WGRAD_WS and BFM_WGRAD_UPFOLD are read once
per process, so every setting runs in a fresh child (tests/wgrad_bits_worker.py).  Needs an MI355X: run with `-m gpu`."""
import json
import os

import pytest

from conftest import GOLDEN
import wgrad_bits_worker as WW
import wgrad_cases as WC

pytestmark = pytest.mark.gpu


def test_wgrad_keeps_its_bits_and_takes_the_expected_route_in_every_environment():
    """Default environment: every case at passes = 3 and the four passes = 0 cases; BFM_WGRAD_WS=0: the wide plain layers
    and both foldable joins (f16 tiles with part_cin = CA under the fold); BFM_WGRAD_UPFOLD=0: both foldable joins on f16
    tiles.  The children run one after the other, 120 s each at the most; one that ends on a signal, a non-zero status or
    the time limit fails the test there, and the children after it are not started."""
    with open(os.path.join(GOLDEN, "wgrad_bits.json")) as f:
        golden = json.load(f)
    assert set(golden) == set(WC.BITS_RUNS)
    from brainfm_amd import _lib as L
    has_plan = "bfm_conv3x3x3_wgrad_plan" in L.SIGNATURES   # False only on the golden file's own build, which has no plan
    for run, (_, allow, cases) in WC.BITS_RUNS.items():
        got = WW.spawn(run)
        assert set(got) == set(golden[run]), run
        for case, passes in cases:
            k = WW.case_id(case, passes)
            assert got[k]["sha"] == golden[run][k]["sha"] and got[k]["head"] == golden[run][k]["head"], (run, k)
            assert (got[k]["plan"] is not None) == has_plan, (run, k)
            if has_plan:
                want = WC.ROUTES[case][allow] if passes == 3 else "fp32"
                assert WC.route_name(got[k]["plan"]) == want, (run, k, got[k]["plan"])
