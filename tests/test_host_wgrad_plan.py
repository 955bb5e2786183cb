"""The route plan of the weight gradient (bfm_conv3x3x3_wgrad_plan, brainfm_amd/csrc/backward.hip) without a GPU: the plan
is host arithmetic on the layer alone, and the library loads on a machine without a device.  The routes the cases of
tests/wgrad_cases.py have to take, the invariants of the one split rule, the regions of the partials in the workspace, and
the workspace bound: every plan's exact total stays under it, and it still has the values of tests/golden/wgrad_plan.json
(made by tests/golden/make_golden_wgrad_plan.py before the bound was written in the plan's terms)."""
import itertools
import json
import os

import pytest

from conftest import GOLDEN
import wgrad_cases as WC

BUDGET = 512                            # workgroups of a tiled launch, over all workgroup columns
ROW_BLOCKS = 2048                       # blocks the column kernel's row split aims at


def _lib():
    from brainfm_amd import _lib as L
    return L.load()


def _cdiv(a, b):
    return -(-a // b)


def _expected_launches(case, passes, route):
    """[(tile extents or None for rows, workgroup columns, bytes of one split)] of a route, from the kernels' tiles: fp32
    4 x 4 x 16 and f16 2 x 4 x 16 voxels over 32 ci x 64 co, wave-specialised and upsampled 1 x 4 x 16 over 32 x 32."""
    ca, cb, cout, dims, lo, _ = case
    cin = ca + cb
    row = cout * 27 * 4
    ws = ((1, 4, 16), dims, (ca // 32) * (cout // 32), row * ca)
    f16_skip = ((2, 4, 16), dims, (ca // 32) * (cout // 64), row * ca)
    up = ((1, 4, 16), lo, (cb // 32) * (cout // 32), cout * cb * 64 * 4)
    return {"ws": [ws], "fold+ws": [ws, up], "fold+f16": [f16_skip, up],
            "f16": [((2, 4, 16), dims, (cin // 32) * (cout // 64), row * cin)],
            "fp32": [((4, 4, 16), dims, (cin // 32) * (cout // 64), row * cin)],
            "cols": [(None, dims, _cdiv(cout, 32) * _cdiv(cin * 27, 32), row * cin)]}[route]


def _check_plan(case, passes, allow, plan, total, bound):
    """The invariants of one plan; returns its route."""
    route = WC.route_name(plan)
    launches = WC.launches(plan)
    want = _expected_launches(case, passes, route)
    assert len(launches) == len(want), (case, passes, allow, route)
    end = 0
    for i, (l, (tile, ext, cols, split_bytes)) in enumerate(zip(launches, want)):
        ctx = (case, passes, allow, route, i, l)
        if tile is None:
            assert (l["nbz"], l["nby"], l["nbx"], l["ntiles"]) == (0, 0, 0, ext[0] * ext[1]), ctx
            cap = max(1, _cdiv(ROW_BLOCKS, cols))
        else:
            grid = tuple(_cdiv(e, t) for e, t in zip(ext, tile))
            assert (l["nbz"], l["nby"], l["nbx"], l["ntiles"]) == grid + (grid[0] * grid[1] * grid[2],), ctx
            cap = max(1, BUDGET // cols)
        assert l["cols"] == cols, ctx
        S, per, n = l["S"], l["per"], l["ntiles"]
        assert S >= 1 and S * per >= n, ctx
        assert (S - 1) * per < n, ctx                      # no workgroup is empty
        assert S <= cap, ctx
        assert per == _cdiv(n, min(n, cap)) and S == _cdiv(n, per), ctx      # the one rule
        assert l["bytes"] == S * split_bytes, ctx
        assert l["off"] >= end and l["off"] % 256 == 0, ctx                  # regions do not overlap
        end = l["off"] + l["bytes"]
    assert launches[0]["off"] == 0
    if len(launches) == 1:
        assert plan[11:] == [0] * 9, (case, passes, allow, plan)
    assert total == end, (case, passes, allow, total, end)
    assert total <= bound, (case, passes, allow, total, bound)
    return route


@pytest.mark.parametrize("allow", range(4))
@pytest.mark.parametrize("case", WC.ALL, ids=WC.ids(WC.ALL))
def test_every_case_takes_the_route_written_next_to_it(case, allow):
    """What the docstrings of tests/test_gpu_backward.py say about kernels, as assertions: at passes = 3 the route of
    wgrad_cases.ROUTES for every `allow`; at passes = 0 the fp32 tiles where the widths allow tiles, else the columns."""
    lib = _lib()
    ca, cb, cout, dims, _, _ = case
    bound = lib.bfm_conv3x3x3_wgrad_workspace(ca + cb, cout, *dims)
    plan, total = WC.plan(lib, case, 3, allow)
    assert _check_plan(case, 3, allow, plan, total, bound) == WC.ROUTES[case][allow]
    plan, total = WC.plan(lib, case, 0, allow)
    want = "cols" if WC.ROUTES[case][0] == "cols" else "fp32"
    assert _check_plan(case, 0, allow, plan, total, bound) == want


def test_the_uneven_cases_split_unevenly():
    """The two cases with 1 < S < tiles: 54 tiles over 8 workgroups of 7 (the last takes 5); 96 skip tiles over 8 of 12
    and 12 low-res tiles over 6 of 2."""
    lib = _lib()
    a, = WC.launches(WC.plan(lib, WC.as_join(WC.PLAIN[8]), 3, 3)[0])
    assert (a["ntiles"], a["cols"], a["S"], a["per"]) == (54, 64, 8, 7)
    a, u = WC.launches(WC.plan(lib, WC.FOLD_JOIN_UNEVEN, 3, 3)[0])
    assert (a["ntiles"], a["cols"], a["S"], a["per"]) == (96, 64, 8, 12)
    assert (u["ntiles"], u["cols"], u["S"], u["per"]) == (12, 64, 6, 2)


def test_every_case_of_the_bits_runs_has_a_route():
    assert set(WC.ROUTES) == set(WC.ALL)
    for env, allow, cases in WC.BITS_RUNS.values():
        assert 0 <= allow <= 3 and all(c in WC.ROUTES and p in (0, 3) for c, p in cases)


def test_split_invariants_and_exact_total_under_the_bound_over_the_grid():
    """Every Cout x (CA, CB) x extent x low-res extent x passes x allow of the grid: the split invariants, the regions, and
    exact total <= bfm_conv3x3x3_wgrad_workspace(CA + CB, Cout, D, H, W) -- the check the hand-derived bound never had.
    Every route has to occur, and a folded join with each skip kernel."""
    lib = _lib()
    seen = set()
    for cout, (ca, cb), dims in itertools.product(WC.GRID_COUT, WC.GRID_CHANNELS, WC.GRID_DIMS):
        bound = lib.bfm_conv3x3x3_wgrad_workspace(ca + cb, cout, *dims)
        for lo in (WC.grid_lows(dims) if cb else [None]):
            case = (ca, cb, cout, dims, lo, 1)
            for passes, allow in itertools.product((0, 3), range(4)):
                plan, total = WC.plan(lib, case, passes, allow)
                seen.add(_check_plan(case, passes, allow, plan, total, bound))
    assert seen == {"ws", "fold+ws", "fold+f16", "f16", "fp32", "cols"}


def test_the_workspace_bound_has_the_values_it_had():
    """bfm_conv3x3x3_wgrad_workspace over the grid == tests/golden/wgrad_plan.json: shrinking the bound changes memory
    behaviour and is not what writing it in the plan's terms is for."""
    lib = _lib()
    with open(os.path.join(GOLDEN, "wgrad_plan.json")) as f:
        d = json.load(f)
    assert d["cin"] == sorted({ca + cb for ca, cb in WC.GRID_CHANNELS})
    assert d["cout"] == list(WC.GRID_COUT) and d["dims"] == [list(v) for v in WC.GRID_DIMS]
    for (i, cin), (j, cout), (k, dims) in itertools.product(enumerate(d["cin"]), enumerate(d["cout"]), enumerate(d["dims"])):
        assert lib.bfm_conv3x3x3_wgrad_workspace(cin, cout, *dims) == d["bytes"][i][j][k], (cin, cout, dims)


def test_plan_rejects_bad_arguments():
    import ctypes as C
    lib = _lib()
    arr, total = (C.c_int64 * WC.PLAN_LEN)(), C.c_size_t(0)
    for args in ((0, 0, 64, 4, 4, 4, 0, 0, 0, 3, 3), (32, -1, 64, 4, 4, 4, 0, 0, 0, 3, 3), (32, 0, 64, 4, 4, 4, 0, 0, 0, 1, 3),
                 (32, 0, 0, 4, 4, 4, 0, 0, 0, 3, 3), (32, 0, 64, 4, 0, 4, 0, 0, 0, 3, 3)):
        assert lib.bfm_conv3x3x3_wgrad_plan(*args, arr, C.byref(total)) == -1, args
    assert lib.bfm_conv3x3x3_wgrad_plan(32, 0, 64, 4, 4, 4, 0, 0, 0, 3, 3, None, C.byref(total)) == -1
    assert lib.bfm_conv3x3x3_wgrad_plan(32, 0, 64, 4, 4, 4, 0, 0, 0, 3, 3, arr, None) == 0
