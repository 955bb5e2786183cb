"""CPU checks for the spline orders 0 to 3 of interpol.grid_pull / push / count / grad: the float64 numpy restatement
(tests/spline_grid_refs.py) against the reference's own results (tests/golden/interpol_spline_grid*.npz), the conditions
the fixture must meet, and the option parsing of brainfm_amd.interpol."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_npz
import spline_grid_refs as SR

ORDERS = {"o0": 0, "o2": 2, "o3": 3, "o312": [3, 1, 2], "o023": [0, 2, 3]}
FILES = ["interpol_spline_grid.npz"] + ["interpol_spline_grid_%s.npz" % t for t in ORDERS]


@pytest.mark.parametrize("otag", list(ORDERS))
def test_restatement_matches_every_pull_push_grad_array_of_the_fixture(otag):
    """Bar: max(1e-6, 4 x the stored max|ref32 - ref64| of the reference's own float32 run); the restatement runs in
    float64 and the stored arrays are float64 results rounded to float32 (2^-24 relative)."""
    base, d = load_npz("interpol_spline_grid.npz"), load_npz("interpol_spline_grid_%s.npz" % otag)
    order = ORDERS[otag]
    worst = {}
    n = 0
    for k in d:
        tag, combo, what = k.split("/")
        if what not in ("pull", "push", "grad"):
            continue
        bound, ext = int(combo[1]), int(combo[4])
        vol, grid, src = base[tag + "/vol"], base[tag + "/grid"], base[tag + "/src"]
        if what == "pull":
            got = SR.pull(vol, grid, order, bound, ext)
        elif what == "push":
            got = SR.push(src, grid, vol.shape[2:], order, bound, ext)
        else:
            got = SR.grad(vol, grid, order, bound, ext)
        assert got.shape == d[k].shape, k
        err = float(np.abs(got - d[k]).max())
        stored = float(d[k + ".err"])
        worst[what] = max(worst.get(what, (0.0, 0.0)), (err, stored))
        assert err <= max(1e-6, 4 * stored), (k, err, stored)
        n += 1
    assert n == 2 * 15 * 3                                   # both shapes, 7 bounds x 2 + 'hist', three outputs
    print(otag, {w: "max|restatement - ref| %.2e (stored max|ref32 - ref64| %.2e)" % v for w, v in worst.items()})


def test_fixture_coordinates_keep_their_margin_and_files_stay_small():
    base = load_npz("interpol_spline_grid.npz")
    for tag in ("A", "T"):
        assert not SR.near_jumps(base[tag + "/grid"], base[tag + "/vol"].shape[2:], 1e-3).any()
        g, shape = base[tag + "/grid"], base[tag + "/vol"].shape[2:]
        for a in range(3):                                   # spills over every face
            assert g[..., a].min() < -1.5 and g[..., a].max() > shape[a] - 1 + 1.5
    assert base["A/vol"].shape == (2, 3, 7, 6, 8) and base["A/grid"].shape == (2, 5, 9, 6, 3)
    assert base["A/src"].shape == (2, 3, 5, 9, 6)
    assert base["T/vol"].shape[2:] == (1, 2, 5) and base["T/grid"].shape[1:] == (3, 4, 5, 3)
    for f in FILES:                                          # one file per order: each below what a committed file may have
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 1 << 20, f


def test_interpolation_orders_by_name_per_axis_and_padded():
    from brainfm_amd import interpol as IP
    assert IP._order_list("nearest") == (0, 0, 0) and IP._order_list("linear") == (1, 1, 1)
    assert IP._order_list("quadratic") == (2, 2, 2) and IP._order_list("Cubic") == (3, 3, 3)
    assert IP._order_list(2) == (2, 2, 2) and IP._order_list([3, 1, 2]) == (3, 1, 2)
    assert IP._order_list([0, 2]) == (0, 2, 2) and IP._order_list(("cubic", "nearest")) == (3, 0, 0)   # pad_list_int
    b, o, ext = IP._opts([2, 3], ["zero", "dft"], "hist")
    assert list(b) == [0, 6, 6] and o == (2, 3, 3) and ext == 2
    # pull / push / count / grad: 'nearest' and 'linear' by name, orders 2 and 3 as integers only (their names keep
    # raising there, as test_gpu_synth.py::test_grid_pull_all_bounds pins); spline_coeff_nd and resize take every name
    assert IP._opts(["nearest", "linear", 3], 0, 1)[1] == (0, 1, 3)
    for name in ("quadratic", "cubic", ["linear", "cubic"]):
        with pytest.raises(NotImplementedError, match="integer"):
            IP._opts(name, 0, 1)
    with pytest.raises(ValueError):
        IP._order_list("septic")
    with pytest.raises(ValueError):
        IP._order_list(8)


@pytest.mark.parametrize("order,n", [(4, 4), (5, 5), (6, 6), (7, 7), ("fourth", 4), ("seventh", 7), ([3, 5], 5)])
def test_orders_four_to_seven_raise_and_name_the_order(order, n):
    from brainfm_amd import interpol as IP
    vol, grid = torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 2, 2, 2, 3)
    calls = [lambda: IP.grid_pull(vol, grid, order), lambda: IP.grid_push(vol[..., :2, :2, :2], grid, None, order),
             lambda: IP.grid_count(grid, [4, 4, 4], order), lambda: IP.grid_grad(vol, grid, order),
             lambda: IP.spline_coeff_nd(vol, order), lambda: IP.resize(vol, shape=[5, 5, 5], interpolation=order)]
    for call in calls:
        with pytest.raises(NotImplementedError, match=str(n)):
            call()


@pytest.mark.parametrize("bound", ["dst1", "dst2", 4, 5, "antimirror", ["dct2", "dst2"]])
def test_prefilter_has_no_dst_conditions(bound):
    from brainfm_amd import interpol as IP
    vol, grid = torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 2, 2, 2, 3)
    for order in (2, 3):
        with pytest.raises(NotImplementedError):
            IP.spline_coeff_nd(vol, order, bound)
        with pytest.raises(NotImplementedError):
            IP.grid_pull(vol, grid, order, bound, prefilter=True)


def test_prefilter_scalars_per_order_and_family():
    """coeff.py:35-57 (poles), :72 / :99 (max_iter) and the closed forms of the three families."""
    from brainfm_amd import interpol as IP
    z2, z3 = 8 ** 0.5 - 3, 3 ** 0.5 - 2
    for order, z, it in ((2, z2, 18), (3, z3, 23)):
        for fam in (0, 1, 2):
            sc = IP._prefilter_scalars(9, order, fam)
            assert sc[0] == z and sc[6] == it and abs(sc[1] - (1 - z) * (1 - 1 / z)) < 1e-15
        assert abs(IP._prefilter_scalars(9, order, 1)[4] - z / (z * z - 1)) < 1e-15
        assert abs(IP._prefilter_scalars(9, order, 2)[3] - 1 / (1 - z ** 9)) < 1e-15
        assert abs(IP._prefilter_scalars(40, order, 2)[3] - 1 / (1 - z ** it)) < 1e-15
    assert len(IP._prefilter_scalars(9, 3, 0)[5]) == 7       # the DCT-II table z^i + z^(2n-1-i), i = 1..n-2
