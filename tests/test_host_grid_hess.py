"""CPU checks for interpol.grid_hess / grid_pushgrad and the backward of grid_grad: the float64 numpy restatement
(tests/grid_hess_refs.py) against the reference's own results (tests/golden/interpol_grid_hess_*.npz), against central
differences of its own grad, its adjointness, and the argument handling of brainfm_amd.interpol that needs no device."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_npz
import grid_hess_refs as HR
import spline_grid_refs as SR

ORDERS = {"o0": 0, "o1": 1, "o2": 2, "o3": 3, "o312": [3, 1, 2], "o023": [0, 2, 3]}
_BASE = {}


def base():
    if not _BASE:
        _BASE.update(load_npz("interpol_spline_grid.npz"))
    return _BASE


def sin_weights(shape):
    """the weights of the fixture's backward arrays: torch's float32 sine, as make_golden_grid_hess.py takes it"""
    return torch.sin(torch.arange(int(np.prod(shape)), dtype=torch.float32)).double().numpy().reshape(shape)


@pytest.mark.parametrize("otag", list(ORDERS))
def test_restatement_matches_every_array_of_the_fixture(otag):
    """Bar: 1e-6 * max(1, max|ref|): the stored arrays are float64 results of the reference rounded to float32 (2^-24
    relative) and the restatement runs in float64.  grad_pf_dinput is the prefilter's own (tested where the prefilter
    is); it is the one kind of array this test does not restate."""
    b, d = base(), load_npz("interpol_grid_hess_%s.npz" % otag)
    order = ORDERS[otag]
    worst, count = {}, {}
    for k in d:
        if k.endswith(".err") or k.startswith("cot/") or k == "inner/grid":
            continue
        tag, combo, what = k.split("/")
        if what == "grad_pf_dinput":
            continue
        bound, ext = int(combo[1]), int(combo[4])
        if tag == "inner":
            vol, grid = b["A/vol"][:1, :1], d["inner/grid"]
        else:
            vol, grid, cot = b[tag + "/vol"], b[tag + "/grid"], d["cot/" + tag]
        if what == "hess":
            got = HR.hess(vol, grid, order, bound, ext)
        elif what == "pushgrad":
            got = HR.pushgrad(cot, grid, vol.shape[2:], order, bound, ext)
        else:
            w = sin_weights(vol.shape[:2] + grid.shape[1:])
            if what == "grad_dinput":
                got = HR.pushgrad(w, grid, vol.shape[2:], order, bound, ext)
            else:
                assert what == "grad_dgrid", k
                got = HR.contract(HR.hess(vol, grid, order, bound, ext), w)
        assert got.shape == d[k].shape, k
        err = float(np.abs(got - d[k]).max())
        worst[what] = max(worst.get(what, (0.0, 0.0)), (err, float(d[k + ".err"])))
        count[what] = count.get(what, 0) + 1
        assert err <= 1e-6 * max(1.0, float(np.abs(d[k]).max())), (k, err)
    e = 3 if otag == "o1" else 1
    assert count["hess"] == 2 * 7 * e + 14                   # A and T, and the B = C = 1 mask cases on the inner grid
    assert count["pushgrad"] == 2 * 7 * (3 if otag == "o1" else 2)
    assert count["grad_dinput"] == 2 * 2 * (3 if otag == "o1" else 2) and count["grad_dgrid"] == 2 * 2 * e
    print(otag, {w: "max|restatement - ref| %.2e (stored max|ref32 - ref64| %.2e)" % v for w, v in worst.items()})


def test_fixture_files_stay_small_and_the_inner_grid_is_half_masked():
    for t in ORDERS:
        assert os.path.getsize(os.path.join(GOLDEN, "interpol_grid_hess_%s.npz" % t)) < 1 << 20, t
    d = load_npz("interpol_grid_hess_o3.npz")
    ins = base()["A/vol"].shape[2:]
    g = d["inner/grid"]
    assert g.shape == (1, 5, 9, 6, 3) and not SR.near_jumps(g, ins, 1e-3).any()
    inside = SR._mask(g.astype(np.float64).reshape(1, -1, 3), ins, 0).mean()
    assert 0.4 <= inside <= 0.9
    for t in ORDERS:                                         # the same grid and cotangents in every file
        e = load_npz("interpol_grid_hess_%s.npz" % t)
        assert np.array_equal(e["inner/grid"], g) and np.array_equal(e["cot/A"], d["cot/A"])


def central_differences(vol, grid, order, bound, ext, eps=1e-6):
    """J[..., i, j] = d grad_i / d grid_j of the restatement's grad, float64"""
    grid = np.asarray(grid, np.float64)
    cols = []
    for j in range(3):
        step = np.zeros(3)
        step[j] = eps
        cols.append((HR.grad(vol, grid + step, order, bound, ext) - HR.grad(vol, grid - step, order, bound, ext)) / (2 * eps))
    return np.stack(cols, axis=-1)


@pytest.mark.parametrize("bound", [0, 3, 4, 6])
@pytest.mark.parametrize("otag", ["o1", "o2", "o3", "o023"])
def test_hess_is_the_derivative_of_grad(otag, bound):
    """Central differences, eps 1e-6, of the restatement's grad on the A shape, whose coordinates keep 1e-3 from every
    multiple of 0.5 and from the mask thresholds.  Relative 1e-6: truncation (eps^2 times a third derivative) and
    rounding (2^-53 / eps) are about 1e-9 at these magnitudes.  With and without the mask."""
    b = base()
    vol, grid = b["A/vol"], b["A/grid"]
    assert not SR.near_jumps(grid, vol.shape[2:], 1e-3).any()
    for ext in (1, 0):
        h = HR.hess(vol, grid, ORDERS[otag], bound, ext)
        j = central_differences(vol, grid, ORDERS[otag], bound, ext)
        err = float(np.abs(h - j).max())
        assert err <= 1e-6 * max(1.0, float(np.abs(h).max())), (otag, bound, ext, err)
        assert np.array_equal(h, np.swapaxes(h, -1, -2))
    assert float(np.abs(h).max()) > 0.1


@pytest.mark.parametrize("bound", [0, 3])
def test_mixed_orders_with_a_linear_axis_keep_the_reference_s_sign(bound):
    """Orders [3, 1, 2]: the first derivative on the linear axis y is sign(x), the opposite of the true slope, so grad_y is
    minus the true derivative and hess pairs y with x and with z through two such factors.  d grad_y / dx and / dz then
    agree with hess, d grad_x / dy and d grad_z / dy are MINUS the stored entries: the reference's analytic d/dgrid is
    inconsistent there (its goldens pin it, and so does this)."""
    b = base()
    vol, grid = b["A/vol"], b["A/grid"]
    h = HR.hess(vol, grid, [3, 1, 2], bound, 1)
    j = central_differences(vol, grid, [3, 1, 2], bound, 1)
    tol = 1e-6 * max(1.0, float(np.abs(h).max()))
    for i, k in ((0, 1), (2, 1)):
        assert float(np.abs(j[..., i, k] + h[..., i, k]).max()) <= tol            # the opposite sign
        assert float(np.abs(j[..., i, k] - h[..., i, k]).max()) > 0.1             # and not a small thing
    for i, k in ((0, 0), (1, 1), (2, 2), (1, 0), (1, 2), (0, 2), (2, 0)):
        assert float(np.abs(j[..., i, k] - h[..., i, k]).max()) <= tol, (i, k)


@pytest.mark.parametrize("ext", [1, 0])
@pytest.mark.parametrize("bound", [0, 3, 5])
@pytest.mark.parametrize("otag", ["o1", "o2", "o3", "o312", "o023"])
def test_pushgrad_is_the_adjoint_of_grad(otag, bound, ext):
    b, d = base(), load_npz("interpol_grid_hess_o1.npz")
    vol, grid, cot = b["A/vol"], b["A/grid"], d["cot/A"].astype(np.float64)
    lhs = float((HR.pushgrad(cot, grid, vol.shape[2:], ORDERS[otag], bound, ext) * vol).sum())
    rhs = float((cot * HR.grad(vol, grid, ORDERS[otag], bound, ext)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(rhs)), (lhs, rhs)
    if not (ext == 0 and bound == 0):
        assert abs(rhs) > 1e-3


def test_all_nearest_is_zero_and_all_linear_takes_the_true_slope():
    b, d = base(), load_npz("interpol_grid_hess_o1.npz")
    vol, grid, cot = b["A/vol"], b["A/grid"], d["cot/A"]
    assert not HR.hess(vol, grid, 0, 3, 1).any() and HR.hess(vol, grid, 0, 3, 1).shape == (2, 3, 5, 9, 6, 3, 3)
    assert not HR.pushgrad(cot, grid, vol.shape[2:], 0, 3, 1).any()
    h = HR.hess(vol, grid, 1, 3, 1)
    assert not h[..., 0, 0].any() and not h[..., 1, 1].any() and not h[..., 2, 2].any()
    # a linear ramp along x: its gradient is +1 along x inside the volume, and pushgrad of e_x sums to the ramp's adjoint
    ramp = np.broadcast_to(np.arange(7.0)[:, None, None], (1, 1, 7, 6, 8))
    inside = np.full((1, 2, 2, 2, 3), 2.25)
    assert np.allclose(HR.grad(ramp, inside, 1, 3, 1)[..., 0], 1.0)
    assert np.allclose(SR.grad(ramp, inside, 1, 3, 1)[..., 0], -1.0)          # the generic path's sign, not used here


@pytest.mark.parametrize("order,n", [(4, 4), (5, 5), (6, 6), (7, 7), ("fourth", 4), ("seventh", 7), ([3, 5], 5)])
def test_orders_four_to_seven_raise_and_name_the_order(order, n):
    from brainfm_amd import interpol as IP
    vol, grid = torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 2, 2, 2, 3)
    for call in (lambda: IP.grid_hess(vol, grid, order), lambda: IP.grid_pushgrad(torch.zeros(1, 1, 2, 2, 2, 3), grid, None, order)):
        with pytest.raises(NotImplementedError, match=str(n)):
            call()


def test_names_shapes_and_dimensions_raise_as_their_siblings_do():
    from brainfm_amd import interpol as IP
    from brainfm_amd import _lib as L
    vol, grid, vec = torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 2, 2, 2, 3), torch.zeros(1, 1, 2, 2, 2, 3)
    for name in ("quadratic", "cubic", ["linear", "cubic"]):
        with pytest.raises(NotImplementedError, match="integer"):
            IP.grid_hess(vol, grid, name)
        with pytest.raises(NotImplementedError, match="integer"):
            IP.grid_pushgrad(vec, grid, None, name)
    with pytest.raises(ValueError):
        IP.grid_hess(vol, grid, "septic")
    with pytest.raises(ValueError, match="same spatial shape"):
        IP.grid_pushgrad(torch.zeros(1, 1, 2, 3, 2, 3), grid)
    for call in (lambda: IP.grid_hess(vol, torch.zeros(1, 2, 2, 2)), lambda: IP.grid_grad(vol, torch.zeros(1, 2, 2, 2)),
                 lambda: IP.grid_pushgrad(torch.zeros(1, 1, 2, 2, 2), torch.zeros(1, 2, 2, 2))):
        with pytest.raises(NotImplementedError, match="3-D"):
            call()
    # 'nearest' and 'linear' by name are taken; on the CPU the call then stops at the device check, not before
    for call in (lambda: IP.grid_hess(vol, grid, "linear"), lambda: IP.grid_pushgrad(vec, grid, None, "nearest")):
        with pytest.raises(L.BfmError, match="HIP device"):
            call()
