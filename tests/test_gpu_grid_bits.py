"""The interpol grid kernels give the bits stored in tests/golden/grid_family_bits.npz (made by
tests/golden/make_golden_grid_bits.py from the kernels as they stood before spline_grid.hip, grid_hess.hip,
label_pull.hip and restrict.hip got their shared node and voxel layer).  torch.equal throughout: no tolerance.  The cases
and the calls are those of tests/grid_bits_cases.py."""
import numpy as np
import pytest
import torch

from conftest import load_npz
import grid_bits_cases as GB

pytestmark = pytest.mark.gpu

_D, _N = {}, {}


def golden():
    if not _D:
        _D.update(load_npz("grid_family_bits.npz"))
    return _D


def golden_nd():
    """grid_nd_bits.npz: what the 2-D kernels and the all-linear 3-D ones gave on the inputs of grid_family_bits.npz before
    both became one dimension-generic set"""
    if not _N:
        _N.update(load_npz("grid_nd_bits.npz"))
    return _N


def same(got, want, what):
    got, want = torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(np.ascontiguousarray(want))
    if not torch.equal(got, want):                       # sized for the report; any difference fails
        diff = (got.double() - want.double()).abs()
        pytest.fail("%s: %d of %d elements differ, max|got - stored| %.3e" % (what, int((got != want).sum()), got.numel(),
                                                                               float(diff.max())))


@pytest.mark.parametrize("order", GB.ORDERS, ids=GB.otag)
def test_pull_grad_hess_and_label_pull_keep_their_bits(order):
    """Volume (2,2,5,6,7), grid (2,3,2,5,3) over [-3, n+2] with floor ties and weight branch points planted, every bound,
    mixed bounds, extrapolate 0 / 1 / 2, both batch broadcasts; four label dtypes under AUTO and each forced variant."""
    from brainfm_amd import interpol as IP
    d = golden()
    names = list(d["cases"])
    n = 0
    for case in GB.det_cases():
        if case[1] != order:
            continue
        i = names.index(case[0])
        got = GB.run_det_case(IP, torch, d, case)
        for k, v in got.items():
            same(v, d[k][i], "%s %s" % (case[0], k))
        n += 1
    assert n >= len(GB.CONFIGS)


def test_axis_tables_keep_their_bits():
    from brainfm_amd import interpol as IP
    d = golden()
    names = list(d["table/names"])
    for case in GB.table_cases():
        i = names.index(case[0])
        rowptr, col, val = GB.run_table_case(IP, torch, d, case)
        same(rowptr, d["table/rowptr"][i], case[0] + " rowptr")
        same(col, d["table/col"][i], case[0] + " col")
        same(val, d["table/val"][i], case[0] + " val")


def test_grid_stride_rounds_keep_their_bits():
    """130^3 voxels are more than 8192 blocks of 256 threads: pull and label pull at order 0, compared by SHA-256"""
    from brainfm_amd import interpol as IP
    d = golden()
    got = GB.run_big(IP, torch)
    for i, name in enumerate(GB.BIG_CASES):
        assert d["big/names"][i] == name
        assert bytes(got[i]) == bytes(d["big/sha"][i]), name


def test_push_and_pushgrad_keep_their_bits_where_two_addends_meet():
    """8 source voxels into 16^3 at coordinates where no address receives more than two atomic adds
    (test_host_grid_bits.py checks the stored coordinates), so the sums do not depend on the order of the adds."""
    from brainfm_amd import interpol as IP
    d = golden()
    names = list(d["atomic/names"])
    for case in GB.atomic_cases():
        i = names.index(case[0])
        push, pushgrad = GB.run_atomic_case(IP, torch, d, case)
        same(push, d["atomic/push"][i], case[0] + " push")
        same(pushgrad, d["atomic/pushgrad"][i], case[0] + " pushgrad")


@pytest.mark.parametrize("order", GB.ORDERS2, ids=GB.otag2)
def test_2d_pull_and_grad_keep_their_bits(order):
    """Image (2,2,5,6), grid (2,6,5,2): the x and y coordinates of the stored grid with their ties, the first two bounds of
    every configuration, extrapolate 0 / 1 / 2; (3,1) also under both batch broadcasts, through the exports."""
    from brainfm_amd import interpol as IP
    d, nd = golden(), golden_nd()
    names = list(nd["cases2d"])
    n = 0
    for case in GB.det2_cases():
        if case[1] != order:
            continue
        i = names.index(case[0])
        pull, grad = GB.run_det2_case(IP, torch, d, case)
        same(pull, nd["pull2d"][i], case[0] + " pull")
        same(grad, nd["grad2d"][i], case[0] + " grad")
        n += 1
    assert n == len(GB.CONFIGS) + (2 if order == (3, 1) else 0)


def test_2d_push_keeps_its_bits_where_two_addends_meet():
    """8 source pixels into 16^2 at coordinates where no address receives more than two atomic adds
    (test_host_grid_bits.py checks them)"""
    from brainfm_amd import interpol as IP
    d, nd = golden(), golden_nd()
    names = list(nd["atomic2d/names"])
    for case in GB.atomic2_cases():
        same(GB.run_atomic2_case(IP, torch, d, case), nd["atomic2d/push"][names.index(case[0])], case[0] + " push")


def test_linear_3d_broadcasts_and_second_grid_stride_round_keep_their_bits():
    """The all-linear 3-D exports with Bi = 1 and with Bg = 1, and their pull at 130^3 compared by SHA-256"""
    from brainfm_amd import interpol as IP
    d, nd = golden(), golden_nd()
    names = list(nd["lin3d/names"])
    for case in GB.LIN3_CASES:
        i = names.index(case[0])
        pull, grad = GB.run_lin3_case(IP, torch, d, case)
        same(pull, nd["lin3d/pull"][i], case[0] + " pull")
        same(grad, nd["lin3d/grad"][i], case[0] + " grad")
    assert tuple(nd["big/names"]) == GB.BIG2_CASES
    assert bytes(GB.run_big2(IP, torch)[0]) == bytes(nd["big/sha"][0]), GB.BIG2_CASES[0]
