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

_D = {}


def golden():
    if not _D:
        _D.update(load_npz("grid_family_bits.npz"))
    return _D


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
