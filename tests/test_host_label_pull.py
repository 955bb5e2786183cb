"""CPU checks for the label branch of interpol.grid_pull, the grid builders and spline_coeff: the float64 restatement
(tests/label_pull_refs.py) against the reference's own label maps (tests/golden/label_pull.npz), the share of voxels that
the comparison has to leave out, and the argument errors of brainfm_amd.interpol."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_npz
import label_pull_refs as LR

ORDERS = {"o0": 0, "o1": 1, "o2": 2, "o3": 3, "o130": [1, 3, 0], "o213": [2, 1, 3]}
IMAGES = {"P": np.int64, "Q": np.uint8, "S": np.int16}
_D = {}


def golden():
    if not _D:
        _D.update(load_npz("label_pull.npz"))
    return _D


@pytest.mark.parametrize("otag", list(ORDERS))
@pytest.mark.parametrize("tag", list(IMAGES))
def test_restatement_equals_the_reference_wherever_the_gap_decides(tag, otag):
    """Every stored case (seven bounds, extrapolate both ways) of one image and one order: equal labels at every voxel
    whose gap exceeds 1e-5, and at most 0.5 % of a case's voxels below it -- with the reference alone, which is what
    lets the GPU test apply the same cap."""
    d = golden()
    img, grid = d[tag + "/img"], d[tag + "/grid"]
    assert img.dtype == IMAGES[tag] and img.shape[:2] == (2, 2) and grid.shape == (2, 6, 7, 5, 3)
    worst, n = 0.0, 0
    for bound in range(7):
        for ext in (0, 1):
            ref = d["%s/%s/b%d_e%d" % (tag, otag, bound, ext)]
            win, gap = LR.label_pull(img, grid, ORDERS[otag], bound, ext)
            assert win.dtype == ref.dtype == img.dtype and win.shape == ref.shape == (2, 2, 6, 7, 5)
            keep, under = LR.decided(gap)
            worst = max(worst, 1.0 - keep.mean())
            assert under, (bound, ext, 1.0 - keep.mean())
            assert np.array_equal(win[keep], ref[keep]), (bound, ext)
            n += 1
    assert n == 14
    print("%s %s: largest undecided share %.4f (cap %.4f)" % (tag, otag, worst, LR.CAP))


def test_fixture_covers_what_it_should_and_stays_small():
    d = golden()
    assert sorted(np.unique(d["P/img"]).tolist()) == [-7, -1, 0, 3, 12, 200, 70000]
    assert sorted(np.unique(d["Q/img"]).tolist()) == [0, 1, 2, 5, 77, 255]
    assert sorted(np.unique(d["S/img"]).tolist()) == [-300, -2, 0, 5, 77, 3000]
    assert d["P/img"].shape[2:] == (9, 8, 7) and d["Q/img"].shape[2:] == (7, 6, 5)
    for tag in IMAGES:
        g, shape = d[tag + "/grid"], d[tag + "/img"].shape[2:]
        for a in range(3):                                   # spills over every face: wraps and out-of-view zeros
            assert g[..., a].min() < -2.0 and g[..., a].max() > shape[a] + 1.0
        # out-of-view voxels give 0 without extrapolation, and some voxel of every case is in view
        ref = d[tag + "/o1/b3_e0"]
        out = np.zeros(g.shape[:-1], bool)
        for a in range(3):
            out |= (g[..., a] <= -0.05) | (g[..., a] >= shape[a] - 1 + 0.05)
        assert out.any() and not out.all() and not ref[:, 0][out].any() and ref[:, 0][~out].any()
    assert os.path.getsize(os.path.join(GOLDEN, "label_pull.npz")) < 1 << 20


def test_restatement_tie_rule_and_zero():
    """Two taps of weight 0.5 each: the smaller label wins, negative labels included; no positive weight gives 0."""
    img = np.array([-4, 9, 3, 3, 7], np.int32).reshape(1, 1, 5, 1, 1)
    grid = np.array([[0.5, 0, 0], [1.5, 0, 0], [3.5, 0, 0], [2.5, 0, 0]], np.float32).reshape(1, 4, 1, 1, 3)
    win, gap = LR.label_pull(img, grid, 1, 3, 1)
    assert win.ravel().tolist() == [-4, 3, 3, 3]
    assert gap.ravel()[0] == 0.0 and gap.ravel()[3] == 1.0
    far = np.array([[-3.0, 0, 0], [9.0, 0, 0]], np.float32).reshape(1, 2, 1, 1, 3)
    win, gap = LR.label_pull(img, far, 1, 0, 1)                     # `zero` drops every tap
    assert win.ravel().tolist() == [0, 0] and np.isinf(gap).all()
    win, gap = LR.label_pull(img, far, 1, 3, 0)                     # masked without extrapolation
    assert win.ravel().tolist() == [0, 0] and np.isinf(gap).all()
    win, _ = LR.label_pull(img, np.array([[-1.0, 0, 0]], np.float32).reshape(1, 1, 1, 1, 3), 0, 5, 1)
    assert win.ravel().tolist() == [0]                              # a reflected dst2 tap: weight -1, never positive


def test_blocky_labels_look_like_a_segmentation():
    lab = LR.blocky_labels((40, 36, 32), 100, 0)
    assert lab.dtype == np.int32 and lab.shape == (40, 36, 32)
    assert lab[0, 0, 0] == 0 and lab[20, 18, 16] != 0
    assert 50 <= len(np.unique(lab)) <= 100
    assert np.array_equal(lab, LR.blocky_labels((40, 36, 32), 100, 0))


def test_argument_errors():
    from brainfm_amd import interpol as IP
    seg = torch.zeros(1, 1, 4, 4, 4, dtype=torch.int32)
    grid = torch.zeros(1, 2, 2, 2, 3)
    with pytest.raises(TypeError, match="bool"):
        IP.grid_pull(seg.bool(), grid)
    for order in (0, 1, 3):
        with pytest.raises(NotImplementedError, match="prefilter"):
            IP.grid_pull(seg, grid, order, "dct2", prefilter=True)
    with pytest.raises(NotImplementedError, match="only 3-D grids are on the hot path"):
        IP.grid_pull(torch.zeros(1, 1, 4, 4, dtype=torch.int32), torch.zeros(1, 2, 2, 2))
    with pytest.raises(NotImplementedError, match="only 3-D grids are on the hot path"):
        IP.grid_pull(torch.zeros(1, 1, 4, dtype=torch.int16), torch.zeros(1, 2, 1))
    with pytest.raises(TypeError, match="int8"):
        IP.grid_pull(seg.to(torch.int8), grid)
    with pytest.raises(NotImplementedError, match="5"):
        IP.grid_pull(seg, grid, 5)
    with pytest.raises(IP.L.BfmError):                                     # no CPU fallback
        IP.grid_pull(seg, grid)
    with pytest.raises(ValueError, match=r"Dimension of the affine matrix \(3\) and shape \(2\) are not the same"):
        IP.affine_grid(torch.eye(4), [3, 3])
    with pytest.raises(ValueError, match="First argument should be"):
        IP.affine_grid(torch.zeros(2, 4), [3, 3, 3])
    with pytest.raises(IP.L.BfmError):
        IP.affine_grid(torch.eye(4), [3, 3, 3])
    with pytest.raises(IP.L.BfmError):
        IP.identity_grid([3, 3, 3], device="cpu")
    for bound in ("dst1", "dst2"):
        with pytest.raises(NotImplementedError):
            IP.spline_coeff(torch.zeros(4, 5), 3, bound)
    with pytest.raises(NotImplementedError, match="6"):
        IP.spline_coeff(torch.zeros(4, 5), 6)
    with pytest.raises(ValueError):
        IP.spline_coeff(torch.zeros(4, 5), [3, 2])
    with pytest.raises(IndexError):
        IP.spline_coeff(torch.zeros(4, 5), 3, "dct2", dim=2)
    with pytest.raises(IP.L.BfmError):
        IP.spline_coeff(torch.zeros(4, 5), 3)
