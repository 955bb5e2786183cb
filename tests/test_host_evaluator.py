"""Host-side checks of the evaluator (brainfm_amd/evaluator.py, models.get_evaluator): the SSIM restatement the kernels are
held to (tests/ssim_refs.py) against a brute-force window sum, the reference's scalar metrics restated in numpy float64
against the fixture made by running the reference (tests/golden/make_golden_evaluator.py), metric lists and signatures,
and the refusal to run without a HIP device."""
import inspect
import json
import os
import types

import numpy as np
import pytest
import torch

import ssim_refs as SR
from conftest import GOLDEN, load_npz


@pytest.fixture(scope="module")
def fx():
    return load_npz("evaluator.npz")


def test_restatement_equals_brute_force_window_sums():
    x, y = SR.smooth_pair((11, 12, 13), seed=1)
    x, y = x.double(), y.double()
    for sigma in (1.5, 0.8):
        s, c = SR.ssim_cs(x[None, None], y[None, None], sigma)
        bs, bc = SR.brute_ssim_cs(x.numpy(), y.numpy(), sigma)
        assert abs(float(s) - bs) < 1e-12 and abs(float(c) - bc) < 1e-12
        assert 0.05 < bs < 0.95


def test_ssim_of_a_volume_with_itself_is_one():
    x, _ = SR.smooth_pair((2, 12, 13, 14), seed=2)
    assert torch.equal(SR.ssim(x[None].double(), x[None].double()), torch.ones(1, dtype=torch.float64))
    assert float(SR.get_ssim(x[None].double(), x[None].double())) == 1.0


def test_ms_ssim_size_assertion_uses_the_last_two_axes():
    a = torch.rand(1, 1, 12, 160, 161, dtype=torch.float64)
    with pytest.raises(AssertionError):
        SR.ms_ssim(a, a)
    b = torch.rand(1, 1, 16, 161, 161, dtype=torch.float64)
    assert abs(float(SR.ms_ssim(b, b)) - 1.0) < 1e-12


def test_an_axis_shorter_than_the_window_is_not_filtered():
    x, y = SR.smooth_pair((8, 16, 40), seed=3)
    x, y = x.double()[None, None], y.double()[None, None]
    win = SR.window(1.5, torch.float64)
    f = SR.gaussian_filter(x, win)
    assert tuple(f.shape) == (1, 1, 8, 6, 30)
    # every depth slice is the 2-D 'valid' filter of that slice alone
    w2 = (win[:, None] * win[None, :])
    want = sum(w2[i, j] * x[0, 0, 3, i:i + 6, j:j + 30] for i in range(11) for j in range(11))
    assert torch.allclose(f[0, 0, 3], want, atol=1e-14, rtol=0)
    s = float(SR.ssim(x, y))
    assert 0.05 < s < 0.95


def test_scalar_metrics_restated_in_float64_equal_the_reference(fx):
    o, t = fx["o"].astype(np.float64), fx["t"].astype(np.float64)
    n = o.size
    assert n % 4 != 0
    assert abs(np.abs(o - t).sum() / n - fx["l1_64"]) < 1e-14
    mse = ((o - t) ** 2).sum() / n
    assert abs(20 * np.log10(t.max() / np.sqrt(mse)) - fx["psnr_64"]) < 1e-12
    w = (o * t).sum() / ((o * o).sum() + 1e-7)
    # the expanded form the evaluator uses
    num = w * w * (o * o).sum() - 2 * w * (o * t).sum() + (t * t).sum()
    assert abs(np.sqrt(num / ((t * t).sum() + 1e-7)) - fx["nl2_64"]) < 1e-13
    nz = fx["l1nz_64"]
    assert nz.shape == o.shape[1:] and np.array_equal(np.isnan(nz), t[0] == 0)
    assert np.array_equal(nz[t[0] != 0], np.abs(t - o)[0][t[0] != 0])
    assert np.isnan(fx["l1nz_32"]).sum() == (t == 0).sum() > 0
    do, dt = fx["dice_o"].astype(np.float64), fx["dice_t"].astype(np.float64)
    dice = np.mean(2 * (do * dt).sum(axis=(2, 3, 4)) / np.maximum((do + dt).sum(axis=(2, 3, 4)), 1e-5))
    assert abs(dice - fx["dice_64"]) < 1e-14


def test_label_dice_from_counts_equals_the_reference_onehot_dice(fx):
    from brainfm_amd import evaluator as E
    lut = np.zeros(10000, dtype=np.int64)
    for l, lab in enumerate(E.label_list_segmentation):
        lut[lab] = l
    for tag in "ab":
        p, t = lut[fx["lab_p_" + tag].astype(np.int64)], lut[fx["lab_t_" + tag].astype(np.int64)]
        cp, ct = np.bincount(p.ravel(), minlength=33), np.bincount(t.ravel(), minlength=33)
        ci = np.bincount(p[p == t].ravel(), minlength=33)
        dice = np.mean(2.0 * ci / np.maximum(cp + ct, 1e-5))
        assert abs(dice - fx["labdice_%s_64" % tag]) < 1e-14


def test_constants_equal_the_reference():
    from brainfm_amd import evaluator as E
    assert E.n_labels == 33 and E.n_neutral_labels == 7 and E.nlat == 13
    assert E.label_list_segmentation[:8] == [0, 14, 15, 16, 24, 77, 85, 2] and E.label_list_segmentation[-1] == 60
    assert list(E.vflip) == list(range(7)) + list(range(20, 33)) + list(range(7, 20))
    a, b = E.align_shape(np.zeros((4, 5, 6)), np.zeros((5, 4, 6)))
    assert a.shape == b.shape == (4, 4, 6)


def test_metric_lists_equal_the_reference(fx):
    from brainfm_amd import models as M
    args = types.SimpleNamespace()                           # no ssim_win_sigma: the default 1.5, not an AttributeError
    i = 0
    while "tasks_%d" % i in fx:
        ev = M.get_evaluator(args, [str(s) for s in fx["tasks_%d" % i]], "cpu")
        assert ev.metric_names == [str(s) for s in fx["metrics_%d" % i]]
        assert ev.win_sigma == 1.5
        assert all(m in ev.metric_map for m in ev.metric_names)
        i += 1
    assert i == 5 and int(fx["empty_asserts"]) == 1
    with pytest.raises(AssertionError):
        M.get_evaluator(args, [], "cpu")
    assert M.get_evaluator(types.SimpleNamespace(ssim_win_sigma=0.8), ["T2"], "cpu").win_sigma == 0.8


def test_signatures_equal_the_reference():
    from brainfm_amd import evaluator as E, models as M
    with open(os.path.join(GOLDEN, "api_signatures_evaluator.json")) as f:
        want = json.load(f)
    got = {"get_onehot": E.get_onehot, "align_shape": E.align_shape, "get_evaluator": M.get_evaluator,
           "Evaluator.__init__": E.Evaluator.__init__}
    for m in ("get_dice", "get_normalized_l2", "get_l1", "get_psnr", "get_ssim", "get_ms_ssim", "get_score", "eval"):
        got["Evaluator." + m] = getattr(E.Evaluator, m)
    assert sorted(want) == sorted(got)
    for name, fn in got.items():
        assert str(inspect.signature(fn)) == want[name], name
    sig = inspect.signature(E.Evaluator.eval_tensors)
    assert str(sig) == "(self, pred, target, clamp=False, is_seg=False, normalize=False, **kwargs)"


def test_every_entry_refuses_to_run_without_a_hip_device(tmp_path):
    from brainfm_amd import evaluator as E, volio
    from brainfm_amd._lib import BfmError
    ev = E.Evaluator(types.SimpleNamespace(), ["feat_l1"], "cpu")
    x = torch.rand(1, 1, 12, 12, 12)
    for name in ("get_dice", "get_normalized_l2", "get_l1", "get_psnr", "get_ssim", "get_ms_ssim"):
        with pytest.raises(BfmError):
            getattr(ev, name)("m", x, x)
    with pytest.raises(BfmError):
        ev.get_score("feat_l1", x, x)
    with pytest.raises(BfmError):
        ev.eval_tensors(x, x)
    with pytest.raises(BfmError):
        ev.eval_tensors(np.zeros((4, 4, 4), dtype=np.int32), np.zeros((4, 4, 4), dtype=np.int32), is_seg=True)
    with pytest.raises(BfmError):
        E.get_onehot(np.zeros((4, 4, 4), dtype=np.int64), "cpu")
    with pytest.raises(BfmError):
        E.label_counts(np.zeros((4, 4, 4)), np.zeros((4, 4, 4)), "cpu")
    p = str(tmp_path / "a.nii.gz")
    volio.MRIwrite(np.zeros((4, 4, 4), dtype=np.float32), np.eye(4), p)
    with pytest.raises(BfmError):
        ev.eval(p, p)
