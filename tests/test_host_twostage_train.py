"""Joint training of the two-stage model, host side (no GPU): the float64 closed forms of tests/twostage_train_refs.py
against torch autograd, the fixture of tests/golden/make_golden_twostage_train.py, the refusals of
train.twostage_train_step that need no device, and the three new bindings."""
import os
from argparse import Namespace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import twostage_train_refs as TR
import twostage_weights as TW

STEM = "backbone.encoders.0.basic_module.SingleConv1."
TASKS = dict(T1=True, T2=True, FLAIR=True, CT=True, segmentation=True, distance=True, bias_field=True, registration=True,
             super_resolution=True, surface=False, pathology=True, contrastive=False)
MARGIN = 0.05           # 25 x the 2e-3 gradient tolerance of the GPU test


def _case(cin, cout, dims, seed):
    g = torch.Generator().manual_seed(seed)
    D, H, W = dims
    x_raw = torch.rand((D, H, W), generator=g, dtype=torch.float64)
    r = 3.0 * torch.randn((D, H, W), generator=g, dtype=torch.float64)
    others = torch.rand((D, H, W, cin - 1), generator=g, dtype=torch.float64)
    others[..., -1] = (torch.rand((D, H, W), generator=g) > 0.6).double()
    dP = torch.randn((D, H, W, cout), generator=g, dtype=torch.float64)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g, dtype=torch.float64) / np.sqrt(27.0 * cin)
    gamma = 1.0 + 0.4 * (torch.rand(cin, generator=g, dtype=torch.float64) - 0.5)
    beta = 0.4 * (torch.rand(cin, generator=g, dtype=torch.float64) - 0.5) + 0.3
    return dP, x_raw, r, others, w, gamma, beta


@pytest.mark.parametrize("dims", [(1, 2, 3), (5, 7, 9)])
@pytest.mark.parametrize("end", ["first", "last"])
@pytest.mark.parametrize("cin", [2, 3, 4])
def test_closed_forms_vs_float64_autograd(cin, end, dims):
    """dX_c = rstd (gamma_c G_c - m1 - xhat_c m2) with the group means taken from dgamma / dbeta, chained through
    x (1 - sigmoid(r)), against autograd of conv3d(group_norm(cat([x (1 - sigmoid(r)), t]), 1, gamma, beta), w, padding=1)
    with respect to r: within 1e-10 of the maximum."""
    channel = 0 if end == "first" else cin - 1
    dP, x_raw, r, others, w, gamma, beta = _case(cin, 32, dims, 11 + cin)
    ref, x_cl = TR.chain_autograd(dP, x_raw, r, others, w, gamma, beta, channel)
    dx = TR.stem_dgrad_ref(dP, x_cl, w, gamma, channel)
    got = TR.mask_chain_ref(dx, x_raw, TR.sigmoid64(r))
    assert TR.rel_err(got, ref) <= 1e-10, TR.rel_err(got, ref)


# ----------------------------------------------------------------------------- the fixture
def _train_args():
    ta = Namespace()
    ta.losses = Namespace(uncertainty=None, implicit_pathol=False, image_grad=True, registration_grad=True)
    ta.weights = Namespace(image=1.0, image_grad=1.0, seg_ce=1.0, seg_dice=1.0, bias_field_log=1.0, distance=1.0,
                           registration=1.0, registration_grad=1.0, pathol_ce=1.0, pathol_dice=1.0)
    return ta


def test_fixture_is_complete():
    from brainfm_amd import models as M
    from brainfm_amd import test_utils as TU
    from brainfm_amd import train as T
    path = os.path.join(TW.GOLDEN, "train_twostage.npz")
    assert os.path.getsize(path) < 1 << 20
    d = TW.load("train_twostage")
    assert tuple(int(v) for v in d["dims"]) == (8, 12, 40) and tuple(int(v) for v in d["cfg"][:2]) == (64, 2)
    sds = {m: TW.fixture_state_dict(d, m) for m in ("pathol", "task")}
    assert tuple(sds["pathol"][STEM + "conv.weight"].shape) == (32, 1, 3, 3, 3)
    assert tuple(sds["task"][STEM + "conv.weight"].shape) == (32, 2, 3, 3, 3)
    assert "head.final_conv_pathology.weight" in sds["pathol"] and "head.final_conv_pathology.weight" not in sds["task"]
    names = [str(s) for s in d["param_names"]]
    assert set(names) == {m + "/" + k for m in sds for k in sds[m]}
    # the loss names in the criterion's order: what criterion_losses builds for the same tasks
    ga, ta = TU.default_inference_args(f_maps=64, num_levels=2, left_hemis_only=True, tasks=dict(TASKS))
    ga, _ = M.process_args(ga, ta, task=ga.task)
    want, _ = T.criterion_losses(_train_args(), ga.tasks)
    losses = [str(s) for s in d["loss_names"]]
    assert losses == want and losses[-2:] == ["pathol_ce", "pathol_dice"]
    assert set(np.unique(d["target/pathology"])) == {0.0, 1.0}
    w = dict(zip((str(s) for s in d["loss_weight_names"]), d["loss_weights"]))
    assert len(set(w.values())) > 1
    for prefix in ("ref32/", "ref64/"):
        assert prefix + "loss_total" in d
        for n in losses:
            assert prefix + "loss/loss_" + n in d
        for i in range(2):
            assert d[prefix + "p%d" % i].shape == (1, 1, 8, 12, 40) == d[prefix + "input_masked%d" % i].shape
        for n in names:
            m, k = n.split("/", 1)
            if k.startswith(STEM) or k.startswith("head."):
                assert d[prefix + "grad/" + n].shape == tuple(sds[m][k].shape), n
            else:
                assert d[prefix + "grad_at/" + n].shape == d["grad_idx/" + n].shape
                assert float(d[prefix + "grad_l2/" + n]) > 0 and float(d[prefix + "grad_max/" + n]) > 0
    # input_masked is the loop's expression of p, and p spans (0, 1)
    for i in range(2):
        x, p = torch.from_numpy(d["sample%d/input" % i]), torch.from_numpy(d["ref32/p%d" % i])
        assert torch.equal(torch.from_numpy(d["ref32/input_masked%d" % i]), x * (1 - p))
        assert float(p.min()) < 0.05 and float(p.max()) > 0.95


def test_fixture_separates_the_coupled_gradient_from_the_cut_one():
    """Stage 0's stem and head weight gradients move by at least 5 % of their maximum when the gradient through the mask is
    cut: 25 x the tolerance of the GPU test, so a build that drops the coupling fails it."""
    d = TW.load("train_twostage")
    for k in (STEM + "conv.weight", "head.final_conv_pathology.weight"):
        a, b = d["ref64/grad/pathol/" + k], d["ref64/grad_cut/pathol/" + k]
        assert a.shape == b.shape
        m = float(np.abs(a - b).max() / np.abs(a).max())
        assert m >= MARGIN, (k, m)
    for n in (str(s) for s in d["param_names"]):
        m, k = n.split("/", 1)
        if m == "pathol" and (k.startswith(STEM) or k.startswith("head.")):
            assert "ref64/grad_cut/" + n in d


# ----------------------------------------------------------------------------- refusals that need no device
def _fake_model(in_channels, device):
    eng = SimpleNamespace(in_channels=in_channels, device=torch.device(device))
    return SimpleNamespace(backbone=SimpleNamespace(engine=lambda head: eng), head=None)


def test_twostage_train_step_refuses_flip_the_cpu_and_wrong_channel_counts():
    from brainfm_amd import _lib as L
    from brainfm_amd import models as M
    from brainfm_amd import test_utils as TU
    from brainfm_amd import train as T
    ga = Namespace(tasks=[], max_surf_distance=3.0)
    ta = _train_args()
    for cond in ("flip", "mask+flip"):
        ta.condition = cond
        with pytest.raises(L.BfmError, match="flip"):
            T.twostage_train_step(ga, ta, _fake_model(1, "cuda:0"), _fake_model(2, "cuda:0"), [1.0], 1.0)
    ta.condition = "blur"
    with pytest.raises(L.BfmError):
        T.twostage_train_step(ga, ta, _fake_model(1, "cuda:0"), _fake_model(2, "cuda:0"), [1.0], 1.0)
    for cond in (None, "mask"):
        ta.condition = cond
        with pytest.raises(L.BfmError, match="HIP device"):
            T.twostage_train_step(ga, ta, _fake_model(1, "cpu"), _fake_model(2, "cpu"), [1.0], 1.0)
        for c0, c1 in ((1, 1), (2, 2), (1, 3)):
            with pytest.raises(L.BfmError, match="channels"):
                T.twostage_train_step(ga, ta, _fake_model(c0, "cuda:0"), _fake_model(c1, "cuda:0"), [1.0], 1.0)
    # the models of build_inpaint_model on the CPU: no engine, no step
    ga2, ta2 = TU.default_inference_args(f_maps=8, num_levels=2, tasks=dict(TASKS))
    ta2.backbone = "unet3d+unet3d"
    ta2.condition = None
    ga2, ta2, pm, tm = M.build_inpaint_model(ga2, ta2, "cpu")[:4]
    with pytest.raises(L.BfmError):
        T.twostage_train_step(ga2, ta2, pm, tm, [1.0], 1.0)


def test_the_input_gradient_request_leaves_the_one_correlation_rule_alone():
    from brainfm_amd import backward as BW
    ly = SimpleNamespace(cout=32, groups=1)
    assert all(BW.stem_mc_dgrad_ok(ly, ca, 0) for ca in (2, 3, 4))
    assert not BW.stem_mc_dgrad_ok(ly, 1, 0) and not BW.stem_mc_dgrad_ok(ly, 2, 2)
    assert not BW.stem_mc_dgrad_ok(SimpleNamespace(cout=16, groups=1), 2, 0)
    assert not BW.stem_mc_dgrad_ok(SimpleNamespace(cout=32, groups=2), 2, 0)
    assert not BW.stem_mc_bwd_ok(ly, 2, 0, True)                        # a bare need_input_grad still goes generic


def test_lib_declares_the_new_exports():
    import ctypes as C
    from brainfm_amd import _lib as L
    want = {"bfm_stem_mc_dgrad": 21, "bfm_mask_chain_bwd": 9, "bfm_twostage_train_input": 10}
    for name, nargs in want.items():
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, name
    header = open(os.path.join(os.path.dirname(TW.GOLDEN), os.pardir, "include", "brainfm_hip.h")).read()
    for name in want:
        assert name + "(" in header, name
