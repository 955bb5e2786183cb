"""Training of the mask-conditioned network, host side: the float64 references of tests/stem_bwd_refs.py against torch
autograd and the torch expressions, the algebra bfm_stem_mc_bwd rests on, the fixtures of
tests/golden/make_golden_condtrain.py, and the argument checks that need no device."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stem_bwd_refs as SR
import twostage_weights as TW

FIXTURES = {"train_cond_mask": ("mask", (8, 12, 40), 2), "train_cond_maskflip": ("mask+flip", (7, 10, 36), 3)}
STEM = "backbone.encoders.0.basic_module.SingleConv1."


def _case(cin, cout, dims, seed):
    g = torch.Generator().manual_seed(seed)
    D, H, W = dims
    x = torch.rand((D, H, W, cin), generator=g, dtype=torch.float64)
    if cin >= 2:
        x[..., 1] = torch.flip(x[..., 0], dims=[0])
    x[..., cin - 1] = (torch.rand((D, H, W), generator=g) > 0.6).double()
    dP = torch.randn((D, H, W, cout), generator=g, dtype=torch.float64)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g, dtype=torch.float64) / np.sqrt(27.0 * cin)
    gamma = 1.0 + 0.4 * (torch.rand(cin, generator=g, dtype=torch.float64) - 0.5)
    beta = 0.4 * (torch.rand(cin, generator=g, dtype=torch.float64) - 0.5) + 0.3
    return dP, x, w, gamma, beta


@pytest.mark.parametrize("cin,cout,dims", [(2, 32, (5, 7, 9)), (3, 32, (1, 2, 3)), (4, 64, (3, 4, 33)), (3, 64, (8, 8, 40))])
def test_stem_bwd_ref_vs_float64_autograd(cin, cout, dims):
    dP, x, w, gamma, beta = _case(cin, cout, dims, 3)
    got = SR.stem_bwd_ref(dP, x, w, gamma, beta)
    ref = SR.stem_bwd_autograd(dP, x, w, gamma, beta)
    for name, a, b in zip(("dW", "dgamma", "dbeta"), got, ref):
        assert SR.rel_err(a, b) <= 1e-12, (name, SR.rel_err(a, b))


@pytest.mark.parametrize("cin,cout,dims", [(2, 32, (5, 7, 9)), (4, 32, (1, 2, 3)), (3, 64, (3, 4, 33))])
def test_one_correlation_over_the_raw_input_gives_all_three_gradients(cin, cout, dims):
    """dW = scale Q + shift S, dgamma = rstd sum W (Q - mean S), dbeta = sum W S, with Q the correlation of dP with the
    raw input and S that with the indicator of the volume (float64: the identity, not the kernel's rounding)."""
    dP, x, w, gamma, beta = _case(cin, cout, dims, 5)
    D, H, W = dims
    mean, rstd = SR.group_stats(x)
    xi = torch.zeros((D + 2, H + 2, W + 2, cin + 1), dtype=torch.float64)
    xi[1:-1, 1:-1, 1:-1, :cin] = x
    xi[1:-1, 1:-1, 1:-1, cin] = 1.0
    QS = torch.zeros((cout, cin + 1, 3, 3, 3), dtype=torch.float64)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                QS[:, :, kd, kh, kw] = torch.einsum("dhwo,dhwc->oc", dP, xi[kd:kd + D, kh:kh + H, kw:kw + W])
    Q, S = QS[:, :cin], QS[:, cin:]
    scale = (gamma * rstd).view(1, cin, 1, 1, 1)
    shift = (beta - mean * rstd * gamma).view(1, cin, 1, 1, 1)
    dW = scale * Q + shift * S
    dgamma = rstd * (w * (Q - mean * S)).sum(dim=(0, 2, 3, 4))
    dbeta = (w * S).sum(dim=(0, 2, 3, 4))
    ref = SR.stem_bwd_ref(dP, x, w, gamma, beta)
    for name, a, b in zip(("dW", "dgamma", "dbeta"), (dW, dgamma, dbeta), ref):
        assert SR.rel_err(a, b) <= 1e-11, (name, SR.rel_err(a, b))


@pytest.mark.parametrize("stem", sorted(FIXTURES))
def test_fixture_is_complete_and_condition_ref_reproduces_it(stem):
    condition, dims, cin = FIXTURES[stem]
    d = TW.load(stem)
    assert str(d["condition"]) == condition and tuple(int(v) for v in d["dims"]) == dims
    sd = TW.fixture_state_dict(d, "model")
    names = [str(s) for s in d["param_names"]]
    assert set(names) == set(sd.keys())
    assert tuple(sd[STEM + "conv.weight"].shape) == (32, cin, 3, 3, 3)
    losses = [str(s) for s in d["loss_names"]]
    assert losses and "pathol_ce" not in losses
    for prefix in ("ref32/", "ref64/"):
        assert prefix + "loss_total" in d
        for n in losses:
            assert prefix + "loss/loss_" + n in d
        for n in names:
            if n.startswith(STEM) or n.startswith("head."):
                assert d[prefix + "grad/" + n].shape == tuple(sd[n].shape), n
            else:
                assert d[prefix + "grad_at/" + n].shape == d["grad_idx/" + n].shape
                assert float(d[prefix + "grad_l2/" + n]) > 0 and float(d[prefix + "grad_max/" + n]) > 0
    p = torch.from_numpy(d["target/pathology"])
    if condition == "mask":
        assert set(np.unique(p.numpy())) == {0.0, 1.0}
    else:
        assert 0 < float(((p > 0) & (p < 1)).float().mean())
    for i in range(2):
        x = torch.from_numpy(d["sample%d/input" % i])
        x_cl, masked, _ = SR.condition_ref(x, p, condition)
        assert x_cl.shape == dims + (cin,)
        ref = torch.concat([torch.from_numpy(d["masked%d" % i]), torch.from_numpy(d["cond%d" % i])], dim=1)
        assert torch.equal(x_cl, ref[0].permute(1, 2, 3, 0))
        assert torch.equal(masked, torch.from_numpy(d["masked%d" % i]))


def test_condition_inputs_rejects_unknown_names_and_wrong_channel_counts():
    from brainfm_amd import _lib as L
    from brainfm_amd import train as TR
    samples = [{"input": torch.zeros((1, 1, 2, 2, 2))}]
    target = {"pathology": torch.zeros((1, 1, 2, 2, 2))}
    for bad in ("blur", "mask+blur", "", None):
        with pytest.raises(L.BfmError):
            TR.condition_inputs(samples, target, bad)
    with pytest.raises(L.BfmError):
        TR.condition_inputs(samples, target, "mask+flip", in_channels=2)
    with pytest.raises(L.BfmError):
        TR.condition_inputs(samples, target, "mask", in_channels=3)


def test_stem_route_is_taken_by_the_conditioned_first_layer_only():
    from brainfm_amd import backward as BW
    ly = SimpleNamespace(cout=32, groups=1)
    assert all(BW.stem_mc_bwd_ok(ly, ca, 0, False) for ca in (2, 3, 4))
    assert not BW.stem_mc_bwd_ok(ly, 1, 0, False)                       # the one-channel stem keeps its kernels
    assert not BW.stem_mc_bwd_ok(ly, 8, 0, False)
    assert not BW.stem_mc_bwd_ok(ly, 2, 0, True)
    assert not BW.stem_mc_bwd_ok(ly, 2, 2, False)
    assert not BW.stem_mc_bwd_ok(SimpleNamespace(cout=16, groups=1), 2, 0, False)
    assert not BW.stem_mc_bwd_ok(SimpleNamespace(cout=32, groups=2), 2, 0, False)


def test_every_step_class_takes_the_cond_that_step_hands_on():
    """TrainStep.step passes cond= to self.loss_and_grads, so a subclass that overrides it has to take the keyword."""
    import inspect
    from brainfm_amd import train as TR
    subs, todo = [], [TR.TrainStep]
    while todo:
        c = todo.pop()
        subs.append(c)
        todo.extend(c.__subclasses__())
    assert TR.ContrastiveStep in subs
    for c in subs:
        p = inspect.signature(c.loss_and_grads).parameters.get("cond")
        assert p is not None and p.default is None, c.__name__
