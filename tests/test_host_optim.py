"""Host side of the Adam / SGD / LARS training steps: the float64 restatements (tests/optim_refs.py) against torch's own
optimisers and against the reference's utils.LARS (tests/golden/optim.npz, made by tests/golden/make_golden_optim.py), the
mirrors build_optimizer / build_schedulers against the reference's signatures and scheduler arrays, and the checkpoint
layouts against the installed torch's.  CPU only."""
import inspect
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import optim_refs as R
from conftest import GOLDEN, load_npz

SHAPES = ((7, 5), (2, 3, 1, 1, 1), (11,), (4, 4))            # the last one never gets a gradient


def _torch_run(make, wd):
    g_ = torch.Generator().manual_seed(11)
    p0 = [torch.randn(s, generator=g_, dtype=torch.float64) for s in SHAPES]
    grads = [[torch.randn(s, generator=g_, dtype=torch.float64) * 10.0 ** (t - 3) for s in SHAPES[:-1]] for t in (1, 2, 3)]
    ps = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = make(ps, wd)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
    return p0, grads, ps, opt


@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_adam_ref_equals_torch_adam_float64(wd):
    p0, grads, ps, opt = _torch_run(lambda ps, wd: torch.optim.Adam(ps, lr=3e-3, weight_decay=wd), wd)
    for i in range(len(SHAPES) - 1):
        p, m, v = p0[i], torch.zeros_like(p0[i]), torch.zeros_like(p0[i])
        for t, gs in enumerate(grads, 1):
            p, m, v = R.adam_step(p, gs[i], m, v, t, 3e-3, weight_decay=wd)
        assert float((p - ps[i].detach()).abs().max()) <= 1e-12
        assert float((m - opt.state[ps[i]]["exp_avg"]).abs().max()) <= 1e-12
        assert float((v - opt.state[ps[i]]["exp_avg_sq"]).abs().max()) <= 1e-12
    assert torch.equal(ps[-1].detach(), p0[-1]) and ps[-1] not in opt.state     # no gradient: no step, no state


@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_adamw_ref_equals_torch_adamw_float64(wd):
    p0, grads, ps, opt = _torch_run(lambda ps, wd: torch.optim.AdamW(ps, lr=3e-3, weight_decay=wd), wd)
    for i in range(len(SHAPES) - 1):
        p, m, v = p0[i], torch.zeros_like(p0[i]), torch.zeros_like(p0[i])
        for t, gs in enumerate(grads, 1):
            p, m, v = R.adamw_step(p, gs[i], m, v, t, 3e-3, weight_decay=wd)
        assert float((p - ps[i].detach()).abs().max()) <= 1e-12
        assert float((m - opt.state[ps[i]]["exp_avg"]).abs().max()) <= 1e-12
        assert float((v - opt.state[ps[i]]["exp_avg_sq"]).abs().max()) <= 1e-12
    assert torch.equal(ps[-1].detach(), p0[-1]) and ps[-1] not in opt.state     # no gradient: no step, no state


@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_sgd_ref_equals_torch_sgd_float64(wd):
    p0, grads, ps, opt = _torch_run(lambda ps, wd: torch.optim.SGD(ps, lr=3e-3, momentum=0.9, weight_decay=wd), wd)
    for i in range(len(SHAPES) - 1):
        p, buf = p0[i], torch.zeros_like(p0[i])
        for gs in grads:
            p, buf = R.sgd_step(p, gs[i], buf, 3e-3, 0.9, wd)
        assert float((p - ps[i].detach()).abs().max()) <= 1e-12
        assert float((buf - opt.state[ps[i]]["momentum_buffer"]).abs().max()) <= 1e-12
    assert torch.equal(ps[-1].detach(), p0[-1]) and ps[-1] not in opt.state


def test_grad_scale_is_a_factor_on_the_gradient():
    g_ = torch.Generator().manual_seed(2)
    p, g = torch.randn(9, generator=g_, dtype=torch.float64), torch.randn(9, generator=g_, dtype=torch.float64)
    z = torch.zeros_like(p)
    for a, b in ((R.adam_step(p, g, z, z, 1, 1e-2, weight_decay=0.1, grad_scale=0.5),
                  R.adam_step(p, 0.5 * g, z, z, 1, 1e-2, weight_decay=0.1)),
                 (R.sgd_step(p, g, z, 1e-2, 0.9, 0.1, grad_scale=0.5), R.sgd_step(p, 0.5 * g, z, 1e-2, 0.9, 0.1)),
                 (R.lars_step(p.view(3, 3), g.view(3, 3), z.view(3, 3), 0.3, 0.1, grad_scale=0.5),
                  R.lars_step(p.view(3, 3), 0.5 * g.view(3, 3), z.view(3, 3), 0.3, 0.1))):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_lars_ref_equals_the_reference_float64():
    """Three utils.LARS steps on a matrix, a 5-D weight, a 1-D parameter (no decay, no trust ratio) and an all-zero
    matrix (q = 1)."""
    d = load_npz("optim.npz")
    lr, wd, mom, eta = (float(v) for v in d["lars_hyper"])
    for n in (str(s) for s in d["lars_names"]):
        p = torch.from_numpy(d["lars_p0/" + n]).double()
        mu = torch.zeros_like(p)
        for t in (1, 2, 3):
            p, mu = R.lars_step(p, torch.from_numpy(d["lars_g%d/%s" % (t, n)]).double(), mu, lr, wd, mom, eta)
            if t == 1:
                assert float((p - torch.from_numpy(d["lars64_p1/" + n])).abs().max()) <= 1e-12, n
        assert float((p - torch.from_numpy(d["lars64_p3/" + n])).abs().max()) <= 1e-12, n
        assert float((mu - torch.from_numpy(d["lars64_mu3/" + n])).abs().max()) <= 1e-12, n
        # the reference's own float32 run stays within float32 rounding of it
        assert float((p - torch.from_numpy(d["lars32_p3/" + n]).double()).abs().max()) <= 2e-6, n


def test_lars_trust_ratio_from_the_three_sums():
    """train.lars_trust_ratio (the host's use of bfm_lars_sums_multi) equals eta |p| / |c g + wd p| formed directly, and
    is 1 for a zero parameter or a zero update."""
    from brainfm_amd import train as TR
    g_ = torch.Generator().manual_seed(4)
    p, g = torch.randn(500, generator=g_, dtype=torch.float64), torch.randn(500, generator=g_, dtype=torch.float64)
    for c, wd in ((1.0, 0.0), (0.5, 0.1), (1e-3, 0.4), (2.0 ** -16, 0.04)):
        q = TR.lars_trust_ratio(float(g @ g), float(p @ p), float(p @ g), c, wd, 1e-3)
        ref = 1e-3 * float(p.norm()) / float((c * g + wd * p).norm())
        assert abs(q - ref) <= 1e-12 * ref
    assert TR.lars_trust_ratio(3.0, 0.0, 0.0, 1.0, 0.1, 1e-3) == 1.0
    assert TR.lars_trust_ratio(0.0, 5.0, 0.0, 1.0, 0.0, 1e-3) == 1.0


def test_mirrors_have_the_reference_signatures():
    from brainfm_amd import models as M
    with open(os.path.join(GOLDEN, "api_signatures_optim.json")) as f:
        sig = json.load(f)
    assert str(inspect.signature(M.build_optimizer)) == sig["build_optimizer"]
    assert str(inspect.signature(M.build_schedulers)) == sig["build_schedulers"]
    # utils.LARS' defaults are the LARS spec's
    ref = sig["LARS.__init__"]
    s = M.OptimizerSpec("lars")
    assert "momentum=%s" % s.momentum in ref and "eta=%s" % s.eta in ref and "lr=0," in ref and "weight_decay=0," in ref
    assert "weight_decay_filter=None" in ref and "lars_adaptation_filter=None" in ref


@pytest.mark.parametrize("kind", ["cosine", "multistep"])
def test_build_schedulers_equals_the_reference(kind):
    from brainfm_amd import models as M
    d = load_npz("optim.npz")
    n_epochs, itr, warm, lr, min_lr, wd0, wd1, gamma = d["sched_args"]
    ta = SimpleNamespace(lr_scheduler=kind, n_epochs=int(n_epochs), warmup_epochs=int(warm),
                         lr_drops=[int(v) for v in d["sched_lr_drops"]], lr_drop_multi=float(gamma), weight_decay=float(wd0),
                         weight_decay_end=float(wd1))
    a, b = M.build_schedulers(ta, int(itr), float(lr), float(min_lr))
    assert np.array_equal(a, d["sched_%s_lr" % kind]) and np.array_equal(b, d["sched_%s_wd" % kind])
    assert len(a) == len(b) == int(n_epochs) * int(itr) and abs(b[0] - float(wd0)) <= 1e-15 and b[-1] < float(wd1)


def test_build_optimizer_spec_defaults_and_unknown_name():
    from brainfm_amd import _lib as L
    from brainfm_amd import models as M
    groups = [{"params": [torch.nn.Parameter(torch.zeros(3))]}]
    mk = lambda name: M.build_optimizer(SimpleNamespace(optimizer=name, momentum=1), groups)      # noqa: E731
    a = mk("adam")
    assert (a.kind, a.betas, a.eps) == ("adam", (0.9, 0.999), 1e-8)
    assert a.param_groups == [dict(lr=1e-3, weight_decay=0.0)]
    w = mk("adamw")
    assert (w.kind, w.betas, w.eps) == ("adamw", (0.9, 0.999), 1e-8) and w.param_groups[0]["weight_decay"] == 1e-2
    s = mk("sgd")
    assert (s.kind, s.momentum) == ("sgd", 0.9) and s.param_groups == [dict(lr=0.0, weight_decay=0.0)]   # momentum: 1 ignored
    la = mk("lars")
    assert (la.kind, la.momentum, la.eta) == ("lars", 0.9, 1e-3) and la.param_groups == [dict(lr=0.0, weight_decay=0.0)]
    # the loop of Trainer/engine.py:95-97 writes into the group
    for g in la.param_groups:
        g["lr"], g["weight_decay"] = 0.2, 0.04
    assert la.param_groups[0] == dict(lr=0.2, weight_decay=0.04)
    with pytest.raises(ValueError, match="rmsprop"):
        mk("rmsprop")
    for bad in (dict(amsgrad=True), dict(nesterov=True), dict(dampening=0.1), dict(weight_decay_filter=lambda p: True),
                dict(lars_adaptation_filter=lambda p: True)):
        with pytest.raises(L.BfmError, match=next(iter(bad))):
            M.OptimizerSpec("lars", **bad)
    assert M.OptimizerSpec("sgd", nesterov=False, dampening=0).kind == "sgd"


def _fake_step(optimizer, lr=1e-3, wd=0.1):
    """A TrainStep with a CPU parameter table: one conv layer, one head (its weight is 5-D in the reference)."""
    from brainfm_amd import train as TR
    g_ = torch.Generator().manual_seed(1)
    ly = SimpleNamespace(name="backbone.encoders.0.basic_module.SingleConv1", gamma=torch.randn(4, generator=g_),
                         beta=torch.randn(4, generator=g_), w_raw=torch.randn(4, 1, 3, 3, 3, generator=g_))
    eng = SimpleNamespace(lib=None, device=torch.device("cpu"), enc=[[ly]], dec=[])
    step = TR.TrainStep.__new__(TR.TrainStep)
    step.tail = SimpleNamespace(row_of={"T1": (0, 1), "T2": (1, 1)}, head_w=torch.randn(2, 4, generator=g_),
                                head_b=torch.randn(2, generator=g_))
    step._init_optim(eng, ["T1"], {"loss_T1": 1.0}, lr, wd, (0.9, 0.999), 1e-8, 0.0, None, optimizer)
    params = step.parameters()
    for k, p in params.items():
        if "T2" in k:
            continue                                       # a head no loss reached: no state
        step.state[k] = tuple(torch.randn(p.numel(), generator=g_) for _ in TR._STATE_KEYS[step.opt_kind])
        step.steps[k] = 1
    step.t = 1
    return step, params


def _torch_twin(step, params, make):
    ps = [torch.nn.Parameter(p.detach().reshape(step._ref_shape(k, p)).clone()) for k, p in params.items()]
    opt = make(ps)
    for k, p in zip(params, ps):
        if "T2" not in k:
            p.grad = torch.ones_like(p)
    opt.step()
    return ps, opt


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_optimizer_state_dict_has_the_installed_torch_layout(kind):
    step, params = _fake_step(kind)
    make = (lambda ps: torch.optim.Adam(ps)) if kind == "adam" else (lambda ps: torch.optim.SGD(ps, lr=0, momentum=0.9))
    ps, opt = _torch_twin(step, params, make)
    ref, got = opt.state_dict(), step.optimizer_state_dict()
    assert set(got.keys()) == set(ref.keys())
    assert set(got["state"].keys()) == set(ref["state"].keys())          # the untouched head has no entry in either
    for i in ref["state"]:
        assert set(got["state"][i].keys()) == set(ref["state"][i].keys()), i
        for k_, v in ref["state"][i].items():
            assert tuple(got["state"][i][k_].shape) == tuple(v.shape), (i, k_)
    assert len(got["param_groups"]) == 1
    assert set(got["param_groups"][0].keys()) == set(ref["param_groups"][0].keys())
    assert got["param_groups"][0]["params"] == ref["param_groups"][0]["params"]
    assert got["param_groups"][0]["lr"] == 1e-3 and got["param_groups"][0]["weight_decay"] == 0.1
    opt2 = make([torch.nn.Parameter(p.detach().clone()) for p in ps])
    opt2.load_state_dict(got)                                            # torch takes it


def test_lars_state_dict_layout_and_spec_hyperparameters():
    from brainfm_amd import models as M
    spec = M.OptimizerSpec("lars", eta=2e-3)
    spec.param_groups[0].update(lr=0.2, weight_decay=0.04)
    step, params = _fake_step(spec)
    assert step.opt_kind == "lars" and step.eta == 2e-3 and step._hyper() == (0.2, 0.04) and step._hyper(0.1, 0.0) == (0.1, 0.0)
    got = step.optimizer_state_dict()
    names = list(params)
    assert set(got["param_groups"][0].keys()) == {"lr", "weight_decay", "momentum", "eta", "weight_decay_filter",
                                                  "lars_adaptation_filter", "params"}
    assert got["param_groups"][0]["lr"] == 0.2 and got["param_groups"][0]["eta"] == 2e-3
    assert set(got["state"].keys()) == {i for i, k in enumerate(names) if "T2" not in k}
    for i, st in got["state"].items():
        assert set(st.keys()) == {"mu"} and tuple(st["mu"].shape) == step._ref_shape(names[i], params[names[i]])
    assert got["state"][names.index("head.final_conv_T1.weight")]["mu"].dim() == 5


def test_adamw_state_dict_is_unchanged_by_the_optimizer_argument():
    a, _ = _fake_step("adamw")
    from brainfm_amd import train as TR
    assert a.opt_kind == "adamw" and inspect.signature(TR.TrainStep.__init__).parameters["optimizer"].default == "adamw"
    assert inspect.signature(TR.ContrastiveStep.__init__).parameters["optimizer"].default == "adamw"
    got = a.optimizer_state_dict()
    assert set(got["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"}
    with pytest.raises(ValueError):
        _fake_step("rmsprop")


def _save(tmp_path, step, **extra):
    path = str(tmp_path / ("ckp_%s.pth" % step.opt_kind))
    ckp = {"model": step.state_dict(), "optimizer": step.optimizer_state_dict(), "epoch": 0}
    ckp.update(extra)
    torch.save(ckp, path)
    return path


def test_load_checkpoint_refuses_another_optimizers_state(tmp_path, monkeypatch):
    """By 'optimizer_kind', or by the state keys for a file the reference wrote; nothing is loaded as something else."""
    from brainfm_amd import _lib as L
    from brainfm_amd import train as TR
    monkeypatch.setattr(TR.TrainStep, "_weights_changed", lambda self: None)
    steps = {k: _fake_step(k)[0] for k in ("adam", "adamw", "sgd", "lars")}
    for src in steps:
        for with_kind in (True, False):
            path = _save(tmp_path, steps[src], **({"optimizer_kind": src} if with_kind else {}))
            for dst in steps:
                fresh, _ = _fake_step(dst)
                fresh.state = {}
                # without the kind an Adam file and an AdamW file look alike (the reference writes neither's name)
                ok = src == dst or (not with_kind and {src, dst} == {"adam", "adamw"})
                if ok:
                    fresh.load_checkpoint(path)
                    k0 = next(iter(steps[src].state))
                    assert all(torch.equal(a, b) for a, b in zip(fresh.state[k0], steps[src].state[k0]))
                    assert "head.final_conv_T2.weight" not in fresh.state
                else:
                    with pytest.raises(L.BfmError, match=dst) as e:
                        fresh.load_checkpoint(path)
                    assert (src in str(e.value)) or (not with_kind and src == "adam" and "adamw" in str(e.value))
                    assert fresh.state == {}
    # no optimiser state: loads as before
    path = str(tmp_path / "bare.pth")
    torch.save({"model": steps["sgd"].state_dict()}, path)
    fresh, _ = _fake_step("lars")
    fresh.state = {}
    fresh.load_checkpoint(path)
    assert fresh.state == {}
