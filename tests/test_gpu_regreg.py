"""The registration regularisers on HIP (bfm_loss_reg_smooth / bfm_loss_reg_hessian, csrc/reg_regularisers.hip) and
TrainStep with losses.registration_smooth / registration_hessian: against tests/golden/regreg.npz (made by running the
reference, tests/golden/make_golden_regreg.py) and the NumPy restatement of tests/test_host_regreg.py.
Needs an MI355X: run with `-m gpu`."""
import numpy as np
import pytest
import torch

from conftest import load_npz, sd_from_npz
import test_host_regreg as HR

pytestmark = pytest.mark.gpu

REG = ("registration_smooth", "registration_hessian")


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _run(u, lname, layout, coef=0.75, seed=0, base=0.0):
    """One launch on a (1, 3, D, H, W) field placed in a wider head-output buffer whose dRaw holds random values, `base`
    times random values in the field's own rows.  Returns (loss, d/du, untouched, (loss, dRaw) as the device gave them)."""
    from brainfm_amd import _lib as L
    lib = L.load()
    nch, (D, H, W) = u.shape[1], u.shape[2:]
    nvox = D * H * W
    n_out, c0 = 7, 2
    g = torch.Generator().manual_seed(seed)
    if layout == "rows":
        pitch = nvox + 5
        raw = torch.randn((n_out, pitch), generator=g)
        raw[c0:c0 + nch, :nvox] = torch.from_numpy(u.reshape(nch, nvox))
        off, cs, vs = c0 * pitch, pitch, 1
    else:
        raw = torch.randn((nvox, n_out), generator=g)
        raw[:, c0:c0 + nch] = torch.from_numpy(u.reshape(nch, nvox)).t()
        off, cs, vs = c0, 1, n_out
    d0 = torch.randn(raw.shape, generator=g)                  # the kernels ADD into dRaw
    if layout == "rows":
        d0[c0:c0 + nch] *= base
    else:
        d0[:, c0:c0 + nch] *= base
    raw_d, dRaw = raw.to(_dev()), d0.to(_dev())
    out = torch.zeros(1, dtype=torch.float64, device=_dev())
    ws = torch.empty(lib.bfm_loss_reg_workspace(nch, D, H, W), dtype=torch.uint8, device=_dev())
    fn = lib.bfm_loss_reg_smooth if lname == "smooth" else lib.bfm_loss_reg_hessian
    L.check(fn(L.ptr(raw_d), off, cs, vs, nch, D, H, W, coef, L.ptr(dRaw), L.ptr(out), L.ptr(ws), ws.numel(),
               L.stream_ptr()), lname)
    torch.cuda.synchronize()
    dr = dRaw.cpu()
    delta = (dr.double() - d0.double())
    if layout == "rows":
        grad = delta[c0:c0 + nch, :nvox].numpy()
        mask = torch.ones(raw.shape, dtype=torch.bool)
        mask[c0:c0 + nch, :nvox] = False
    else:
        grad = delta[:, c0:c0 + nch].t().numpy()
        mask = torch.ones(raw.shape, dtype=torch.bool)
        mask[:, c0:c0 + nch] = False
    untouched = torch.equal(dr[mask], d0[mask])
    return float(out.item()), grad.reshape(u.shape) / coef, untouched, (out.cpu(), dr)


@pytest.mark.parametrize("layout", ["rows", "cl"])
@pytest.mark.parametrize("lname", ["smooth", "hessian"])
def test_kernels_vs_reference_golden(lname, layout):
    """Value to 1e-6 relative and d/du to 1e-5 of its max-norm, against the reference in float64 on the same fp32 field."""
    d = load_npz("regreg.npz")
    for case in ("rand", "slab"):
        u = d["unit/%s/u" % case]
        val, grad, untouched, _ = _run(u, lname, layout)
        ref = float(d["unit/%s/%s" % (case, lname)])
        rg = d["unit/%s/%s_grad" % (case, lname)].astype(np.float64)
        assert abs(val - ref) <= 1e-6 * abs(ref), (case, val, ref)
        err = np.abs(grad - rg).max() / np.abs(rg).max()
        assert err <= 1e-5, (case, err)
        assert untouched, "a launch wrote outside the registration columns"


@pytest.mark.parametrize("dims", [(37, 45, 70), (2, 3, 33), (1, 9, 64), (5, 1, 1)])
def test_kernels_vs_float64_on_tiled_shapes(dims):
    """Several tiles, partial tiles and one- or two-voxel axes, against the NumPy restatement in float64."""
    rs = np.random.RandomState(sum(dims))
    u = rs.randn(1, 3, *dims).astype(np.float32)
    for lname, fn in (("smooth", HR.smooth), ("hessian", HR.hessian)):
        ref, rg = fn(u.astype(np.float64))
        for layout in ("rows", "cl"):
            val, grad, untouched, _ = _run(u, lname, layout, coef=1.25)
            assert abs(val - ref) <= 1e-6 * max(abs(ref), 1e-30), (lname, layout, val, ref)
            scale = np.abs(rg).max()
            assert np.abs(grad - rg).max() <= 1e-5 * max(scale, 1e-30), (lname, layout)
            assert untouched


def test_kernels_give_the_same_bits_twice_and_add_into_dRaw():
    rs = np.random.RandomState(7)
    u = (rs.randn(1, 3, 40, 48, 56) * 3).astype(np.float32)
    for lname in ("smooth", "hessian"):
        for layout in ("rows", "cl"):
            _, g0, _, (o1, d1) = _run(u, lname, layout)
            _, _, _, (o2, d2) = _run(u, lname, layout)
            assert torch.equal(o1, o2) and torch.equal(d1, d2), (lname, layout)
            # on top of what dRaw holds: the same gradient to the rounding of that sum
            scale = float(np.abs(g0).max()) * 0.75
            _, g1, _, _ = _run(u, lname, layout, base=scale)
            assert np.abs(g1 - g0).max() * 0.75 <= 1e-6 * 5 * scale, (lname, layout)


def _case():
    d = load_npz("regreg.npz")
    hyper = d["hyper"]
    return dict(d=d, f_maps=int(d["cfg"][0]), levels=int(d["cfg"][1]), groups=int(d["cfg"][2]),
                names=[str(s) for s in d["param_names"]], lr=float(hyper[0]), wd=float(hyper[1]), clip=float(hyper[2]),
                b1=float(hyper[3]), b2=float(hyper[4]), eps=float(hyper[5]), all_samples=float(hyper[6]),
                loss_names=[str(s) for s in d["loss_names"]],
                loss_weights={str(k): float(v) for k, v in zip(d["loss_weight_names"], d["loss_weights"])})


def _build(c, loss_names=None):
    from brainfm_amd import test_utils as TU
    from brainfm_amd import train as TR
    d = c["d"]
    ga, ta = TU.default_inference_args(f_maps=c["f_maps"], num_levels=c["levels"], num_groups=c["groups"],
                                       tasks=dict(registration=True))
    s = TU.InferenceSession(ga, ta, _dev(), state_dict=sd_from_npz(d), passes=3)
    names = c["loss_names"] if loss_names is None else loss_names
    step = TR.TrainStep(s.engine, s.model.head.tail(s.engine), names, c["loss_weights"], d["weights_ce"], c["all_samples"],
                        lr=c["lr"], weight_decay=c["wd"], betas=(c["b1"], c["b2"]), eps=c["eps"], clip_max_norm=c["clip"])
    target = {k[7:]: torch.from_numpy(v) for k, v in d.items() if k.startswith("target/")}
    n = sum(1 for k in d if k.startswith("x") and k[1:].isdigit())
    xs = [torch.from_numpy(d["x%d" % i]) for i in range(n)]
    return step, xs, target, [{} for _ in range(n)]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


def test_training_iteration_vs_reference_golden():
    """registration + registration_grad + both regularisers, two samples, a 3-level net: loss dictionary, every gradient,
    the clipping norms and one AdamW step, at the tolerances of test_gpu_train.py."""
    from oracle import train_ref as T
    c = _case()
    d = c["d"]
    assert c["loss_names"] == ["registration", "registration_grad"] + list(REG)
    step, xs, target, samples = _build(c)
    loss_dict, total, grads = step.loss_and_grads(xs, target, samples)
    assert list(loss_dict.keys()) == ["loss_" + n for n in c["loss_names"]]
    for k, v in loss_dict.items():
        ref = float(d["loss/" + k])
        assert abs(v - ref) <= 1e-4 * max(abs(ref), 1e-3), (k, v, ref)
    assert abs(total - float(d["loss_total"])) <= 1e-4 * float(d["loss_total"])
    assert set(grads.keys()) == set(c["names"])
    worst = {k: _rel(grads[k].reshape(d["grad/" + k].shape).cpu().numpy(), d["grad/" + k]) for k in c["names"]}
    print("max rel grad err vs reference fp64: %.2e (%s)" % (max(worst.values()), max(worst, key=worst.get)))
    bad = {k: v for k, v in worst.items() if v > 2e-3}
    assert not bad, bad
    before = {k: v.clone() for k, v in step.parameters().items()}
    mine = {k: grads[k].double().cpu() for k in c["names"]}
    stepped, norms = step.apply(grads)
    assert stepped and step.t == 1
    assert np.allclose(norms, d["clip_norms"], rtol=2e-3, atol=1e-7)
    after = step.parameters()
    clipped, _ = T.clip_gradients(mine, c["clip"])
    ref_clipped, _ = T.clip_gradients({k: torch.from_numpy(d["grad/" + k]).double() for k in c["names"]}, c["clip"])
    for k in c["names"]:
        p0 = before[k].double().cpu()
        if ("delta/" + k) in d:
            ref_delta = d["delta/" + k].astype(np.float64)
            got_delta = (after[k].double() - before[k].double()).reshape(ref_delta.shape).cpu().numpy()
            well = np.abs(ref_clipped[k].numpy()) > 1e-6
            assert np.abs(got_delta - ref_delta)[well].max(initial=0.0) <= 2e-2 * c["lr"], k
        p1, _, _ = T.adamw_step(p0, clipped[k].reshape(p0.shape), torch.zeros_like(p0), torch.zeros_like(p0), 1, c["lr"],
                                c["b1"], c["b2"], c["eps"], c["wd"])
        assert float((after[k].double().cpu() - p1).abs().max()) <= 2e-3 * c["lr"] + 2e-7 * float(p0.abs().max()), k


def test_switches_leave_the_other_losses_alone_and_repeat_bitwise():
    """With the switches off the step is the one without them (the builder's list, no extra launch); with them on the other
    losses' values keep their bits, and two runs give the same bits."""
    from types import SimpleNamespace as NS
    from brainfm_amd import train as TR
    c = _case()
    w = NS(**{k[5:]: v for k, v in c["loss_weights"].items()})
    ta = NS(losses=NS(registration_grad=True), weights=w)
    off_names, _ = TR.criterion_losses(ta, ["registration"])
    assert off_names == ["registration", "registration_grad"]
    a, xs, target, samples = _build(c, off_names)
    la, ta_, ga = a.loss_and_grads(xs, target, samples)
    assert list(la) == ["loss_registration", "loss_registration_grad"]
    b, _, _, _ = _build(c)
    lb, tb, gb = b.loss_and_grads(xs, target, samples)
    lb2, tb2, gb2 = b.loss_and_grads(xs, target, samples)
    for k in la:
        assert la[k] == lb[k], k                             # the regularisers only add into dRaw after those values
    assert lb == lb2 and tb == tb2
    assert all(torch.equal(gb[k], gb2[k]) for k in gb)
    assert any(not torch.equal(ga[k], gb[k]) for k in ga)
    a2, _, _, _ = _build(c, off_names)
    la2, _, ga2 = a2.loss_and_grads(xs, target, samples)
    assert la2 == la and all(torch.equal(ga[k], ga2[k]) for k in ga)


def test_regularisers_need_the_registration_head():
    from brainfm_amd import _lib as L
    from brainfm_amd import test_utils as TU
    from brainfm_amd import train as TR
    from oracle import unet_ref as O
    ga, ta = TU.default_inference_args(f_maps=8, num_levels=2, tasks=dict(T1=True))
    s = TU.InferenceSession(ga, ta, _dev(), state_dict=O.random_state_dict(1, 8, 2, seed=1,
                                                                               out_channels={"T1": 1}))
    with pytest.raises(L.BfmError, match="registration head"):
        TR.TrainStep(s.engine, s.model.head.tail(s.engine), ["T1", "registration_hessian"], {"loss_T1": 1.0},
                     torch.ones(1), 1.0)
