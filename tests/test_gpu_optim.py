"""The AdamW, Adam, SGD and LARS training steps on the HIP kernels (brainfm_amd/csrc/optim.hip): the multi-tensor kernels
through the C ABI against the float64 restatements of tests/optim_refs.py, TrainStep(optimizer=...) on the golden iteration
of tests/golden/train_step.npz, and the checkpoints of each kind.  Needs an MI355X: run with `-m gpu`."""
import math

import numpy as np
import pytest
import torch

import optim_refs as R
from conftest import sd_from_npz
from test_oracle_train import load_case

pytestmark = pytest.mark.gpu

CH = 65536
SIZES = (1, 3, 4, 5, 4099, 65535, 65536, 65537, 131073)
KINDS = ("adamw", "adam", "sgd", "lars")
GRAD_SCALE, WD = 0.5, 0.1
LR = {"adamw": 3e-3, "adam": 3e-3, "sgd": 3e-3, "lars": 0.3}
B1, B2, EPS, MOM, ETA = 0.9, 0.999, 1e-8, 0.9, 1e-3


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _tensor_list(kind):
    """[(name, shape the reference sees, start values (CPU fp32), per-tensor wd, zero gradient?)].  'view' becomes a view at
    an odd float offset of a larger buffer: its length is a multiple of 4, so only the alignment sends it down the scalar
    path."""
    g_ = torch.Generator().manual_seed(17)
    out = [("n%d" % n, (n, 1), torch.randn(n, generator=g_), WD, False) for n in SIZES]
    out.append(("view", (256, 4), torch.randn(1024, generator=g_), WD, False))
    if kind == "lars":
        out.append(("mat", (73, 137), torch.randn(73 * 137, generator=g_), WD, False))
        out.append(("vec", (41,), torch.randn(41, generator=g_), WD, False))                 # 1-D: no decay, no q
        out.append(("zero_p", (5, 7), torch.zeros(35), WD, False))                          # |p| = 0: q = 1
        out.append(("zero_g", (6, 6), torch.randn(36, generator=g_), 0.0, True))             # |dp| = 0: q = 1
    return out


def _grads(tensors, t):
    g_ = torch.Generator().manual_seed(100 + t)
    return [torch.zeros(p.numel()) if zg else torch.randn(p.numel(), generator=g_) * 10.0 ** (t - 3)
            for _, _, p, _, zg in tensors]


def _run_kernels(kind, tensors):
    """Three steps of `kind` on the device.  Returns (parameters, state buffers, what the kind's measuring launch gave at step
    1: [n][3] of bfm_lars_sums_multi for LARS, [n] of bfm_grad_sumsq_multi for the rest) as CPU tensors."""
    from brainfm_amd import _lib as L
    from brainfm_amd import train as TR
    lib, dev = L.load(), _dev()
    two = kind in ("adam", "adamw")
    big_p, big_g = torch.zeros(1024 + 8, device=dev), torch.zeros(1024 + 8, device=dev)
    ps, gs, s0, s1 = [], [], [], []
    for name, _, p0, _, _ in tensors:
        if name == "view":
            big_p[1:1025] = p0.to(dev)
            ps.append(big_p[1:1025])
            gs.append(big_g[1:1025])
            assert ps[-1].data_ptr() % 16 == 4 and gs[-1].data_ptr() % 16 == 4
        else:
            ps.append(p0.clone().to(dev))
            gs.append(torch.zeros(p0.numel(), device=dev))
        s0.append(torch.zeros(p0.numel(), device=dev))
        s1.append(torch.zeros(p0.numel(), device=dev) if two else None)
        assert s0[-1].data_ptr() % 16 == 0
    desc = np.zeros(len(tensors), dtype=TR._OPT_DESC)
    cmap, first = [], 0
    for i, p in enumerate(ps):
        n = p.numel()
        desc[i] = (p.data_ptr(), gs[i].data_ptr(), s0[i].data_ptr(), s1[i].data_ptr() if two else 0, n, GRAD_SCALE, 1.0, 1.0,
                   first, 1.0, 0.0)
        nch = (n + CH - 1) // CH
        cmap += [i] * nch
        first += nch
    cmap_d = torch.tensor(cmap, dtype=torch.int32, device=dev)
    sums_first = None
    for t in (1, 2, 3):
        for g_dev, g in zip(gs, _grads(tensors, t)):
            g_dev.copy_(g.to(dev))
        if two:
            desc["bias1"] = np.float32(1.0) - np.power(np.float32(B1), np.float32(t), dtype=np.float32)
            desc["bias2_sqrt"] = np.sqrt(np.float32(1.0) - np.power(np.float32(B2), np.float32(t), dtype=np.float32))
        tdev = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(dev)
        head = (L.ptr(tdev), len(tensors), L.ptr(cmap_d), len(cmap), CH)
        if kind == "lars":
            sums = torch.zeros(3 * len(tensors), dtype=torch.float64, device=dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            ws = torch.empty(3 * len(cmap), dtype=torch.float64, device=dev)
            L.check(lib.bfm_lars_sums_multi(*head, L.ptr(sums), L.ptr(flag), L.ptr(ws), ws.numel() * 8, L.stream_ptr()), "sums")
            assert int(flag.item()) == 0
            sums = sums.cpu().reshape(-1, 3)
            if t == 1:
                sums_first = sums.clone()
            for i, (_, shape, _, wd, _) in enumerate(tensors):
                if len(shape) != 1:
                    desc[i]["wd"] = wd
                    desc[i]["q"] = TR.lars_trust_ratio(*(float(v) for v in sums[i]), float(np.float32(GRAD_SCALE)),
                                                       float(np.float32(wd)), ETA)
            tdev = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(dev)
            head = (L.ptr(tdev),) + head[1:]
            rc = lib.bfm_lars_step_multi(*head, LR[kind], MOM, L.stream_ptr())
        else:
            if t == 1:
                sums = torch.zeros(len(tensors), dtype=torch.float64, device=dev)
                flag = torch.zeros(1, dtype=torch.int32, device=dev)
                ws = torch.empty(len(cmap), dtype=torch.float64, device=dev)
                L.check(lib.bfm_grad_sumsq_multi(*head, L.ptr(sums), L.ptr(flag), L.ptr(ws), ws.numel() * 8, L.stream_ptr()),
                        "sumsq")
                assert int(flag.item()) == 0
                sums_first = sums.cpu()
            if kind == "sgd":
                rc = lib.bfm_sgd_step_multi(*head, LR[kind], MOM, WD, L.stream_ptr())
            elif kind == "adam":
                rc = lib.bfm_adam_step_multi(*head, LR[kind], B1, B2, EPS, WD, L.stream_ptr())
            else:
                rc = lib.bfm_adamw_step_multi(*head, LR[kind], B1, B2, EPS, WD, L.stream_ptr())
        L.check(rc, kind)
        torch.cuda.synchronize()
    assert float(big_p[0]) == 0.0 and float(big_p[1025:].abs().max()) == 0.0          # nothing written beside the view
    return [p.cpu().clone() for p in ps], [(a.cpu(), b.cpu() if two else None) for a, b in zip(s0, s1)], sums_first


def _run_refs(kind, tensors):
    """[(p, s0, s1)] in float64.  AdamW's kernel forms 1 - beta2 in float32, 1.3e-5 below the exact value (optim_one says why
    it stays so), and its exp_avg_sq is low by that share: far past 2e-6.  So that row alone, bf, comes from a second float64
    chain that is given the float-rounded 1 - beta2; parameters and exp_avg are held to the exact chain."""
    omb2 = float(np.float32(1.0) - np.float32(B2))
    out = []
    for i, (_, shape, p0, wd, _) in enumerate(tensors):
        p = p0.double()
        a, b = torch.zeros_like(p), torch.zeros_like(p)
        pf, af, bf = p, a, b
        for t in (1, 2, 3):
            g = _grads(tensors, t)[i].double()
            if kind == "adamw":
                p, a, b = R.adamw_step(p, g, a, b, t, LR[kind], B1, B2, EPS, wd, GRAD_SCALE)
                pf, af, bf = R.adamw_step(pf, g, af, bf, t, LR[kind], B1, B2, EPS, wd, GRAD_SCALE, one_minus_beta2=omb2)
            elif kind == "adam":
                p, a, b = R.adam_step(p, g, a, b, t, LR[kind], B1, B2, EPS, wd, GRAD_SCALE)
            elif kind == "sgd":
                p, a = R.sgd_step(p, g, a, LR[kind], MOM, wd, GRAD_SCALE)
            else:
                p, a = R.lars_step(p, g, a, LR[kind], wd, MOM, ETA, ndim=len(shape), grad_scale=GRAD_SCALE)
        out.append((p, a, bf if kind == "adamw" else b))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_multi_tensor_kernels_vs_float64_and_bit_repeatable(kind):
    """Three steps over tensors chosen to break chunking (1 .. 2 chunks + 1 element) and alignment (a view at an odd float
    offset), for LARS also the ndim rule and both q = 1 cases.  torch's own fp32 optimisers sit at 2.4e-7 .. 3.4e-7 from
    float64 on these inputs, so 2e-6 leaves about 6x."""
    tensors = _tensor_list(kind)
    got_p, got_s, sums = _run_kernels(kind, tensors)
    refs = _run_refs(kind, tensors)
    for (name, _, p0, _, _), p, (a, b), (rp, ra, rb) in zip(tensors, got_p, got_s, refs):
        err_p = float((p.double() - rp).abs().max())
        err_a = float((a.double() - ra).abs().max())
        print("%s %-7s |dp| %.2e  state %.2e of %.2e" % (kind, name, err_p, err_a, float(ra.abs().max())))
        assert err_p <= 2e-6, (name, err_p)
        assert err_a <= 2e-6 * float(ra.abs().max()), (name, err_a)
        if b is not None:
            assert float((b.double() - rb).abs().max()) <= 2e-6 * float(rb.abs().max()), name
        if name != "zero_g":                                                             # (no update at all there)
            assert not torch.equal(p, p0), name                                          # the step did move it
    if kind == "lars":
        g1 = _grads(tensors, 1)
        for i, (name, _, p0, _, _) in enumerate(tensors):
            p, g = p0.double(), g1[i].double()
            ref = torch.stack([g @ g, p @ p, p @ g])
            assert float((sums[i] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), (name, sums[i], ref)
    again_p, again_s, _ = _run_kernels(kind, tensors)
    for name, x, y in zip((t[0] for t in tensors), got_p, again_p):
        assert torch.equal(x, y), name
    for (a, b), (a2, b2) in zip(got_s, again_s):
        assert torch.equal(a, a2) and (b is None or torch.equal(b, b2))


def test_lars_sums_flag_a_non_finite_gradient():
    from brainfm_amd import _lib as L
    from brainfm_amd import train as TR
    lib, dev = L.load(), _dev()
    p = torch.randn(CH + 7, device=dev)
    g = torch.randn(CH + 7, device=dev)
    g[CH + 3] = float("inf")
    desc = np.zeros(1, dtype=TR._OPT_DESC)
    desc[0] = (p.data_ptr(), g.data_ptr(), 0, 0, p.numel(), 1.0, 1.0, 1.0, 0, 1.0, 0.0)
    tdev = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(dev)
    cmap = torch.zeros(2, dtype=torch.int32, device=dev)
    sums = torch.zeros(3, dtype=torch.float64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(6, dtype=torch.float64, device=dev)
    L.check(lib.bfm_lars_sums_multi(L.ptr(tdev), 1, L.ptr(cmap), 2, CH, L.ptr(sums), L.ptr(flag), L.ptr(ws), 48,
                                    L.stream_ptr()), "sums")
    assert int(flag.item()) == 1 and math.isfinite(float(sums[1]))
    assert lib.bfm_lars_sums_multi(L.ptr(tdev), 1, L.ptr(cmap), 2, CH, L.ptr(sums), L.ptr(flag), L.ptr(ws), 40,
                                   L.stream_ptr()) == -3                                  # BFM_E_WORKSPACE


# ---------------------------------------------------------------------------------------------- TrainStep
STEP_LR = {"adam": None, "adamw": None, "sgd": 0.05, "lars": 1.0}        # None: the fixture's (1e-3)


def _build(c, optimizer="adamw", scaler=None, default=False):
    """tests/test_gpu_train.py::_build with optimizer= (default=True: the argument is left out)."""
    from brainfm_amd import test_utils as TU
    from brainfm_amd import train as TR
    d = c["d"]
    ga, ta = TU.default_inference_args(f_maps=c["f_maps"], num_levels=c["levels"], left_hemis_only=True,
                                       num_groups=c["groups"])
    s = TU.InferenceSession(ga, ta, _dev(), state_dict=sd_from_npz(d), passes=3)
    kw = {} if default else {"optimizer": optimizer}
    kind = optimizer if isinstance(optimizer, str) else optimizer.kind
    step = TR.TrainStep(s.engine, s.model.head.tail(s.engine), c["loss_names"], c["loss_weights"], d["weights_ce"], c["all_samples"],
                        max_surf_distance=c["max_dist"], bias_field_log_type="l2" if c["bias_l2"] else "l1",
                        lr=STEP_LR[kind] or c["lr"], weight_decay=c["wd"], betas=(c["b1"], c["b2"]), eps=c["eps"],
                        clip_max_norm=c["clip"], scaler=scaler, **kw)
    target = {k[7:]: torch.from_numpy(v) for k, v in d.items() if k.startswith("target/")}
    xs = [torch.from_numpy(d["x%d" % i]) for i in range(c["n_samples"])]
    samples = [{"bias_field_log": torch.from_numpy(d["bias_field_log%d" % i]),
                "high_res_residual": torch.from_numpy(d["high_res_residual%d" % i])} for i in range(c["n_samples"])]
    return step, xs, target, samples


@pytest.mark.parametrize("kind", KINDS)
def test_train_step_applies_each_optimizer_like_the_float64_ref(kind):
    """loss_and_grads, then apply: every parameter against optim_refs in float64 on the gradients this path returned, with
    the unscale and the per-parameter clip coefficient of the reference.  A head no loss reached keeps its values and gets
    no state; an inf in one gradient skips the step, leaves parameters and buffers bit-identical and halves the scale; the
    next forward sees the new weights."""
    from brainfm_amd import train as TR
    c = load_case()
    scale = 1024.0
    step, xs, target, samples = _build(c, kind, scaler=TR.LossScaler(init_scale=scale, growth_interval=1000))
    lr, wd = STEP_LR[kind] or c["lr"], c["wd"]
    assert step.opt_kind == kind
    loss_dict, total, grads = step.loss_and_grads(xs, target, samples)
    skipped = ("head.final_conv_T2.weight", "head.final_conv_T2.bias")
    for k in skipped:
        grads.pop(k)
    before = {k: v.clone() for k, v in step.parameters().items()}
    mine = {k: v.double().cpu() for k, v in grads.items()}
    stepped, norms = step.apply(grads)
    assert stepped and step.t == 1 and step.scaler.scale == scale
    after = step.parameters()
    moved = 0.0
    for k, p_dev in before.items():
        p0 = p_dev.double().cpu()
        if k in skipped:
            assert torch.equal(after[k], p_dev) and k not in step.state and k not in step.steps
            continue
        assert len(step.state[k]) == (2 if kind in ("adam", "adamw") else 1)
        g = mine[k].reshape(p0.shape)
        coef = R.clip_coef(g, c["clip"], 1.0 / scale) / scale
        z = torch.zeros_like(p0)
        if kind in ("adam", "adamw"):
            ref_step = R.adam_step if kind == "adam" else R.adamw_step
            p1 = ref_step(p0, g, z, z, 1, lr, c["b1"], c["b2"], c["eps"], wd, coef)[0]
            bound = 2e-3 * lr + 2e-7 * float(p0.abs().max())
        elif kind == "sgd":
            p1 = R.sgd_step(p0, g, z, lr, 0.9, wd, coef)[0]
        else:
            p1 = R.lars_step(p0, g, z, lr, wd, 0.9, 1e-3, ndim=len(step._ref_shape(k, p_dev)), grad_scale=coef)[0]
        delta = float((p1 - p0).abs().max())
        if kind in ("sgd", "lars"):
            bound = 2e-7 * float(p0.abs().max()) + 1e-5 * delta
            moved = max(moved, delta / (2e-7 * float(p0.abs().max())))
        err = float((after[k].double().cpu() - p1).abs().max())
        assert err <= bound, (k, err, bound, delta)
    if kind in ("sgd", "lars"):
        assert moved > 100.0, moved                        # the updates are far above the rounding the bound allows
    _, total2, grads2 = step.loss_and_grads(xs, target, samples)
    assert total2 != total                                 # the next forward sees the new weights
    k = "backbone.decoders.1.basic_module.SingleConv2.conv.weight"
    grads2[k][0, 0, 0, 0, 0] = float("inf")
    snap_p = {n: v.clone() for n, v in step.parameters().items()}
    snap_s = {n: tuple(b.clone() for b in bufs) for n, bufs in step.state.items()}
    stepped, _ = step.apply(grads2)
    assert not stepped and step.scaler.scale == scale / 2 and step.t == 1
    for n, v in step.parameters().items():
        assert torch.equal(v, snap_p[n]), n
    for n, bufs in snap_s.items():
        assert all(torch.equal(a, b) for a, b in zip(step.state[n], bufs)), n


@pytest.mark.parametrize("kind", KINDS)
def test_checkpoint_of_each_optimizer_resumes_bit_identically(kind, tmp_path):
    """Save after one step; a fresh session that loads the file continues exactly like the one that kept running, torch's
    own Adam / SGD take the optimiser part, and the file names its kind."""
    from brainfm_amd import _lib as L
    c = load_case()
    a, xs, target, samples = _build(c, kind)
    _, _, ok = a.step(xs, target, samples)
    assert ok
    path = str(tmp_path / ("ckp_%s.pth" % kind))
    a.save_checkpoint(path, epoch=1)
    ckp = torch.load(path, map_location="cpu", weights_only=False)
    assert ckp["optimizer_kind"] == kind
    ps = [torch.nn.Parameter(v.clone()) for v in ckp["model"].values()]
    if kind in ("adam", "adamw"):
        opt = torch.optim.Adam(ps) if kind == "adam" else torch.optim.AdamW(ps)
        opt.load_state_dict(ckp["optimizer"])
        assert float(opt.state[ps[0]]["step"]) == 1.0 and opt.state[ps[2]]["exp_avg"].shape == ps[2].shape
    elif kind == "sgd":
        opt = torch.optim.SGD(ps, lr=0, momentum=0.9)
        opt.load_state_dict(ckp["optimizer"])
        assert opt.state[ps[2]]["momentum_buffer"].shape == ps[2].shape
    else:
        assert set(ckp["optimizer"]["state"][2].keys()) == {"mu"}
    b, _, _, _ = _build(c, kind)
    b.load_checkpoint(path)
    assert b.t == 1
    _, ta, _ = a.step(xs, target, samples)
    _, tb, _ = b.step(xs, target, samples)
    assert ta == tb
    pa, pb = a.parameters(), b.parameters()
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
        assert all(torch.equal(x, y) for x, y in zip(a.state[k], b.state[k])), k
    if kind == "sgd":
        w, _, _, _ = _build(c, "adamw")
        w.step(xs, target, samples)
        wpath = str(tmp_path / "ckp_adamw.pth")
        w.save_checkpoint(wpath)
        fresh, _, _, _ = _build(c, "sgd")
        with pytest.raises(L.BfmError, match="adamw.*sgd"):
            fresh.load_checkpoint(wpath)
        assert fresh.state == {}


def test_optimizer_adamw_is_the_default_bit_for_bit():
    c = load_case()
    a, xs, target, samples = _build(c, "adamw")
    b, _, _, _ = _build(c, default=True)
    _, ta, _ = a.step(xs, target, samples)
    _, tb, _ = b.step(xs, target, samples)
    assert ta == tb and a.opt_kind == b.opt_kind == "adamw"
    pa, pb = a.parameters(), b.parameters()
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
        assert all(torch.equal(x, y) for x, y in zip(a.state[k], b.state[k])), k


def test_spec_from_build_optimizer_drives_the_step():
    """models.build_optimizer's object in place of a name: the loop writes lr / weight_decay into its param group
    (Trainer/engine.py:95-97) and step() reads them there."""
    from types import SimpleNamespace
    from brainfm_amd import models as M
    c = load_case()
    spec = M.build_optimizer(SimpleNamespace(optimizer="sgd", momentum=1), [{"params": []}])
    a, xs, target, samples = _build(c, spec)
    b, _, _, _ = _build(c, "sgd")
    for g in spec.param_groups:
        g["lr"], g["weight_decay"] = 0.02, 0.01
    a.step(xs, target, samples)
    b.step(xs, target, samples, lr=0.02, weight_decay=0.01)
    pa, pb = a.parameters(), b.parameters()
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    assert a.optimizer_state_dict()["param_groups"][0]["lr"] == 0.02
