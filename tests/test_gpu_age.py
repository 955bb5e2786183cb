"""The pooled scalar (brain-age) head on the HIP kernels: inference and one training iteration against the float64 golden
vectors made by running the reference (tests/golden/make_golden_age.py), the kernels alone against torch, determinism, the
shipped 160^3 shape on two sample lanes, and the generator's age target.  Needs an MI355X: run with `-m gpu`."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import sd_from_npz

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_age.npz")


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


def _case():
    d = dict(np.load(GOLDEN))
    f_maps, levels, groups, size = (int(v) for v in d["cfg"])
    xs = [torch.from_numpy(d["xq%d" % i].astype(np.float32) / np.float32(255)) for i in range(2)]
    t1 = torch.from_numpy(d["target_T1q"].astype(np.float32) / np.float32(255))
    return d, f_maps, levels, groups, size, xs, t1


def _session(tasks, d, f_maps, levels, groups, size, sd=True):
    from brainfm_amd import test_utils as TU
    ga, ta = TU.default_inference_args(f_maps=f_maps, num_levels=levels, num_groups=groups, size=(size,) * 3, tasks=tasks)
    state = sd_from_npz(d) if sd else None
    if state is not None and "age" not in tasks:
        state = {k: v for k, v in state.items() if "_age." not in k and "pool_layers" not in k}
    return TU.InferenceSession(ga, ta, _dev(), state_dict=state, passes=3)


def test_model_age_output_vs_reference_golden():
    """model(samples) -> processors: age (B,) against the reference in float64; the dense T1 head is bitwise the output of
    the same model without the age head."""
    d, f_maps, levels, groups, size, xs, _ = _case()
    s = _session(dict(T1=True, age=True), d, f_maps, levels, groups, size)
    s0 = _session(dict(T1=True), d, f_maps, levels, groups, size)
    samples = [{"input": x.to(_dev())} for x in xs]
    outs, _ = s.model(samples)
    outs0, _ = s0.model([{"input": x.to(_dev())} for x in xs])
    for p in s.processors:
        outs = p(outs)
    for i, o in enumerate(outs):
        assert list(o.keys())[-1] == "age" and tuple(o["age"].shape) == (1,)
        got = o["age"].cpu().numpy()
        assert _rel(got, d["age_%d" % i]) <= 1e-4, (got, d["age_%d" % i])
        assert torch.equal(o["T1"], outs0[i]["T1"])
        assert _rel(o["T1"].cpu().numpy()[..., ::3, ::3, ::3], d["out_T1_%d" % i]) <= 1e-4
    # a batch of two: shape (B,), same values
    both, _ = s.model([{"input": torch.cat(xs, 0).to(_dev())}])
    assert tuple(both[0]["age"].shape) == (2,)
    assert torch.equal(both[0]["age"].abs(), torch.cat([o["age"] for o in outs]))
    # the head called on its own features gives the same raw age
    feats = s.model.backbone.get_feature(xs[0].to(_dev()))
    h = s.model.head(feats)
    assert _rel(h["age"].abs().cpu().numpy(), outs[0]["age"].cpu().numpy()) <= 1e-6
    # a spatial shape whose flatten does not give final_linear1_age's width is refused, naming both
    from brainfm_amd import _lib as L
    with pytest.raises(L.BfmError, match="108"):
        s.model([{"input": xs[0][..., :40, :, :].to(_dev())}])


def _train_step(d, f_maps, levels, groups, size, lanes=None):
    from brainfm_amd import train as TR
    s = _session(dict(T1=True, age=True), d, f_maps, levels, groups, size)
    hyper = d["hyper"]
    names = [str(n)[5:] for n in d["loss_names"]] if str(d["loss_names"][0]).startswith("loss_") else [str(n) for n in d["loss_names"]]
    wts = {str(k): float(v) for k, v in zip(d["loss_weight_names"], d["loss_weights"])}
    step = TR.TrainStep(s.engine, s.model.head.tail(s.engine), names, wts, torch.ones(1), float(hyper[5]),
                        lr=float(hyper[0]), weight_decay=float(hyper[1]), betas=(float(hyper[2]), float(hyper[3])),
                        eps=float(hyper[4]), age_head=s.model.head.age_head())
    if lanes is not None:
        step.sample_lanes = lanes
    return step


def test_training_iteration_with_age_vs_reference_golden():
    """loss_age and the total, every gradient (the backbone's carries the pooled scatter) and the parameters after
    AdamW, for two samples on either side of the target age (one with a negative raw output)."""
    d, f_maps, levels, groups, size, xs, t1 = _case()
    step = _train_step(d, f_maps, levels, groups, size)
    target = {"T1": t1, "age": torch.tensor([float(d["target_age"])], dtype=torch.float64)}
    samples = [{} for _ in xs]
    loss_dict, total, grads = step.loss_and_grads(xs, target, samples)
    assert list(loss_dict.keys()) == ["loss_" + n for n in step.loss_names]
    for k, v in loss_dict.items():
        ref = float(d["loss/" + k])
        assert abs(v - ref) <= 1e-4 * max(abs(ref), 1e-3), (k, v, ref)
    assert abs(total - float(d["loss_total"])) <= 1e-4 * float(d["loss_total"])
    names = [str(n) for n in d["param_names"]]
    assert set(grads.keys()) == set(names)
    assert [k for k in step.parameters() if k.startswith("head.")] == [k for k in names if k.startswith("head.")]
    worst = {k: _rel(grads[k].reshape(d["grad/" + k].shape).cpu().numpy(), d["grad/" + k]) for k in names}
    print("max rel grad err vs reference fp64: %.2e (%s)" % (max(worst.values()), max(worst, key=worst.get)))
    bad = {k: v for k, v in worst.items() if v > 2e-3}
    assert not bad, bad
    assert worst["head.final_linear1_age.weight"] <= 1e-4 and worst["head.pool_layers.1.main.weight"] <= 1e-4
    before = {k: v.detach().double().cpu().clone() for k, v in step.parameters().items()}
    stepped, _ = step.apply(grads)
    assert stepped
    after = step.parameters()
    lr = float(d["hyper"][0])
    # the reference's AdamW move: stored for the head; for the backbone, torch.optim.AdamW on the reference's state and
    # gradient (what make_golden_age.py ran)
    params = {k: torch.nn.Parameter(torch.from_numpy(d["sd/" + k]).double().clone()) for k in names}
    opt = torch.optim.AdamW(list(params.values()), lr=lr, weight_decay=float(d["hyper"][1]),
                            betas=(float(d["hyper"][2]), float(d["hyper"][3])), eps=float(d["hyper"][4]))
    for k in names:
        params[k].grad = torch.from_numpy(d["grad/" + k]).double()
    opt.step()
    for k in names:
        ref_delta = d["delta/" + k] if ("delta/" + k) in d else (params[k].detach().numpy() - d["sd/" + k])
        got = (after[k].double().cpu() - before[k]).reshape(ref_delta.shape).numpy()
        # step 1 of Adam moves a weight by about lr * sign(g): compared where the reference's gradient is well clear of the
        # fp32 gradient's error, so that its sign is not in doubt
        well = np.abs(d["grad/" + k]) > 1e-2 * np.abs(d["grad/" + k]).max()
        # + the fp32 rounding of the parameter itself (final_linear3_age was scaled up by the fixture)
        tol = 2e-2 * lr + 4e-7 * float(before[k].abs().max())
        assert np.abs(got - ref_delta)[well].max(initial=0.0) <= tol, k
    # checkpoint round trip under the reference names / shapes
    sd = step.state_dict()
    for k in names:
        assert tuple(sd[k].shape) == tuple(d["sd/" + k].shape), k


def test_age_kernels_vs_torch():
    """maxpool4 (values, argmax, scattered gradient: bitwise vs F.max_pool3d / its backward, with ties and a NaN), both
    ConvBlocks and the MLP (forward, data and weight gradients) against float64 torch, at C = 64."""
    import torch.nn.functional as F
    from brainfm_amd import _lib as L
    lib = L.load()
    dev = _dev()
    st = L.stream_ptr()
    g = torch.Generator().manual_seed(7)
    D, H, W, Cf = 20, 16, 24, 64
    x = torch.randn((D, H, W, Cf), generator=g)
    x[:4, :4, :4, 3] = 0.5                               # a whole window tied
    x[4:8, :4, :4, 5] = 0.25
    x[5, 1, 2, 5] = 0.75                                 # two maxima of the same value in one window
    x[6, 3, 1, 5] = 0.75
    x[8:12, 4:8, 8:12, 9] = float("nan")
    x[9, 5, 10, 9] = 10.0
    x[1, 1, 1, 11] = float("nan")
    xd = x.to(dev).contiguous()
    P = (D // 4, H // 4, W // 4)
    pooled = torch.empty(P + (Cf,), device=dev)
    arg = torch.empty(P + (Cf,), dtype=torch.uint8, device=dev)
    L.check(lib.bfm_maxpool4(L.ptr(xd), Cf, D, H, W, L.ptr(pooled), L.ptr(arg), st), "maxpool4")
    xt = xd.permute(3, 0, 1, 2).unsqueeze(0).contiguous().requires_grad_(True)
    ref, idx = F.max_pool3d(xt, 4, 4, return_indices=True)
    got = pooled.permute(3, 0, 1, 2).unsqueeze(0)
    assert torch.equal(torch.nan_to_num(got, nan=123.0), torch.nan_to_num(ref.detach(), nan=123.0))
    assert torch.equal(torch.isnan(got), torch.isnan(ref.detach()))
    gp = torch.randn(ref.shape, generator=g).to(dev)
    ref.backward(gp)
    dst = torch.zeros((D, H, W, Cf), device=dev)
    gcl = gp[0].permute(1, 2, 3, 0).contiguous()
    L.check(lib.bfm_maxpool4_bwd(L.ptr(gcl), L.ptr(arg), Cf, D, H, W, L.ptr(dst), 1, st), "maxpool4 scatter")
    assert torch.equal(dst, xt.grad[0].permute(1, 2, 3, 0))
    dst2 = torch.full((D, H, W, Cf), 7.0, device=dev)
    L.check(lib.bfm_maxpool4_bwd(L.ptr(gcl), L.ptr(arg), Cf, D, H, W, L.ptr(dst2), 0, st), "maxpool4 gather")
    assert torch.equal(dst2, xt.grad[0].permute(1, 2, 3, 0))

    def conv_case(cin, cout, dims):
        xx = torch.randn(dims + (cin,), generator=g)
        w = torch.randn((cout, cin, 3, 3, 3), generator=g) * 0.1
        b = torch.randn(cout, generator=g) * 0.1
        dy = torch.randn(dims + (cout,), generator=g)
        xd_, wd_, bd_, dyd = (t.to(dev).contiguous() for t in (xx, w, b, dy))
        y = torch.empty(dims + (cout,), device=dev)
        L.check(lib.bfm_age_conv_fwd(L.ptr(xd_), cin, *dims, L.ptr(wd_), L.ptr(bd_), cout, L.ptr(y), st), "conv fwd")
        dx = torch.empty_like(xd_)
        dw = torch.empty_like(wd_)
        db = torch.empty_like(bd_)
        ws = torch.empty(lib.bfm_age_conv_bwd_workspace(cin, *dims, cout), dtype=torch.uint8, device=dev)
        L.check(lib.bfm_age_conv_bwd(L.ptr(xd_), cin, *dims, L.ptr(wd_), cout, L.ptr(y), L.ptr(dyd), L.ptr(dx), L.ptr(dw),
                                     L.ptr(db), L.ptr(ws), ws.numel(), st), "conv bwd")
        x64 = xx.double().permute(3, 0, 1, 2).unsqueeze(0).requires_grad_(True)
        w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
        y64 = F.leaky_relu(F.conv3d(x64, w64, b64, padding=1), 0.2)
        y64.backward(dy.double().permute(3, 0, 1, 2).unsqueeze(0))
        assert _rel(y.cpu().permute(3, 0, 1, 2).unsqueeze(0).numpy(), y64.detach().numpy()) <= 1e-5
        assert _rel(dx.cpu().numpy(), x64.grad[0].permute(1, 2, 3, 0).numpy()) <= 1e-5
        assert _rel(dw.cpu().numpy(), w64.grad.numpy()) <= 1e-5
        assert _rel(db.cpu().numpy(), b64.grad.numpy()) <= 1e-5

    conv_case(64, 16, (12, 10, 14))
    conv_case(16, 4, (5, 4, 6))

    nv = 27
    N = 4 * nv
    y2 = torch.randn((nv, 4), generator=g)
    shapes = [(160, N), (160,), (10, 160), (10,), (1, 10), (1,)]
    prm_t = [torch.randn(s, generator=g) * 0.3 for s in shapes]
    y2d = y2.to(dev)
    pd = [t.to(dev).contiguous() for t in prm_t]
    zero = torch.zeros(1, device=dev)
    prm = L.AgeParams(zero.data_ptr(), zero.data_ptr(), zero.data_ptr(), zero.data_ptr(), *[t.data_ptr() for t in pd])
    h1 = torch.empty(160, device=dev)
    h2 = torch.empty(10, device=dev)
    p = torch.empty(1, device=dev)
    L.check(lib.bfm_age_mlp_fwd(L.ptr(y2d), nv, C.byref(prm), N, L.ptr(h1), L.ptr(h2), L.ptr(p), st), "mlp fwd")
    y64 = y2.double().requires_grad_(True)
    p64 = [t.double().requires_grad_(True) for t in prm_t]
    flat = y64.t().reshape(1, -1)                       # NCDHW flatten of the (nv, 4) channels-last tensor
    a = F.relu(F.linear(flat, p64[0], p64[1]))
    bb = F.relu(F.linear(a, p64[2], p64[3]))
    out = F.linear(bb, p64[4], p64[5]).squeeze(1)
    assert _rel(p.cpu().numpy(), out.detach().numpy()) <= 1e-5
    dp = torch.tensor([0.7])
    out.backward(dp.double())
    grads = [torch.empty_like(t) for t in pd]
    gr = L.AgeGrads(zero.data_ptr(), zero.data_ptr(), zero.data_ptr(), zero.data_ptr(), *[t.data_ptr() for t in grads])
    dy2 = torch.empty_like(y2d)
    dpd = dp.to(dev)
    wsm = torch.empty(lib.bfm_age_mlp_bwd_workspace(), dtype=torch.uint8, device=dev)
    L.check(lib.bfm_age_mlp_bwd(L.ptr(y2d), nv, C.byref(prm), N, L.ptr(h1), L.ptr(h2), L.ptr(p), L.ptr(dpd), 0.0, 0.0, None,
                                C.byref(gr), L.ptr(dy2), L.ptr(wsm), wsm.numel(), st), "mlp bwd")
    assert _rel(dy2.cpu().numpy(), y64.grad.numpy()) <= 1e-5
    for t, r in zip(grads, p64):
        assert _rel(t.cpu().numpy(), r.grad.numpy()) <= 1e-5
    # N must be 4 * nv
    assert lib.bfm_age_mlp_fwd(L.ptr(y2d), nv, C.byref(prm), N + 4, L.ptr(h1), L.ptr(h2), L.ptr(p), st) == -2


def test_age_forward_backward_is_deterministic():
    """Two forward + backward passes of the head on the same inputs: the same bits everywhere."""
    from brainfm_amd import models as M
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    dims, cf = (48, 40, 44), 64
    n_flat = 4 * 3 * 2 * 2
    shapes = {"pool_layers.1.main.weight": (16, cf, 3, 3, 3), "pool_layers.1.main.bias": (16,),
              "pool_layers.3.main.weight": (4, 16, 3, 3, 3), "pool_layers.3.main.bias": (4,),
              "final_linear1_age.weight": (160, n_flat), "final_linear1_age.bias": (160,),
              "final_linear2_age.weight": (10, 160), "final_linear2_age.bias": (10,),
              "final_linear3_age.weight": (1, 10), "final_linear3_age.bias": (1,)}
    prm = {k: (torch.randn(s, generator=g) * 0.2).to(dev) for k, s in shapes.items()}
    ah = M.AgeHead(prm, cf, n_flat, dev)
    feat = torch.randn(dims + (cf,), generator=g).to(dev)

    def run():
        p, tape = ah.forward(feat, dims)
        grads = {k: torch.empty_like(v) for k, v in prm.items()}
        dfeat = torch.ones_like(feat)
        loss = torch.zeros(1, dtype=torch.float64, device=dev)
        ah.backward(tape, float(p.abs().item()) + 1.0, 0.5, L_ptr(loss), grads, dfeat)
        torch.cuda.synchronize()
        return [p.clone(), loss.clone(), dfeat.clone()] + [grads[k].clone() for k in shapes]

    a, b = run(), run()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert float(a[1]) == 1.0 or abs(float(a[1]) - 1.0) < 1e-6
    assert float(a[2].sub(1).abs().sum()) > 0                  # the pooled gradient reached the feature gradient


def L_ptr(t):
    from brainfm_amd import _lib as L
    return L.ptr(t)


def test_shipped_shape_two_lanes_equal_one_lane():
    """160^3, C = 64, 6 levels: a training iteration with the age loss on the two sample lanes gives the single-lane bits."""
    from brainfm_amd import test_utils as TU
    from brainfm_amd import train as TR
    ga, ta = TU.default_inference_args(tasks=dict(T1=True, age=True))
    torch.manual_seed(0)
    s = TU.InferenceSession(ga, ta, _dev(), passes=3)
    assert s.model.head.n_flat == 4000
    step = TR.TrainStep(s.engine, s.model.head.tail(s.engine), ["T1", "age"], {"loss_T1": 1.0, "loss_age": 1.0},
                        torch.ones(1), 2, lr=1e-4, age_head=s.model.head.age_head())
    g = torch.Generator().manual_seed(1)
    xs = [torch.rand((1, 1, 160, 160, 160), generator=g) for _ in range(2)]
    target = {"T1": torch.rand((1, 1, 160, 160, 160), generator=g), "age": 57.0}
    step.t = 1                                                # lanes are used from the second iteration on
    res = {}
    for lanes in (1, 2):
        step.sample_lanes = lanes
        ld, total, grads = step.loss_and_grads(xs, target, [{}, {}])
        torch.cuda.synchronize()
        res[lanes] = (ld, total, {k: v.detach().clone() for k, v in grads.items()})
    assert res[1][0] == res[2][0] and res[1][1] == res[2][1]
    assert "loss_age" in res[1][0]
    for k, v in res[1][2].items():
        assert torch.equal(v, res[2][2][k]), k
    assert float(res[1][2]["head.final_linear1_age.weight"].abs().sum()) > 0


def test_generator_age_target():
    """A case with an age yields target['age'] == that age (datasets.py:678-679); a case without one yields no key."""
    from brainfm_amd import generator as G
    import test_gpu_synth as SY
    rs = np.random.RandomState(0)
    shp = (48, 44, 52)
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shp], indexing="ij")
    ell = (((zz - 24) / 20.) ** 2 + ((yy - 22) / 18.) ** 2 + ((xx - 26) / 22.) ** 2) <= 1
    lab = ((zz // 8) * 7 + (yy // 8) * 3 + (xx // 8)) % 10
    ids = np.array([2, 3, 4, 41, 42, 17, 10, 11, 12, 13])[lab] * ell
    case = {"name": "toy", "Gen": ids.astype(np.float32), "T1": rs.rand(*shp).astype(np.float32) * ell,
            "segmentation": ids.astype(np.int32),
            "distance": [rs.rand(*shp).astype(np.float32) * 255 for _ in range(4)],
            "registration": [rs.randn(*shp).astype(np.float32) * 500 for _ in range(3)]}
    ds = G.build_datasets(SY._gen_args(), "cuda:0", cases=[dict(case, age=57.0), case])["all"]
    t_age = ds[0][3]
    t_none = ds[1][3]
    assert t_age["age"] == 57.0 and isinstance(t_age["age"], float)
    assert "age" not in t_none
