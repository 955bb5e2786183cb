"""brainfm_amd.autograd on the device: loss.backward() through the backbone, the heads and the processors for losses written
in torch, against float64 autograd of the oracle; the two processor-backward kernels against tests/autograd_refs.py at their
derived bounds; forward bits, the frozen backbone, the engine after an optimiser step, consistency with TrainStep and the
refusals.  Needs an MI355X: run with `-m gpu`.

Shapes are those of test_backbone_backward_vs_fp64_autograd (tests/test_gpu_infer.py): 64 wide (matrix-core routes), 8 wide
(direct kernels), 16 wide on odd sizes (floor pooling, non-2x upsampling).  Bars: max |got - ref| <= 5e-4 max |ref| per
parameter tensor, 3e-3 for the stem GroupNorm's affine (that test's bars); the input gradient, which passes through the stem's
GroupNorm backward, is held to INPUT_BAR (measured values: DESIGN.md, 'Autograd bridge')."""
import ctypes as C
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import autograd_refs as AR
from oracle import train_ref as TRF
from oracle import unet_ref as O

pytestmark = pytest.mark.gpu

TOL_NET = 1e-3              # whole network (tests/test_gpu_infer.py:17)
PARAM_BAR, STEM_BAR = 5e-4, 3e-3
INPUT_BAR = 5e-4            # measured 1.1e-6 .. 1.7e-6 on these shapes: the parameters' bar, not the stem GroupNorm's 3e-3
STEM = "backbone.encoders.0.basic_module.SingleConv1.groupnorm."
SHAPES = [(64, 3, (16, 12, 20)), (8, 3, (12, 16, 10)), (16, 3, (9, 14, 11))]
HEAD_TASKS = ["T1", "segmentation", "distance", "pathology"]
MAX_DIST = 0.2              # small enough that the random heads' distances reach the clamp at a good share of the voxels


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1e-9, np.abs(b).max()))


def _tasks(names):
    t = dict(T1=False, T2=False, FLAIR=False, CT=False, segmentation=False, distance=False, bias_field=False,
             registration=False, super_resolution=False, surface=False, pathology=False, contrastive=False)
    t.update({n: True for n in names})
    return t


def _build(f_maps, levels, names, seed, unit_feat=True):
    """(gen_args, model, processors, state dict) of a left-hemisphere net with the heads `names` on oracle weights."""
    from brainfm_amd import models as M
    from brainfm_amd import test_utils as TU
    oc = O.default_out_channels(left_hemis_only=True, tasks=names)
    sd = O.random_state_dict(1, f_maps, levels, out_channels=oc, seed=seed)
    ga, ta = TU.default_inference_args(f_maps=f_maps, num_levels=levels, left_hemis_only=True, tasks=_tasks(names),
                                       max_surf_distance=MAX_DIST, unit_feat=unit_feat)
    ga, ta, model, processors = M.build_model(ga, ta, _dev())[:4]
    M.load_state_dict_by_suffix(model, sd)
    return ga, model, processors, sd, oc


def _bars(worst):
    return {k: v for k, v in worst.items() if v > (STEM_BAR if k.startswith(STEM) else PARAM_BAR)}


def _param_errors(model, ref_params):
    own = dict(model.named_parameters())
    worst = {}
    for k, p in ref_params.items():
        assert own[k].grad is not None, k
        worst[k] = _rel(own[k].grad.cpu().numpy(), p.grad.numpy())
    return worst


# ----------------------------------------------------------------------------- 1. the backbone alone
@functools.lru_cache(maxsize=None)
def _backbone_reference(f_maps, levels, dims):
    """float64 autograd of oracle.get_feature for sum_level (feat * R).sum(): computed once per shape, never modified."""
    sd = O.random_state_dict(1, f_maps, levels, out_channels=OrderedDict(T1=1), seed=31)
    g = torch.Generator().manual_seed(12)
    x = torch.rand((1, 1) + dims, generator=g)
    params = {k: v.clone().double().requires_grad_(True) for k, v in sd.items() if k.startswith("backbone.")}
    x64 = x.double().requires_grad_(True)
    feats = O.get_feature(x64, params, f_maps=f_maps, num_levels=levels, unit_feat=False)
    R = [torch.randn(f.shape, generator=g) for f in feats]
    sum((f * r.double()).sum() for f, r in zip(feats, R)).backward()
    return x, R, [f.detach() for f in feats], params, x64.grad


@pytest.mark.parametrize("f_maps,levels,dims,fast", [s + (False,) for s in SHAPES] + [SHAPES[0] + (True,)])
def test_backbone_gradients_vs_fp64_autograd(f_maps, levels, dims, fast):
    """dm.backbone.get_feature(x), a loss linear in every decoder level, loss.backward(): every backbone parameter's .grad
    and the gradient of the input against float64 autograd of the oracle."""
    from brainfm_amd import autograd as AG
    x, R, feats_ref, params, dx_ref = _backbone_reference(f_maps, levels, dims)
    _, model, _, _, _ = _build(f_maps, levels, ["T1"], seed=31, unit_feat=False)
    dm = AG.differentiable(model, fast=fast)
    xd = x.to(_dev()).requires_grad_(True)
    feats = dm.backbone.get_feature(xd)
    assert len(feats) == len(feats_ref)
    for f, fr in zip(feats, feats_ref):
        assert f.grad_fn is not None and tuple(f.shape) == tuple(fr.shape)
        assert _rel(f.detach().cpu().numpy(), fr.numpy()) <= TOL_NET
    sum((f * r.to(_dev())).sum() for f, r in zip(feats, R)).backward()
    worst = _param_errors(model, params)
    e_in = _rel(xd.grad.cpu().numpy(), dx_ref.numpy())
    print("backbone %s fast=%s: max rel grad err vs fp64 %.2e over %d tensors (%s); input gradient %.2e"
          % ((f_maps, levels, dims), fast, max(worst.values()), len(worst), max(worst, key=worst.get), e_in))
    assert all(p.grad is None for k, p in model.named_parameters() if k.startswith("head."))
    assert not _bars(worst), _bars(worst)
    assert e_in <= INPUT_BAR, e_in
    last = dm.backbone(xd)                                        # forward() is the last map, with a grad_fn too
    assert last.grad_fn is not None and tuple(last.shape) == tuple(feats_ref[-1].shape)


# ----------------------------------------------------------------------------- 2. the full model
def _smooth_loss(out, tgt):
    """A loss the criterion does not have: MSE on T1, unweighted -log p[label], MSE on the clamped distance and on the
    sigmoid, and a linear term on the last (unit) feature map."""
    p = out["segmentation"].gather(1, tgt["label"])
    return (((out["T1"] - tgt["T1"]) ** 2).mean() - torch.log(p).mean()
            + ((out["distance"] - tgt["distance"]) ** 2).mean() + ((out["pathology"] - tgt["pathology"]) ** 2).mean()
            + (out["feat"][-1] * tgt["R"]).sum() * 1e-3)


@pytest.mark.parametrize("f_maps,levels,dims", SHAPES)
def test_full_model_gradients_vs_fp64_autograd(f_maps, levels, dims):
    """dm(samples) -> differentiable processors -> a smooth torch loss -> backward(): every parameter gradient, head weights
    and biases included, against float64 autograd of oracle.get_feature / task_heads / train_ref.processors."""
    from brainfm_amd import autograd as AG
    # the backbone weights and the input of case 1 (seeds 31 / 12, those of test_backbone_backward_vs_fp64_autograd, whose bars
    # these are): the heads' weights are drawn after the backbone's, the targets after the input
    ga, model, processors, sd, oc = _build(f_maps, levels, HEAD_TASKS, seed=31)
    g = torch.Generator().manual_seed(12)
    x = torch.rand((1, 1) + dims, generator=g)
    tgt = {"T1": torch.rand((1, 1) + dims, generator=g), "label": torch.randint(0, oc["segmentation"], (1, 1) + dims, generator=g),
           "distance": torch.randn((1, 2) + dims, generator=g) * MAX_DIST, "pathology": torch.rand((1, 1) + dims, generator=g),
           "R": torch.randn((1, f_maps) + dims, generator=g)}
    params = {k: v.clone().double().requires_grad_(True) for k, v in sd.items()}
    feats = O.get_feature(x.double(), params, f_maps=f_maps, num_levels=levels, unit_feat=True)
    ref = TRF.processors(O.task_heads(feats[-1], params, oc), max_surf_distance=MAX_DIST)
    ref["feat"] = feats
    clamped = float((ref["distance"].detach().abs() == MAX_DIST).double().mean())
    assert 0.01 < clamped < 0.99, clamped                         # the clamp passes gradient at some voxels, none at others
    _smooth_loss(ref, {k: (v.double() if v.dtype.is_floating_point else v) for k, v in tgt.items()}).backward()
    dm = AG.differentiable(model, fast=False)
    outs, inputs = dm([{"input": x.to(_dev())}])
    assert len(outs) == 1 and list(outs[0].keys()) == ["feat"] + list(oc.keys()) and inputs[0].shape == x.shape
    for p in AG.differentiable_processors(processors):
        outs = p(outs)
    out = outs[0]
    for k in oc:
        assert out[k].grad_fn is not None and _rel(out[k].detach().cpu().numpy(), ref[k].detach().numpy()) <= TOL_NET, k
    _smooth_loss(out, {k: v.to(_dev()) for k, v in tgt.items()}).backward()
    worst = _param_errors(model, params)
    assert set(worst) == set(k for k, _ in model.named_parameters())
    heads = {k: v for k, v in worst.items() if k.startswith("head.")}
    print("full model %s: max rel grad err vs fp64 %.2e (%s); heads %.2e (%s)"
          % ((f_maps, levels, dims), max(worst.values()), max(worst, key=worst.get), max(heads.values()),
             max(heads, key=heads.get)))
    assert not _bars(worst), _bars(worst)


# ----------------------------------------------------------------------------- 3. the two kernels alone
GRID_THREADS = 4096 * 256           # elementwise.hip's grid_for cap: more rows than this run the grid-stride loop


@pytest.mark.parametrize("C_,n", [(2, 4099), (7, 4099), (56, 4099), (2, GRID_THREADS + 77)])
def test_softmax_bwd_kernel_at_its_bound(C_, n):
    """bfm_softmax_cl_bwd against the float64 closed form at the derived bound: contiguous rows, and rows that are views
    into wider buffers (what is outside the views stays untouched); 4099 rows end in a partial block, the last case also
    runs the grid-stride loop."""
    from brainfm_amd import _lib as L
    lib, dev = L.load(), _dev()
    x, g = AR.softmax_case(C_, n, seed=100 + C_)
    p = AR.softmax32(x)
    ref, bound = AR.softmax_bwd64(p, g), AR.softmax_bwd_bound(p, g)
    pd, gd = torch.from_numpy(p).to(dev), torch.from_numpy(g).to(dev)
    dx = torch.full((n, C_), float("nan"), device=dev)
    L.check(lib.bfm_softmax_cl_bwd(L.ptr(pd), C_, L.ptr(gd), C_, C_, L.ptr(dx), C_, n, L.stream_ptr()), "softmax_bwd")
    worst = AR.check(dx.cpu().numpy(), ref, bound, "softmax_bwd C=%d n=%d" % (C_, n))
    print("softmax_bwd C=%d n=%d: worst error %.2f of its bound" % (C_, n, worst))
    wide = [torch.full((n, C_ + 5 + i), float("nan"), device=dev) for i in range(3)]
    wide[0][:, 3:3 + C_] = pd
    wide[1][:, 1:1 + C_] = gd
    ptr = lambda t, c0: C.c_void_p(t.data_ptr() + 4 * c0)
    L.check(lib.bfm_softmax_cl_bwd(ptr(wide[0], 3), C_ + 5, ptr(wide[1], 1), C_ + 6, C_, ptr(wide[2], 2), C_ + 7, n,
                                   L.stream_ptr()), "softmax_bwd strided")
    assert torch.equal(wide[2][:, 2:2 + C_], dx)
    assert bool(torch.isnan(wide[2][:, :2]).all()) and bool(torch.isnan(wide[2][:, 2 + C_:]).all())
    assert lib.bfm_softmax_cl_bwd(L.ptr(pd), C_ - 1, L.ptr(gd), C_, C_, L.ptr(dx), C_, n, L.stream_ptr()) == -1


@pytest.mark.parametrize("n", [4099, GRID_THREADS + 77])
def test_unary_bwd_kernel_at_its_bound(n):
    """bfm_ew_unary_bwd: sigmoid from the output, clamp from the input with inclusive edges, each on contiguous vectors
    and on one column of a 3-wide buffer; other ops are refused."""
    from brainfm_amd import _lib as L
    lib, dev = L.load(), _dev()
    xs, gs = AR.sigmoid_case(n, seed=8)
    y = AR.sigmoid32(xs)
    xc, gc = AR.clamp_case(n, seed=9)
    cases = [("sigmoid", L.EW_SIGMOID, y, gs, 0.0, 0.0, AR.sigmoid_bwd64(y, gs), AR.sigmoid_bwd_bound(y, gs)),
             ("clamp", L.EW_CLAMP, xc, gc, -3.0, 3.0, AR.clamp_bwd64(xc, gc, -3.0, 3.0), AR.clamp_bwd_bound(xc, gc, -3.0, 3.0))]
    for what, op, v, g, a, b, ref, bound in cases:
        vd, gd = torch.from_numpy(v).to(dev), torch.from_numpy(g).to(dev)
        dx = torch.full((n,), float("nan"), device=dev)
        L.check(lib.bfm_ew_unary_bwd(op, L.ptr(vd), 1, L.ptr(gd), 1, L.ptr(dx), 1, n, a, b, L.stream_ptr()), what)
        AR.check(dx.cpu().numpy(), ref, bound, "%s_bwd n=%d" % (what, n))
        wide = [torch.full((n, 3), float("nan"), device=dev) for _ in range(3)]
        wide[0][:, 1], wide[1][:, 2] = vd, gd
        L.check(lib.bfm_ew_unary_bwd(op, C.c_void_p(wide[0].data_ptr() + 4), 3, C.c_void_p(wide[1].data_ptr() + 8), 3,
                                     L.ptr(wide[2]), 3, n, a, b, L.stream_ptr()), what + " strided")
        assert torch.equal(wide[2][:, 0], dx) and bool(torch.isnan(wide[2][:, 1:]).all())
    assert lib.bfm_ew_unary_bwd(L.EW_EXP, L.ptr(dx), 1, L.ptr(dx), 1, L.ptr(dx), 1, n, 0.0, 0.0, L.stream_ptr()) == -1


# ----------------------------------------------------------------------------- 4. forward values
def test_forward_values_and_processor_bits():
    from brainfm_amd import autograd as AG
    f_maps, levels, dims = SHAPES[2]
    ga, model, processors, sd, oc = _build(f_maps, levels, HEAD_TASKS, seed=43)
    dm = AG.differentiable(model, fast=False)
    x = torch.rand((2, 1) + dims, generator=torch.Generator().manual_seed(3)).to(_dev())
    base, _ = model([{"input": x[:1]}])

    def same(a, b):
        assert list(a.keys()) == list(b.keys())
        for k in a:
            for u, v in zip(a[k] if k == "feat" else [a[k]], b[k] if k == "feat" else [b[k]]):
                assert u.grad_fn is None and torch.equal(u, v) and u.stride() == v.stride(), k

    with torch.no_grad():
        same(dm([{"input": x[:1]}])[0][0], base[0])
    for p in model.parameters():
        p.requires_grad_(False)
    same(dm([{"input": x[:1]}])[0][0], base[0])                   # nothing requires grad: the inference path itself
    feats_ng = dm.backbone.get_feature(x[:1])
    for p in model.parameters():
        p.requires_grad_(True)
    outs, _ = dm([{"input": x[:1]}])
    for k in base[0]:
        for u, v in zip(outs[0][k] if k == "feat" else [outs[0][k]], base[0][k] if k == "feat" else [base[0][k]]):
            assert u.grad_fn is not None and u.shape == v.shape and u.stride() == v.stride(), k
            assert _rel(u.detach().cpu().numpy(), v.cpu().numpy()) <= TOL_NET, k
    # the processors: the same kernels, the same bits, on the same inputs
    a = [OrderedDict((k, v) for k, v in base[0].items())]
    b = [OrderedDict((k, (v.clone().requires_grad_(True) if k != "feat" else v)) for k, v in base[0].items())]
    for p, q in zip(processors, AG.differentiable_processors(processors)):
        a, b = p(a), q(b)
    for k in oc:
        assert torch.equal(a[0][k], b[0][k]), k
        assert (b[0][k].grad_fn is not None) == (k != "T1"), k   # T1 has no processor: it stays the leaf it was
        assert k == "T1" or a[0][k].stride() == b[0][k].stride(), k
    # a batch of two loops per sample, as the joiner does
    outs2, _ = dm([{"input": x}])
    assert outs2[0]["T1"].shape[0] == 2 and outs2[0]["feat"][-1].shape[0] == 2
    assert _rel(outs2[0]["T1"][:1].detach().cpu().numpy(), outs[0]["T1"].detach().cpu().numpy()) <= 1e-5
    (outs2[0]["T1"] ** 2).mean().backward()
    assert model.head.final_conv_T1.weight.grad is not None
    # the backbone alone without grad: UNet3D.get_feature's values (that call builds an engine of its own, whose tuned conv
    # variants may differ in the last bits: 1e-4, the bar of the single-block parity tests)
    for f, b in zip(feats_ng, model.backbone.get_feature(x[:1])):
        assert f.grad_fn is None and f.stride() == b.stride()
        assert _rel(f.cpu().numpy(), b.cpu().numpy()) <= 1e-4


def test_contrastive_processor_bits_and_gradient():
    """DifferentiableContrastiveProcessor: ContrastiveProcessor's bits; its backward against float64 autograd of
    F.normalize(dim=1) within 20 fp32 roundings of the largest entry (the normalisation's own bound, tests/tail_refs.py)."""
    from brainfm_amd import autograd as AG
    from brainfm_amd import models as M
    g = torch.Generator().manual_seed(5)
    f = torch.randn((1, 16, 5, 6, 7), generator=g)
    r = torch.randn(f.shape, generator=g)
    a = M.ContrastiveProcessor()([{"feat": [f.to(_dev())]}])[0]["feat"][-1]
    fd = f.to(_dev()).requires_grad_(True)
    b = AG.differentiable_processors([M.ContrastiveProcessor()])[0]([{"feat": [fd]}])[0]["feat"][-1]
    assert torch.equal(a, b)
    (b * r.to(_dev())).sum().backward()
    f64 = f.double().requires_grad_(True)
    (torch.nn.functional.normalize(f64, dim=1) * r.double()).sum().backward()
    assert _rel(fd.grad.cpu().numpy(), f64.grad.numpy()) <= 20 * AR.EPS * 16


# ----------------------------------------------------------------------------- 5. the frozen backbone
def test_frozen_backbone_gets_head_gradients_only(monkeypatch):
    """requires_grad_(False) on the backbone: no tape is made, only the head's parameters get a .grad, and it is the
    unfrozen run's to fp32 rounding: bfm_head_wgrad and bfm_head_bwd each stay within 2e-5 of the largest entry of the
    float64 sums (test_head_wgrad_kernel_vs_float64, test_heads_backward_fused_pass_vs_float64), so within 4e-5 of each
    other.  Both runs take the inference layer path forward (fast=True), so that they see the same features."""
    from brainfm_amd import autograd as AG
    from brainfm_amd import backward as BW
    f_maps, levels, dims = SHAPES[0]
    ga, model, processors, sd, oc = _build(f_maps, levels, HEAD_TASKS, seed=45)
    dm = AG.differentiable(model, fast=True)
    procs = AG.differentiable_processors(processors)
    g = torch.Generator().manual_seed(9)
    x = torch.rand((1, 1) + dims, generator=g).to(_dev())
    tgt = {"T1": torch.rand((1, 1) + dims, generator=g), "label": torch.randint(0, oc["segmentation"], (1, 1) + dims, generator=g),
           "distance": torch.randn((1, 2) + dims, generator=g) * MAX_DIST, "pathology": torch.rand((1, 1) + dims, generator=g),
           "R": torch.zeros((1, f_maps) + dims)}
    tgt = {k: v.to(_dev()) for k, v in tgt.items()}

    def run():
        for p in model.parameters():
            p.grad = None
        outs, _ = dm([{"input": x}])
        for p in procs:
            outs = p(outs)
        _smooth_loss(outs[0], tgt).backward()
        return {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}

    full = run()
    taped = []
    real = BW.backbone_forward_train
    monkeypatch.setattr(BW, "backbone_forward_train", lambda *a, **k: taped.append(1) or real(*a, **k))
    model.backbone.requires_grad_(False)
    frozen = run()
    assert not taped
    for k, v in frozen.items():
        if k.startswith("head."):
            e = _rel(v.cpu().numpy(), full[k].cpu().numpy())
            print("frozen vs unfrozen %-40s %.2e" % (k, e))
            assert e <= 4e-5, (k, e)
        else:
            assert v is None, k
    model.backbone.requires_grad_(True)
    run()
    assert taped                                                  # the counter does see a taped run


# ----------------------------------------------------------------------------- 6. the engine after an optimiser step
def test_engine_is_refreshed_in_place_after_optimizer_steps(monkeypatch):
    from brainfm_amd import autograd as AG
    from brainfm_amd import engine as E
    from brainfm_amd import models as M
    f_maps, levels, dims = SHAPES[0]
    ga, model, processors, sd, oc = _build(f_maps, levels, ["T1", "distance"], seed=47)
    dm = AG.differentiable(model)
    g = torch.Generator().manual_seed(11)
    x = torch.rand((1, 1) + dims, generator=g).to(_dev())
    t1 = torch.rand((1, 1) + dims, generator=g).to(_dev())
    samples = [{"input": x}]
    first = model(samples)[0][0]["T1"].clone()
    eng = model.backbone._engine
    built = []
    real_init = E.UNetEngine.__init__
    monkeypatch.setattr(E.UNetEngine, "__init__", lambda self, *a, **k: built.append(1) or real_init(self, *a, **k))
    opt = torch.optim.SGD(model.parameters(), lr=0.02)
    tuned = None
    for it in range(2):
        opt.zero_grad()
        out = dm(samples)[0][0]
        ((out["T1"] - t1) ** 2).mean().backward()
        opt.step()
        if it == 0:
            tuned = set(eng._tuned)
    with torch.no_grad():
        after = dm(samples)[0][0]
    again = model(samples)[0][0]
    assert model.backbone._engine is eng and not built
    assert set(eng._tuned) == tuned                              # no convolution was tuned again after the first iteration
    change = _rel(after["T1"].cpu().numpy(), first.cpu().numpy())
    assert change > 1e-2, change                                  # the steps moved the output by far more than any tolerance below
    for k in ("T1", "distance"):
        assert torch.equal(after[k], again[k]), k
    for u, v in zip(after["feat"], again["feat"]):
        assert torch.equal(u, v)
    assert model.backbone._engine is eng and not built
    # a fresh model on the stepped weights: its packed forms were all made from them (conv variants may differ in the last
    # bits: 1e-4, the bar of the single-block parity tests, against a change of > 1e-2)
    monkeypatch.undo()
    ga2, model2, _, _, _ = _build(f_maps, levels, ["T1", "distance"], seed=48)
    model2.load_state_dict(model.state_dict())
    fresh = model2(samples)[0][0]
    for k in ("T1", "distance"):
        assert _rel(fresh[k].cpu().numpy(), again[k].cpu().numpy()) <= 1e-4, k
    assert _rel(fresh["feat"][-1].cpu().numpy(), again["feat"][-1].cpu().numpy()) <= 1e-4
    # ten steps of a small fine-tune lower the loss
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    losses = []
    for it in range(10):
        opt.zero_grad()
        loss = ((dm(samples)[0][0]["T1"] - t1) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("fine-tune losses: " + " ".join("%.5f" % v for v in losses))
    assert losses[-1] < losses[0] and model.backbone._engine is eng


# ----------------------------------------------------------------------------- 7. consistency with the training step
@pytest.mark.parametrize("f_maps,levels,dims", [SHAPES[0], SHAPES[2]])
def test_l1_gradients_agree_with_trainstep(f_maps, levels, dims):
    """mean |T1 - target| written in torch through the bridge against TrainStep.loss_and_grads(loss_names=['T1']) on the
    same engine: every gradient to 2e-3 of its largest entry (the bar test_training_iteration_vs_reference_golden gives
    sign-type losses)."""
    from brainfm_amd import autograd as AG
    from brainfm_amd import train as TR
    ga, model, processors, sd, oc = _build(f_maps, levels, ["T1"], seed=49)
    dm = AG.differentiable(model)
    g = torch.Generator().manual_seed(13)
    x = torch.rand((1, 1) + dims, generator=g)
    t1 = torch.rand((1, 1) + dims, generator=g)
    out = dm([{"input": x.to(_dev())}])[0][0]
    loss = (out["T1"] - t1.to(_dev())).abs().mean()
    loss.backward()
    eng = AG.sync_engine(model.backbone, model.head)
    step = TR.TrainStep(eng, model.head.tail(eng), ["T1"], {"loss_T1": 1.0}, torch.ones(1), 1)
    loss_dict, total, grads = step.loss_and_grads([x], {"T1": t1}, [{}])
    assert abs(total - float(loss.detach())) <= 1e-5 * abs(total)
    own = dict(model.named_parameters())
    assert set(grads.keys()) == set(own.keys())
    worst = {k: _rel(own[k].grad.cpu().numpy(), grads[k].reshape(own[k].shape).cpu().numpy()) for k in own}
    print("bridge vs TrainStep %s: max rel difference %.2e (%s)" % ((f_maps, levels, dims), max(worst.values()),
                                                                    max(worst, key=worst.get)))
    bad = {k: v for k, v in worst.items() if v > 2e-3}
    assert not bad, bad


# ----------------------------------------------------------------------------- 8. refusals on the device
def test_second_order_backward_and_autocast_are_refused():
    from brainfm_amd import _lib as L
    from brainfm_amd import autograd as AG
    f_maps, levels, dims = SHAPES[1]
    ga, model, processors, sd, oc = _build(f_maps, levels, ["T1"], seed=51)
    dm = AG.differentiable(model)
    x = torch.rand((1, 1) + dims, generator=torch.Generator().manual_seed(1)).to(_dev())
    loss = (dm([{"input": x}])[0][0]["T1"] ** 2).mean()
    with pytest.raises(NotImplementedError, match="create_graph"):
        loss.backward(create_graph=True)
    with torch.autocast("cuda", dtype=torch.float16):
        with pytest.raises(L.BfmError, match="autocast"):
            dm([{"input": x}])
        with pytest.raises(L.BfmError, match="autocast"):
            dm.backbone.get_feature(x)
