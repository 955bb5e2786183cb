"""Training of the mask-conditioned network on the GPU: the stem's one-correlation backward (bfm_stem_mc_bwd) alone against
float64, its determinism, scaling and error paths; bfm_condition_input against the torch expressions; and one training
iteration per fixture of tests/golden/make_golden_condtrain.py, with the fused and with the generic first-layer backward.
Needs an MI355X: run with `-m gpu`."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import stem_bwd_refs as SR
import twostage_weights as TW

pytestmark = pytest.mark.gpu

# the bounds of tests/test_gpu_backward.py for the same three quantities (max |err| / max |ref|)
TOL = {"dW": 2e-5, "dgamma": 1e-5, "dbeta": 2e-6}
BFM_E_ARG, BFM_E_SHAPE, BFM_E_WORKSPACE = -1, -2, -3
STEM = "backbone.encoders.0.basic_module.SingleConv1."
TASKS = dict(T1=True, T2=True, FLAIR=True, CT=True, segmentation=True, distance=True, bias_field=True, registration=True,
             super_resolution=True, surface=False, pathology=True, contrastive=False)


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _lib():
    from brainfm_amd import _lib as L
    return L, L.load()


# ----------------------------------------------------------------------------- 1. the kernel on its own
class _Case:
    """Inputs of one first layer on the device, its GroupNorm statistics as float32 roundings of the float64 ones, and
    the float64 gradients.  Channels: an image in [0,1], its flip, a binary mask; beta and the mean are far from 0."""

    def __init__(self, cin, cout, dims, seed=1, mag=1.0):
        dev = _dev()
        g = torch.Generator().manual_seed(seed)
        D, H, W = dims
        x = torch.rand((D, H, W, cin), generator=g)
        x[..., 1] = torch.flip(x[..., 0], dims=[0])
        x[..., cin - 1] = (torch.rand((D, H, W), generator=g) > 0.6).float()
        self.dP = (torch.randn((D, H, W, cout), generator=g) * mag).float()
        self.w = ((torch.rand((cout, cin, 3, 3, 3), generator=g) * 2 - 1) / np.sqrt(27.0 * cin)).float()
        self.gamma = (1.0 + 0.4 * (torch.rand(cin, generator=g) - 0.5)).float()
        self.beta = (0.4 * (torch.rand(cin, generator=g) - 0.5) + 0.3).float()
        self.x, self.cin, self.cout, self.dims = x, cin, cout, dims
        mean, rstd = SR.group_stats(x)
        self.mean, self.rstd = mean.float().reshape(1), rstd.float().reshape(1)
        self.scale = (self.gamma.double() * rstd).float()
        self.shift = (self.beta.double() - mean * rstd * self.gamma.double()).float()
        self.ref = dict(zip(("dW", "dgamma", "dbeta"), SR.stem_bwd_ref(self.dP, x, self.w, self.gamma, self.beta)))
        self.d = {k: getattr(self, k).to(dev).contiguous() for k in ("dP", "x", "w", "gamma", "beta", "mean", "rstd", "scale", "shift")}

    def outputs(self):
        dev = _dev()
        return {"dW": torch.full((self.cout, self.cin, 3, 3, 3), float("nan"), device=dev),
                "dgamma": torch.full((self.cin,), float("nan"), device=dev),
                "dbeta": torch.full((self.cin,), float("nan"), device=dev)}

    def launch(self, out=None, dP=None, ws_bytes=None, cin=None, cout=None, dims=None):
        L, lib = _lib()
        d = self.d
        out = self.outputs() if out is None else out
        cin, cout = self.cin if cin is None else cin, self.cout if cout is None else cout
        D, H, W = self.dims if dims is None else dims
        need = lib.bfm_stem_mc_bwd_workspace(self.cin, self.cout, *self.dims)
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=_dev())
        rc = lib.bfm_stem_mc_bwd(L.ptr(d["dP"] if dP is None else dP), cout, L.ptr(d["x"]), cin, D, H, W, L.ptr(d["w"]),
                                 L.ptr(d["scale"]), L.ptr(d["shift"]), L.ptr(d["mean"]), L.ptr(d["rstd"]), L.ptr(out["dW"]),
                                 L.ptr(out["dgamma"]), L.ptr(out["dbeta"]), L.ptr(ws), need if ws_bytes is None else ws_bytes,
                                 L.stream_ptr())
        torch.cuda.synchronize()
        return rc, out

    def errors(self, out):
        return {k: SR.rel_err(out[k], self.ref[k]) for k in TOL}


_ENGINES = {}


def _engine(cin, cout):
    """An engine whose first layer is cin -> cout (two levels, 2 * cout feature maps)."""
    from brainfm_amd.engine import UNetEngine
    from oracle import unet_ref as O
    if (cin, cout) not in _ENGINES:
        sd = O.random_state_dict(cin, 2 * cout, 2, out_channels={}, seed=3)
        _ENGINES[(cin, cout)] = UNetEngine(sd, cin, 2 * cout, 2, device=_dev())
    return _ENGINES[(cin, cout)]


def _through_backward(c, fused, monkeypatch):
    """The same layer through backward.backward_single_conv (need_input_grad=False): the fused route or, with the switch
    off, the generic kernels (weight gradient by columns, data-gradient conv, bfm_gn_bwd)."""
    from brainfm_amd import backward as BW
    eng = _engine(c.cin, c.cout)
    ly = eng.enc[0][0]
    assert (ly.cin, ly.cout, ly.groups) == (c.cin, c.cout, 1)
    ly.w_raw.copy_(c.d["w"])
    ly.gamma.copy_(c.d["gamma"])
    ly.beta.copy_(c.d["beta"])
    dg = ly.packs.get("dgrad_layer")
    if dg is not None:
        BW.refresh_dgrad(ly, dg)
    t = BW.ConvTape()
    t.ly, t.A, t.B, t.dims, t.lo_dims = ly, c.d["x"], None, tuple(c.dims), None
    t.scale, t.shift, t.mean, t.rstd = c.d["scale"], c.d["shift"], c.d["mean"], c.d["rstd"]
    t.out = torch.ones(tuple(c.dims) + (c.cout,), device=_dev())           # LeakyReLU' = 1: dP = dY
    t.bound = (c.d["x"] * c.d["scale"] + c.d["shift"]).abs().max().reshape(1) * 1.00001
    monkeypatch.setattr(BW, "STEM_MC_BWD", fused)
    dA, dB, gr = BW.backward_single_conv(eng, t, c.d["dP"], need_input_grad=False)
    torch.cuda.synchronize()
    return {"dW": gr[ly.name + ".conv.weight"], "dgamma": gr[ly.name + ".groupnorm.weight"],
            "dbeta": gr[ly.name + ".groupnorm.bias"]}


DIMS = [(1, 2, 3),      # every voxel on a face
        (5, 7, 9),      # all odd, below one tile
        (3, 4, 33),     # an x run past 32 with a tail
        (8, 8, 40)]     # even, several tiles


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("cin", [2, 3, 4])
def test_stem_mc_bwd_vs_float64(cin, cout, dims, monkeypatch):
    """dW, dgamma, dbeta of bfm_stem_mc_bwd (outputs pre-filled with NaN) against the float64 closed form, within the
    bounds of tests/test_gpu_backward.py (dW 2e-5, dgamma 1e-5, dbeta 2e-6 of the reference's maximum) or twice the error
    of the generic path on the same inputs, whichever is larger; both errors are printed.  The route
    backward_single_conv takes for this layer gives the bits of the direct call."""
    c = _Case(cin, cout, dims)
    rc, out = c.launch()
    assert rc == 0
    for k in TOL:
        assert bool(torch.isfinite(out[k]).all()), k
    e = c.errors(out)
    eg = c.errors(_through_backward(c, False, monkeypatch))
    for k in TOL:
        print("stem_mc_bwd %d->%d %s %-6s fused %.2e  generic %.2e" % (cin, cout, dims, k, e[k], eg[k]))
    routed = _through_backward(c, True, monkeypatch)
    for k in TOL:
        assert torch.equal(routed[k].view(torch.int32), out[k].view(torch.int32)), k
    bad = {k: (e[k], eg[k]) for k in TOL if e[k] > max(TOL[k], 2.0 * eg[k])}
    assert not bad, bad


def test_stem_mc_bwd_is_deterministic_and_exact_on_zero():
    c = _Case(3, 64, (8, 8, 40), seed=2)
    _, a = c.launch()
    _, b = c.launch()
    for k in TOL:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    _, z = c.launch(dP=torch.zeros_like(c.d["dP"]))
    for k in TOL:
        assert bool((z[k] == 0).all()), k


@pytest.mark.parametrize("mag", [1e-9, 1e4])
def test_stem_mc_bwd_keeps_its_relative_error_at_other_magnitudes_of_dp(mag):
    """dP at 1e-9 and at 1e4 (loss scaling): exact fp32 products and sums scale with dP, so the same bounds hold."""
    c = _Case(4, 32, (5, 7, 9), seed=4, mag=mag)
    rc, out = c.launch()
    assert rc == 0
    e = c.errors(out)
    print("stem_mc_bwd dP x %g: %s" % (mag, {k: "%.2e" % v for k, v in e.items()}))
    bad = {k: v for k, v in e.items() if v > TOL[k]}
    assert not bad, bad


def test_stem_mc_bwd_error_paths_write_nothing():
    L, lib = _lib()
    c = _Case(2, 32, (3, 4, 5))
    out = c.outputs()
    for kw in (dict(cin=1), dict(cin=5), dict(cout=16), dict(cout=48), dict(cout=128), dict(dims=(0, 4, 5)),
               dict(dims=(3, 4, -1))):
        rc, _ = c.launch(out=out, **kw)
        assert rc == BFM_E_SHAPE, (kw, rc)
    rc, _ = c.launch(out=out, ws_bytes=lib.bfm_stem_mc_bwd_workspace(2, 32, 3, 4, 5) - 1)
    assert rc == BFM_E_WORKSPACE
    d = c.d
    rc = lib.bfm_stem_mc_bwd(None, 32, L.ptr(d["x"]), 2, 3, 4, 5, L.ptr(d["w"]), L.ptr(d["scale"]), L.ptr(d["shift"]),
                             L.ptr(d["mean"]), L.ptr(d["rstd"]), L.ptr(out["dW"]), L.ptr(out["dgamma"]), L.ptr(out["dbeta"]),
                             L.ptr(d["dP"]), 1 << 20, L.stream_ptr())
    assert rc == BFM_E_ARG
    assert lib.bfm_stem_mc_bwd_workspace(5, 32, 3, 4, 5) == 0
    torch.cuda.synchronize()
    for k in TOL:
        assert bool(torch.isnan(out[k]).all()), k


# ----------------------------------------------------------------------------- 2. the condition inputs
def _pathology(kind, shape, g):
    if kind == "zeros":
        return torch.zeros(shape)
    if kind == "ones":
        return torch.ones(shape)
    p = torch.rand(shape, generator=g)
    p.reshape(-1)[:4] = torch.tensor([0.0, 1.0, 1e-40, 2.0 ** -25])
    return p


@pytest.mark.parametrize("kind", ["zeros", "ones", "soft"])
@pytest.mark.parametrize("dims", [(5, 3, 3), (4, 3, 5), (1, 2, 2)])
@pytest.mark.parametrize("condition", ["mask", "flip", "mask+flip"])
def test_condition_input_is_bit_equal_to_torch(condition, dims, kind):
    """The three modes against the torch expressions of the reference's loop on the device: odd and even D (D = 5: the
    middle slice maps to itself), p in {0, 1, soft}, denormals and negative values in x, an odd voxel count."""
    from brainfm_amd import train as TR
    dev = _dev()
    g = torch.Generator().manual_seed(7)
    shape = (1, 1) + dims
    x = torch.rand(shape, generator=g) * 3.0 - 1.0
    k = min(6, x.numel())
    x.reshape(-1)[:k] = torch.tensor([0.0, 1.0, 1e-40, -1e-40, 1.4e-45, 1.17549435e-38])[:k]
    p = _pathology(kind, shape, g)
    want_cl, want_x, want_flip = SR.condition_ref(x.to(dev), p.to(dev), condition)
    samples = [{"input": x.clone()}]
    (x_cl,) = TR.condition_inputs(samples, {"pathology": p}, condition, device=dev)
    assert x_cl.shape == want_cl.shape
    assert torch.equal(x_cl.view(torch.int32), want_cl.view(torch.int32))
    if "mask" in condition:
        assert torch.equal(samples[0]["input"].view(torch.int32), want_x.view(torch.int32))
    else:
        assert torch.equal(samples[0]["input"], x)
    if "flip" in condition:
        assert torch.equal(samples[0]["input_flip"].view(torch.int32), want_flip.view(torch.int32))
    else:
        assert "input_flip" not in samples[0]


# ----------------------------------------------------------------------------- 3. one iteration per fixture
_FIX = {}


def _fixture(stem):
    if stem not in _FIX:
        d = TW.load(stem)
        _FIX[stem] = (d, TW.fixture_state_dict(d, "model"))
    return _FIX[stem]


def _model_and_step(stem):
    from brainfm_amd import models as M
    from brainfm_amd import test_utils as TU
    from brainfm_amd import train as TR
    d, sd = _fixture(stem)
    ga, ta = TU.default_inference_args(f_maps=int(d["cfg"][0]), num_levels=int(d["cfg"][1]), left_hemis_only=True,
                                       tasks=dict(TASKS))
    ta.condition = str(d["condition"])
    ta.losses = Namespace(uncertainty=None, implicit_pathol=False, image_grad=True, registration_grad=True,
                          bias_field_log_type=str(d["bias_field_log_type"]))
    ta.weights = Namespace(image=1.0, image_grad=1.0, seg_ce=1.0, seg_dice=1.0, bias_field_log=1.0, distance=1.0,
                           registration=1.0, registration_grad=1.0)
    ga, ta, model, _, _, _ = M.build_conditioned_model(ga, ta, _dev())
    M.load_state_dict_by_suffix(model, sd)
    step = TR.conditioned_train_step(ga, ta, model, d["weights_ce"], float(d["hyper"][0]), max_surf_distance=float(d["hyper"][1]),
                                     bias_field_log_type=str(d["bias_field_log_type"]))
    assert step.loss_names == [str(s) for s in d["loss_names"]]           # the reference's criterion, pathology excluded
    step.loss_weights = dict(zip((str(s) for s in d["loss_weight_names"]), (float(v) for v in d["loss_weights"])))
    return d, ta, step


def _data(d):
    n_seg = int(d["weights_ce"].size)
    lab = torch.from_numpy(d["target_label"].astype(np.int64))
    target = {"segmentation": torch.nn.functional.one_hot(lab, n_seg).permute(0, 4, 1, 2, 3).float().contiguous()}
    target.update({k[7:]: torch.from_numpy(v) for k, v in d.items() if k.startswith("target/")})
    samples = [{k.split("/", 1)[1]: torch.from_numpy(v) for k, v in d.items() if k.startswith("sample%d/" % i)}
               for i in range(2)]
    return target, samples


def _distance(d, prefix, name, got):
    """max |got - ref64| over what the fixture holds of a gradient, over the float64 gradient's maximum."""
    if "ref64/grad/" + name in d:
        ref = d["ref64/grad/" + name]
        val = got if isinstance(got, np.ndarray) else d[prefix + "grad/" + name]
        return float(np.abs(np.asarray(val, np.float64).reshape(ref.shape) - ref).max() / np.abs(ref).max())
    ref = d["ref64/grad_at/" + name]
    val = got.reshape(-1)[d["grad_idx/" + name]] if isinstance(got, np.ndarray) else d[prefix + "grad_at/" + name]
    return float(np.abs(np.asarray(val, np.float64) - ref).max() / float(d["ref64/grad_max/" + name]))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
@pytest.mark.parametrize("stem", ["train_cond_mask", "train_cond_maskflip"])
def test_conditioned_iteration_vs_reference(stem, fused, monkeypatch):
    """condition_inputs -> TrainStep.loss_and_grads(cond=) against the reference's own iteration in float64: the network
    inputs bit for bit, every loss within 1e-4 (the bound of test_training_iteration_vs_reference_golden), every parameter's
    gradient within max(2e-3, 3 x the distance of the reference's float32 run) of the float64 gradient's maximum -- with
    the stem's backward as one correlation and, BFM_STEM_MC_BWD=0, through the generic kernels."""
    from brainfm_amd import backward as BW
    from brainfm_amd import train as TR
    monkeypatch.setattr(BW, "STEM_MC_BWD", fused)
    d, ta, step = _model_and_step(stem)
    target, samples = _data(d)
    xs = [s["input"] for s in samples]
    cond = TR.condition_inputs(samples, target, ta.condition, device=_dev(), in_channels=step.eng.in_channels)
    for i, x_cl in enumerate(cond):
        ref = torch.concat([torch.from_numpy(d["masked%d" % i]), torch.from_numpy(d["cond%d" % i])], dim=1)
        assert torch.equal(x_cl.cpu(), ref[0].permute(1, 2, 3, 0))
        assert torch.equal(samples[i]["input"].cpu(), torch.from_numpy(d["masked%d" % i]))
    loss_dict, total, grads = step.loss_and_grads(xs, target, samples, cond=cond)
    assert list(loss_dict.keys()) == ["loss_" + n for n in step.loss_names]
    for k, v in loss_dict.items():
        ref = float(d["ref64/loss/" + k])
        assert abs(v - ref) <= 1e-4 * max(abs(ref), 1e-3), (k, v, ref)
    assert abs(total - float(d["ref64/loss_total"])) <= 1e-4 * float(d["ref64/loss_total"])
    names = [str(s) for s in d["param_names"]]
    assert set(grads.keys()) == set(names)
    worst, bad = (0.0, None), {}
    for n in names:
        e = _distance(d, None, n, grads[n].cpu().numpy())
        e32 = _distance(d, "ref32/", n, None)
        if e > worst[0]:
            worst = (e, n)
        if n.startswith(STEM):
            print("%s %s %-45s hip %.2e  ref32 %.2e" % (stem, "fused" if fused else "generic", n, e, e32))
        if e > max(2e-3, 3.0 * e32):
            bad[n] = (e, e32)
    print("%s %s worst gradient distance %.2e (%s)" % (stem, "fused" if fused else "generic", worst[0], worst[1]))
    assert not bad, bad


def test_a_case_without_pathology_trains_as_a_zero_mask():
    """The generator stores 0. as target['pathology'] for a case without pathology: an all-zero mask."""
    from brainfm_amd import train as TR
    d, ta, step = _model_and_step("train_cond_mask")
    target, samples = _data(d)
    zeros = [dict(s) for s in samples]
    xs = [s["input"] for s in samples]
    target["pathology"] = 0.
    cond = TR.condition_inputs(samples, target, ta.condition, device=_dev(), in_channels=step.eng.in_channels)
    want = TR.condition_inputs(zeros, dict(target, pathology=torch.zeros_like(xs[0])), ta.condition, device=_dev())
    for a, b, x in zip(cond, want, xs):
        assert torch.equal(a, b)
        assert torch.equal(a[..., 0].cpu(), x[0, 0]) and bool((a[..., 1] == 0).all())
    before = step.parameters()[STEM + "conv.weight"].clone()
    loss_dict, total, stepped = step.step(xs, target, samples, cond=cond)
    assert stepped and np.isfinite(total)
    assert not torch.equal(step.parameters()[STEM + "conv.weight"], before)


def test_a_wrong_channel_count_raises():
    from brainfm_amd import _lib as L
    from brainfm_amd import train as TR
    d, ta, step = _model_and_step("train_cond_mask")
    target, samples = _data(d)
    xs = [s["input"] for s in samples]
    with pytest.raises(L.BfmError):
        TR.condition_inputs(samples, target, "mask+flip", device=_dev(), in_channels=step.eng.in_channels)
    three = TR.condition_inputs([dict(s) for s in samples], target, "mask+flip", device=_dev())
    with pytest.raises(L.BfmError):
        step.loss_and_grads(xs, target, samples, cond=three)
    with pytest.raises(L.BfmError):
        step.loss_and_grads(xs, target, samples, cond=three[:1])
    ta2 = Namespace(**vars(ta))
    ta2.condition = "mask+flip"
    ga = Namespace(tasks=[], max_surf_distance=3.0)
    with pytest.raises(L.BfmError):
        TR.conditioned_train_step(ga, ta2, Namespace(backbone=Namespace(engine=lambda head: step.eng), head=None),
                                  d["weights_ce"], 1.0)
