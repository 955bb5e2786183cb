"""Joint training of the two-stage model on the GPU: the stem's one-channel input gradient (bfm_stem_mc_dgrad) alone against
float64, the fused mask chain against bfm_mask_chain_bwd, accumulation, determinism, scaling and error paths;
bfm_twostage_train_input against the torch expressions; one joint iteration against the fixture of
tests/golden/make_golden_twostage_train.py with BFM_STEM_MC_DGRAD on and off; step(), the zero mask and the checkpoints.
Needs an MI355X: run with `-m gpu`."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import stem_bwd_refs as SR
import twostage_train_refs as TR
import twostage_weights as TW

pytestmark = pytest.mark.gpu

TOL = 2e-5                  # the bound tests/test_gpu_backward.py holds the convolution class to (max |err| / max |ref|)
BFM_E_ARG, BFM_E_SHAPE = -1, -2
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
    """One first layer on the device: channel `channel` of its input is x_raw (1 - p), the last other channel a binary
    mask.  GroupNorm statistics are float32 roundings of the float64 ones, dgamma / dbeta float32 roundings of the float64
    reference; the references are float64 closed forms (tests/twostage_train_refs.py)."""

    def __init__(self, cin, cout, dims, channel, seed=1, mag=1.0):
        dev = _dev()
        g = torch.Generator().manual_seed(seed)
        D, H, W = dims
        self.x_raw = torch.rand((D, H, W), generator=g)
        self.p = torch.sigmoid(3.0 * torch.randn((D, H, W), generator=g))
        x = torch.rand((D, H, W, cin), generator=g)
        x[..., cin - 1] = (torch.rand((D, H, W), generator=g) > 0.6).float()
        x[..., channel] = self.x_raw * (1 - self.p)
        self.dP = (torch.randn((D, H, W, cout), generator=g) * mag).float()
        self.w = ((torch.rand((cout, cin, 3, 3, 3), generator=g) * 2 - 1) / np.sqrt(27.0 * cin)).float()
        self.gamma = (1.0 + 0.4 * (torch.rand(cin, generator=g) - 0.5)).float()
        self.beta = (0.4 * (torch.rand(cin, generator=g) - 0.5) + 0.3).float()
        self.x, self.cin, self.cout, self.dims, self.channel = x, cin, cout, dims, channel
        mean, rstd = SR.group_stats(x)
        self.mean, self.rstd = mean.float().reshape(1), rstd.float().reshape(1)
        self.scale = (self.gamma.double() * rstd).float()
        self.shift = (self.beta.double() - mean * rstd * self.gamma.double()).float()
        _, dgamma, dbeta = SR.stem_bwd_ref(self.dP, x, self.w, self.gamma, self.beta)
        self.dgamma, self.dbeta = dgamma.float(), dbeta.float()
        self.ref_dx = TR.stem_dgrad_ref(self.dP, x, self.w, self.gamma, channel, dgamma, dbeta)
        self.ref_inc = TR.mask_chain_ref(self.ref_dx, self.x_raw, self.p)
        self.d = {k: getattr(self, k).to(dev).contiguous() for k in
                  ("dP", "x", "w", "gamma", "beta", "mean", "rstd", "scale", "shift", "dgamma", "dbeta", "x_raw", "p")}

    def launch(self, dx="nan", dRaw="nan", chain=True, dP=None, cin=None, cout=None, dims=None, channel=None, null_dp=False):
        """dx / dRaw: 'nan' = a NaN-filled buffer, None = not asked for, or a tensor.  Returns (rc, dx, dRaw)."""
        L, lib = _lib()
        d, dev = self.d, _dev()
        if isinstance(dx, str):
            dx = torch.full(self.dims, float("nan"), device=dev)
        if isinstance(dRaw, str):
            dRaw = torch.full(self.dims, float("nan"), device=dev)
        cin, cout = self.cin if cin is None else cin, self.cout if cout is None else cout
        D, H, W = self.dims if dims is None else dims
        rc = lib.bfm_stem_mc_dgrad(None if null_dp else L.ptr(d["dP"] if dP is None else dP), cout, L.ptr(d["x"]), cin, D, H, W,
                                   L.ptr(d["w"]), L.ptr(d["gamma"]), L.ptr(d["mean"]), L.ptr(d["rstd"]), L.ptr(d["dgamma"]),
                                   L.ptr(d["dbeta"]), self.channel if channel is None else channel, L.ptr(dx),
                                   L.ptr(d["x_raw"]) if chain else None, L.ptr(d["p"]) if chain else None,
                                   L.ptr(dRaw) if chain else None, 0, 1, L.stream_ptr())
        torch.cuda.synchronize()
        return rc, dx, dRaw


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
    """The same layer through backward.backward_single_conv with an input-gradient request: the fused pair or, with the
    switch off, the generic kernels (weight gradient, padded data-gradient conv, bfm_gn_bwd, bfm_mask_chain_bwd).
    Returns (dA or None, the increment of a zeroed dRaw, the parameter gradients)."""
    from brainfm_amd import backward as BW
    eng = _engine(c.cin, c.cout)
    ly = eng.enc[0][0]
    assert (ly.cin, ly.cout, ly.groups) == (c.cin, c.cout, 1)
    ly.w_raw.copy_(c.d["w"])
    ly.gamma.copy_(c.d["gamma"])
    ly.beta.copy_(c.d["beta"])
    ly.packs.pop("dgrad_layer", None)          # the engine is shared between cases: the transposed weights and their packs anew
    t = BW.ConvTape()
    t.ly, t.A, t.B, t.dims, t.lo_dims = ly, c.d["x"], None, tuple(c.dims), None
    t.scale, t.shift, t.mean, t.rstd = c.d["scale"], c.d["shift"], c.d["mean"], c.d["rstd"]
    t.out = torch.ones(tuple(c.dims) + (c.cout,), device=_dev())           # LeakyReLU' = 1: dP = dY
    t.bound = (c.d["x"] * c.d["scale"] + c.d["shift"]).abs().max().reshape(1) * 1.00001
    monkeypatch.setattr(BW, "STEM_MC_DGRAD", fused)
    dRaw = torch.zeros(c.dims, device=_dev())
    ig = BW.InputGrad(c.channel, c.d["x_raw"], c.d["p"], dRaw, 0, 1)
    dA, _, gr = BW.backward_single_conv(eng, t, c.d["dP"], need_input_grad=True, input_grad=ig)
    torch.cuda.synchronize()
    return dA, dRaw, gr


DIMS = [(1, 2, 3),      # every voxel on a face
        (5, 7, 9),      # all odd, below one tile
        (3, 4, 33),     # an x run past 32 with a tail
        (8, 8, 40)]     # even, several tiles


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("end", ["first", "last"])
@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("cin", [2, 3, 4])
def test_stem_mc_dgrad_vs_float64(cin, cout, end, dims, monkeypatch):
    """dx and the chained dRaw increment of bfm_stem_mc_dgrad (outputs pre-filled with NaN / zero) against the float64 closed
    form: max |err| / max |ref| within max(2e-5, 2 x the generic route's error on the same inputs); both are printed."""
    channel = 0 if end == "first" else cin - 1
    c = _Case(cin, cout, dims, channel)
    rc, dx, _ = c.launch(chain=False)
    assert rc == 0 and bool(torch.isfinite(dx).all())
    rc, dx2, inc = c.launch(dRaw=torch.zeros(dims, device=_dev()))
    assert rc == 0 and bool(torch.isfinite(inc).all())
    assert torch.equal(dx.view(torch.int32), dx2.view(torch.int32))
    e = {"dx": TR.rel_err(dx, c.ref_dx), "dRaw": TR.rel_err(inc, c.ref_inc)}
    dA, ginc, _ = _through_backward(c, False, monkeypatch)
    eg = {"dx": TR.rel_err(dA[..., channel], c.ref_dx), "dRaw": TR.rel_err(ginc, c.ref_inc)}
    for k in e:
        print("stem_mc_dgrad %d->%d ch %d %s %-4s fused %.2e  generic %.2e" % (cin, cout, channel, dims, k, e[k], eg[k]))
    bad = {k: (e[k], eg[k]) for k in e if e[k] > max(TOL, 2.0 * eg[k])}
    assert not bad, bad


def test_the_fused_route_of_backward_gives_the_kernels_bits(monkeypatch):
    """backward_single_conv with the switch on: bfm_stem_mc_bwd's parameter gradients and the chain of bfm_stem_mc_dgrad
    called with them."""
    L, lib = _lib()
    c = _Case(2, 32, (5, 7, 9), 0, seed=6)
    dA, inc, gr = _through_backward(c, True, monkeypatch)
    assert dA is None
    name = _engine(2, 32).enc[0][0].name
    c.d["dgamma"], c.d["dbeta"] = gr[name + ".groupnorm.weight"], gr[name + ".groupnorm.bias"]
    rc, _, want = c.launch(dx=None, dRaw=torch.zeros(c.dims, device=_dev()))
    assert rc == 0
    assert torch.equal(inc.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("cin,cout,dims,channel", [(2, 32, (5, 7, 9), 0), (4, 64, (8, 8, 40), 3)])
def test_fused_chain_equals_the_standalone_chain_bit_for_bit(cin, cout, dims, channel):
    L, lib = _lib()
    c = _Case(cin, cout, dims, channel, seed=5)
    g = torch.Generator().manual_seed(9)
    pattern = torch.randn(dims, generator=g).to(_dev())
    rc, dx, fused = c.launch(dRaw=pattern.clone())
    assert rc == 0
    alone = pattern.clone()
    rc = lib.bfm_mask_chain_bwd(L.ptr(dx), 1, L.ptr(c.d["x_raw"]), L.ptr(c.d["p"]), dx.numel(), L.ptr(alone), 0, 1,
                                L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(fused.view(torch.int32), alone.view(torch.int32))
    # the accumulator is added to, not overwritten
    rc, _, inc = c.launch(dx=None, dRaw=torch.zeros(dims, device=_dev()))
    assert torch.equal(fused.view(torch.int32), (pattern + inc).view(torch.int32))
    assert not torch.equal(fused, inc)
    # a strided dx (the generic route reads channel c of dA) and a strided dRaw (a channels-last head buffer)
    wide = torch.zeros(dims + (3,), device=_dev())
    wide[..., 1] = dx
    out = torch.zeros(dims + (2,), device=_dev())
    rc = lib.bfm_mask_chain_bwd(_offset_ptr(wide, 1), 3, L.ptr(c.d["x_raw"]), L.ptr(c.d["p"]), dx.numel(), L.ptr(out), 1, 2,
                                L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(out[..., 1].contiguous().view(torch.int32), inc.view(torch.int32)) and bool((out[..., 0] == 0).all())


def _offset_ptr(t, offset_elems):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + 4 * offset_elems)


def test_zero_dp_changes_nothing_and_two_runs_give_the_same_bits():
    c = _Case(3, 64, (8, 8, 40), 1, seed=2)
    g = torch.Generator().manual_seed(4)
    pattern = torch.randn(c.dims, generator=g).to(_dev())
    # dgamma = dbeta = 0 belong to dP = 0
    c.d["dgamma"], c.d["dbeta"] = torch.zeros(3, device=_dev()), torch.zeros(3, device=_dev())
    rc, dx, dRaw = c.launch(dRaw=pattern.clone(), dP=torch.zeros_like(c.d["dP"]))
    assert rc == 0
    assert bool((dx == 0).all()) and torch.equal(dRaw.view(torch.int32), pattern.view(torch.int32))
    c = _Case(3, 64, (8, 8, 40), 1, seed=2)
    _, dx_a, inc_a = c.launch(dRaw=pattern.clone())
    _, dx_b, inc_b = c.launch(dRaw=pattern.clone())
    assert torch.equal(dx_a.view(torch.int32), dx_b.view(torch.int32))
    assert torch.equal(inc_a.view(torch.int32), inc_b.view(torch.int32))


@pytest.mark.parametrize("mag", [1e-9, 1e4])
def test_stem_mc_dgrad_keeps_its_relative_error_at_other_magnitudes_of_dp(mag):
    """dP at 1e-9 and at 1e4 (loss scaling): exact fp32 products and sums scale with dP, so the same bound holds."""
    c = _Case(4, 32, (5, 7, 9), 0, seed=4, mag=mag)
    rc, dx, inc = c.launch(dRaw=torch.zeros(c.dims, device=_dev()))
    assert rc == 0
    e = {"dx": TR.rel_err(dx, c.ref_dx), "dRaw": TR.rel_err(inc, c.ref_inc)}
    print("stem_mc_dgrad dP x %g: %s" % (mag, {k: "%.2e" % v for k, v in e.items()}))
    bad = {k: v for k, v in e.items() if v > TOL}
    assert not bad, bad


def test_stem_mc_dgrad_error_paths_write_nothing():
    c = _Case(2, 32, (3, 4, 5), 0)
    dx = torch.full(c.dims, float("nan"), device=_dev())
    dRaw = torch.full(c.dims, float("nan"), device=_dev())
    for kw in (dict(cin=1), dict(cin=5), dict(cout=16), dict(cout=48), dict(cout=128), dict(dims=(0, 4, 5)),
               dict(dims=(3, 4, -1)), dict(channel=-1), dict(channel=2)):
        rc, _, _ = c.launch(dx=dx, dRaw=dRaw, **kw)
        assert rc == BFM_E_SHAPE, (kw, rc)
    rc, _, _ = c.launch(dx=dx, dRaw=dRaw, null_dp=True)
    assert rc == BFM_E_ARG
    rc, _, _ = c.launch(dx=None, chain=False)                              # neither output asked for
    assert rc == BFM_E_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bool(torch.isnan(dRaw).all())


# ----------------------------------------------------------------------------- 2. the stage-1 training input
def _sigmoid_bound(raw_dev, got):
    """(distance of `got` from the float64 sigmoid, max(2^-23, 2 x the distance of torch.sigmoid in fp32 on the same device
    inputs))."""
    ref = torch.sigmoid(raw_dev.double())
    e_torch = float((torch.sigmoid(raw_dev).double() - ref).abs().max())
    return float((got.double() - ref).abs().max()), max(2.0 ** -23, 2.0 * e_torch)


@pytest.mark.parametrize("with_target", [True, False], ids=["mask", "null"])
@pytest.mark.parametrize("layout", ["rows", "channels_last"])
def test_twostage_train_input(layout, with_target):
    """Channel 0 bit-equal to torch's x * (1 - p_out), channel 1 bit-equal to t (NULL: zeros), p_out within the sigmoid
    bound; raw values include 0, +-1e-30, +-20, +-100; an odd voxel count; both addressings of the head output."""
    L, lib = _lib()
    dev = _dev()
    g = torch.Generator().manual_seed(13)
    n = 3 * 5 * 7
    x = (torch.rand(n, generator=g) * 3.0 - 1.0).to(dev)
    r = 4.0 * torch.randn(n, generator=g)
    r[:9] = torch.tensor([0.0, 1e-30, -1e-30, 20.0, -20.0, 100.0, -100.0, 88.0, -88.0])
    t = (torch.rand(n, generator=g) > 0.5).float().to(dev) if with_target else None
    if layout == "rows":
        buf = torch.zeros((3, n), device=dev)
        buf[1] = r.to(dev)
        off, vs = n, 1
    else:
        buf = torch.zeros((n, 3), device=dev)
        buf[:, 2] = r.to(dev)
        off, vs = 2, 3
    out = torch.full((n, 2), float("nan"), device=dev)
    p_out = torch.full((n,), float("nan"), device=dev)
    masked = torch.full((n,), float("nan"), device=dev)
    rc = lib.bfm_twostage_train_input(L.ptr(x), L.ptr(buf), off, vs, L.ptr(t), n, L.ptr(out), L.ptr(p_out), L.ptr(masked),
                                      L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    want, wm = TR.train_input_ref(x, p_out, t)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    assert torch.equal(masked.view(torch.int32), wm.view(torch.int32))
    e, bound = _sigmoid_bound(r.to(dev), p_out)
    print("twostage_train_input %s: sigmoid distance %.2e (bound %.2e)" % (layout, e, bound))
    assert e <= bound
    rc = lib.bfm_twostage_train_input(L.ptr(x), L.ptr(buf), off, vs, L.ptr(t), n, L.ptr(out), L.ptr(p_out), None,
                                      L.stream_ptr())
    assert rc == 0
    assert lib.bfm_twostage_train_input(None, L.ptr(buf), off, vs, None, n, L.ptr(out), L.ptr(p_out), None,
                                        L.stream_ptr()) == BFM_E_ARG
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 3. the joint iteration
_FIX = {}


def _fixture():
    if not _FIX:
        d = TW.load("train_twostage")
        _FIX["d"] = d
        _FIX["sd"] = {m: TW.fixture_state_dict(d, m) for m in ("pathol", "task")}
    return _FIX["d"], _FIX["sd"]


def _args(d):
    from brainfm_amd import test_utils as TU
    ga, ta = TU.default_inference_args(f_maps=int(d["cfg"][0]), num_levels=int(d["cfg"][1]), left_hemis_only=True,
                                       tasks=dict(TASKS))
    ta.backbone = "unet3d+unet3d"
    ta.condition = None
    ta.losses = Namespace(uncertainty=None, implicit_pathol=False, image_grad=True, registration_grad=True,
                          bias_field_log_type=str(d["bias_field_log_type"]))
    ta.weights = Namespace(image=1.0, image_grad=1.0, seg_ce=1.0, seg_dice=1.0, bias_field_log=1.0, distance=1.0,
                           registration=1.0, registration_grad=1.0, pathol_ce=1.0, pathol_dice=1.0)
    return ga, ta


def _step(scaler=None):
    from brainfm_amd import models as M
    from brainfm_amd import train as T
    d, sds = _fixture()
    ga, ta = _args(d)
    ga, ta, pm, tm = M.build_inpaint_model(ga, ta, _dev())[:4]
    M.load_state_dict_by_suffix(pm, sds["pathol"])
    M.load_state_dict_by_suffix(tm, sds["task"])
    step = T.twostage_train_step(ga, ta, pm, tm, d["weights_ce"], float(d["hyper"][0]), max_surf_distance=float(d["hyper"][1]),
                                 bias_field_log_type=str(d["bias_field_log_type"]), scaler=scaler)
    assert step.loss_names == [str(s) for s in d["loss_names"]]
    w = dict(zip((str(s) for s in d["loss_weight_names"]), (float(v) for v in d["loss_weights"])))
    step.loss_weights = w
    step.pathol_step.loss_weights = dict(w)
    step.task_step.loss_weights = dict(w)
    return d, ga, ta, step


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
def test_joint_iteration_vs_reference(fused, monkeypatch):
    """TwoStageTrainStep.loss_and_grads against the reference's own joint iteration in float64: p within the sigmoid bound
    of the device logits and input_masked bit-equal to torch's x * (1 - p) for every sample, both within max(2e-3, 3 x the float32 run's
    distance) of the float64 run, every loss within 1e-4, every gradient of both models within max(2e-3, 3 x the distance of
    the reference's float32 run) of the float64 gradient's maximum, and stage 0's stem and head gradients closer to the
    coupled float64 gradients than to those with the coupling cut."""
    from brainfm_amd import backward as BW
    monkeypatch.setattr(BW, "STEM_MC_DGRAD", fused)
    tag = "fused" if fused else "generic"
    d, ga, ta, step = _step()
    target, samples = _data(d)
    xs = [s["input"] for s in samples]
    masks = []
    loss_dict, total, grads = step.loss_and_grads(xs, target, samples, masks=masks)
    assert len(masks) == 2
    for i, (raw0, p) in enumerate(masks):                                 # every sample's mask
        e, bound = _sigmoid_bound(raw0.contiguous(), p.reshape(-1))
        print("%s sample %d p against float64 sigmoid of the device logits %.2e (bound %.2e)" % (tag, i, e, bound))
        assert e <= bound
        xi = xs[i].to(_dev())
        assert torch.equal(samples[i]["input_masked"], xi * (1 - p.reshape(xi.shape)))
        for key, got in (("p%d" % i, p), ("input_masked%d" % i, samples[i]["input_masked"])):
            e = float(np.abs(got.cpu().numpy().reshape(-1).astype(np.float64) - d["ref64/" + key].reshape(-1)).max())
            e32 = float(np.abs(d["ref32/" + key].astype(np.float64) - d["ref64/" + key]).max())
            print("%s %s against the float64 run %.2e  ref32 %.2e" % (tag, key, e, e32))
            assert e <= max(2e-3, 3.0 * e32), (key, e, e32)
    assert list(loss_dict.keys()) == ["loss_" + n for n in step.loss_names]
    for k, v in loss_dict.items():
        ref = float(d["ref64/loss/" + k])
        assert abs(v - ref) <= 1e-4 * max(abs(ref), 1e-3), (k, v, ref)
    assert abs(total - float(d["ref64/loss_total"])) <= 1e-4 * float(d["ref64/loss_total"])
    names = [str(s) for s in d["param_names"]]
    got = {k.replace(".", "/", 1): v for k, v in grads.items()}           # 'pathol.<name>' -> 'pathol/<name>'
    assert set(got.keys()) == set(names)
    worst, worst_l2, bad = (0.0, None), 0.0, {}
    for n in names:
        e = _distance(d, None, n, got[n].cpu().numpy())
        e32 = _distance(d, "ref32/", n, None)
        if e > worst[0]:
            worst = (e, n)
        if STEM in n:
            print("%s %-60s hip %.2e  ref32 %.2e" % (tag, n, e, e32))
        if e > max(2e-3, 3.0 * e32):
            bad[n] = (e, e32)
        if "ref64/grad_l2/" + n in d:
            # the parameters held by sampled entries: the whole tensor through its L2 norm, by the same rule
            l64 = float(d["ref64/grad_l2/" + n])
            el = abs(float(got[n].double().norm()) - l64) / l64
            el32 = abs(float(d["ref32/grad_l2/" + n]) - l64) / l64
            worst_l2 = max(worst_l2, el)
            if el > max(2e-3, 3.0 * el32):
                bad[n + " (L2 norm)"] = (el, el32)
    print("%s worst gradient distance %.2e (%s), worst L2-norm distance %.2e" % (tag, worst[0], worst[1], worst_l2))
    assert not bad, bad
    for k in (STEM + "conv.weight", "head.final_conv_pathology.weight"):
        n = "pathol/" + k
        g = got[n].cpu().numpy()
        e_c = _distance(d, None, n, g)
        cut = d["ref64/grad_cut/" + n]
        e_cut = float(np.abs(g.astype(np.float64).reshape(cut.shape) - cut).max() / np.abs(d["ref64/grad/" + n]).max())
        print("%s %-60s to coupled %.2e  to cut %.2e" % (tag, n, e_c, e_cut))
        assert e_c < e_cut, (n, e_c, e_cut)


def _params(step):
    return {k: v.clone() for k, v in step.parameters().items()}


def test_step_updates_both_models_and_skips_both_on_overflow():
    from brainfm_amd import train as T
    scaler = T.LossScaler(init_scale=1024.0)
    d, ga, ta, step = _step(scaler=scaler)
    assert step.scaler is scaler and step.pathol_step.scaler is scaler and step.task_step.scaler is scaler
    target, samples = _data(d)
    xs = [s["input"] for s in samples]
    before = _params(step)
    loss_dict, total, stepped = step.step(xs, target, samples, lr=1e-3)
    assert stepped and np.isfinite(total) and scaler.scale == 1024.0
    after = _params(step)
    for k in ("pathol." + STEM + "conv.weight", "pathol.head.final_conv_pathology.weight", "task." + STEM + "conv.weight",
              "task.head.final_conv_T1.weight"):
        assert not torch.equal(before[k], after[k]), k
    assert step.pathol_step.t == 1 and step.task_step.t == 1
    # overflowing gradients: neither model changes, the one scale halves exactly once
    scaler.scale = 1e38
    loss_dict, total, stepped = step.step(xs, target, [dict(s) for s in samples], lr=1e-3)
    assert not stepped
    assert scaler.scale == 0.5e38
    for k, v in step.parameters().items():
        assert torch.equal(v, after[k]), k
    assert step.pathol_step.t == 1 and step.task_step.t == 1


def test_a_case_without_pathology_trains_as_a_zero_mask():
    """target['pathology'] = 0. (the generator's value for a case without pathology): a zero mask in channel 1, no pathology
    loss in the dictionary, and stage 0 still trains through the mask."""
    d, ga, ta, step = _step()
    target, samples = _data(d)
    xs = [s["input"] for s in samples]
    target["pathology"] = 0.
    loss_dict, total, grads = step.loss_and_grads(xs, target, samples)
    assert "loss_pathol_ce" not in loss_dict and "loss_pathol_dice" not in loss_dict
    assert list(loss_dict.keys()) == ["loss_" + n for n in step.loss_names if not n.startswith("pathol_")]
    assert float(grads["pathol.head.final_conv_pathology.weight"].abs().max()) > 0
    assert float(grads["pathol." + STEM + "conv.weight"].abs().max()) > 0
    before = _params(step)
    _, total, stepped = step.step(xs, target, samples)
    assert stepped and np.isfinite(total)
    assert not torch.equal(step.parameters()["pathol." + STEM + "conv.weight"], before["pathol." + STEM + "conv.weight"])


def test_checkpoints_load_into_the_two_stage_session(tmp_path):
    from brainfm_amd import _lib as L
    from brainfm_amd import twostage as TS
    d, ga, ta, step = _step()
    target, samples = _data(d)
    xs = [s["input"] for s in samples]
    _, _, stepped = step.step(xs, target, samples, lr=1e-3)
    assert stepped
    pp, tp = str(tmp_path / "pathol.pth"), str(tmp_path / "task.pth")
    step.save_checkpoint(pp, tp, epoch=3)
    ga2, ta2 = _args(d)
    sess = TS.TwoStageSession(ga2, ta2, _dev(), pathol_ckp_path=pp, task_ckp_path=tp)
    for model, s_ in ((sess.pathol_model, step.pathol_step), (sess.task_model, step.task_step)):
        sd = model.state_dict()
        for k, v in s_.state_dict().items():
            assert torch.equal(sd[k].cpu().reshape(v.shape), v), k
    eng = sess.task_engine
    dims = tuple(int(v) for v in d["dims"])
    x_cl = eng.to_cl(xs[0].to(_dev()))
    (_, maps0, _), _, xin = sess.run_stages(x_cl, dims, want_feat=False, want_seg=False)
    # a fresh stage-0 forward with the stepped weights, in the training step's own engine
    eng0, tail0 = step.pathol_step.eng, step.pathol_step.tail
    feats = eng0.backbone_cl(x_cl, dims)
    fresh, _, _, _ = tail0.run(feats[-1][0], dims, input_cl=x_cl, want_feat=False, want_seg=False)
    torch.cuda.synchronize()
    assert torch.equal(maps0["pathology"].view(torch.int32), fresh["pathology"].view(torch.int32))
    assert xin.shape == dims + (2,)
