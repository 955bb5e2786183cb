"""The two-stage (pathology-conditioned) inference path on the GPU: the multi-channel stem kernel alone against float64,
the fused mask-and-concat, the engine's dispatch, and the whole flow against the fixtures that
tests/golden/make_golden_twostage.py made by running the reference's own pieces.  Needs an MI355X: run with `-m gpu`."""
import ctypes as C
from argparse import Namespace
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import twostage_weights as TW

pytestmark = pytest.mark.gpu

TOL_PARITY = 1e-4      # single blocks (tests/test_gpu_infer.py:14)
TOL_NET = 1e-3         # whole network (tests/test_gpu_infer.py:17)
TIE = 1e-4             # fp32 relative top-2 gap below which the fixture lists a voxel as a tie
BFM_E_SHAPE = -2

TASKS = dict(T1=True, T2=True, FLAIR=True, CT=True, segmentation=True, distance=True, bias_field=True, registration=True,
             super_resolution=True, surface=False, pathology=True, contrastive=False)


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _relerr(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) / max(1e-6, float(np.abs(b).max()))


def _args(d, backbone="unet3d+unet3d"):
    from brainfm_amd import test_utils as TU
    ga, ta = TU.default_inference_args(f_maps=int(d["cfg"][0]), num_levels=int(d["cfg"][1]), tasks=dict(TASKS))
    ta.backbone = backbone
    return ga, ta


_FIX = {}


def _fixture(stem):
    """(arrays, {prefix: state dict}) of a fixture, loaded (and its drawn weights hashed) once."""
    if stem not in _FIX:
        d = TW.load(stem)
        prefixes = ("model",) if "model/names" in d else ("pathol", "task")
        _FIX[stem] = (d, {p: TW.fixture_state_dict(d, p) for p in prefixes})
    return _FIX[stem]


_SESS = {}


def _session(stem):
    from brainfm_amd import twostage as TS
    if stem not in _SESS:
        d, sds = _fixture(stem)
        ga, ta = _args(d)
        _SESS[stem] = TS.TwoStageSession(ga, ta, _dev(), pathol_state_dict=sds["pathol"], task_state_dict=sds["task"])
    return _SESS[stem]


# ----------------------------------------------------------------------------- 1. the stem kernel alone
def _stem_case(lib, L, cin, cout, dims, seed, rows=True):
    dev = _dev()
    D, H, W = dims
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((D, H, W, cin), generator=g)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g) / np.sqrt(27.0 * cin)
    scale = torch.tensor([[1.0, 100.0, 0.01, 3.0][c] for c in range(cin)]) * (1.0 + 0.1 * torch.rand(cin, generator=g))
    shift = torch.tensor([[0.1, -20.0, 0.002, 0.5][c] for c in range(cin)])
    slope = 0.01
    xa = x.double() * scale.double() + shift.double()                # the affine, then the zero padding
    bound = torch.tensor([float((x * scale + shift).abs().max())])   # one bound for all channels
    ref = F.leaky_relu(F.conv3d(xa.permute(3, 0, 1, 2)[None], w.double(), padding=1), slope)[0].permute(1, 2, 3, 0)
    xd, wd, sc, sh, bd = (t.to(dev).contiguous() for t in (x, w, scale, shift, bound))
    wp = torch.empty(27 * cin * cout, dtype=torch.float32, device=dev)
    L.check(lib.bfm_pack_conv_weights_direct(L.ptr(wd), cin, cout, L.ptr(wp), L.stream_ptr()), "pack_direct")
    out = torch.full((D, H, W, cout), float("nan"), dtype=torch.float32, device=dev)
    n = lib.bfm_conv3x3x3_stem_rows(D, H, W)
    buf = torch.zeros(lib.bfm_moment_rows_bytes(n, cout), dtype=torch.uint8, device=dev) if rows else None
    rc = lib.bfm_conv3x3x3_stem_mc_ex(L.ptr(xd), cin, D, H, W, L.ptr(sc), L.ptr(sh), L.ptr(bd), L.ptr(wp), cout, slope,
                                      L.ptr(out), L.ptr(buf), L.stream_ptr())
    return rc, out, ref, buf, n


@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("cin", [2, 3, 4])
def test_stem_mc_kernel_against_float64(cin, cout):
    """(3,3,3): every voxel on a face; (5,6,37): a full 32-voxel row block and a ragged 5, W no multiple of 32; (2,1,70).
    Channel scales 100x apart under one bound.  The moment rows are the stored output's moments."""
    from brainfm_amd import _lib as L
    lib = L.load()
    for i, dims in enumerate([(3, 3, 3), (5, 6, 37), (2, 1, 70)]):
        rc, out, ref, buf, n = _stem_case(lib, L, cin, cout, dims, seed=100 * cin + cout + i)
        assert rc == 0
        torch.cuda.synchronize()
        e = _relerr(out.cpu().numpy(), ref.numpy())
        print("stem_mc %d -> %d %s: relerr %.2e" % (cin, cout, dims, e))
        assert e <= TOL_PARITY, (dims, e)
        c, k = cout, n * cout
        rs = buf[:k * 8].view(torch.float64).view(n, c).sum(0)
        rq = buf[k * 8:k * 16].view(torch.float64).view(n, c).sum(0)
        # waves without a row block keep +inf / -inf, which min / max ignore
        rmn = buf[k * 16:k * 20].view(torch.float32).view(n, c).min(0)[0]
        rmx = buf[k * 20:k * 24].view(torch.float32).view(n, c).max(0)[0]
        td = out.double().reshape(-1, c)
        tol_s = 2e-7 * float(td.abs().sum(0).max())       # as test_producer_moment_rows_equal_activation_moments
        tol_q = 2e-7 * float((td * td).sum(0).max())
        assert float((rs - td.sum(0)).abs().max()) <= tol_s
        assert float((rq - (td * td).sum(0)).abs().max()) <= tol_q
        assert torch.equal(rmn, out.reshape(-1, c).min(0)[0]) and torch.equal(rmx, out.reshape(-1, c).max(0)[0])


def test_stem_mc_refuses_other_widths():
    from brainfm_amd import _lib as L
    lib = L.load()
    dev = _dev()
    z = torch.zeros(4 * 4 * 4 * 8, dtype=torch.float32, device=dev)
    o = torch.zeros(4 * 4 * 4 * 64, dtype=torch.float32, device=dev)
    w = torch.zeros(27 * 8 * 64, dtype=torch.float32, device=dev)

    def call(cin, cout):
        return lib.bfm_conv3x3x3_stem_mc_ex(L.ptr(z), cin, 4, 4, 4, L.ptr(z), L.ptr(z), L.ptr(z), L.ptr(w), cout, 0.01,
                                            L.ptr(o), None, L.stream_ptr())
    assert call(5, 32) == BFM_E_SHAPE
    assert call(1, 32) == BFM_E_SHAPE
    assert call(2, 48) == BFM_E_SHAPE
    assert call(2, 32) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 2. mask and concat
@pytest.mark.parametrize("n,offset", [(4099, 0), (1024, 0), (777, 1)])
def test_mask_concat2_is_bit_equal_to_torch(n, offset):
    """out[v] = {x * (1 - p), p}: two separately rounded fp32 operations, no fma.  0, 1, denormals and p in {0, 1} included;
    an odd count (the last voxel alone) and sources off 8-byte alignment (the one-voxel-per-lane kernel)."""
    from brainfm_amd import _lib as L
    lib = L.load()
    dev = _dev()
    g = torch.Generator().manual_seed(n)
    x = torch.rand(n + offset, generator=g) * 3.0
    p = torch.rand(n + offset, generator=g)
    special = torch.tensor([0.0, 1.0, 1e-40, -1e-40, 1.4e-45, 1.17549435e-38, 0.3333333, 1.0 - 2.0 ** -24])
    x[offset:offset + 8] = special
    p[offset:offset + 8] = torch.tensor([0.0, 1.0, 0.5, 1.0, 0.0, 0.75, 1e-40, 2.0 ** -25])
    p[offset + 8:offset + 12] = torch.tensor([0.0, 1.0, 0.0, 1.0])
    x, p = x.to(dev)[offset:], p.to(dev)[offset:]
    out = torch.full((n, 2), float("nan"), dtype=torch.float32, device=dev)
    L.check(lib.bfm_mask_concat2(L.ptr(x), L.ptr(p), n, L.ptr(out), L.stream_ptr()), "mask_concat2")
    want = torch.stack([x * (1 - p), p], dim=1)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


# ----------------------------------------------------------------------------- 3. dispatch
def test_engine_takes_the_multichannel_stem(monkeypatch):
    """The 2 -> 32 first layer of the wide stage-1 net runs conv_stem_mc; BFM_STEM_MC=0 restores the direct kernel."""
    from brainfm_amd.engine import UNetEngine
    d, sds = _fixture("twostage_wide")
    f_maps, levels = int(d["cfg"][0]), int(d["cfg"][1])
    dims = tuple(int(v) for v in d["shape"])
    xin = torch.cat([torch.from_numpy(d["input_masked"]), torch.from_numpy(d["p"])], 1)[0].permute(1, 2, 3, 0)
    xin = xin.contiguous().to(_dev())
    eng = UNetEngine(sds["task"], 2, f_maps, levels, 8, True, device=_dev())
    ly = eng.enc[0][0]
    assert (ly.cin, ly.cout) == (2, 32)
    got = eng.single_conv(ly, xin, dims)
    assert ly.kind == "stem_mc"
    assert hasattr(got, "_bfm_rows")
    monkeypatch.setenv("BFM_STEM_MC", "0")
    eng0 = UNetEngine(sds["task"], 2, f_maps, levels, 8, True, device=_dev())
    ref = eng0.single_conv(eng0.enc[0][0], xin, dims)
    assert eng0.enc[0][0].kind == "direct"
    e = _relerr(got.cpu().numpy(), ref.cpu().numpy())
    print("stem_mc against the direct kernel: %.2e" % e)
    assert e <= TOL_PARITY


# ----------------------------------------------------------------------------- 4. end to end
def _samples_of(out, d):
    """The fixture's sampled entries of an output dict: {name: values}."""
    idx = torch.from_numpy(d["idx"])
    got = OrderedDict()
    for j, k in enumerate(str(s) for s in d["float_keys"]):
        got[k] = (out[k].detach().cpu().reshape(-1)[idx].numpy(), j)
    seg = out["segmentation"].detach().cpu()
    got["segmentation"] = (seg[0].reshape(seg.shape[1], -1)[:, torch.from_numpy(d["seg_idx"])].numpy(), None)
    for k in (str(s) for s in d["feat_keys"]):
        assert isinstance(out[k], list)
        for i, f in enumerate(out[k]):
            assert tuple(f.shape) == tuple(d["%s%d_shape" % (k, i)]), (k, i, tuple(f.shape))
            got["%s%d" % (k, i)] = (f.detach().cpu().reshape(-1)[torch.from_numpy(d["%s%d_idx" % (k, i)])].numpy(), None)
    return got


def _ref_of(d, name, j, prefix=""):
    if j is not None:
        return d[prefix + "floats"][j]
    if name == "segmentation":
        return d[prefix + "seg"]
    return d[prefix + name + "_vals"]


def _check_labels(out, d, what):
    lab = out["label"]
    assert lab.dtype == torch.int64 and tuple(lab.shape[2:]) == tuple(d["shape"])
    got = lab.detach().cpu().numpy().reshape(-1)
    want = d["label"].reshape(-1).astype(np.int64)
    flips = np.nonzero(got != want)[0]
    ties = {int(i): float(gp) for i, gp in zip(d["tie_idx"], d["tie_gap"])}
    for i in flips:
        print("%s: label flip at voxel %d (%d for %d), reference top-2 gap %s"
              % (what, i, got[i], want[i], ties.get(int(i), ">= %g" % TIE)))
    assert all(int(i) in ties for i in flips), "%s: %d label flips outside the listed ties" % (what, len(flips))


def _check_against_ref64(out, d, what):
    """relerr(hip, ref64) <= max(TOL_NET, 3 * relerr(ref32, ref64)) for every key: the reference's own fp32-to-fp64
    distance is the yardstick, three times because stage 0's error re-enters as stage 1's input."""
    assert sorted(out.keys()) == sorted(str(s) for s in d["out_keys"])
    for name, (got, j) in _samples_of(out, d).items():
        r32, r64 = _ref_of(d, name, j), _ref_of(d, name, j, "ref64/")
        e, e_ref = _relerr(got, r64), _relerr(r32, r64)
        print("%s %-20s hip-ref64 %.2e   ref32-ref64 %.2e   hip-ref32 %.2e" % (what, name, e, e_ref, _relerr(got, r32)))
        assert e <= max(TOL_NET, 3.0 * e_ref), (what, name, e, e_ref)
    _check_labels(out, d, what)


@pytest.mark.parametrize("stem", ["twostage_small", "twostage_wide"])
def test_twostage_session_against_the_reference(stem):
    d, _ = _fixture(stem)
    s = _session(stem)
    x = torch.from_numpy(d["x"]).to(_dev())
    out = s.evaluate(x, feature_only=False)
    e = _relerr(out["pathology"].cpu().numpy(), d["ref64/p"])
    print("%s stage-0 p: hip-ref64 %.2e   ref32-ref64 %.2e" % (stem, e, _relerr(d["p"], d["ref64/p"])))
    _check_against_ref64(out, d, stem)
    fp, ft = s.evaluate(x, feature_only=True)
    assert torch.equal(fp, out["feat_pathol"][-1]) and torch.equal(ft, out["feat_task"][-1])
    if stem == "twostage_wide":
        assert s.task_engine.enc[0][0].kind == "stem_mc"          # the new stem is what ran


@pytest.mark.parametrize("stem", ["twostage_small", "twostage_wide"])
def test_evaluate_image_twostage_from_checkpoints_and_yaml_files(stem, tmp_path):
    """utils/test_utils.py:316-350 through its front door: cfg files, two checkpoints in scripts/train.py's layout."""
    from brainfm_amd import test_utils as TU
    from brainfm_amd import twostage as TS
    d, sds = _fixture(stem)
    f_maps, levels = int(d["cfg"][0]), int(d["cfg"][1])
    gen_default = tmp_path / "gen_default.yaml"
    gen_default.write_text("task:\n" + "".join("  %s: %s\n" % kv for kv in TASKS.items())
                           + "max_surf_distance: 3.0\ngenerator:\n  size: [160, 160, 160]\n  left_hemis_only: False\n")
    train_default = tmp_path / "train_default.yaml"
    train_default.write_text(
        "backbone: unet3d\nin_channels: 1\nf_maps: 64\nlayer_order: gcl\nnum_groups: 8\nnum_levels: 6\nunit_feat: True\n"
        "task_f_maps: [64]\nlosses:\n  uncertainty: null\n  implicit_pathol: False\n")
    model_cfg = tmp_path / "twostage.yaml"
    model_cfg.write_text("backbone: unet3d+unet3d\nf_maps: %d\nnum_levels: %d\ntask_f_maps: [%d]\n" % (f_maps, levels, f_maps))
    paths = {}
    for prefix in ("pathol", "task"):
        paths[prefix] = tmp_path / ("%s.pth" % prefix)
        torch.save({"model": {"module." + k: v for k, v in sds[prefix].items()}, "epoch": 3,
                    "train_args": Namespace(f_maps=f_maps)}, str(paths[prefix]))
    prev = (TU.default_gen_cfg_file, TU.default_train_cfg_file, TU.default_val_file)
    TU.default_gen_cfg_file, TU.default_train_cfg_file, TU.default_val_file = str(gen_default), str(train_default), None
    try:
        x = torch.from_numpy(d["x"]).to(_dev())
        out = TS.evaluate_image_twostage(x, str(paths["pathol"]), str(paths["task"]), feature_only=False, device=0,
                                         model_cfg=str(model_cfg))
        _check_against_ref64(out, d, stem + " (files)")
        n_before = len(TU._SESSIONS)
        fp, ft = TS.evaluate_image_twostage(x, str(paths["pathol"]), str(paths["task"]), device=0, model_cfg=str(model_cfg))
        assert len(TU._SESSIONS) == n_before                          # both models stay resident
        assert torch.equal(ft, out["feat_task"][-1]) and torch.equal(fp, out["feat_pathol"][-1])
    finally:
        TU.default_gen_cfg_file, TU.default_train_cfg_file, TU.default_val_file = prev


def _postprocessed(model, processors, ga, ta, samples, **kw):
    from brainfm_amd import models as M
    outs, _ = model(samples, **kw)
    for p in processors:
        outs = p(outs, samples)
    outs, _, _ = M.get_postprocessor(ga, ta, outs, samples, target=None, feats=None, tasks=ga.tasks)
    return outs[0]


def test_stage1_teacher_forced_with_the_reference_p():
    """Stage 1 alone on the fixture's p and input_masked, through model(samples, input_name='input_masked', cond=[p]):
    every float map and feature within TOL_NET of the reference's fp32 values on the wide net."""
    d, _ = _fixture("twostage_wide")
    s = _session("twostage_wide")
    dev = _dev()
    samples = [{"input": torch.from_numpy(d["x"]).to(dev), "input_masked": torch.from_numpy(d["input_masked"]).to(dev)}]
    out = _postprocessed(s.task_model, s.task_processors, s.gen_args, s.train_args, samples, input_name="input_masked",
                         cond=[torch.from_numpy(d["p"]).to(dev)])
    assert "high_res" in out and "pathology" not in out and isinstance(out["feat_task"], list)
    full = dict(out, pathology=torch.from_numpy(d["p"]), feat_pathol=[])     # stage 0 did not run: the fixture's own p
    for name, (got, j) in _samples_of(full, d).items():
        if name == "pathology":
            continue
        e = _relerr(got, _ref_of(d, name, j))
        print("teacher-forced %-20s hip-ref32 %.2e" % (name, e))
        assert e <= TOL_NET, (name, e)
    _check_labels(out, d, "teacher-forced")


# ----------------------------------------------------------------------------- 5. the conditioned model
def test_conditioned_model_against_the_reference():
    """build_conditioned_model, condition 'mask+flip': three input channels through model(samples, cond=cond)."""
    from brainfm_amd import models as M
    d, sds = _fixture("conditioned_wide")
    ga, ta = _args(d, backbone="unet3d")
    ta.condition = "mask+flip"
    ga, ta, model, processors, _, _ = M.build_conditioned_model(ga, ta, _dev())
    M.load_state_dict_by_suffix(model, sds["model"])
    x = torch.from_numpy(d["x"]).to(_dev())
    cond = [torch.concat([torch.flip(x, dims=[2]), (x != 0).to(x.dtype)], dim=1)]
    out = _postprocessed(model, processors, ga, ta, [{"input": x}], cond=cond)
    assert sorted(out.keys()) == sorted(str(s) for s in d["out_keys"])
    ly = model.backbone.engine(model.head).enc[0][0]
    assert (ly.cin, ly.cout, ly.kind) == (3, 32, "stem_mc")
    for name, (got, j) in _samples_of(out, d).items():
        e = _relerr(got, _ref_of(d, name, j))
        print("conditioned %-20s hip-ref32 %.2e" % (name, e))
        assert e <= TOL_NET, (name, e)
    _check_labels(out, d, "conditioned")


# ----------------------------------------------------------------------------- 6. tiles
def test_tiled_inference_twostage_equals_the_per_tile_stitch():
    from brainfm_amd import test_utils as TU
    from brainfm_amd import twostage as TS
    s = _session("twostage_small")
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    full = torch.zeros(1, 1, 40, 40, 56)
    full[:, :, 5:35, 4:36, 6:50] = torch.rand(1, 1, 30, 32, 44, generator=g)            # a zero border
    full = full.to(dev)
    acc, ranges, cnt = TS.tiled_inference_twostage(full, s, stride=[16] * 3, win_size=[32] * 3)
    keys = list(acc.keys())
    assert keys == [k for k in TU.STITCH_KEYS + ["pathology"] if k in keys] and "pathology" in keys and "label" in keys
    assert len(keys) == 17                                            # the 16 keys without the atlas, and pathology
    assert len(ranges) > 1
    want = {k: torch.zeros(40, 40, 56, device=dev) for k in keys}
    for (x0, x1), (y0, y1), (z0, z1) in ranges:
        im = full[:, :, x0:x1, y0:y1, z0:z1]
        o = s.evaluate(im, feature_only=False)
        mask = (im != 0).to(torch.float32)
        for k in keys:
            v = torch.squeeze(o[k] * mask)
            if k == "label":
                v = v.to(torch.int).to(torch.float32)
            want[k][x0:x1, y0:y1, z0:z1] += v
    for k in keys:
        w = want[k] / cnt.reshape(want[k].shape)
        e = _relerr(acc[k].cpu().numpy(), w.cpu().numpy())
        assert e <= TOL_PARITY, (k, e)


# ----------------------------------------------------------------------------- 7. the shortcut guard
def test_multichannel_engine_takes_no_one_channel_shortcut():
    """A stage-1 engine whose image channel has a constant zero slab while p varies there: the uniform-box and tile-mask
    shortcuts read ONE input channel, so they must stay off -- same bits with their switches off."""
    from brainfm_amd.engine import UNetEngine
    d, sds = _fixture("twostage_wide")
    dev = _dev()
    eng = UNetEngine(sds["task"], 2, int(d["cfg"][0]), int(d["cfg"][1]), 8, True, device=dev)
    dims = (24, 24, 64)
    g = torch.Generator().manual_seed(5)
    xin = torch.rand(dims + (2,), generator=g)
    xin[:, :, :40, 0] = 0                                             # the masked image is zero, the probability is not
    xin = xin.to(dev)
    assert eng.uniform_skip and eng.mask_skip
    a = [f.clone() for f, _ in eng.backbone_cl(xin, dims, mask_last=True)]
    assert eng.uniform_flags(xin, dims, 2) is None
    eng.uniform_skip = False
    eng.mask_skip = False
    b = [f for f, _ in eng.backbone_cl(xin, dims, mask_last=True)]
    assert len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))
