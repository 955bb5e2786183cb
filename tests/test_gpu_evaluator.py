"""The evaluator on the device (brainfm_amd/evaluator.py, csrc/eval_metrics.hip).  Needs an MI355X: run with `-m gpu`.

Rule for every float score: |hip - ref64| <= max(1e-6, 8 |ref32 - ref64|), relative to |ref64| where that exceeds 1 (PSNR).
ref64 / ref32 are the reference's own values on float64 / fp32 tensors (tests/golden/evaluator.npz, made by running the
reference's Evaluator), or, for SSIM and MS-SSIM, tests/ssim_refs.py in float64 / fp32 on the CPU.

SSIM parity is with that restatement of pytorch_msssim 1.0's public algorithm, NOT with the library: pytorch_msssim is not
installed where this project is built, so the library itself is unpinned.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import ssim_refs as SR
from conftest import load_npz, sd_from_npz

pytestmark = pytest.mark.gpu

NS = types.SimpleNamespace


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _fx():
    return load_npz("evaluator.npz")


def _ev(names=("feat_l1",), sigma=None):
    from brainfm_amd import evaluator as E
    return E.Evaluator(NS() if sigma is None else NS(ssim_win_sigma=sigma), list(names), _dev())


def _rule(tag, got, ref64, ref32):
    got, ref64, ref32 = float(got), float(ref64), float(ref32)
    scale = max(1.0, abs(ref64))
    dist, yard = abs(got - ref64) / scale, abs(ref32 - ref64) / scale
    print("DIST %-44s hip-ref64 %.3e   ref32-ref64 %.3e   value %.9g" % (tag, dist, yard, got))
    assert dist <= max(1e-6, 8.0 * yard), (tag, got, ref64, ref32)


# --------------------------------------------------------------------------------------------------------------- SSIM
SSIM_SHAPES = [(11, 11, 11), (12, 13, 27), (8, 16, 40), (19, 40, 75), (2, 3, 12, 13, 27)]


@functools.lru_cache(maxsize=None)
def _ssim_case(shape, sigma):
    o, t = SR.smooth_pair(shape, seed=7 + len(shape) + shape[-1])
    o5 = o.reshape((1,) * (5 - o.dim()) + tuple(o.shape))
    t5 = t.reshape(o5.shape)
    r64 = float(SR.get_ssim(o5.double(), t5.double(), sigma))
    r32 = float(SR.get_ssim(o5, t5, sigma))
    return o, t, r64, r32


def _ssim_dev(o, t, sigma, fused):
    """mean over (b, c) of the per-plane SSIM means, in fp64, through get_ssim's own steps"""
    from brainfm_amd import evaluator as E
    o5, t5 = E._pair(o, t, _dev(), "test")
    stats = E.pair_stats_dev(o5, t5)
    res = E.ssim_planes_dev(o5, t5, E.gaussian_window(sigma), stats[5:9], fused=fused)
    B, Cc = o5.shape[:2]
    return res, float(res.cpu().numpy()[:, 0].reshape(B, Cc).mean(1).mean())


@pytest.mark.parametrize("sigma", [1.5, 0.8])
@pytest.mark.parametrize("shape", SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_fused_vs_restatement_and_composed_route(shape, sigma, monkeypatch):
    o, t, r64, r32 = _ssim_case(shape, sigma)
    assert 0.05 < r64 < 0.95
    tag = "ssim %s sigma %.1f" % ("x".join(map(str, shape)), sigma)
    raw1, fused = _ssim_dev(o, t, sigma, True)
    _rule(tag + " fused", fused, r64, r32)
    _, comp = _ssim_dev(o, t, sigma, False)
    _rule(tag + " composed", comp, r64, r32)
    print("DIST %-44s fused-composed %.3e" % (tag, abs(fused - comp)))
    assert abs(fused - comp) <= max(1e-6, 8.0 * abs(r32 - r64))
    raw2, again = _ssim_dev(o, t, sigma, True)
    assert torch.equal(raw1, raw2) and fused == again                         # the same bits on every run
    # the public entry: fp32 0-d numpy value, and the switch
    ev = _ev(sigma=sigma)
    got = ev.get_ssim("feat_ssim", o.to(_dev()), t.to(_dev()))["feat_ssim"]
    assert isinstance(got, np.ndarray) and got.shape == () and got.dtype == np.float32
    assert got == np.float32(fused)
    monkeypatch.setenv("BFM_SSIM_FUSED", "0")
    assert ev.get_ssim("feat_ssim", o, t)["feat_ssim"] == np.float32(comp)


def test_ssim_of_a_constant_volume_is_nan_and_2d_is_refused():
    ev = _ev()
    o, t, _, _ = _ssim_case((12, 13, 27), 1.5)
    assert np.isnan(ev.get_ssim("m", torch.full((12, 13, 27), 0.25), t)["m"])
    assert np.isnan(ev.get_ms_ssim("m", torch.full((16, 161, 161), 0.25), torch.rand(16, 161, 161))["m"])
    with pytest.raises(NotImplementedError):
        ev.get_ssim("m", torch.rand(1, 1, 1, 20, 20), torch.rand(1, 1, 1, 20, 20))
    assert float(ev.get_ssim("m", o, o)["m"]) == 1.0


def test_ms_ssim_smallest_passing_size_and_the_size_check(capsys):
    shape = (24, 161, 162)
    o, t = SR.smooth_pair(shape, seed=11)
    r64 = float(SR.get_ms_ssim(o[None, None].double(), t[None, None].double()))
    r32 = float(SR.get_ms_ssim(o[None, None], t[None, None]))
    assert 0.05 < r64 < 0.99
    from brainfm_amd import evaluator as E
    o5, t5 = E._pair(o, t, _dev(), "test")
    w = np.asarray(E.MS_WEIGHTS)[:, None]

    def run(fused):
        stats = E.pair_stats_dev(o5, t5)
        res = E.ms_ssim_levels_dev(o5, t5, E.gaussian_window(1.5), stats[5:9], fused=fused).cpu().numpy()
        lev = np.maximum(np.concatenate([res[:-1, :, 1], res[-1:, :, 0]], axis=0), 0.0)
        return res, float(np.prod(lev ** w, axis=0).mean())

    res1, fused = run(True)
    _, comp = run(False)
    with capsys.disabled():                                                  # the distances belong in the log
        _rule("ms_ssim 24x161x162 fused", fused, r64, r32)
        _rule("ms_ssim 24x161x162 composed", comp, r64, r32)
    res2, again = run(True)
    assert np.array_equal(res1, res2) and fused == again
    ev = _ev()
    got = ev.get_ms_ssim("sr_ms_ssim", o, t)["sr_ms_ssim"]
    assert got.dtype == np.float32 and got == np.float32(fused)
    capsys.readouterr()
    small = ev.get_ms_ssim("sr_ms_ssim", torch.rand(24, 160, 161), torch.rand(24, 160, 161))["sr_ms_ssim"]
    assert isinstance(small, float) and np.isnan(small)
    assert "Image too small for Multi-scale SSIM" in capsys.readouterr().out


# --------------------------------------------------------------------------------------------------------- label Dice
@pytest.mark.parametrize("tag", ["a", "b"])
def test_label_counts_are_exact_and_the_dice_follows_the_rule(tag):
    from brainfm_amd import evaluator as E
    fx = _fx()
    P, T = fx["lab_p_" + tag].astype(np.int64), fx["lab_t_" + tag].astype(np.int64)
    lut = np.zeros(10000, dtype=np.int64)
    for l, lab in enumerate(E.label_list_segmentation):
        lut[lab] = l
    p, t = lut[P], lut[T]
    cp, ct, ci = E.label_counts(P, T, _dev())
    assert np.array_equal(cp, np.bincount(p.ravel(), minlength=33))
    assert np.array_equal(ct, np.bincount(t.ravel(), minlength=33))
    assert np.array_equal(ci, np.bincount(p[p == t].ravel(), minlength=33))
    assert cp[0] > (P == 0).sum()                                            # labels outside the list went to class 0
    ev = _ev(["seg_dice"])
    for pp, tt in ((P, T), (torch.from_numpy(P).to(_dev()), torch.from_numpy(T).to(_dev())), (P.astype(np.float64), T)):
        got = ev.eval_tensors(pp, tt, is_seg=True)["seg_dice"]
        assert got.dtype == np.float32 and got.shape == ()
        _rule("label dice " + tag, got, fx["labdice_%s_64" % tag], fx["labdice_%s_32" % tag])
    # the one-hot route stays available and agrees
    hp, ht = E.get_onehot(P, _dev()), E.get_onehot(T, _dev())
    assert tuple(hp.shape) == (33,) + P.shape and hp.dtype == torch.float32
    assert np.array_equal(hp.cpu().numpy().argmax(0), p) and float(hp.sum()) == P.size
    _rule("onehot dice " + tag, ev.get_dice("m", hp[None], ht[None])["m"], fx["labdice_%s_64" % tag],
          fx["labdice_%s_32" % tag])


def test_label_counts_of_structured_volumes_are_exact():
    """Blocks of one label (whole waves hit one histogram bin: the aggregated add) next to noisy regions and a ragged tail
    (lanes of a wave disagree: the per-lane add), sizes that are no multiple of 4, and pointers that are not 16-byte aligned."""
    from brainfm_amd import evaluator as E
    rs = np.random.RandomState(9)
    labs = np.array(E.label_list_segmentation)
    lut = np.zeros(10000, dtype=np.int64)
    for l, lab in enumerate(E.label_list_segmentation):
        lut[lab] = l
    for shape in ((24, 40, 72), (9, 21, 67)):
        coarse = labs[rs.randint(0, len(labs), size=tuple(-(-n // 8) for n in shape))] * (rs.rand(*tuple(-(-n // 8) for n in shape)) < 0.6)
        T = np.kron(coarse, np.ones((8, 8, 8), dtype=np.int64))[:shape[0], :shape[1], :shape[2]]
        P = np.roll(T, 3, axis=1)
        noisy = rs.rand(*shape) < 0.1
        P[noisy] = labs[rs.randint(0, len(labs), size=int(noisy.sum()))]
        p, t = lut[P], lut[T]
        want = (np.bincount(p.ravel(), minlength=33), np.bincount(t.ravel(), minlength=33),
                np.bincount(p[p == t].ravel(), minlength=33))
        for off in (0, 1):
            n = P.size
            dp = torch.empty(n + off, dtype=torch.int32, device=_dev())[off:].copy_(torch.from_numpy(P.ravel().astype(np.int32)))
            dt = torch.empty(n + off, dtype=torch.int32, device=_dev())[off:].copy_(torch.from_numpy(T.ravel().astype(np.int32)))
            got = E.label_counts(dp, dt, _dev())
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (shape, off)


def test_a_label_outside_the_lut_raises_index_error():
    from brainfm_amd import evaluator as E
    ev = _ev(["seg_dice"])
    P = np.zeros((7, 5, 3), dtype=np.int64)
    for bad in (10000, -1):
        Q = P.copy()
        Q[3, 2, 1] = bad
        with pytest.raises(IndexError):
            ev.eval_tensors(Q, P, is_seg=True)
        with pytest.raises(IndexError):
            ev.eval_tensors(P, Q, is_seg=True)
        with pytest.raises(IndexError):
            E.get_onehot(Q, _dev())
    Q = P.copy()
    Q[0, 0, 0] = 9999
    assert float(ev.eval_tensors(Q, P, is_seg=True)["seg_dice"]) == pytest.approx(1.0 / 33, abs=1e-7)


# ------------------------------------------------------------------------------------------ scalar metrics, soft Dice
def test_scalar_metrics_and_soft_dice_vs_the_reference_fixture():
    fx = _fx()
    ev = _ev()
    dev = _dev()
    o, t = torch.from_numpy(fx["o"]).to(dev), torch.from_numpy(fx["t"]).to(dev)
    assert o.numel() % 4 and o.numel() > 2048                                # a tail and more than one block
    # the same values behind pointers that are not 16-byte aligned: the scalar path
    ou = torch.empty(o.numel() + 1, device=dev)[1:].view(o.shape).copy_(o)
    tu = torch.empty(t.numel() + 1, device=dev)[1:].view(t.shape).copy_(t)
    assert ou.data_ptr() % 16 == 4 and ou.is_contiguous()
    for tag, a, b in (("aligned", o, t), ("unaligned", ou, tu)):
        l1 = ev.get_l1("m", a, b)["m"]
        assert isinstance(l1, np.ndarray) and l1.shape == () and l1.dtype == np.float32
        _rule("l1 " + tag, l1, fx["l1_64"], fx["l1_32"])
        psnr = ev.get_psnr("m", a, b)["m"]
        assert isinstance(psnr, float)
        _rule("psnr " + tag, psnr, fx["psnr_64"], fx["psnr_32"])
        _rule("normalized_l2 " + tag, ev.get_normalized_l2("m", a, b)["m"], fx["nl2_64"], fx["nl2_32"])
    nz = ev.get_l1("m", o, t, nonzero_only=True)["m"]
    r64, r32 = fx["l1nz_64"], fx["l1nz_32"]
    assert nz.shape == r64.shape == tuple(o.shape[1:]) and nz.dtype == np.float32
    assert np.array_equal(np.isnan(nz), np.isnan(r64)) and np.isnan(nz).sum() == int((fx["t"] == 0).sum())
    ok = ~np.isnan(r64)
    dist, yard = np.abs(nz[ok] - r64[ok]), np.abs(r32[ok] - r64[ok])
    print("DIST %-44s hip-ref64 %.3e   ref32-ref64 %.3e" % ("l1 nonzero_only (max over voxels)", dist.max(), yard.max()))
    assert bool((dist <= np.maximum(1e-6, 8.0 * yard)).all())
    # all-zero target
    z = torch.zeros_like(t)
    _rule("l1 zero target", ev.get_l1("m", o, z)["m"], fx["z_l1_64"], fx["z_l1_32"])
    _rule("normalized_l2 zero target", ev.get_normalized_l2("m", o, z)["m"], fx["z_nl2_64"], fx["z_nl2_32"])
    assert bool(np.isnan(ev.get_l1("m", o, z, nonzero_only=True)["m"]).all())
    with pytest.raises(ValueError):                                         # log10(0), as in the reference
        ev.get_psnr("m", o, z)
    assert ev.get_psnr("m", o, o)["m"] == float("inf")
    assert float(ev.get_l1("m", o, o)["m"]) == 0.0
    # soft Dice
    do, dt = torch.from_numpy(fx["dice_o"]).to(dev), torch.from_numpy(fx["dice_t"]).to(dev)
    d = ev.get_dice("seg_dice", do, dt)["seg_dice"]
    assert d.dtype == np.float32 and d.shape == ()
    _rule("soft dice", d, fx["dice_64"], fx["dice_32"])
    assert float(ev.get_dice("m", torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 2, 4, 4, 4))["m"]) == 0.0   # the 1e-5 clamp
    # get_score dispatches by name and refuses unknown names
    assert ev.get_score("bf_corrected_l1", o, t)["bf_corrected_l1"] == ev.get_l1("m", o, t)["m"]
    with pytest.raises(AssertionError):
        ev.get_score("nonsense", o, t)


# --------------------------------------------------------------------------------------------------------------- eval
def test_eval_round_trip_through_files_equals_eval_tensors(tmp_path):
    from brainfm_amd import evaluator as E, volio
    rs = np.random.RandomState(3)
    aff = np.diag([1.0, 1.0, 1.0, 1.0])
    pred = (rs.rand(10, 12, 14) * 1.4 - 0.2).astype(np.float32)
    target = rs.rand(11, 12, 13).astype(np.float32)
    target[rs.rand(11, 12, 13) < 0.3] = 0
    pp, tp = str(tmp_path / "pred_T1.nii.gz"), str(tmp_path / "gt_T1.nii.gz")
    volio.MRIwrite(pred, aff, pp)
    volio.MRIwrite(target, aff, tp)
    names = ["recon_l1", "recon_psnr", "recon_ssim", "bf_normalized_l2"]
    ev = _ev(names)
    got = ev.eval(pp, tp, clamp=True, normalize=True, add_mask=True, flip=True)
    assert sorted(got) == sorted(names)
    # the same steps by hand (evaluator.py:149-179)
    p, t = pred[:10, :12, :13].astype(np.float64), target[:10, :12, :13].astype(np.float64)        # align_shape
    p = np.flip(p, 0).copy()
    p[t == 0] = 0
    p[p < 0] = 0
    masked = volio.MRIread(str(tmp_path / "pred_T1_masked.nii.gz"), im_only=True)
    assert np.array_equal(masked, p)
    p = (p - p.min()) / (p.max() - p.min())
    want = ev.eval_tensors(torch.tensor(p, dtype=torch.float32), torch.tensor(t, dtype=torch.float32), clamp=True)
    for k in names:
        assert got[k] == want[k], k
    pc, tc = np.clip(p.astype(np.float32).astype(np.float64), 0, 1), np.clip(t, 0, 1)
    assert abs(float(got["recon_l1"]) - np.abs(pc - tc).mean()) < 1e-6
    # normalize inside eval_tensors (device min / max) gives the same volume as the host normalisation up to fp32 rounding
    raw = torch.tensor(np.where(t == 0, 0, np.maximum(np.flip(pred[:10, :12, :13].astype(np.float64), 0), 0)),
                       dtype=torch.float32)
    dn = ev.eval_tensors(raw, torch.tensor(t, dtype=torch.float32), clamp=True, normalize=True)
    assert abs(float(dn["recon_l1"]) - float(got["recon_l1"])) < 1e-6
    # a file that is already masked is not written again
    got2 = ev.eval(str(tmp_path / "pred_T1_masked.nii.gz"), tp, add_mask=True)
    assert not (tmp_path / "pred_T1_masked_masked.nii.gz").exists() and sorted(got2) == sorted(names)

    # label files: 'label' in the name reads integers; kill_target_labels zeroes both volumes
    labs = np.array(E.label_list_segmentation + [5])
    T = labs[rs.randint(0, len(labs), size=(9, 8, 7))]
    P = np.where(rs.rand(9, 8, 7) < 0.3, labs[rs.randint(0, len(labs), size=(9, 8, 7))], T)
    lp, lt = str(tmp_path / "pred_label.nii.gz"), str(tmp_path / "gt_label.nii.gz")
    volio.MRIwrite(P.astype(np.int16), aff, lp)
    volio.MRIwrite(T.astype(np.int16), aff, lt)
    evs = _ev(["seg_dice"])
    got = evs.eval(lp, lt, is_seg=True, kill_target_labels=[2, 41], clamp=True)
    Pk, Tk = np.where(np.isin(P, [2, 41]), 0, P), np.where(np.isin(T, [2, 41]), 0, T)
    assert got["seg_dice"] == evs.eval_tensors(Pk, Tk, is_seg=True)["seg_dice"]
    lut = np.zeros(10000, dtype=np.int64)
    for l, lab in enumerate(E.label_list_segmentation):
        lut[lab] = l
    a, b = lut[Pk], lut[Tk]
    dice = np.mean([2.0 * ((a == l) & (b == l)).sum() / max(((a == l).sum() + (b == l).sum()), 1e-5) for l in range(33)])
    assert abs(float(got["seg_dice"]) - dice) < 1e-6
    assert not np.array_equal(a, lut[P])                                     # the kill list changed something


# --------------------------------------------------------------------------------------------------------------- flow
def test_scores_of_evaluate_image_outputs_without_leaving_the_device(tmp_path):
    """evaluate_image on the small golden net, then eval_tensors straight on its device outputs, against the same scores
    from the outputs copied to the host."""
    from argparse import Namespace
    from brainfm_amd import evaluator as E, models as M, test_utils as TU
    d = load_npz("infer_small.npz")
    f_maps, levels = int(d["cfg"][0]), int(d["cfg"][1])
    gen_default = tmp_path / "gen_default.yaml"
    gen_default.write_text(
        "task:\n  T1: True\n  T2: True\n  FLAIR: True\n  CT: True\n  segmentation: True\n  distance: True\n"
        "  bias_field: True\n  registration: True\n  super_resolution: True\n  surface: False\n  pathology: False\n"
        "  contrastive: False\nmax_surf_distance: 2.0\ngenerator:\n  size: [128, 128, 128]\n  left_hemis_only: False\n")
    gen_test = tmp_path / "gen_test.yaml"
    gen_test.write_text("max_surf_distance: 3.0\ngenerator:\n  size: [160, 160, 160]\n")
    train_default = tmp_path / "train_default.yaml"
    train_default.write_text(
        "backbone: unet3d\nin_channels: 1\nf_maps: 64\nlayer_order: gcl\nnum_groups: 8\nnum_levels: 6\nunit_feat: True\n"
        "task_f_maps: [64]\nlosses:\n  uncertainty: null\n  implicit_pathol: False\nlr: 1e-4\n")
    model_cfg = tmp_path / "model_test.yaml"
    model_cfg.write_text("f_maps: %d\nnum_levels: %d\ntask_f_maps: [%d]\n" % (f_maps, levels, f_maps))
    ckp = tmp_path / "brainfm_pretrained.pth"
    torch.save({"model": {"module." + k: v for k, v in sd_from_npz(d).items()}, "epoch": 7,
                "train_args": Namespace(f_maps=f_maps)}, str(ckp))
    prev = (TU.default_gen_cfg_file, TU.default_train_cfg_file, TU.default_val_file)
    TU.default_gen_cfg_file, TU.default_train_cfg_file, TU.default_val_file = str(gen_default), str(train_default), None
    try:
        x = torch.from_numpy(d["x"]).to(_dev())
        out = TU.evaluate_image(x, str(ckp), feature_only=False, device=0, gen_cfg=str(gen_test), model_cfg=str(model_cfg))
    finally:
        TU.default_gen_cfg_file, TU.default_train_cfg_file, TU.default_val_file = prev
    lab, img = out["label"], out["T1"]
    assert lab.is_cuda and img.is_cuda
    # "ground truth": the outputs shifted by one voxel, so that the scores are not trivial
    lab_gt, img_gt = torch.roll(lab, 1, dims=-1), torch.roll(img, 1, dims=-2)
    seg = M.get_evaluator(NS(), ["segmentation"], _dev())
    got = seg.eval_tensors(lab.squeeze(), lab_gt.squeeze(), is_seg=True)["seg_dice"]
    lut = np.zeros(10000, dtype=np.int64)
    for l, v in enumerate(E.label_list_segmentation):
        lut[v] = l
    a, b = lut[lab.squeeze().cpu().numpy()], lut[lab_gt.squeeze().cpu().numpy()]
    dice = np.mean([2.0 * ((a == l) & (b == l)).sum() / max(((a == l).sum() + (b == l).sum()), 1e-5) for l in range(33)])
    print("DIST %-44s hip-host %.3e   value %.9g" % ("flow seg_dice", abs(float(got) - dice), float(got)))
    assert abs(float(got) - dice) <= 1e-6 and 0.0 < dice < 1.0
    sr = M.get_evaluator(NS(), ["super_resolution"], _dev())
    assert sr.metric_names == ["sr_l1", "sr_psnr", "sr_ssim", "sr_ms_ssim"]
    sc = sr.eval_tensors(img.reshape(img.shape[-3:]), img_gt.reshape(img.shape[-3:]))
    o64, t64 = img.reshape((1, 1) + tuple(img.shape[-3:])).cpu().double(), img_gt.reshape((1, 1) + tuple(img.shape[-3:])).cpu().double()
    o32, t32 = o64.float(), t64.float()
    _rule("flow sr_l1", sc["sr_l1"], (o64 - t64).abs().mean(), (o32 - t32).abs().mean())
    mse64, mse32 = ((o64 - t64) ** 2).mean(), ((o32 - t32) ** 2).mean()
    _rule("flow sr_psnr", sc["sr_psnr"], 20 * np.log10(float(t64.max()) / np.sqrt(float(mse64))),
          20 * np.log10(float(t32.max()) / np.sqrt(float(mse32))))
    _rule("flow sr_ssim", sc["sr_ssim"], SR.get_ssim(o64, t64), SR.get_ssim(o32, t32))
    assert np.isnan(sc["sr_ms_ssim"])                                        # the golden volume is smaller than 161


# -------------------------------------------------------------------------------------------------------- error paths
def test_exports_reject_bad_arguments_and_write_nothing():
    from brainfm_amd import _lib as L
    lib = L.load()
    dev = _dev()
    st = L.stream_ptr()
    n = 1000
    x = torch.rand(n, device=dev)
    li = torch.zeros(n, dtype=torch.int32, device=dev)
    lut = torch.zeros(10000, dtype=torch.int32, device=dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    SENT = -7.0
    o64 = torch.full((256,), SENT, dtype=torch.float64, device=dev)
    o32 = torch.full((n,), SENT, dtype=torch.float32, device=dev)
    oi = torch.full((100,), -7, dtype=torch.int64, device=dev)
    win = (C.c_float * 11)(*([1.0 / 11] * 11))
    p = L.ptr
    ARG, SHAPE, WSP = -1, -2, -3
    assert lib.bfm_eval_pair_stats_workspace() > 0 and lib.bfm_eval_ssim3d_workspace(1, 10, 10, 10) > 0
    assert lib.bfm_eval_channel_sums_workspace(2, 500) > 0 and lib.bfm_eval_channel_sums_workspace(0, 500) == 0
    assert lib.bfm_eval_ssim3d_workspace(1, 0, 10, 10) == 0
    calls = [
        (ARG, lambda: lib.bfm_eval_pair_stats(None, p(x), n, p(o64), p(ws), ws.numel(), st)),
        (ARG, lambda: lib.bfm_eval_pair_stats(p(x), None, n, p(o64), p(ws), ws.numel(), st)),
        (ARG, lambda: lib.bfm_eval_pair_stats(p(x), p(x), 0, p(o64), p(ws), ws.numel(), st)),
        (ARG, lambda: lib.bfm_eval_pair_stats(p(x), p(x), n, None, p(ws), ws.numel(), st)),
        (ARG, lambda: lib.bfm_eval_pair_stats(p(x), p(x), n, p(o64), None, ws.numel(), st)),
        (WSP, lambda: lib.bfm_eval_pair_stats(p(x), p(x), n, p(o64), p(ws), 16, st)),
        (ARG, lambda: lib.bfm_eval_l1_nonzero(None, p(x), 1, n, p(o32), st)),
        (ARG, lambda: lib.bfm_eval_l1_nonzero(p(x), p(x), 0, n, p(o32), st)),
        (ARG, lambda: lib.bfm_eval_l1_nonzero(p(x), p(x), 1, 0, p(o32), st)),
        (ARG, lambda: lib.bfm_eval_channel_sums(None, p(x), 2, 500, p(o64), p(ws), ws.numel(), st)),
        (ARG, lambda: lib.bfm_eval_channel_sums(p(x), p(x), 0, 500, p(o64), p(ws), ws.numel(), st)),
        (ARG, lambda: lib.bfm_eval_channel_sums(p(x), p(x), 2, 0, p(o64), p(ws), ws.numel(), st)),
        (SHAPE, lambda: lib.bfm_eval_channel_sums(p(x), p(x), 70000, 500, p(o64), p(ws), ws.numel(), st)),
        (WSP, lambda: lib.bfm_eval_channel_sums(p(x), p(x), 2, 500, p(o64), p(ws), 8, st)),
        (ARG, lambda: lib.bfm_eval_label_counts(None, p(li), n, p(lut), 10000, 33, p(oi), st)),
        (ARG, lambda: lib.bfm_eval_label_counts(p(li), p(li), 0, p(lut), 10000, 33, p(oi), st)),
        (ARG, lambda: lib.bfm_eval_label_counts(p(li), p(li), n, None, 10000, 33, p(oi), st)),
        (ARG, lambda: lib.bfm_eval_label_counts(p(li), p(li), n, p(lut), 0, 33, p(oi), st)),
        (ARG, lambda: lib.bfm_eval_label_counts(p(li), p(li), n, p(lut), 10000, 33, None, st)),
        (SHAPE, lambda: lib.bfm_eval_label_counts(p(li), p(li), n, p(lut), 10000, 257, p(oi), st)),
        (ARG, lambda: lib.bfm_eval_ssim3d(None, p(x), 1, 10, 10, 10, win, None, p(o64), p(ws), ws.numel(), st)),
        (ARG, lambda: lib.bfm_eval_ssim3d(p(x), p(x), 1, 10, 10, 10, None, None, p(o64), p(ws), ws.numel(), st)),
        (ARG, lambda: lib.bfm_eval_ssim3d(p(x), p(x), 1, 0, 10, 10, win, None, p(o64), p(ws), ws.numel(), st)),
        (ARG, lambda: lib.bfm_eval_ssim3d(p(x), p(x), 1, 10, 10, 10, win, None, None, p(ws), ws.numel(), st)),
        (SHAPE, lambda: lib.bfm_eval_ssim3d(p(x), p(x), 70000, 10, 10, 10, win, None, p(o64), p(ws), ws.numel(), st)),
        (WSP, lambda: lib.bfm_eval_ssim3d(p(x), p(x), 1, 10, 10, 10, win, None, p(o64), p(ws), 8, st)),
        (ARG, lambda: lib.bfm_eval_avgpool2_pair(None, p(x), 1, 10, 10, 10, None, p(o32), p(o32), st)),
        (ARG, lambda: lib.bfm_eval_avgpool2_pair(p(x), p(x), 1, 10, 0, 10, None, p(o32), p(o32), st)),
        (ARG, lambda: lib.bfm_eval_avgpool2_pair(p(x), p(x), 1, 10, 10, 10, None, None, p(o32), st)),
    ]
    for i, (want, call) in enumerate(calls):
        assert call() == want, i
    torch.cuda.synchronize()
    assert bool((o64 == SENT).all()) and bool((o32 == SENT).all()) and bool((oi == -7).all())
    # and the good calls do write
    assert lib.bfm_eval_pair_stats(p(x), p(x), n, p(o64), p(ws), ws.numel(), st) == 0
    assert lib.bfm_eval_label_counts(p(li), p(li), n, p(lut), 10000, 33, p(oi), st) == 0
    torch.cuda.synchronize()
    assert float(o64[0]) == 0.0 and float(o64[9]) == float((x != 0).sum()) and float(o64[10]) == SENT
    assert oi[:100].tolist() == [n] + [0] * 32 + [n] + [0] * 32 + [n] + [0] * 32 + [0]


def test_avgpool2_pair_equals_torch_avg_pool3d_with_padding():
    import torch.nn.functional as F
    from brainfm_amd import evaluator as E
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    X, Y = torch.rand(2, 1, 7, 10, 13, generator=g), torch.rand(2, 1, 7, 10, 13, generator=g)
    Xo, Yo = E.avgpool2_pair_dev(X.to(dev), Y.to(dev))
    pad = [1, 0, 1]
    wx, wy = F.avg_pool3d(X.double(), 2, padding=pad), F.avg_pool3d(Y.double(), 2, padding=pad)
    assert tuple(Xo.shape) == tuple(wx.shape) == (2, 1, 4, 5, 7)
    assert float((Xo.cpu().double() - wx).abs().max()) <= 2e-7 and float((Yo.cpu().double() - wy).abs().max()) <= 2e-7
