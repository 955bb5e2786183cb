"""The CPU oracle against golden vectors produced by the real reference
(tests/golden/make_golden_infer.py).  CPU only."""
import numpy as np
import torch

from conftest import load_npz, sd_from_npz
from oracle import unet_ref as O

RTOL = 2e-5  # same ATen kernels, but thread count / op order may differ slightly


def _close(a, b, tol=RTOL, w=1.0):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    scale = max(1e-6, float(np.abs(b).max()))
    err = float((np.abs(a - b) * w).max()) / scale
    assert err <= tol, err


def _unit_feat_weight(x, sd, f_maps, levels, groups):
    """Per-voxel weight for everything computed from the L2-normalised last feature (model.py:207): min(1, |f| / median|f|)
    of the feature before F.normalize, shape (1, 1, D, H, W).  F.normalize divides the rounding of f by |f|, so at a voxel
    of small norm a reference value carries its own machine's fp32 rounding magnified by median|f| / |f| (2e-4 of max on
    infer_small.npz, as far from an fp64 evaluation as from this oracle; tests/test_gpu_infer.py TOL_NET).  Weighting the
    difference by the same factor holds every voxel to the tolerance on the un-normalised feature: unchanged for the
    voxels at or above the median norm."""
    n = O.get_feature(x, sd, 1, f_maps, levels, groups, unit_feat=False)[-1].norm(dim=1, keepdim=True).double()
    return torch.clamp(n / n.median(), max=1.0).numpy()


def test_small_net_all_outputs():
    d = load_npz("infer_small.npz")
    f_maps, levels, groups = [int(v) for v in d["cfg"]]
    sd = sd_from_npz(d)
    x = torch.from_numpy(d["x"])
    out = O.forward_all(x, sd, f_maps=f_maps, num_levels=levels, num_groups=groups)
    w = _unit_feat_weight(x, sd, f_maps, levels, groups)
    for i, f in enumerate(out["feat"]):
        _close(f.numpy(), d["feat%d" % i], w=w if i == len(out["feat"]) - 1 else 1.0)
    keys = [k[4:] for k in d if k.startswith("out/")]
    assert sorted(keys) == sorted(k for k in out if k != "feat")
    for k in keys:
        if k == "label":
            assert out[k].dtype == torch.int64
            assert np.array_equal(out[k].numpy(), d["out/label"])
        else:
            _close(out[k].numpy(), d["out/" + k], w=w)


def test_left_hemis_head_set():
    d = load_npz("infer_hemis.npz")
    f_maps, levels, groups = [int(v) for v in d["cfg"]]
    sd = sd_from_npz(d)
    x = torch.from_numpy(d["x"])
    out = O.forward_all(x, sd, f_maps=f_maps, num_levels=levels, num_groups=groups, left_hemis_only=True)
    assert "rp" not in out and out["segmentation"].shape[1] == 18
    w = _unit_feat_weight(x, sd, f_maps, levels, groups)
    for k in [k[4:] for k in d if k.startswith("out/")]:
        if k == "label":
            assert np.array_equal(out[k].numpy(), d["out/label"])
        else:
            _close(out[k].numpy(), d["out/" + k], w=w)


def test_full_width_blocks():
    d = load_npz("infer_layers.npz")
    sd = {}
    for blk, pre in (("enc0", "backbone.encoders.0."), ("enc1", "backbone.encoders.1."), ("dec", "backbone.decoders.0.")):
        for k, v in d.items():
            if k.startswith(blk + "/"):
                sd[pre + k[len(blk) + 1:]] = torch.from_numpy(v)
    x = torch.from_numpy(d["x"])
    e0 = O.single_conv(O.single_conv(x, sd, "backbone.encoders.0.basic_module.SingleConv1"), sd,
                       "backbone.encoders.0.basic_module.SingleConv2")
    _close(e0.numpy(), d["e0"])
    p = torch.nn.functional.max_pool3d(e0, 2)
    e1 = O.single_conv(O.single_conv(p, sd, "backbone.encoders.1.basic_module.SingleConv1"), sd,
                       "backbone.encoders.1.basic_module.SingleConv2")
    _close(e1.numpy(), d["e1"])
    up = torch.nn.functional.interpolate(e1, size=e0.shape[2:], mode="nearest")
    y = torch.cat((e0, up), 1)
    y = O.single_conv(O.single_conv(y, sd, "backbone.decoders.0.basic_module.SingleConv1"), sd,
                      "backbone.decoders.0.basic_module.SingleConv2")
    _close(y.numpy(), d["y"])


def test_tiling_ranges_match_reference():
    d = load_npz("tiling_ranges.npz")
    for n in (160, 200, 256, 512):
        ranges, cnt = O.tiling_ranges((n, n, n), [80] * 3, [160] * 3)
        assert np.array_equal(np.array(ranges), d["ranges_%d" % n])
        assert np.array_equal(np.bincount(cnt.astype(np.int64).ravel(), minlength=9), d["cnt_%d_hist" % n])
        assert np.array_equal(cnt[np.arange(n), np.arange(n), np.arange(n)], d["cnt_%d_diag" % n])
    assert np.array_equal(np.array(O.axis_intervals(512, 160, 80)), d["ranges_512_x"])
    # 256 -> (0,160),(160,240),(176,256)
    assert O.axis_intervals(256, 160, 80) == [(0, 160), (160, 240), (176, 256)]


def test_tiled_stitch_toy():
    d = load_npz("infer_tiled.npz")
    f_maps, levels, groups, stride, win = [int(v) for v in d["cfg"]]
    sd = sd_from_npz(d)
    full = torch.from_numpy(d["full"])
    out, ranges, cnt = O.tiled_inference(full, sd, [stride] * 3, [win] * 3, atlas=(d["atlas"], d["atlas_aff"]),
                                         f_maps=f_maps, num_levels=levels, num_groups=groups)
    assert np.array_equal(np.array(ranges), d["ranges"])
    assert np.array_equal(cnt, d["cnt"])
    keys = [k[9:] for k in d if k.startswith("stitched/")]
    assert len(keys) == 17 and keys[-1] == "deformed_atlas" and list(out.keys()) == keys    # scripts/demo_test.py:107-119
    w = np.ones(full.shape[2:])                            # a stitched voxel: the smallest weight of the tiles over it
    for (x0, x1), (y0, y1), (z0, z1) in ranges:
        wt = _unit_feat_weight(full[:, :, x0:x1, y0:y1, z0:z1], sd, f_maps, levels, groups)[0, 0]
        w[x0:x1, y0:y1, z0:z1] = np.minimum(w[x0:x1, y0:y1, z0:z1], wt)
    for k in keys:
        _close(out[k].numpy(), d["stitched/" + k], 5e-5, w=w)


def test_wide_net_all_outputs_and_tiled_stitch():
    """The 64-wide 2-level net of infer_wide.npz (the fixture that pins the build's matrix-core kernels to the reference):
    the oracle reproduces the reference's single-volume outputs, labels included, and the 17 stitched keys."""
    d = load_npz("infer_wide.npz")
    f_maps, levels, groups, stride, win = [int(v) for v in d["cfg"]]
    sd = sd_from_npz(d)
    out = O.forward_all(torch.from_numpy(d["x"]), sd, f_maps=f_maps, num_levels=levels, num_groups=groups)
    for i, f in enumerate(out["feat"]):
        _close(f.numpy(), d["feat%d" % i])
    for k in [k[4:] for k in d if k.startswith("out/")]:
        if k == "label":
            assert np.array_equal(out[k].numpy(), d["out/label"])
        else:
            _close(out[k].numpy(), d["out/" + k])
    st, ranges, cnt = O.tiled_inference(torch.from_numpy(d["full"]), sd, [stride] * 3, [win] * 3,
                                        atlas=(d["atlas"], d["atlas_aff"]), f_maps=f_maps, num_levels=levels,
                                        num_groups=groups)
    keys = [k[9:] for k in d if k.startswith("stitched/")]
    assert len(keys) == 17 and list(st.keys()) == keys
    for k in keys:
        _close(st[k].numpy(), d["stitched/" + k], 5e-5)


def test_uncertainty_head_set():
    """`losses.uncertainty` (Trainer/models/__init__.py:57-111): two channels per regression head, both kept in one
    tensor by the reference (its UncertaintyProcessor matches no output name) and post-processed together."""
    d = load_npz("infer_uncert.npz")
    f_maps, levels, groups = [int(v) for v in d["cfg"]]
    assert list(d["processors"]) == ["UncertaintyProcessor", "SegProcessor", "DistProcessor"]
    x, sd = torch.from_numpy(d["x"]), sd_from_npz(d)
    out = O.forward_all(x, sd, f_maps=f_maps, num_levels=levels, num_groups=groups, uncertainty=True)
    w = _unit_feat_weight(x, sd, f_maps, levels, groups)
    keys = [k[4:] for k in d if k.startswith("out/")]
    assert sorted(keys) == sorted(k for k in out if k != "feat")
    for k in ("T1", "T2", "FLAIR", "CT", "bias_field", "high_res_residual", "high_res"):
        assert out[k].shape[1] == 2 and d["out/" + k].shape[1] == 2
    for k in keys:
        assert tuple(out[k].shape) == d["out/" + k].shape, k
        if k == "label":
            assert np.array_equal(out[k].numpy(), d["out/label"])
        else:
            _close(out[k].numpy(), d["out/" + k], w=w)
    _close(out["feat"][-1].numpy(), d["feat_last"], w=w)


# ---------------------------------------------------------------- infer_deep_*.npz: the shipped 6-level net
# tests/golden/make_golden_deep.py ran the reference on its default initialisation under torch.manual_seed(1) -- the
# weights bench.py runs -- and stored their sha256 hashes, not the 1 GB of weights.  The helpers below are shared with
# tests/test_gpu_infer.py, which holds the HIP path to the same fixture.

def load_deep():
    """infer_deep_a.npz (hashes, configuration, case A), _b.npz and _c.npz as one dict (one file per case keeps each
    fixture under 1 MiB)."""
    d = {}
    for case in "abc":
        d.update(load_npz("infer_deep_%s.npz" % case))
    return d


def sha256(t):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def deep_case_c_input(d):
    """Case C of the deep fixture: a seeded 64 x 80 x 96 draw with a zero slab (pooling 5 -> 2, upsampling 2 -> 5)."""
    seed, shape = int(d["cfg"][5]), tuple(int(v) for v in d["cfg"][6:9])
    x = torch.rand((1, 1) + shape, generator=torch.Generator().manual_seed(seed))
    x[:, :, :, :, :9] = 0
    return x


_DEEP_SD = {}


def deep_state_dict():
    """The product's full-width model under torch.manual_seed(1), the construction bench.py uses (CPU tensors)."""
    if not _DEEP_SD:
        from brainfm_amd import models as M, test_utils as TU
        torch.manual_seed(1)
        _, _, model, _, _, _ = M.build_model(*TU.default_inference_args(64, 6), "cpu")
        _DEEP_SD.update({k: v.detach() for k, v in model.state_dict().items()})
    return _DEEP_SD


def _maxerr(a, b, scale):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) / max(1e-30, scale)


def deep_compare_single(out, d, p, tie_gap):
    """One unstitched output dict (tensors on any device) against case p ("B/" or "C/") of the deep fixture. Returns
    ({name: worst error relative to the map's max |reference|}, [(flat voxel, gap) of every label exception]). Float
    maps and segmentation: max-norm at the sampled voxels (segmentation at every fourth of them).  Features, per level
    with M = max |reference|: the sampled entries, and per channel the mean, the RMS (| |a| - |b| | <= |a - b|), min and
    max, each within err * M. Labels: the 1/8 sublattice equals the reference's except at voxels the fixture lists as
    ties; over the whole map, the histogram of the non-tie voxels equals the reference's (tie voxels are compared one by
    one).  An exception must have a reference gap below tie_gap."""
    shape = tuple(int(v) for v in d[p + "shape"])
    dev = out["segmentation"].device
    idx = torch.from_numpy(d[p + "idx"]).to(dev)
    errs = {}
    for i, k in enumerate(d[p + "float_keys"]):
        ref = d[p + "floats"][i]
        errs[str(k)] = _maxerr(out[str(k)].detach().reshape(-1)[idx].cpu().numpy(), ref, np.abs(ref).max())
    seg_idx = torch.from_numpy(d[p + "seg_idx"]).to(dev)
    seg = out["segmentation"][0].reshape(out["segmentation"].shape[1], -1)[:, seg_idx].cpu().numpy()
    errs["segmentation"] = _maxerr(seg, d[p + "seg"], np.abs(d[p + "seg"]).max())
    for i, f in enumerate(out["feat"]):
        pre = p + "feat%d_" % i
        c = f.shape[1]
        assert c == d[pre + "mean"].shape[0], (i, tuple(f.shape))
        M = float(max(np.abs(d[pre + "min"]).max(), np.abs(d[pre + "max"]).max()))
        f64 = f.detach()[0].reshape(c, -1).double()
        n = f64.shape[1]
        e = [_maxerr(f.detach().reshape(-1)[torch.from_numpy(d[pre + "idx"]).to(dev)].cpu().numpy(), d[pre + "vals"], M),
             _maxerr(f64.mean(1).cpu().numpy(), d[pre + "mean"], M),
             _maxerr(((f64 * f64).sum(1) / n).sqrt().cpu().numpy(), np.sqrt(d[pre + "sumsq"] / n), M),
             _maxerr(f64.min(1).values.cpu().numpy(), d[pre + "min"], M),
             _maxerr(f64.max(1).values.cpu().numpy(), d[pre + "max"], M)]
        errs["feat%d" % i] = max(e)
    lab = out["label"].detach()[0, 0].cpu()
    assert tuple(lab.shape) == shape
    tie_idx, tie_gaps, tie_lab = d[p + "tie_idx"], d[p + "tie_gap"], d[p + "tie_label"].astype(np.int64)
    flat = lab.reshape(-1).numpy()
    exc = np.nonzero(flat[tie_idx] != tie_lab)[0]
    exceptions = [(int(tie_idx[j]), float(tie_gaps[j])) for j in exc]
    sub = lab[::2, ::2, ::2].numpy()
    zi, yi, xi = np.nonzero(sub != d[p + "label_sub"])
    sub_flat = ((2 * zi) * shape[1] + 2 * yi) * shape[2] + 2 * xi
    assert np.isin(sub_flat, tie_idx).all(), "sublattice label differences at voxels that are not ties: %s" % \
        sub_flat[~np.isin(sub_flat, tie_idx)][:20]
    hist_ref = d[p + "label_hist"].astype(np.int64)
    nb = max(len(hist_ref), int(flat.max()) + 1)
    non_tie = (np.bincount(flat, minlength=nb) - np.bincount(flat[tie_idx], minlength=nb))
    non_tie_ref = np.bincount(np.arange(len(hist_ref)), weights=hist_ref, minlength=nb).astype(np.int64) - \
        np.bincount(tie_lab, minlength=nb)
    assert np.array_equal(non_tie, non_tie_ref), "label histogram off the tie voxels: %s" % \
        np.nonzero(non_tie != non_tie_ref)[0]
    for v, gap in exceptions:
        print("%slabel exception at voxel %d: reference gap %.2e" % (p, v, gap))
        assert gap < tie_gap, (v, gap)
    return errs, exceptions


def test_deep_fixture_weights_and_inputs_are_regenerated_here():
    """The deep fixture holds hashes, not weights or volumes: the product's build_model under torch.manual_seed(1) draws
    the reference's 84 state-dict tensors bit for bit, and bench.make_volume(256), bench.make_atlas() and the case-C
    draw are the inputs the reference ran."""
    import bench
    d = load_deep()
    sd = deep_state_dict()
    assert list(sd.keys()) == [str(k) for k in d["sd_names"]] and len(sd) == 84
    bad = [k for k, h in zip(d["sd_names"], d["sd_sha256"]) if sha256(sd[str(k)]) != str(h)]
    assert not bad, bad
    assert sha256(bench.make_volume(256, "cpu")) == str(d["sha_volume"])
    atlas, aff = bench.make_atlas()
    assert sha256(atlas) == str(d["sha_atlas"]) and np.array_equal(aff, d["atlas_aff"])
    assert sha256(deep_case_c_input(d)) == str(d["sha_C_input"])


def test_oracle_six_levels_odd_shape_vs_reference_deep_golden():
    """The oracle at the shipped architecture (64 maps, 6 levels: GroupNorm over 1024 / 2048 channels, a 2048-channel
    first feature) on case C, 64 x 80 x 96: floor pooling 5 -> 2 and nearest 2 -> 5 upsampling inside the net.  Floats and
    features within 1e-3 (north-star tolerance) of the reference; labels equal except at reference ties (gap < 1e-5).
    Measured: worst float error 4e-17 (the same ATen kernels), no label exception.  With ceil instead of floor pooling
    the feature shapes already differ."""
    d = load_deep()
    x = deep_case_c_input(d)
    with torch.no_grad():
        out = O.forward_all(x, deep_state_dict(), f_maps=64, num_levels=6)
    assert [tuple(f.shape[1:]) for f in out["feat"]] == [(2048, 2, 2, 3), (1024, 4, 5, 6), (512, 8, 10, 12),
                                                        (256, 16, 20, 24), (128, 32, 40, 48), (64, 64, 80, 96)]
    errs, exc = deep_compare_single(out, d, "C/", tie_gap=1e-5)
    print("oracle vs reference, case C: worst %.2e (%s), %d label exceptions" %
          (max(errs.values()), max(errs, key=errs.get), len(exc)))
    assert max(errs.values()) <= 1e-3, errs
