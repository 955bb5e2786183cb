"""Parity of the HIP synthesis kernels (through the C ABI / host mirrors) against the golden vectors
of the real reference and the NumPy oracle: one golden shape per operation, mostly through the Python fronts, plus the
whole-generator goldens.  The kernels one at a time -- every route of bfm_zoom_linear and bfm_conv1d_axis, the edge
coordinates of the gathers, the small kernels of prep.hip, guard bands and sentinel tails -- are in
tests/test_gpu_synth_kernels.py (references: tests/synth_kernel_refs.py).  Needs an MI355X: run with `-m gpu`."""
import os

import numpy as np
import pytest
import torch

from conftest import load_npz
from oracle import synth_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(dtype) if dtype is not None else t


def N(t):
    return t.detach().cpu().numpy()


def _close(a, b, tol):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    e = float(np.abs(a - b).max()) / max(1e-6, float(np.abs(b).max()))
    assert e <= tol, e


def test_fast_3d_interp_bit_exact():
    from brainfm_amd.generator_utils import fast_3D_interp_torch as interp
    d = load_npz("synth_interp.npz")
    II, JJ, KK = T(d["II"]), T(d["JJ"]), T(d["KK"])
    assert np.array_equal(N(interp(T(d["X1"]), II, JJ, KK, "linear")), d["lin1"])
    assert np.array_equal(N(interp(T(d["X1"]), II, JJ, KK, "linear", 7.5)), d["lin1_def"])
    assert np.array_equal(N(interp(T(d["X3"]), II, JJ, KK, "linear")), d["lin3"])
    assert np.array_equal(N(interp(T(d["X1"]), T(d["G3i"]), T(d["G3j"]), T(d["G3k"]))), d["lin_grid"])
    g = [T(d["N3i"]), T(d["N3j"]), T(d["N3k"])]
    out = interp(T(d["S"]), *g, "nearest")
    assert out.dtype == torch.int32 and np.array_equal(N(out), d["near_i"])
    assert np.array_equal(N(interp(T(d["X3"]), *g, "nearest")), d["near_f"])
    Xc = T((np.arange(27).reshape(3, 3, 3) + 1).astype(np.float32))
    p = T(d["appc_pts"])
    assert np.array_equal(N(interp(Xc, p[:, 0].contiguous(), p[:, 1].contiguous(), p[:, 2].contiguous())), d["appc_lin"])
    nn = T(np.array([0.5, 1.5, 2.5, -0.6], np.float32).reshape(4, 1, 1))
    z = torch.zeros(4, 1, 1, device=DEV)
    assert N(interp(Xc, nn, z, z, "nearest")).ravel().tolist() == [1, 19, 19, 1]
    with pytest.raises(Exception, match="mode must be linear or nearest"):
        interp(Xc, nn, z, z, "cubic")
    assert interp(Xc, None, None, None) is Xc


def test_myzoom_blur_and_augmentations():
    from brainfm_amd import generator_utils as GU
    from brainfm_amd import _lib as L
    d = load_npz("synth_zoom_blur_aug.npz")
    assert np.array_equal(N(GU.myzoom_torch(T(d["zx"]), d["zf"])), d["zy"])
    assert np.array_equal(N(GU.myzoom_torch(T(d["zx2"]), d["zf2"])), d["zy2"])
    assert np.array_equal(N(GU.myzoom_torch(T(d["zx3"]), d["zf3"])), d["zy3"])
    z = GU.myzoom_torch(T(np.arange(4, dtype=np.float32).reshape(4, 1, 1)), np.array([2.5, 1, 1]))
    assert np.array_equal(N(z), d["appc_zoom"])
    _close(N(GU.make_gaussian_kernel(1.0, DEV)), d["gk1"], 1e-6)
    _close(N(GU.gaussian_blur_3d(T(d["bI"]), d["bstd"], DEV)), d["bO"], 2e-6)
    I = T(d["aug_I"])
    _close(N(GU.ew_unary(L.EW_GAMMA, I, 300.0, float(d["aug_gamma"]))), d["aug_Ig"], 3e-6)
    bflog = GU.myzoom_torch(T(d["bf_small"]), np.array([40, 40, 40]) / np.array(d["bf_small"].shape))
    assert np.array_equal(N(bflog), d["bf_log"])
    _close(N(GU.ew_binary(L.EW_MUL_EXP, I, bflog)), d["bf_I"], 2e-6)
    shifted = GU.ew_unary(L.EW_AFFINE, I, 1.0, -100.0)
    out = GU.ew_binary(L.EW_AXPY_CLAMP0, shifted, T(d["noise_randn"]), float(d["noise_std"][0]))
    _close(N(out), d["noise_out"], 1e-6)
    assert float(out.min()) >= 0
    # reductions used by the augmentation chain
    assert abs(GU.tensor_max(I) - float(d["aug_I"].max())) == 0
    assert abs(GU.tensor_min(I) - float(d["aug_I"].min())) == 0
    assert abs(GU.tensor_sum(I) - float(d["aug_I"].astype(np.float64).sum())) <= 1e-6 * float(d["aug_I"].sum())


def test_resample_resolution_chain_with_reference_rng():
    """resample_resolution draws one np.random value; with the same seed the whole chain must agree."""
    from brainfm_amd import generator_utils as GU
    d = load_npz("synth_zoom_blur_aug.npz")
    np.random.seed(8)
    setups = {"thickness": np.array([1.0, 4.2, 1.0]), "resolution": np.array([1.0, 3.5, 1.0])}
    small, aux = GU.resample_resolution(T(d["aug_I"]), {}, setups, np.array([1.0, 1.0, 1.0]), [40, 40, 40], DEV)
    assert np.array_equal(aux["factors"], d["rs_factors"])
    _close(N(small), d["rs_small"], 3e-6)
    assert np.array_equal(N(GU.myzoom_torch(T(d["rs_small"]), 1 / d["rs_factors"])), d["rs_back"])
    # gamma with the reference's RNG draw
    from argparse import Namespace
    np.random.seed(5)
    Ig, _ = GU.add_gamma_transform(T(d["aug_I"]), {}, Namespace(gamma_std=0.1), DEV)
    _close(N(Ig), d["aug_Ig"], 3e-6)


def test_perlin_percentile_curl_bit_exact():
    from brainfm_amd import shapeid as SH
    d = load_npz("synth_perlin_pde.npz")
    shape, res = tuple(int(v) for v in d["p_shape"]), tuple(int(v) for v in d["p_res"])
    g = SH.gradients_from_angles(d["p_theta"], d["p_phi"], (True, False, False))
    assert np.array_equal(N(SH.perlin_from_gradients(shape, res, g, DEV)), d["p_noise"])
    # with the reference's np.random stream the public entry point reproduces the golden directly
    np.random.seed(11)
    assert np.array_equal(N(SH.generate_perlin_noise_3d(shape, res, tileable=(True, False, False), device=DEV)),
                          d["p_noise"])
    np.random.seed(12)
    pm, m = SH.generate_perlin_noise_3d(shape, res, tileable=(True, False, False), percentile=73.5, device=DEV)
    assert np.array_equal(N(pm), d["pm_noise"]) and np.array_equal(N(m), d["pm_mask"])
    np.random.seed(13)
    assert np.array_equal(N(SH.generate_perlin_noise_3d((12, 12, 18), [3, 2, 3], device=DEV)), d["p2_noise"])
    np.random.seed(14)
    V = SH.generate_velocity_3d(shape, res, 500, DEV)
    for k in ("Vx", "Vy", "Vz"):
        assert V[k].dtype == torch.float32 and np.array_equal(N(V[k]), d[k]), k
    with pytest.raises(ValueError):
        SH.generate_perlin_noise_3d((10, 10, 10), [3, 2, 2], device=DEV)
    # order statistics / percentile helper against numpy on an awkward array (duplicates, negatives)
    x = np.concatenate([np.random.randn(5000), np.zeros(700), -np.ones(300)])
    xt = T(x)
    for q in (0.0, 12.5, 50.0, 73.5, 99.9, 100.0):
        assert SH.percentile_linear(xt, q) == float(np.percentile(x, q)), q


def test_advection_rhs_and_dopri5():
    from brainfm_amd import shapeid as SH
    d = load_npz("synth_perlin_pde.npz")
    V = {"Vx": T(d["Vx40"]), "Vy": T(d["Vy40"]), "Vz": T(d["Vz40"])}
    pde = SH.AdvDiffPDE(data_spacing=[1., 1., 1.], perf_pattern="adv", V_type="vector_div_free", V_dict=V,
                        BC="neumann", dt=0.1, device=DEV)
    assert np.array_equal(N(pde(torch.tensor(0.), T(d["C32"]))), d["rhs32"])
    assert np.array_equal(N(pde(torch.tensor(0.), T(d["C64"]))), d["rhs64"])
    t = torch.from_numpy(np.arange(10) * 0.1)
    for tag, nt, tol in (("ode64", 6, 1e-6), ("ode32", 4, 3e-5)):
        pde.nfe = 0
        sol = SH.odeint_adjoint(pde, T(d[tag + "_y0"]), t[:nt], 0.1, method="dopri5")
        assert sol.dtype == torch.from_numpy(d[tag + "_sol"]).dtype
        assert tuple(sol.shape) == d[tag + "_sol"].shape
        assert pde.nfe == int(d[tag + "_nfe"]), (pde.nfe, int(d[tag + "_nfe"]))
        _close(N(sol), d[tag + "_sol"], tol)
    with pytest.raises(NotImplementedError):
        SH.odeint(pde, T(d["ode32_y0"]), t[:3], 0.1, method="rk4")
    with pytest.raises(ValueError):
        SH.odeint_adjoint(lambda t, y: y, T(d["ode32_y0"]), t[:3], 0.1)


def test_grid_pull_all_bounds():
    from brainfm_amd.interpol import grid_pull
    d = load_npz("synth_grid_pull.npz")
    vol, grid = T(d["vol"]), T(d["grid"])
    for b in ["zero", "replicate", "dct1", "dct2", "dst1", "dst2", "dft"]:
        for ex in (0, 1):
            out = grid_pull(vol, grid, interpolation="linear", bound=b, extrapolate=bool(ex), prefilter=False)
            _close(N(out), d["out_%s_%d" % (b, ex)], 1e-6)
    X = T((np.arange(27).reshape(1, 1, 3, 3, 3) + 1).astype(np.float32))
    pts = T(d["appc_pts"])
    _close(N(grid_pull(X, pts, bound="zero", extrapolate=False)), d["appc_zero_0"], 1e-6)
    _close(N(grid_pull(X, pts, bound="zero", extrapolate=True)), d["appc_zero_1"], 1e-6)
    _close(N(grid_pull(X, pts, bound="dct2", extrapolate=True)), d["appc_dct2_1"], 1e-6)
    # broadcasting rules of the high-level API: no batch / no channel
    out = grid_pull(vol[0, 0], grid[0])
    assert tuple(out.shape) == tuple(grid.shape[1:4])
    _close(N(out), d["out_zero_0"][0, 0], 1e-6)
    with pytest.raises(NotImplementedError):
        grid_pull(vol, grid, interpolation="cubic")


def test_deform_grid_atlas_contrast_onehot():
    from argparse import Namespace
    from brainfm_amd import generator as G, generator_utils as GU, test_utils as TU, _lib as L
    d = load_npz("synth_deform_atlas.npz")
    A = GU.make_affine_matrix(np.array([0.1, -0.2, 0.15]), np.array([0.05, -0.1, 0.02]), np.array([1.1, 0.9, 1.05]))
    assert np.array_equal(A, d["affine_mat"])
    F = GU.myzoom_torch(T(d["dg_Fsmall"]), np.array(d["dg_size"]) / np.array([3, 3, 3]))
    assert np.array_equal(N(F), d["dg_F"])
    gen = object.__new__(G.BaseGen)
    gen.device = torch.device(DEV)
    gen.size = [int(v) for v in d["dg_size"]]
    xx, yy, zz, x1, y1, z1, x2, y2, z2 = gen.deform_grid([int(v) for v in d["dg_shp"]], d["dg_A"], d["dg_c2"], F)
    assert [x1, y1, z1] == list(d["dg_lo"]) and [x2, y2, z2] == list(d["dg_hi"])
    _close(N(xx), d["dg_xx"], 1e-6); _close(N(yy), d["dg_yy"], 1e-6); _close(N(zz), d["dg_zz"], 1e-6)
    out = TU.get_deformed_atlas(T(d["at_mask"]), T(d["at_rx"]), T(d["at_ry"]), T(d["at_rz"]), T(d["at_MNI"]), d["at_A"])
    _close(N(out), d["at_out"], 1e-6)
    syn = torch.empty(d["cs_G"].shape, device=DEV)
    Gt, mu, sg, rn = T(d["cs_G"]), T(d["cs_mus"]), T(d["cs_sigmas"]), T(d["cs_randn"])
    assert L.load().bfm_label_gauss(L.ptr(Gt), L.ptr(mu), L.ptr(sg), L.ptr(rn), Gt.numel(), 256, L.ptr(syn),
                                    L.stream_ptr()) == 0
    assert np.array_equal(N(syn), d["cs_out"])
    lut = torch.zeros(10000, dtype=torch.int32, device=DEV)
    lut[:64] = T(d["oh_lut"]).to(torch.int32)
    St = T(d["oh_S"]).to(torch.int32).contiguous()
    oh = torch.empty(d["oh_out"].shape, device=DEV)
    assert L.load().bfm_onehot_lut(L.ptr(St), L.ptr(lut), 10000, 56, St.numel(), L.ptr(oh), L.stream_ptr()) == 0
    assert np.array_equal(N(oh), d["oh_out"])


def _gen_args(size=(32, 32, 32)):
    from argparse import Namespace
    g = Namespace(size=list(size), photo_prob=0.2, max_rotation=15, max_shear=0.2, max_scaling=0.2,
                  nonlin_scale_min=0.03, nonlin_scale_max=0.06, nonlin_std_max=4, bf_scale_min=0.02, bf_scale_max=0.04,
                  bf_std_min=0.1, bf_std_max=0.6, gamma_std=0.1, noise_std_min=0.05, noise_std_max=1.,
                  random_shift=False, nonlinear_transform=True, left_hemis_only=False, low_res_only=False, ct_prob=0,
                  flip_prob=0., pathology_prob=1.0, random_shape_prob=1.0, augment_pathology=True, bspline_zooming=False,
                  mild_samples=1, all_samples=2)
    shp = Namespace(perlin_res=[2, 2, 2], integ_method="dopri5", bc="neumann", V_multiplier=40, dt=0.1, max_nt=4,
                    pathol_thres=0.2, pathol_tol=1e-5, mask_percentile_min=85., mask_percentile_max=99.)
    task = Namespace(T1=True, T2=False, FLAIR=False, CT=False, segmentation=True, distance=True, bias_field=True,
                     registration=True, super_resolution=True, surface=False, pathology=True, contrastive=False)
    return Namespace(generator=g, pathology_shape_generator=shp, task=task, max_surf_distance=3.0,
                     augmentation_steps=["gamma", "bias_field", "resample", "noise"], dataset_option="brain_id",
                     mix_synth_prob=0.)


def test_generator_getitem_structure_and_properties():
    """BrainIDGen.__getitem__ counterpart on an in-memory case: return structure, shapes, dtypes and the
    invariants of the chain (inputs normalised to max 1, one-hot targets, clamped distances)."""
    from brainfm_amd import generator as G
    rs = np.random.RandomState(0)
    shp = (48, 44, 52)
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shp], indexing="ij")
    ell = (((zz - 24) / 20.) ** 2 + ((yy - 22) / 18.) ** 2 + ((xx - 26) / 22.) ** 2) <= 1
    seeds = rs.rand(30, 3) * np.array(shp)
    lab = np.argmin(((np.stack([zz, yy, xx], -1)[..., None, :] - seeds) ** 2).sum(-1), -1)
    gen_labels = (np.array([2, 3, 4, 41, 42, 17, 10, 11, 12, 13])[lab % 10] * ell).astype(np.float32)
    seg = (np.array([2, 3, 4, 41, 42, 17, 10, 11, 12, 13])[lab % 10] * ell).astype(np.int32)
    case = {"name": "toy", "Gen": gen_labels, "T1": rs.rand(*shp).astype(np.float32) * ell, "segmentation": seg,
            "distance": [rs.rand(*shp).astype(np.float32) * 255 for _ in range(4)],
            "registration": [rs.randn(*shp).astype(np.float32) * 500 for _ in range(3)]}
    np.random.seed(3); torch.manual_seed(3)
    ds = G.build_datasets(_gen_args(), DEV, cases=[case])["all"]
    n, name, mode, target, samples = ds[0]
    assert (n, name, mode) == (1, "synth", "synth") and len(samples) == 2
    for s in samples:
        assert tuple(s["input"].shape) == (1, 32, 32, 32) and s["input"].dtype == torch.float32
        assert abs(float(s["input"].max()) - 1.0) < 1e-6 and float(s["input"].min()) >= 0
        assert tuple(s["bias_field_log"].shape) == (1, 32, 32, 32)
        assert tuple(s["high_res_residual"].shape) == (1, 32, 32, 32)
        assert torch.isfinite(s["input"]).all()
    assert tuple(target["segmentation"].shape) == (56, 32, 32, 32)
    assert torch.equal(target["segmentation"].sum(0), torch.ones(32, 32, 32, device=DEV))
    assert tuple(target["distance"].shape) == (4, 32, 32, 32) and float(target["distance"].abs().max()) <= 3.0
    assert tuple(target["registration"].shape) == (3, 32, 32, 32)
    assert tuple(target["T1"].shape) == (1, 32, 32, 32) and abs(float(target["T1"].max()) - 1) < 1e-6
    p = target["pathology"]
    assert (isinstance(p, float) and p == 0.) or set(np.unique(N(p))) <= {0.0, 1.0}


@pytest.mark.gpu
@pytest.mark.parametrize("case,kw", [
    ("A", dict(win_size=[32, 32, 32], zero_crop_first=False)),
    ("B", dict(win_size=None, zero_crop_first=True, is_CT=True)),
    ("C", dict(win_size=[30, 30, 30], spacing=[1.5, 1.5, 3.0], add_bf=True)),
])
def test_prepare_image_chain_vs_reference_golden(case, kw):
    """utils/test_utils.py::prepare_image on the device (min-max, Gaussian + anisotropic zoom, axis alignment, zero /
    centre crop, bias field, low-res simulation) against the reference run on the CPU; values live in [0, 1]."""
    from brainfm_amd import test_utils as TU
    d = load_npz("prep_image.npz")
    np.random.seed(11)
    torch.manual_seed(11)
    final, orig, high_res, bf, aff, crop_start, orig_shp = TU.prepare_image(
        (d[case + "/vol"].copy(), d[case + "/aff"].copy()), device="cuda:0", **kw)
    assert list(crop_start) == list(d[case + "/crop_start"])
    assert tuple(orig_shp) == tuple(d[case + "/orig_shp"])
    assert np.allclose(aff, d[case + "/aff_out"], atol=1e-10)
    for name, t in (("final", final), ("orig", orig), ("high_res", high_res), ("bf", bf)):
        if t is None:
            assert case + "/" + name not in d
            continue
        ref = d[case + "/" + name]
        got = t.cpu().numpy()
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        err = float(np.abs(got - ref).max())
        assert err <= 5e-6 * max(1.0, float(np.abs(ref).max())), (case, name, err)


@pytest.mark.gpu
@pytest.mark.parametrize("name,anchor", [("up", "edge"), ("down", "edge"), ("centers", "c")])
def test_cubic_bspline_resize_vs_reference_golden(name, anchor):
    """interpol.resize(interpolation=3, bound='dct2', prefilter=True) -- the bspline_zooming call of
    Generator/datasets.py:337-338 -- on the device (prefilter kernel + three separable 4-tap passes) against the
    reference's CPU result; also the prefilter alone, and the oracle on the same input."""
    from brainfm_amd import interpol as IP
    d = load_npz("interpol_resize.npz")
    x = torch.from_numpy(d[name + "/x"]).to("cuda:0")
    shape = [int(v) for v in d[name + "/shape"]]
    coeff = IP.spline_coeff_nd(x, interpolation=3, bound="dct2", dim=3)
    ref_c = d[name + "/coeff"]
    assert float(np.abs(coeff.cpu().numpy() - ref_c).max()) <= 1e-5 * float(np.abs(ref_c).max())
    y = IP.resize(x, shape=shape, anchor=anchor, interpolation=3, bound="dct2", prefilter=True)
    ref = d[name + "/y"]
    assert tuple(y.shape) == ref.shape
    assert float(np.abs(y.cpu().numpy() - ref).max()) <= 1e-5 * float(np.abs(ref).max())
    orc = S.resize_cubic_ref(d[name + "/x"], shape, anchor)
    assert float(np.abs(y.cpu().numpy() - orc).max()) <= 1e-5 * float(np.abs(orc).max())
    # linear resize goes through grid_pull
    y1 = IP.resize(x, shape=shape, anchor=anchor, interpolation=1, bound="dct2")
    assert tuple(y1.shape) == tuple(shape)


@pytest.mark.gpu
def test_prepare_image_from_nifti_file_equals_in_memory(tmp_path):
    """File boundary: a volume written with brainfm_amd.volio.MRIwrite and read back through the default
    reader gives the same prepare_image result as the in-memory (array, affine) form."""
    from brainfm_amd import test_utils as TU, volio as V
    d = load_npz("prep_image.npz")
    vol, aff = d["A/vol"], d["A/aff"]
    f = str(tmp_path / "case_A.nii.gz")
    V.MRIwrite(vol, aff, f)
    a = TU.prepare_image(f, win_size=[32, 32, 32], device="cuda:0")
    b = TU.prepare_image((vol.copy(), aff.copy()), win_size=[32, 32, 32], device="cuda:0")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and np.allclose(a[4], b[4], atol=1e-5)
    out = str(tmp_path / "final.nii.gz")
    V.MRIwrite(a[0][0, 0].cpu().numpy(), a[4], out)
    back, aff_back = V.MRIread(out)
    assert np.array_equal(back.astype(np.float32), a[0][0, 0].cpu().numpy()) and np.allclose(aff_back, a[4], atol=1e-4)


@pytest.mark.gpu
def test_grid_push_grad_count_and_first_order_backward_vs_reference_golden():
    """interpol.grid_push / grid_count / grid_grad on the device for every boundary condition, and the first-order
    backward of grid_pull / grid_push (d/dinput through the adjoint kernel, d/dgrid through grid_grad), against the
    vendored torch-interpol run on the CPU (fp32 atomics in push: tolerance, not bit equality)."""
    from brainfm_amd import interpol as IP
    d = load_npz("interpol_pushgrad.npz")
    dev = "cuda:0"
    vol, grid, src = (torch.from_numpy(d[k]).to(dev) for k in ("vol", "grid", "src"))
    ins = tuple(vol.shape[2:])

    def close(got, ref, what):
        err = float(np.abs(got.detach().cpu().numpy() - ref).max())
        assert err <= 2e-5 * max(1.0, float(np.abs(ref).max())), (what, err)

    for bound in range(7):
        for ext in (0, 1):
            k = "b%d_e%d/" % (bound, ext)
            close(IP.grid_push(src, grid, list(ins), 1, bound, bool(ext)), d[k + "push"], k + "push")
            close(IP.grid_grad(vol, grid, 1, bound, bool(ext)), d[k + "grad"], k + "grad")
            close(IP.grid_push(src, grid, list(ins), 1, bound, bool(ext)),
                  S.grid_push_linear(d["src"], d["grid"], ins, bound, bool(ext)), k + "push-vs-oracle")
            if k + "count" in d:
                close(IP.grid_count(grid, list(ins), 1, bound, bool(ext)), d[k + "count"], k + "count")
                v = vol.clone().requires_grad_(True)
                gr = grid.clone().requires_grad_(True)
                y = IP.grid_pull(v, gr, 1, bound, bool(ext))
                w = torch.sin(torch.arange(y.numel(), dtype=torch.float32)).reshape(y.shape).to(dev)
                (y * w).sum().backward()
                close(v.grad, d[k + "pull_dinput"], k + "pull_dinput")
                close(gr.grad, d[k + "pull_dgrid"], k + "pull_dgrid")
                s_ = src.clone().requires_grad_(True)
                gr = grid.clone().requires_grad_(True)
                y = IP.grid_push(s_, gr, list(ins), 1, bound, bool(ext))
                w2 = torch.cos(torch.arange(y.numel(), dtype=torch.float32)).reshape(y.shape).to(dev)
                (y * w2).sum().backward()
                close(s_.grad, d[k + "push_dinput"], k + "push_dinput")
                close(gr.grad, d[k + "push_dgrid"], k + "push_dgrid")


@pytest.mark.gpu
def test_write_device_volumes_round_trip(tmp_path):
    """volio.write_device_volumes (device-side axis reversal, pinned staging, threaded NIfTI / MGH writers) against
    MRIread: float maps bit-exact, int64 labels as int32, affine preserved, plain and multi-member gzip files."""
    from brainfm_amd import volio
    g = torch.Generator().manual_seed(0)
    vols = {"T1": torch.rand((20, 31, 17), generator=g).to("cuda:0"),
            "label": torch.randint(0, 2000, (20, 31, 17), generator=g).to("cuda:0")}
    aff = np.array([[0, 0, 1.5, -10.0], [-1.0, 0, 0, 20.0], [0, 2.0, 0, 5.0], [0, 0, 0, 1]])
    for ext in (".nii", ".nii.gz", ".mgz"):
        paths = volio.write_device_volumes(vols, aff, str(tmp_path / ext.strip(".").replace(".", "_")), ext=ext)
        for (k, v), p in zip(vols.items(), paths):
            out = volio.MRIread(p)
            arr, aff2 = (out[0], out[1]) if isinstance(out, tuple) else (out, None)
            assert arr.shape == tuple(v.shape)
            assert np.array_equal(np.asarray(arr).astype(np.float64), v.cpu().numpy().astype(np.float64)), (k, ext)
            if aff2 is not None:
                assert np.allclose(aff2, aff, atol=1e-5), (k, ext)


def _ns(d):
    from argparse import Namespace
    if isinstance(d, dict):
        return Namespace(**{k: _ns(v) for k, v in d.items()})
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["A", "B", "C"])
def test_generator_getitem_vs_reference_golden(tag):
    """SURVEY rows a19-a21 against the reference itself: tests/golden/gen_chain.npz holds what the reference's own
    BrainIDGen.__getitem__ (A: synthetic input mixed with the real T1, two samples; B: flipped, random Perlin pathology
    through generate_sample's pathology branch and encode_pathology) and BaseGen.__getitem__ (C: real T1 input, pathology
    encoded with the T1 direction) returned on in-memory cases, with every torch draw it made.  The device chain replays
    those draws (generator_utils.ReplayDraws) and follows NumPy's / random's streams by the seed: every target and every
    sample must come out the same."""
    import random
    from brainfm_amd import generator as G
    from brainfm_amd import generator_utils as GU
    from test_oracle_gen import load_case, relerr
    c = load_case(tag)
    cfg = dict(c["cfg"])
    cfg["dataset_option"] = "brain_id" if c["cls"] == "BrainIDGen" else "default"
    ga = _ns(cfg)
    case = dict(c["case"], name=tag, dataset="MEM")
    np.random.seed(c["seed"])
    random.seed(c["seed"])
    prev = GU.draws
    GU.draws = GU.ReplayDraws(c["draws"])
    try:
        ds = G.build_datasets(ga, DEV, cases=[case])["all"]
        assert type(ds).__name__ == c["cls"]
        n, dname, mode, target, samples = ds[0]
        assert GU.draws.pos == len(c["draws"])                 # the reference's draw sequence, consumed exactly
    finally:
        GU.draws = prev
    if not isinstance(samples, list):
        samples = [samples]
    assert mode == c["mode"] and n == 1 and len(samples) == len(c["samples"])
    for k, ref in c["target"].items():
        got = target[k]
        if np.ndim(ref) == 0:
            assert not isinstance(got, torch.Tensor) and float(got) == float(ref), (k, got, ref)
            continue
        got = N(got)
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        if k in ("segmentation", "pathology"):
            assert np.mean(got != ref) <= 1e-4, (k, float(np.mean(got != ref)))
        else:
            assert relerr(got, ref) <= 2e-5, (k, relerr(got, ref))
    for i, (s, r) in enumerate(zip(samples, c["samples"])):
        assert sorted(s.keys()) == sorted(r.keys())
        for k in r:
            got = N(s[k])
            assert got.shape == r[k].shape, (i, k)
            assert relerr(got, r[k]) <= 1e-4, (i, k, relerr(got, r[k]))


def test_gathers_inside_captured_graphs_on_two_lanes_keep_their_goldens():
    """The gathers of the library that read texels with plain loads -- fast_3D_interp_torch (bfm_interp3d_linear) and
    interpol.grid_pull (bfm_grid_pull3d_linear) -- had only ever run on one stream outside any graph, while the atlas
    gather misbehaved exactly inside two concurrently replaying graphs (HISTORY.md section 3.3).  Each is captured in a
    hipGraph per lane (own coordinate and output buffers, one shared source volume), the two graphs are replayed
    concurrently on two streams 100 times with a third stream beside them running a convolution that fills its LDS by
    LDS-DMA (global_load_lds: round 3 found that THIS is what the atlas gather's ordinary loads went wrong beside,
    tests/diag/diag_atlas_repro.py), and every replay must give the reference's golden bits (interp: exact; grid_pull:
    1e-6).  The co-runner alternates conv_mfma and conv_wino4d.  Rounds 3-5 held grid_pull to its goldens in the conv_mfma
    rounds only, because beside conv_wino4d it returned about 100 wrong elements per 400 eager rounds; round 6 found the
    cause (profiles/r06_hazard_root_cause.txt: not a load at all -- the low half of a packed-FP32 multiply, v_pk_mul_f32 with
    bank-conflicting sources, lost in lanes 48..63 beside the MFMA tap loop) and the library is built without packed-FP32
    instructions since (brainfm_amd/build.py), so EVERY round asserts both gathers again."""
    import ctypes as C
    from brainfm_amd import _lib as L, test_utils as TU
    from brainfm_amd.engine import _Layer
    from brainfm_amd.generator_utils import fast_3D_interp_torch
    from brainfm_amd.interpol import grid_pull
    d = load_npz("synth_interp.npz")
    X = T(d["X1"])
    d2 = load_npz("synth_grid_pull.npz")
    vol, grid = T(d2["vol"]), T(d2["grid"])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    side = torch.cuda.Stream()
    ga, ta = TU.default_inference_args(f_maps=64, num_levels=6)
    eng = TU.InferenceSession(ga, ta, torch.device(DEV)).engine
    cin = cout = 128
    cd = (40, 40, 40)
    cA = torch.randn(*cd, cin, device=DEV)
    csc, csh, cbd = torch.rand(cin, device=DEV) + 0.5, torch.randn(cin, device=DEV) * 0.1, torch.full((8,), 6.0, device=DEV)
    cout_t, cws = torch.empty(*cd, cout, device=DEV), torch.empty(1 << 26, dtype=torch.uint8, device=DEV)
    ly = _Layer()
    ly.name, ly.cin, ly.cout, ly.groups = "corunner", cin, cout, 8
    ly.w_raw = (torch.randn(cout, cin, 3, 3, 3, device=DEV) * 0.05).contiguous()
    ly.packs, ly.kind, ly.wpacked, ly.wexp, ly.skip = {}, None, None, 0, None
    ccfgs = []
    for ver in (0, 4):          # conv_mfma: weights through an LDS-DMA ring; conv_wino4d: raw activation chunks by LDS-DMA --
        c = (C.c_int * 8)()     # the strongest trigger of the hazard found so far (profiles/r05_atlas_hazard_bisect.txt)
        L.check(eng.lib.bfm_conv3x3x3_mfma_plan(cin, cout, cd[0], cd[1], cd[2], c), "plan")
        c[6] = ver
        ccfgs.append(c)
    state = {"it": 0}

    def conv_beside():
        ccfg = ccfgs[state["it"] % 2]
        state["it"] += 1
        for _ in range(6):
            eng._conv_launch(ly, cA, cin, None, 0, cd, None, csc, csh, cbd, 8, ccfg, cout_t, cws)

    conv_beside()
    conv_beside()
    torch.cuda.synchronize()
    lanes = []
    for lane in range(2):
        ii, jj, kk = T(d["II"]), T(d["JJ"]), T(d["KK"])            # private coordinate buffers per lane
        gcopy = grid.clone()
        outs = {}

        def body(ii=ii, jj=jj, kk=kk, gcopy=gcopy, outs=outs):
            outs["interp"] = fast_3D_interp_torch(X, ii, jj, kk, "linear")
            outs["pull_zero"] = grid_pull(vol, gcopy, interpolation="linear", bound="zero", extrapolate=False, prefilter=False)
            outs["pull_dct2"] = grid_pull(vol, gcopy, interpolation="linear", bound="dct2", extrapolate=True, prefilter=False)

        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(streams[lane]):
            body()                                                # warm-up (library load, allocations)
            streams[lane].synchronize()
            with torch.cuda.graph(g, stream=streams[lane]):
                body()
        lanes.append((g, outs))
    for it in range(100):
        for _, outs in lanes:
            for v in outs.values():
                v.fill_(float("nan"))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            conv_beside()
        for lane, (g, _) in enumerate(lanes):
            with torch.cuda.stream(streams[lane]):
                g.replay()
        torch.cuda.synchronize()
        for lane, (_, outs) in enumerate(lanes):
            assert np.array_equal(N(outs["interp"]), d["lin1"]), (it, lane)
            _close(N(outs["pull_zero"]), d2["out_zero_0"], 1e-6)
            _close(N(outs["pull_dct2"]), d2["out_dct2_1"], 1e-6)


def _cu_masked_stream(bits):
    """A stream confined to the CUs whose mask bits are given (hipExtStreamCreateWithCUMask of the HIP runtime torch has
    loaded; bit i -> XCD i % 8, shader engine (i // 8) % 4, CU (i // 32) of it)."""
    import ctypes as C
    hip = None
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            hip = C.CDLL(line.split()[-1])
            break
    assert hip is not None
    words = (C.c_uint32 * 8)()
    for i in bits:
        words[i // 32] |= 1 << (i % 32)
    st = C.c_void_p()
    assert hip.hipExtStreamCreateWithCUMask(C.byref(st), 8, words) == 0
    return torch.cuda.ExternalStream(st.value)


def test_grid_pull_beside_conv_wino4d_on_the_same_compute_units():
    """The high-rate form of the hazard round 6 closed (profiles/r06_hazard_root_cause.txt): interpol.grid_pull on the golden
    grid repeated 16 times (15 workgroups) on two streams, six launches of conv_wino4d (128 -> 128 on 40^3) on a third, all
    three streams confined to the SAME half of the compute units so that victim and MFMA waves share SIMDs.  With the library
    built WITH packed-FP32 instructions 40 % of the rounds return wrong elements (83-166 of 250-400 rounds on three boxes,
    always the trilinear sum minus corner 010 or 100 in lanes 48..63); built without them -- what ships -- none: 300 rounds,
    every element within 1e-6 of the reference's golden values, fast_3D_interp_torch exact."""
    import ctypes as C
    from brainfm_amd import _lib as L, test_utils as TU
    from brainfm_amd.engine import _Layer
    from brainfm_amd.generator_utils import fast_3D_interp_torch
    from brainfm_amd.interpol import grid_pull
    d = load_npz("synth_interp.npz")
    d2 = load_npz("synth_grid_pull.npz")
    X = T(d["X1"])
    vol = T(d2["vol"])
    grid = T(np.concatenate([d2["grid"]] * 16, axis=1))
    want = np.concatenate([d2["out_zero_0"]] * 16, axis=2)
    half = [i for i in range(256) if (i // 8) % 2 == 0]
    streams = [_cu_masked_stream(half), _cu_masked_stream(half)]
    side = _cu_masked_stream(half)
    ga, ta = TU.default_inference_args(f_maps=64, num_levels=6)
    eng = TU.InferenceSession(ga, ta, torch.device(DEV)).engine
    cin = cout = 128
    cd = (40, 40, 40)
    cA = torch.randn(*cd, cin, device=DEV)
    csc, csh, cbd = torch.rand(cin, device=DEV) + 0.5, torch.randn(cin, device=DEV) * 0.1, torch.full((8,), 6.0, device=DEV)
    cout_t, cws = torch.empty(*cd, cout, device=DEV), torch.empty(1 << 26, dtype=torch.uint8, device=DEV)
    ly = _Layer()
    ly.name, ly.cin, ly.cout, ly.groups = "corunner", cin, cout, 8
    ly.w_raw = (torch.randn(cout, cin, 3, 3, 3, device=DEV) * 0.05).contiguous()
    ly.packs, ly.kind, ly.wpacked, ly.wexp, ly.skip = {}, None, None, 0, None
    ccfg = (C.c_int * 8)()
    L.check(eng.lib.bfm_conv3x3x3_mfma_plan(cin, cout, cd[0], cd[1], cd[2], ccfg), "plan")
    ccfg[6] = 4                                                        # conv_wino4d

    def conv_beside():
        for _ in range(6):
            eng._conv_launch(ly, cA, cin, None, 0, cd, None, csc, csh, cbd, 8, ccfg, cout_t, cws)

    conv_beside()
    torch.cuda.synchronize()
    lanes = []
    for lane in range(2):
        lanes.append((T(d["II"]), T(d["JJ"]), T(d["KK"]), grid.clone()))
    wrong_rounds = 0
    for it in range(int(os.environ.get("BFM_TEST_HAZARD_ROUNDS", "300"))):
        outs = []
        with torch.cuda.stream(side):
            conv_beside()
        for lane, (ii, jj, kk, gcopy) in enumerate(lanes):
            with torch.cuda.stream(streams[lane]):
                a = fast_3D_interp_torch(X, ii, jj, kk, "linear")
                b = grid_pull(vol, gcopy, interpolation="linear", bound="zero", extrapolate=False, prefilter=False)
                outs.append((a, b))
        torch.cuda.synchronize()
        for a, b in outs:
            assert np.array_equal(N(a), d["lin1"]), it
            wrong_rounds += int(np.abs(N(b) - want).max() > 1e-6 * np.abs(want).max())
    assert wrong_rounds == 0, wrong_rounds


def test_streaming_kernels_with_l1_reuse_beside_an_lds_dma_corunner_keep_their_bits():
    """HISTORY.md section 3.3 / VERDICT r3 #6: besides the gathers, three kernels of the tile flow read with ordinary
    vector loads that re-use L1 lines between neighbouring lanes -- the stem's halo gather (bfm_conv3x3x3_stem_ex),
    maxpool2 (bfm_maxpool2_ex) and the uniform-box flags (bfm_uniform_boxes_level).  Each runs on two streams at once
    beside the LDS-DMA co-runners the atlas gather went wrong beside (conv_mfma and -- the strongest trigger -- conv_wino4d,
    alternating), 40 rounds; every output must equal the kernel's own serial result bit for bit.  Round 5 added a victim of
    the tile flow whose ordinary loads re-use L1 lines: the F(2,3) Winograd convolution."""
    import ctypes as C
    from brainfm_amd import _lib as L, test_utils as TU
    from brainfm_amd.engine import _Layer
    dev = torch.device(DEV)
    ga, ta = TU.default_inference_args(f_maps=64, num_levels=6)
    eng = TU.InferenceSession(ga, ta, dev).engine
    lib = eng.lib
    cin = cout = 128
    cd = (40, 40, 40)
    cA = torch.randn(*cd, cin, device=DEV)
    csc, csh, cbd = torch.rand(cin, device=DEV) + 0.5, torch.randn(cin, device=DEV) * 0.1, torch.full((8,), 6.0, device=DEV)
    cout_t, cws = torch.empty(*cd, cout, device=DEV), torch.empty(1 << 26, dtype=torch.uint8, device=DEV)
    ly = _Layer()
    ly.name, ly.cin, ly.cout, ly.groups = "corunner", cin, cout, 8
    ly.w_raw = (torch.randn(cout, cin, 3, 3, 3, device=DEV) * 0.05).contiguous()
    ly.packs, ly.kind, ly.wpacked, ly.wexp, ly.skip = {}, None, None, 0, None
    ccfgs = []
    for ver in (0, 4):          # conv_mfma (LDS-DMA weight ring) and conv_wino4d (LDS-DMA raw chunks: the strongest trigger of
        c = (C.c_int * 8)()     # the atlas hazard found so far, profiles/r05_atlas_hazard_bisect.txt), alternating
        L.check(lib.bfm_conv3x3x3_mfma_plan(cin, cout, cd[0], cd[1], cd[2], c), "plan")
        c[6] = ver
        ccfgs.append(c)
    state = {"it": 0}

    def conv_beside():
        ccfg = ccfgs[state["it"] % 2]
        state["it"] += 1
        for _ in range(6):
            eng._conv_launch(ly, cA, cin, None, 0, cd, None, csc, csh, cbd, 8, ccfg, cout_t, cws)

    # a victim with ordinary loads that DO re-use L1 lines: the F(2,3) Winograd convolution (neighbouring boxes share halo
    # rows, the two workgroups of a CU share weight fragments) -- in the two-lane tile flow it runs beside conv_wino4d
    vly = _Layer()
    vly.name, vly.cin, vly.cout, vly.groups = "victim", 64, 64, 8
    vly.w_raw = (torch.randn(64, 64, 3, 3, 3, generator=torch.Generator().manual_seed(8)) * 0.05).to(DEV).contiguous()
    vly.packs, vly.kind, vly.wpacked, vly.wexp, vly.skip = {}, None, None, 0, None
    vd = (32, 40, 48)
    vA = torch.randn(*vd, 64, generator=torch.Generator().manual_seed(9)).to(DEV)
    vsc, vsh, vbd = torch.rand(64, device=DEV) + 0.5, torch.randn(64, device=DEV) * 0.1, torch.full((8,), 6.0, device=DEV)
    vcfg = (C.c_int * 8)()
    L.check(lib.bfm_conv3x3x3_mfma_plan(64, 64, vd[0], vd[1], vd[2], vcfg), "plan")
    vcfg[6] = 3
    vws = [torch.empty(1 << 24, dtype=torch.uint8, device=DEV) for _ in range(3)]

    g = torch.Generator().manual_seed(3)
    dims = (96, 80, 112)
    img = torch.rand(dims, generator=g).to(DEV)
    img[:20] = 0
    img[:, :, 90:] = 0
    x_cl = img.reshape(*dims, 1).contiguous()
    stem = eng.enc[0][0]
    eng._pack(stem, False)                                            # the stem kernel reads the direct [27][1][Cout] layout
    sc1, sh1, bd1 = torch.ones(1, device=DEV), torch.zeros(1, device=DEV), torch.full((1,), 1.0, device=DEV)
    act = torch.randn(*(48, 40, 56), 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    side = torch.cuda.Stream()

    def run_all(store):
        # stem: 1 -> 32/64 channels, halo gather of the one-channel image
        out = torch.empty(*dims, stem.cout, device=DEV)
        L.check(lib.bfm_conv3x3x3_stem_ex(L.ptr(x_cl), dims[0], dims[1], dims[2], L.ptr(sc1), L.ptr(sh1), L.ptr(bd1),
                                          L.ptr(stem.wpacked), stem.cout, 0.01, L.ptr(out), None, L.stream_ptr()), "stem")
        store["stem"] = out
        pooled = torch.empty(24, 20, 28, 64, device=DEV)
        L.check(lib.bfm_maxpool2_ex(L.ptr(act), 64, 48, 40, 56, L.ptr(pooled), None, L.stream_ptr()), "maxpool2")
        store["pool"] = pooled
        for level in (0, 1):
            n = lib.bfm_uniform_boxes_bytes(dims[0] >> level, dims[1] >> level, dims[2] >> level, eng.passes)
            fl = torch.zeros(n, dtype=torch.uint8, device=DEV)
            L.check(lib.bfm_uniform_boxes_level(L.ptr(x_cl), dims[0], dims[1], dims[2], level, 3, eng.passes, L.ptr(fl),
                                                L.stream_ptr()), "uniform_boxes")
            store["flags%d" % level] = fl
        vout = torch.empty(*vd, 64, device=DEV)
        eng._conv_launch(vly, vA, 64, None, 0, vd, None, vsc, vsh, vbd, 8, vcfg, vout, vws[store.get("_slot", 2)])
        store["conv_wino"] = vout

    want = {}
    run_all(want)
    conv_beside()
    conv_beside()
    torch.cuda.synchronize()
    assert int((want["flags0"] != 0).sum()) > 0                       # the zero slabs give flagged boxes
    for it in range(40):
        got = [{"_slot": 0}, {"_slot": 1}]
        with torch.cuda.stream(side):
            conv_beside()
        for lane in range(2):
            with torch.cuda.stream(streams[lane]):
                run_all(got[lane])
        torch.cuda.synchronize()
        for lane in range(2):
            for k, v in want.items():
                if k != "_slot":
                    assert torch.equal(got[lane][k], v), (it, lane, k)
