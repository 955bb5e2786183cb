"""The fixed-grid ODE solvers (euler, midpoint, rk4) behind shapeid.odeint_adjoint on the GPU: against golden vectors of
the real reference (tests/golden/make_golden_ode_fixed.py), the fused device route against the unfused one, the
generator hook and the names that stay refused.  Needs an MI355X: run with `-m gpu`."""
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

import ode_fixed_refs as R
from conftest import load_npz

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NTS = (2, 5, 10)
T10 = np.arange(10) * 0.1

# Against the golden.  The project's tolerance for dopri5 states (test_advection_rhs_and_dopri5) is 1e-6 for an fp64
# and 3e-5 for an fp32 state.  Measured here (profiles/ode_fixed.txt), max over every case, volume and nt:
#   euler, midpoint   0 for both state dtypes: the RHS is bit exact and the stage expressions are the reference's
#   rk4               3.800e-7 (fp32 state), 1.424e-7 (fp64 state): `dt * k1 / 3`, `dt * (k1 / -3 + k2)` and
#                     `(k1 + 3 k2 + 3 k3 + k4) * (dt / 8)` are formed as sums of fp32(dt c_j) k_j (bfm_rk_combine)
# so the bound is 4 x the measured maximum: equality for euler and midpoint, and for rk4
TOL_RK4 = {"f32": 4 * 3.800e-7, "f64": 4 * 1.424e-7}

GOLDEN_CASES = [c + (nt,) for c in R.golden_cases() for nt in NTS]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _dev_npz(name):
    """One fixture file: the arrays on the host, and y0 (both dtypes) and V on the device, uploaded once."""
    d = load_npz(name)
    V = {k: T(d[k]) for k in ("Vx", "Vy", "Vz")}
    y0 = {"f64": T(d["y0"]), "f32": T(d["y0"].astype(np.float32))}
    return d, V, y0


def _pde(V, bc):
    from brainfm_amd import shapeid as SH
    return SH.AdvDiffPDE(data_spacing=[1., 1., 1.], perf_pattern="adv", V_type="vector_div_free", V_dict=V,
                         BC=None if bc == "none" else bc, dt=0.1, device=DEV)


def _run(V, y0, bc, m, nt):
    from brainfm_amd import shapeid as SH
    pde = _pde(V, bc)
    sol = SH.odeint_adjoint(pde, y0, torch.from_numpy(T10[:nt]), 0.1, method=m)
    return sol, pde.nfe


@pytest.mark.parametrize("file,vol,m,dt,bc,nt", GOLDEN_CASES)
def test_against_the_reference_golden(file, vol, m, dt, bc, nt):
    d, V, y0 = _dev_npz(file)
    tag = "%s_%s_%s" % (m, dt, bc)
    gold = d["sol_" + tag]
    sol, nfe = _run(V, y0[dt], bc, m, nt)
    assert sol.dtype == torch.from_numpy(gold).dtype
    assert tuple(sol.shape) == (nt,) + tuple(d["y0"].shape)
    assert nfe == int(d["nfe_" + tag][NTS.index(nt)]) == R.STAGES[m] * (nt - 1)
    if vol == "small":
        got, want = N(sol), gold[:nt]                           # every row
    else:
        rows = [int(r) for r in d["rows"] if r < nt]            # the rows the large fixture keeps: 1, 4, 9
        got, want = N(sol)[rows], gold[:len(rows)]
        assert rows and rows[-1] == nt - 1
    e = R.rel_err(got, want)
    print("ode_fixed measured: %s %s nt=%d rel err %.3e" % (vol, tag, nt, e))
    if m == "rk4":
        assert e <= TOL_RK4[dt], e
    else:
        assert np.array_equal(got, want), e


def _both_routes(monkeypatch, V, y0, bc, m, nt):
    monkeypatch.setenv("BFM_ODE_DEVICE", "1")
    fused, n1 = _run(V, y0, bc, m, nt)
    monkeypatch.setenv("BFM_ODE_DEVICE", "0")
    unfused, n0 = _run(V, y0, bc, m, nt)
    assert n1 == n0 == R.STAGES[m] * (nt - 1)
    assert fused.dtype == unfused.dtype == y0.dtype and fused.shape == unfused.shape
    assert torch.isfinite(unfused).all()
    assert torch.equal(fused, unfused), float((fused - unfused).abs().max())


@pytest.mark.parametrize("file,vol,m,dt,bc,nt", GOLDEN_CASES)
def test_fused_route_equals_the_unfused_route(file, vol, m, dt, bc, nt, monkeypatch):
    d, V, y0 = _dev_npz(file)
    _both_routes(monkeypatch, V, y0[dt], bc, m, nt)


# the stage kernel works on boxes of 8 x 8 x 32 voxels: a volume inside one box in every axis, and one with a remainder
# in every axis (2 x 2 x 2 boxes, the last of each axis 3, 5 and 5 voxels wide)
@pytest.mark.parametrize("shape", [(6, 4, 8), (11, 13, 37)])
@pytest.mark.parametrize("bc", ["neumann", "none"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("m", R.METHODS)
def test_fused_route_equals_the_unfused_route_on_shapes_that_stress_the_tiling(m, dt, bc, shape, monkeypatch):
    g = torch.Generator().manual_seed(7)
    V = {k: ((torch.rand(shape, generator=g) * 2 - 1) * 1.5).to(DEV) for k in ("Vx", "Vy", "Vz")}   # CFL sum 0.45 at most
    y0 = torch.rand((1,) + shape, generator=g, dtype=torch.float64)
    y0 = (y0 if dt == "f64" else y0.float()).to(DEV)
    _both_routes(monkeypatch, V, y0, bc, m, 4)


def _shape_args(method, max_nt=10):
    return Namespace(perlin_res=[2, 2, 2], integ_method=method, bc="neumann", V_multiplier=40, dt=0.1, max_nt=max_nt)


def test_augment_pathology_with_rk4_reproduces_the_generator_golden():
    from brainfm_amd import generator_utils as GU
    d = load_npz("ode_fixed.npz")
    t = torch.from_numpy(np.arange(10) * 0.1)
    states = {}
    for m in ("rk4", "dopri5"):
        pde = _pde({}, "neumann")
        np.random.seed(int(d["gen_seed"]))
        out = GU.augment_pathology(T(d["gen_P"]), pde, t, _shape_args(m), DEV)
        states[m] = np.random.get_state()
        if m == "rk4":
            assert np.array_equal(N(pde.V_dict["Vx"]), d["gen_Vx"])
            assert pde.nfe == 4 * (int(d["gen_nt"]) - 1)
            assert out.dtype == torch.float64 and tuple(out.shape) == d["gen_out"].shape
            e = R.rel_err(N(out), d["gen_out"])
            print("ode_fixed measured: augment_pathology rk4 rel err %.3e" % e)
            assert e <= TOL_RK4["f64"], e
    # the np.random draws (nt, the velocity potentials) are consumed as with dopri5
    a, b = states["rk4"], states["dopri5"]
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _toy_case():
    rs = np.random.RandomState(0)
    shp = (48, 44, 52)
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shp], indexing="ij")
    ell = (((zz - 24) / 20.) ** 2 + ((yy - 22) / 18.) ** 2 + ((xx - 26) / 22.) ** 2) <= 1
    seeds = rs.rand(30, 3) * np.array(shp)
    lab = np.argmin(((np.stack([zz, yy, xx], -1)[..., None, :] - seeds) ** 2).sum(-1), -1)
    ids = np.array([2, 3, 4, 41, 42, 17, 10, 11, 12, 13])[lab % 10] * ell
    # a resident lesion-probability volume: with random_shape_prob = 0 the item takes the file-based branch of
    # read_and_deform_pathology, the one that calls augment_pathology (Generator/utils.py:428-459)
    blob = np.exp(-((zz - 22) ** 2 + (yy - 24) ** 2 + (xx - 28) ** 2) / (2.0 * 6.0 ** 2)).astype(np.float32) * ell
    return {"name": "toy", "Gen": ids.astype(np.float32), "T1": rs.rand(*shp).astype(np.float32) * ell,
            "pathology_prob": blob,
            "segmentation": ids.astype(np.int32),
            "distance": [rs.rand(*shp).astype(np.float32) * 255 for _ in range(4)],
            "registration": [rs.randn(*shp).astype(np.float32) * 500 for _ in range(3)]}


@pytest.mark.parametrize("m", R.METHODS)
def test_generator_configured_with_a_fixed_grid_method_produces_items(m, monkeypatch):
    """BaseGen with pathology_shape_generator.integ_method = euler / midpoint / rk4 runs augment_pathology on the new
    path (it raised NotImplementedError from inside __getitem__ before)."""
    from brainfm_amd import generator as G
    from brainfm_amd import shapeid as SH
    g = Namespace(size=[32, 32, 32], photo_prob=0.2, max_rotation=15, max_shear=0.2, max_scaling=0.2,
                  nonlin_scale_min=0.03, nonlin_scale_max=0.06, nonlin_std_max=4, bf_scale_min=0.02, bf_scale_max=0.04,
                  bf_std_min=0.1, bf_std_max=0.6, gamma_std=0.1, noise_std_min=0.05, noise_std_max=1.,
                  random_shift=False, nonlinear_transform=True, left_hemis_only=False, low_res_only=False, ct_prob=0,
                  flip_prob=0., pathology_prob=1.0, random_shape_prob=0.0, augment_pathology=True, bspline_zooming=False,
                  mild_samples=1, all_samples=2)
    shp = Namespace(perlin_res=[2, 2, 2], integ_method=m, bc="neumann", V_multiplier=40, dt=0.1, max_nt=4,
                    pathol_thres=0.2, pathol_tol=1e-5, mask_percentile_min=85., mask_percentile_max=99.)
    task = Namespace(T1=True, T2=False, FLAIR=False, CT=False, segmentation=True, distance=True, bias_field=True,
                     registration=True, super_resolution=True, surface=False, pathology=True, contrastive=False)
    args = Namespace(generator=g, pathology_shape_generator=shp, task=task, max_surf_distance=3.0,
                     augmentation_steps=["gamma", "bias_field", "resample", "noise"], dataset_option="brain_id",
                     mix_synth_prob=0.)
    calls = []
    orig = SH.odeint_adjoint

    def spy(*a, **k):
        calls.append(k.get("method"))
        return orig(*a, **k)
    monkeypatch.setattr(SH, "odeint_adjoint", spy)
    np.random.seed(3); torch.manual_seed(3)
    ds = G.build_datasets(args, DEV, cases=[_toy_case()])["all"]
    for _ in range(3):                                   # nt is drawn per item: a few items so that one asks for steps
        n, name, mode, target, samples = ds[0]
        p = target["pathology"]
        assert (isinstance(p, float) and p == 0.) or set(np.unique(N(p))) <= {0.0, 1.0}
        assert torch.isfinite(samples[0]["input"]).all()
    assert calls and set(calls) == {m}, calls


def test_refused_names_still_raise():
    from brainfm_amd import shapeid as SH
    d, V, y0 = _dev_npz("ode_fixed.npz")
    pde = _pde(V, "neumann")
    t = torch.from_numpy(T10[:3])
    for name in ("adams", "tsit5", "fixed_adams", "explicit_adams"):
        with pytest.raises(NotImplementedError, match=r"'%s'.*'euler', 'midpoint' and 'rk4'" % name):
            SH.odeint_adjoint(pde, y0["f32"], t, 0.1, method=name)
    for name in ("rk4", "euler", "midpoint", "adams"):
        with pytest.raises(NotImplementedError):
            SH.odeint(pde, y0["f32"], t, 0.1, method=name)
    with pytest.raises(ValueError):
        SH.odeint_adjoint(lambda t, y: y, y0["f32"], t, 0.1, method="rk4")
