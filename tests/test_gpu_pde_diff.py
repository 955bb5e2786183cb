"""The diffusion terms and the general velocity of shapeid.AdvDiffPDE on the GPU: the stand-alone right-hand side against
the float64 restatement (tests/pde_diff_refs.py) within 3 x the reference's own fp32 distance to it, integrations against
golden solutions of the real reference (tests/golden/make_golden_pde_diff.py), the fused stage kernels against the unfused
route, and the derived fields never going stale.  Needs an MI355X: run with `-m gpu`."""
import functools

import numpy as np
import pytest
import torch

import pde_diff_refs as R
from conftest import load_npz
from test_host_pde_diff import ALL_RHS, restated

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T7 = torch.from_numpy(R.T7)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _dev_fields(vol):
    """One volume of the fixture on the device, uploaded once: state (both dtypes), V and D as (1, s, r, c)."""
    d = load_npz("pde_diff.npz")
    C, V, D = R.fields(d, vol)
    return ({"f64": T(C[None]), "f32": T(C[None].astype(np.float32))}, {k: T(v[None]) for k, v in V.items()},
            {k: T(v[None]) for k, v in D.items()}, float(d["D_const"]))


def _pde(vol, perf, vt, dty, bc, clone=False):
    from brainfm_amd import shapeid as SH
    C, V, D, const = _dev_fields(vol)
    Dd = R.d_dict(dty, D, torch.tensor(const))
    if clone:
        V, Dd = {k: v.clone() for k, v in V.items()}, {k: v.clone() for k, v in Dd.items()}
    return SH.AdvDiffPDE([1., 1., 1.], perf, D_type=dty, V_type=vt, BC=None if bc == "none" else bc, dt=0.1, V_dict=V,
                         D_dict=Dd, device=DEV)


@pytest.mark.parametrize("vol,perf,vt,dty,bc,dt", ALL_RHS)
def test_rhs_within_three_times_the_reference_fp32_distance(vol, perf, vt, dty, bc, dt):
    gold, want = restated(vol, (perf, vt, dty, bc, dt))
    bound, ref_dist = R.rhs_bound(gold, want)
    pde = _pde(vol, perf, vt, dty, bc)
    out = pde(0., _dev_fields(vol)[0][dt])
    assert pde.nfe == 1
    assert out.dtype == torch.from_numpy(gold).dtype and tuple(out.shape) == (1,) + gold.shape
    dist = float(np.abs(N(out)[0].astype(np.float64) - want).max())
    print("pde_diff measured: rhs %s dist %.3e (reference %.3e, bound %.3e)"
          % (R.case_tag(vol, perf, vt, dty, bc, dt), dist, ref_dist, bound))
    assert dist <= bound, (dist, bound)


def test_rhs_reads_fields_given_without_the_batch_axis_and_a_float_constant():
    from brainfm_amd import shapeid as SH
    C, V, D, const = _dev_fields("a")
    for dty in ("full", "constant"):
        a = _pde("a", "adv_diff", "vector", dty, "neumann")(0., C["f32"])
        Dd = {k: (v[0] if torch.is_tensor(v) and v.dim() == 4 else const)
              for k, v in R.d_dict(dty, D, torch.tensor(const)).items()}
        b = SH.AdvDiffPDE([1., 1., 1.], "adv_diff", D_type=dty, V_type="vector", BC="neumann",
                          V_dict={k: v[0] for k, v in V.items()}, D_dict=Dd)(0., C["f32"])
        assert torch.equal(a, b)


INTEG = [(v, perf, vt, dty, m, dt) for v, perf, vt, dty, ms in R.INTEG_CASES for m in ms for dt in R.DTS]


def _integrate(vol, perf, vt, dty, m, dt, pde=None):
    from brainfm_amd import shapeid as SH
    pde = pde or _pde(vol, perf, vt, dty, "neumann")
    sol = SH.odeint_adjoint(pde, _dev_fields(vol)[0][dt], T7, 0.1, method=m)
    return sol, pde.nfe


@pytest.mark.parametrize("vol,perf,vt,dty,m,dt", INTEG)
def test_integration_against_the_reference_golden(vol, perf, vt, dty, m, dt):
    d = load_npz("pde_diff.npz")
    tag = R.case_tag(vol, perf, vt, dty, m)
    gold = d["sol_%s_%s" % (tag, dt)]
    sol, nfe = _integrate(vol, perf, vt, dty, m, dt)
    assert sol.dtype == torch.from_numpy(gold).dtype and tuple(sol.shape) == (7,) + gold.shape
    assert torch.equal(sol[0], _dev_fields(vol)[0][dt])
    err = float(np.abs(N(sol[-1]).astype(np.float64) - gold).max())
    bound = max(3 * float(d["dist_" + tag]), 1e-6) * float(np.abs(gold).max())
    print("pde_diff measured: %s %s err %.3e bound %.3e nfe %d (golden %d)" % (tag, dt, err, bound, nfe,
                                                                                int(d["nfe_" + tag])))
    assert err <= bound, (err, bound)
    assert nfe == int(d["nfe_" + tag])


@pytest.mark.parametrize("dt", R.DTS)
def test_every_row_of_a_dopri5_integration_against_the_reference_golden(dt):
    """The dense output at the inner times: every row of the one case whose rows the fixture keeps.  The bound is the
    integration bound above taken row by row: max(3 x the reference's own fp32-state against fp64-state distance on
    that row, 1e-6) x max|golden|, never more than the whole-solution distance would allow.  The rows differ a lot: an
    fp32 dense output evaluates a quartic whose coefficients are sums like -8 y0 - 8 y1 + 16 y_mid, so the reference's
    own distance is 9.1e-7 and 1.9e-6 on rows 1 and 3 (of max|sol| 0.754, where the time lies inside a step) against
    1.8e-7 to 2.9e-7 on the others; measured here 1.25e-6 and 2.62e-6 on those rows, 3.0e-7 to 4.2e-7 on the others
    (fp32 state), at most 1.1e-8 with an fp64 state."""
    d = load_npz("pde_diff.npz")
    tag = R.case_tag(*R.ALL_ROWS_CASE)
    gold = d["rows_%s_%s" % (tag, dt)]
    assert np.array_equal(gold[-1], d["sol_%s_%s" % (tag, dt)])
    r32, r64 = d["rows_%s_f32" % tag].astype(np.float64), d["rows_%s_f64" % tag]
    ref_dist = np.abs(r32 - r64).reshape(7, -1).max(axis=1) / np.abs(r64).max()
    assert float(np.abs(r32[-1] - r64[-1]).max() / np.abs(r64[-1]).max()) == float(d["dist_" + tag])   # as recorded
    sol, nfe = _integrate(*R.ALL_ROWS_CASE, dt)
    assert tuple(sol.shape) == gold.shape == (7, 1) + R.SHAPES["a"]
    bound = np.maximum(3 * ref_dist, 1e-6) * float(np.abs(gold).max())
    err = np.abs(N(sol).astype(np.float64) - gold).reshape(7, -1).max(axis=1)
    print("pde_diff measured: rows %s %s err %s bound %s" % (tag, dt, " ".join("%.3e" % e for e in err),
                                                             " ".join("%.3e" % e for e in bound)))
    assert (err <= bound).all(), (err, bound)


@pytest.mark.parametrize("m", ["euler", "rk4", "dopri5"])
def test_batch_of_two_fp64_states_with_a_general_velocity_equals_the_single_integrations(m):
    """A (2, s, r, c) state takes the host loop; its stages must be the fp32 `stage`, not the fp64 `forward` of
    V_type='vector'.  The fixed-grid methods work voxel by voxel, so each half equals its single-volume integration bit
    for bit.  dopri5 controls the step by the norm over the whole batch, so two copies of one state are integrated (the
    mean squared error, and with it every step, is that of the single integration up to the order of a sum) and held
    to 1e-6 of max|sol|, the floor of the integration bound above."""
    from brainfm_amd import shapeid as SH
    C = _dev_fields("a")[0]["f64"]
    states = (C, C) if m == "dopri5" else (C, (C * 0.5 + 0.25).contiguous())
    pde = _pde("a", "adv_diff", "vector", "full", "neumann")
    single, nfe1 = [], []
    for y in states:
        pde.nfe = 0
        single.append(SH.odeint_adjoint(pde, y, T7, 0.1, method=m))
        nfe1.append(pde.nfe)
    pde.nfe = 0
    both = SH.odeint_adjoint(pde, torch.cat(states, 0), T7, 0.1, method=m)
    assert both.dtype == torch.float64 and tuple(both.shape) == (7, 2) + R.SHAPES["a"]
    assert pde.nfe == 2 * nfe1[0] == 2 * nfe1[1]               # forward counts one evaluation per volume
    for b in range(2):
        got, want = both[:, b:b + 1], single[b]
        if m == "dopri5":
            assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
        else:
            assert torch.equal(got, want), (m, b, float((got - want).abs().max()))


ROUTES = [(v, perf, vt, dty) for v in ("a", "b") for perf, vt, dty in
          (("diff", "vector", "full"), ("adv_diff", "vector", "scalar"), ("adv_diff", "vector_div_free", "diag"),
           ("diff", "vector", "constant"), ("adv", "vector", "scalar"))]


@pytest.mark.parametrize("dt", R.DTS)
@pytest.mark.parametrize("vol,perf,vt,dty", ROUTES)
def test_fused_route_equals_the_unfused_route(vol, perf, vt, dty, dt, monkeypatch):
    for m in ("euler", "midpoint", "rk4", "dopri5"):
        monkeypatch.setenv("BFM_ODE_DEVICE", "1")
        fused, n1 = _integrate(vol, perf, vt, dty, m, dt)
        monkeypatch.setenv("BFM_ODE_DEVICE", "0")
        unfused, n0 = _integrate(vol, perf, vt, dty, m, dt)
        assert n1 == n0 and fused.dtype == unfused.dtype and torch.isfinite(unfused).all()
        if m != "dopri5":
            assert n1 == 6 * R.STAGES[m]
            assert torch.equal(fused, unfused), (m, float((fused - unfused).abs().max()))
        else:
            # the device controller's pow() may differ from the host's in its last place, which moves dt by one part in
            # 1e16 and so at most flips the fp32 rounding of a (dt * c) coefficient: a few 2^-24 of the state's change
            assert float((fused - unfused).abs().max()) <= 1e-6 * float(unfused.abs().max()), m


@pytest.mark.parametrize("m", ["rk4", "dopri5"])
def test_derived_fields_follow_an_in_place_edit_and_a_replaced_dict(m):
    from brainfm_amd import shapeid as SH
    y0 = _dev_fields("a")[0]["f32"]
    pde = _pde("a", "adv_diff", "vector", "full", "neumann", clone=True)
    first = SH.odeint_adjoint(pde, y0, T7, 0.1, method=m)
    f_first = pde(0., y0)
    # scale a D field in place: c_x Dxx, a row sum of the derived fields, changes with it
    pde.D_dict["Dxx"].mul_(1.5)
    fresh = _pde("a", "adv_diff", "vector", "full", "neumann", clone=True)
    fresh.D_dict["Dxx"].mul_(1.5)
    assert torch.equal(pde(0., y0), fresh(0., y0)) and not torch.equal(pde(0., y0), f_first)
    second = SH.odeint_adjoint(pde, y0, T7, 0.1, method=m)
    assert torch.equal(second, SH.odeint_adjoint(fresh, y0, T7, 0.1, method=m))
    assert not torch.equal(second, first)
    # replace V_dict, as the generator does between items: div V changes with it
    newV = {k: (v * 0.5 + 0.1).contiguous() for k, v in pde.V_dict.items()}
    pde.V_dict = newV
    fresh2 = SH.AdvDiffPDE([1., 1., 1.], "adv_diff", D_type="full", V_type="vector", BC="neumann", dt=0.1,
                           V_dict={k: v.clone() for k, v in newV.items()}, D_dict=fresh.D_dict, device=DEV)
    assert torch.equal(pde(0., y0), fresh2(0., y0))
    third = SH.odeint_adjoint(pde, y0, T7, 0.1, method=m)
    assert torch.equal(third, SH.odeint_adjoint(fresh2, y0, T7, 0.1, method=m))
    assert not torch.equal(third, second)
    # an entry replaced inside the same dict
    pde.V_dict["Vx"] = pde.V_dict["Vx"] * 2
    fresh2.V_dict["Vx"] = fresh2.V_dict["Vx"] * 2
    fresh3 = SH.AdvDiffPDE([1., 1., 1.], "adv_diff", D_type="full", V_type="vector", BC="neumann", dt=0.1,
                           V_dict=dict(fresh2.V_dict), D_dict=fresh.D_dict, device=DEV)
    assert torch.equal(pde(0., y0), fresh3(0., y0))


def test_adv_configuration_still_gives_the_fixed_grid_golden():
    """Smoke check only (tests/test_gpu_ode_fixed.py asserts every case): euler is bit exact against the reference."""
    from brainfm_amd import shapeid as SH
    d = load_npz("ode_fixed.npz")
    assert d["y0"].shape == (1, 12, 10, 14)
    V = {k: T(d[k]) for k in ("Vx", "Vy", "Vz")}
    pde = SH.AdvDiffPDE([1., 1., 1.], "adv", V_type="vector_div_free", V_dict=V, BC="neumann", dt=0.1, device=DEV)
    sol = SH.odeint_adjoint(pde, T(d["y0"].astype(np.float32)), torch.from_numpy(np.arange(10) * 0.1), 0.1,
                            method="euler")
    assert np.array_equal(N(sol), d["sol_euler_f32_neumann"])
