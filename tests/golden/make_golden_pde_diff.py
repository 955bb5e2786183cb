"""Golden vectors for the diffusion terms and the general velocity of AdvDiffPDE by RUNNING the reference on the CPU
(build container only).

    python tests/golden/make_golden_pde_diff.py

Writes tests/golden/pde_diff.npz: recorded inputs and outputs only.  The cases are listed in tests/pde_diff_refs.py:
  * `forward` on the 4 x 3 x 5 volume for every (perf_pattern, V_type, D_type, BC, state dtype), stacked into two
    arrays (fp32 results, and the fp64 results of V_type='vector' with an fp64 state);
  * `forward` on 12 x 10 x 14 (one partial box of the stage kernels) and 11 x 9 x 37 (2 x 2 x 2 partial boxes) for a
    covering choice of nine configurations;
  * odeint_adjoint over t = 0.1 * arange(7) with BC 'neumann' for dopri5 / rk4 / midpoint / euler and both state dtypes:
    the last solution row (to stay inside the size limit of a committed file; every row for one dopri5 case on
    12 x 10 x 14, pde_diff_refs.ALL_ROWS_CASE), the number of evaluations, and the reference's own distance between its
    fp32-state and its fp64-state solution on that row, relative to max|sol|.
The script asserts that every dopri5 case takes the same number of evaluations with an fp32 and an fp64 state and that
every stored array is finite; a seed that fails either is to be changed, not the assertion.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import  # noqa: E402

ref_import.setup()
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

torch.set_num_threads(4)
from ShapeID.DiffEqs.pde import AdvDiffPDE  # noqa: E402
from ShapeID.DiffEqs.adjoint import odeint_adjoint  # noqa: E402

import pde_diff_refs as R  # noqa: E402

SEED = 11
D_CONST = 0.3


def smooth(x):
    """3^3 box mean with replicated borders."""
    return F.avg_pool3d(F.pad(x[None, None], (1,) * 6, mode="replicate"), 3, stride=1)[0, 0]


def make_fields(shape, g):
    d = {}
    for k in ("Vx", "Vy", "Vz"):
        d[k] = 2 * torch.randn(shape, generator=g)
    for k in R.D_FIELDS[:3]:
        d[k] = 0.05 + 0.4 * smooth(torch.rand(shape, generator=g))
    for k in R.D_FIELDS[3:]:
        d[k] = 0.1 * smooth(torch.randn(shape, generator=g))
    d["C"] = smooth(torch.rand(shape, generator=g, dtype=torch.float64))
    return d


class Counted:
    def __init__(self, pde):
        self.n = 0
        self.orig = pde.forward
        pde.forward = self

    def __call__(self, t, y):
        self.n += 1
        return self.orig(t, y)


def build_pde(f, perf, vt, dty, bc):
    V = {k: f[k][None] for k in ("Vx", "Vy", "Vz")}
    D = {k: f[k][None] for k in R.D_FIELDS}
    D["D"] = f["Dxx"][None]
    Dd = {k: (torch.tensor(v) if np.isscalar(v) else v) for k, v in R.d_dict(dty, D, D_CONST).items()}
    return AdvDiffPDE([1., 1., 1.], perf, D_type=dty, V_type=vt, BC=None if bc == "none" else bc, dt=0.1, V_dict=V,
                      D_dict=Dd, device="cpu")


def forward(f, case):
    perf, vt, dty, bc, dt = case
    C = f["C"] if dt == "f64" else f["C"].float()
    with torch.no_grad():
        out = build_pde(f, perf, vt, dty, bc)(0., C[None].clone())
    want = torch.float64 if (dt == "f64" and perf == "adv_diff" and vt == "vector") else torch.float32
    assert out.dtype == want and tuple(out.shape) == (1,) + tuple(C.shape), (case, out.dtype)
    return out[0].numpy()


if __name__ == "__main__":
    g = torch.Generator().manual_seed(SEED)
    fld = {v: make_fields(R.SHAPES[v], g) for v in ("a", "b", "c")}
    out = {"D_const": np.array(D_CONST), "t": R.T7}
    for v, f in fld.items():
        for k, t in f.items():
            out["%s_%s" % (v, k)] = t.numpy()

    r32, r64 = [], []
    for case in R.small_rhs_cases():
        r = forward(fld["c"], case)
        (r64 if r.dtype == np.float64 else r32).append(r)
    out["c_rhs_f32"], out["c_rhs_f64"] = np.stack(r32), np.stack(r64)
    for v in ("a", "b"):
        for case in R.BOX_RHS_CASES:
            out["rhs_" + R.case_tag(v, *case)] = forward(fld[v], case)

    t = torch.from_numpy(R.T7)
    for v, perf, vt, dty, methods in R.INTEG_CASES:
        f = fld[v]
        for m in methods:
            sols, nfe = {}, {}
            for dt in R.DTS:
                pde = build_pde(f, perf, vt, dty, "neumann")
                cnt = Counted(pde)
                y0 = (f["C"] if dt == "f64" else f["C"].float())[None]
                with torch.no_grad():
                    sols[dt] = odeint_adjoint(pde, y0, t, 0.1, method=m).numpy()
                nfe[dt] = cnt.n
                assert sols[dt].dtype == y0.numpy().dtype and sols[dt].shape == (7,) + tuple(y0.shape)
            if m == "dopri5":
                assert nfe["f32"] == nfe["f64"], (v, perf, vt, dty, nfe)
            else:
                assert nfe["f32"] == nfe["f64"] == 6 * R.STAGES[m]
            a, b = sols["f32"][-1].astype(np.float64), sols["f64"][-1]
            dist = float(np.abs(a - b).max() / np.abs(b).max())
            tag = R.case_tag(v, perf, vt, dty, m)
            for dt in R.DTS:
                out["sol_%s_%s" % (tag, dt)] = sols[dt][-1]
                if (v, perf, vt, dty, m) == R.ALL_ROWS_CASE:
                    out["rows_%s_%s" % (tag, dt)] = sols[dt]
            out["nfe_" + tag] = np.array(nfe["f64"])
            out["dist_" + tag] = np.array(dist)
            print(tag, "nfe", nfe["f64"], "fp32-vs-fp64 %.3e" % dist, "max|sol| %.4f" % float(np.abs(b).max()))

    for k, a in out.items():
        assert np.isfinite(a).all(), k
    path = os.path.join(HERE, "pde_diff.npz")
    np.savez_compressed(path, **out)
    print("pde_diff.npz", os.path.getsize(path), "bytes,", len(out), "arrays")
    assert os.path.getsize(path) < 1000000
