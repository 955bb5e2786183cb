"""Golden vectors for the fixed-grid ODE solvers (euler, midpoint, rk4) by RUNNING the reference on the CPU
(build container only).

    python tests/golden/make_golden_ode_fixed.py

Writes tests/golden/ode_fixed.npz (12 x 10 x 14 volume, every solution row, and one augment_pathology case) and
tests/golden/ode_fixed_large_f32.npz / ode_fixed_large_f64.npz (20 x 36 x 12 volume).

For every (volume, method, state dtype, BC) the reference is run with nt = 2, 5 and 10 requested times.  The fixed-grid
solvers take the requested times as their grid (DiffEqs/solvers.py:128-131), so the nt = 2 and nt = 5 solutions are the
leading rows of the nt = 10 one; the script asserts that bit for bit and stores the nt = 10 rows once.  The large
volume keeps rows 1, 4 and 9 only (the last row of each nt case) to stay inside the size limit of a committed file.
"""
import os
import sys
from argparse import Namespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

R = ref_import.setup()
import torch  # noqa: E402

torch.set_num_threads(4)
import Generator.utils as GU  # noqa: E402
from ShapeID import perlin3d as P3  # noqa: E402
from ShapeID.DiffEqs.pde import AdvDiffPDE  # noqa: E402
from ShapeID.DiffEqs.adjoint import odeint_adjoint  # noqa: E402

METHODS = ("euler", "midpoint", "rk4")
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
NTS = (2, 5, 10)
RES = [2, 2, 2]
LARGE_ROWS = (1, 4, 9)


def save(name, **d):
    np.savez_compressed(os.path.join(HERE, name), **d)
    print(name, os.path.getsize(os.path.join(HERE, name)), "bytes,", len(d), "arrays")


class BlowUp(Exception):
    pass


def stable_volume_cases(shape, seed):
    """The velocity strength of synth_perlin_pde.npz (V_multiplier = 40), halved until every reference solution on the
    volume meets the finiteness condition (an explicit fixed step can blow up at a large velocity; that is the
    reference's behaviour and not what these fixtures are about)."""
    vm = 40.0
    while True:
        try:
            return volume_cases(shape, seed, vm)
        except BlowUp as e:
            print("lowering the velocity:", e)
            vm /= 2


class Counted:
    def __init__(self, pde):
        self.n = 0
        self.orig = pde.forward
        pde.forward = self

    def __call__(self, t, y):
        self.n += 1
        return self.orig(t, y)


def volume_cases(shape, seed, V_multiplier):
    """y0 (a Perlin shape, as generate_shape_3d makes it), V and the reference's solutions on one volume."""
    np.random.seed(seed)
    pm, _ = P3.generate_perlin_noise_3d(shape, RES, tileable=(True, False, False), percentile=73.5)
    V = P3.generate_velocity_3d(shape, RES, V_multiplier, "cpu")
    t = torch.from_numpy(np.arange(10) * 0.1)
    out = {"y0": pm[None], "Vx": V["Vx"].numpy(), "Vy": V["Vy"].numpy(), "Vz": V["Vz"].numpy(),
           "V_multiplier": np.array(V_multiplier), "t": t.numpy()}
    ymax = float(np.abs(pm).max())
    for bc in ("neumann", None):
        pde = AdvDiffPDE(data_spacing=[1., 1., 1.], perf_pattern="adv", V_type="vector_div_free", V_dict=V, BC=bc,
                         dt=0.1, device="cpu")
        cnt = Counted(pde)
        for f64 in (False, True):
            y0 = torch.from_numpy(pm if f64 else pm.astype(np.float32))[None]
            for m in METHODS:
                sols = {}
                for nt in NTS:
                    cnt.n = 0
                    with torch.no_grad():
                        sols[nt] = odeint_adjoint(pde, y0, t[:nt], 0.1, method=m).numpy()
                    assert cnt.n == STAGES[m] * (nt - 1), (m, nt, cnt.n)
                    assert sols[nt].dtype == y0.numpy().dtype and sols[nt].shape == (nt,) + tuple(y0.shape)
                full = sols[10]
                for nt in NTS:
                    assert np.array_equal(sols[nt], full[:nt]), (m, nt)
                # the finiteness condition of the fixtures: an explicit fixed step may blow up at a large velocity
                if not (np.isfinite(full).all() and float(np.abs(full).max()) <= 10 * ymax):
                    raise BlowUp("%s bc=%s f64=%s at V_multiplier=%g: max|sol| %g against max|y0| %g"
                                 % (m, bc, f64, V_multiplier, float(np.abs(full).max()), ymax))
                tag = "%s_%s_%s" % (m, "f64" if f64 else "f32", bc or "none")
                out["sol_" + tag] = full
                out["nfe_" + tag] = np.array([STAGES[m] * (nt - 1) for nt in NTS])
                print(shape, tag, "max|sol| %.4f (y0 %.4f)" % (float(np.abs(full).max()), ymax))
    return out


def generator_case():
    """augment_pathology (Generator/utils.py:542-560) with integ_method='rk4' and a recorded np.random seed."""
    shape = (12, 10, 14)
    np.random.seed(41)
    pm, _ = P3.generate_perlin_noise_3d(shape, RES, tileable=(True, False, False), percentile=73.5)
    args = Namespace(perlin_res=RES, integ_method="rk4", bc="neumann", V_multiplier=40, dt=0.1, max_nt=10)
    t = torch.from_numpy(np.arange(args.max_nt) * args.dt)
    pde = AdvDiffPDE(data_spacing=[1., 1., 1.], perf_pattern="adv", V_type="vector_div_free", BC="neumann", dt=args.dt,
                     device="cpu")
    seed = None
    for s in range(100, 200):                       # a seed whose first draw asks for more than a few steps
        np.random.seed(s)
        if np.random.randint(1, args.max_nt + 1) >= 6:
            seed = s
            break
    np.random.seed(seed)
    nt = np.random.randint(1, args.max_nt + 1)
    np.random.seed(seed)
    with torch.no_grad():
        out = GU.augment_pathology(torch.from_numpy(pm)[None], pde, t, args, "cpu")
    assert np.isfinite(out.numpy()).all()
    return {"gen_P": pm[None], "gen_out": out.numpy(), "gen_seed": np.array(seed), "gen_nt": np.array(nt),
            "gen_Vx": pde.V_dict["Vx"].numpy()}


if __name__ == "__main__":
    small = stable_volume_cases((12, 10, 14), 51)
    small.update(generator_case())
    save("ode_fixed.npz", **small)
    large = stable_volume_cases((20, 36, 12), 52)
    for dt in ("f32", "f64"):
        d = {k: v for k, v in large.items() if not k.startswith(("sol_", "nfe_"))}
        for k, v in large.items():
            if k.startswith("nfe_") and ("_%s_" % dt) in k:
                d[k] = v
            if k.startswith("sol_") and ("_%s_" % dt) in k:
                d[k] = v[list(LARGE_ROWS)]
        d["rows"] = np.array(LARGE_ROWS)
        save("ode_fixed_large_%s.npz" % dt, **d)
