"""The diffusion terms of AdvDiffPDE at 160^3: one right-hand side evaluation, and rk4 / dopri5 integrations over
nt = 10 times, for perf_pattern 'diff' and 'adv_diff' at every D_type, fused and unfused.

    python scripts/bench_pde_diff.py [size=160] [reps=5] [out=path of a copy of the printed summary]

Every timed call is between two device events and ends in a synchronise.  COLD: each call works on its own set of buffers
(state, V, the D fields, the derived fields the PDE object caches), taken round-robin from K sets that together hold more
than 1.2 GB, several times the 256 MB Infinity Cache, so no call finds its inputs on the die.  The variants are run
alternately, round by round; round 0 warms up; the median over the other rounds is reported with min and max.

  rhs       AdvDiffPDE.stage on a state: bfm_advdiff_rhs, one launch (the derived fields are cached, as in an integration)
  fused     odeint_adjoint, one kernel per stage (bfm_ode_fixed_advdiff / bfm_dopri5_advdiff_*)
  unfused   BFM_ODE_DEVICE=0: one bfm_advdiff_rhs and one bfm_rk_combine launch per stage from a host loop

Fraction of the HBM peak: algorithmic bytes over the time, over 8 TB/s.  Per RHS evaluation and voxel: the state in (8 B,
fp64), Vx, Vy, Vz in (12 B, with 'adv'), the D fields in (4 B each: 0 / 1 / 3 / 6), the derived fields in (c_a D or the
row sums: 12 B, none for 'constant'; div V 4 B for V_type='vector'), k out (4 B).  An integration adds scripts/bench_ode.py's
count per combination: the state in and out and 4 B per k read.  For an integration it is a whole-integration rate over
peak, not one kernel's.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from brainfm_amd import shapeid as SH

N = int(sys.argv[1]) if len(sys.argv) > 1 else 160
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else None
NT, DT = 10, 0.1
SB = 8
N_D = {"constant": 0, "scalar": 1, "diag": 3, "full": 6}
STAGES = {"rk4": 4}
COMBINES = {"rk4": [1, 2, 3, 4]}
CONFIGS = [(p, "vector_div_free", d) for p in ("diff", "adv_diff") for d in ("constant", "scalar", "diag", "full")]
CONFIGS.append(("adv_diff", "vector", "full"))

assert torch.cuda.is_available(), "bench_pde_diff.py measures on the GPU only"
dev = torch.device("cuda:0")
t = torch.from_numpy(np.arange(NT) * DT)
shape = (N, N, N)


def smooth(x):
    return F.avg_pool3d(F.pad(x[None, None], (1,) * 6, mode="replicate"), 3, stride=1)[0, 0].contiguous()


def buffer_set(seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    V = {k: (2 * torch.randn(shape, generator=g, device=dev))[None] for k in ("Vx", "Vy", "Vz")}
    D = {k: (0.05 + 0.4 * smooth(torch.rand(shape, generator=g, device=dev)))[None] for k in ("Dxx", "Dyy", "Dzz")}
    D.update({k: (0.1 * smooth(torch.randn(shape, generator=g, device=dev)))[None] for k in ("Dxy", "Dyz", "Dxz")})
    y0 = smooth(torch.rand(shape, generator=g, device=dev, dtype=torch.float64))[None]
    return y0, V, D


set_bytes = N ** 3 * (SB + 4 * (3 + 6 + 4))                 # state, V, D, the derived fields of 'full' + 'vector'
K = int(np.ceil(1.2e9 / set_bytes)) + 1
sets = [buffer_set(20 + j) for j in range(K)]


def d_dict(D, d_type):
    if d_type == "constant":
        return {"D": 0.3}
    if d_type == "scalar":
        return {"D": D["Dxx"]}
    return {k: D[k] for k in (("Dxx", "Dyy", "Dzz") if d_type == "diag" else D)}


# one PDE object per (configuration, buffer set): each keeps the derived fields of its own set
pdes = {c: [SH.AdvDiffPDE([1., 1., 1.], c[0], D_type=c[2], V_type=c[1], BC="neumann", dt=DT, V_dict=V,
                          D_dict=d_dict(D, c[2]), device=dev) for _, V, D in sets] for c in CONFIGS}


def rhs_bytes(c):
    perf, vt, d_type = c
    b = SB + 4 + 4 * N_D[d_type] + (12 if d_type != "constant" else 0)
    if "adv" in perf:
        b += 12 + (4 if vt == "vector" else 0)
    return b


def algorithmic_bytes(c, what, nfe):
    nv = N ** 3
    if what == "rhs":
        return rhs_bytes(c) * nv
    if what == "dopri5":
        return (nfe - 2) // 6 * (6 * rhs_bytes(c) + 4 * 21 + SB) * nv
    return (NT - 1) * (STAGES[what] * rhs_bytes(c) + sum(2 * SB + 4 * nk for nk in COMBINES[what])) * nv


def one(c, what, route, j):
    os.environ["BFM_ODE_DEVICE"] = route
    pde = pdes[c][j % K]
    y0 = sets[j % K][0]
    pde.nfe = 0
    if what == "rhs":
        pde.prepare(shape, dev)                              # the derived fields, outside the timed window
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    res = pde.stage(0., y0) if what == "rhs" else SH.odeint_adjoint(pde, y0, t, DT, method=what)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), pde.nfe, res


variants = [(c, "rhs", "1") for c in CONFIGS] + [(c, m, r) for c in CONFIGS for m in ("rk4", "dopri5") for r in ("1", "0")]
res = {v: [] for v in variants}
last = {}
for rnd in range(reps + 1):
    for v in variants:
        ev, nfe, r = one(v[0], v[1], v[2], rnd)
        if rnd:
            res[v].append((ev, nfe))
        if rnd == reps:
            last[v] = r[-1].clone()
        del r

lines = ["AdvDiffPDE at %d^3, fp64 state, BC neumann, nt = %d, %d buffer sets of %.0f MB, %d rounds, cold"
         % (N, NT, K, set_bytes / 1e6, reps)]
for v in variants:
    c, what, route = v
    ev = np.array([r[0] for r in res[v]])
    nfe = int(np.median([r[1] for r in res[v]]))
    b = algorithmic_bytes(c, what, nfe)
    med = float(np.median(ev))
    lines.append("  %-8s %-16s %-8s %-7s %-7s median %8.3f ms (min %8.3f, max %8.3f)  nfe %4d  algorithmic %6.2f GB  "
                 "%5.2f TB/s = %.3f of the 8 TB/s HBM peak  finite: %s"
                 % (c[0], c[1], c[2], what, "" if what == "rhs" else ("fused" if route == "1" else "unfused"), med,
                    ev.min(), ev.max(), nfe, b / 1e9, b / med / 1e9, b / med / 1e9 / 8.0,
                    bool(torch.isfinite(last[v]).all())))
for c in CONFIGS:
    for m in ("rk4", "dopri5"):
        f, u = (float(np.median([r[0] for r in res[(c, m, r_)]])) for r_ in ("1", "0"))
        d = float((last[(c, m, "1")] - last[(c, m, "0")]).abs().max())
        lines.append("  %-8s %-16s %-8s %-7s fused / unfused time %.3f; final rows max difference %.3e"
                     % (c[0], c[1], c[2], m, f / u, d))
print("\n".join(lines))
if out_path:
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
