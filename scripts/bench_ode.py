"""The pathology PDE (Generator/utils.py:542-560) at 160^3, nt = max_nt = 10: odeint_adjoint of the advection PDE along a
Perlin curl velocity, by integration method and route.

    python scripts/bench_ode.py [size=160] [reps=7] [methods=dopri5,rk4,midpoint,euler] [item=1]

Per method it times the fused device route (dopri5: controller on the device; fixed grid: one kernel per stage, all steps
enqueued at once) and the unfused route (BFM_ODE_DEVICE=0: one bfm_advect_upwind_rhs and one bfm_rk_combine launch per
stage from a host loop; dopri5: the host-controlled loop).  Every timed call is the integration alone (the velocity is
built before), between two device events, ending in a synchronise; the host clock around the same window is printed
beside it.  COLD: each call works on its own copy of the state and the velocity, taken round-robin from a pool, and
writes a fresh (nt, 160^3) solution of 10 x 33 MB, more than the 256 MB Infinity Cache holds, so no call finds its
inputs on the die.  The variants are run alternately, round by round, and the median over rounds is reported.

Fraction of the HBM peak: algorithmic bytes (SURVEY's roofline row: per RHS evaluation and voxel the state, Vx, Vy, Vz in
and k out -- 20 B with an fp32 state, 24 B with fp64 --, plus per combination the state in and out and 4 B per k read)
over the time, over 8 TB/s.  It is a whole-integration rate over peak, not one kernel's.

item=1 adds the time of one generator item with the PDE inside (bench.py's item_with_pde_ms workload) under dopri5 and
under each fixed-grid method asked for.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from brainfm_amd import shapeid as SH

N = int(sys.argv[1]) if len(sys.argv) > 1 else 160
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
methods = sys.argv[3].split(",") if len(sys.argv) > 3 else ["dopri5", "rk4", "midpoint", "euler"]
with_item = bool(int(sys.argv[4])) if len(sys.argv) > 4 else True
NT, DT, VMULT, POOL = 10, 0.1, 500, 4
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}
COMBINES = {"euler": [1], "midpoint": [1, 1], "rk4": [1, 2, 3, 4]}       # k's read by each bfm_rk_combine of a step

assert torch.cuda.is_available(), "bench_ode.py measures on the GPU only"
dev = torch.device("cuda:0")
t = torch.from_numpy(np.arange(NT) * DT)
np.random.seed(0)
_, P0 = SH.generate_shape_3d((N, N, N), [2, 2, 2], 90.0, dev)
SB = P0.element_size()
pool = []
for j in range(POOL):
    np.random.seed(10 + j)
    pool.append((P0.clone()[None], SH.generate_velocity_3d((N, N, N), [2, 2, 2], VMULT, dev)))
pde = SH.AdvDiffPDE(data_spacing=[1., 1., 1.], perf_pattern="adv", V_type="vector_div_free", V_dict={}, BC="neumann",
                    dt=DT, device=dev)


def algorithmic_bytes(method, nfe):
    nv = N ** 3
    if method == "dopri5":                                   # bench.py's count: 6 stages + the k_j read + y1 per step
        steps = (nfe - 2) // 6
        return steps * (6 * (SB + 12 + 4) + 4 * 21 + SB) * nv
    per_step = STAGES[method] * (SB + 12 + 4) + sum(2 * SB + 4 * nk for nk in COMBINES[method])
    return (NT - 1) * per_step * nv


def one(method, route, j):
    os.environ["BFM_ODE_DEVICE"] = route
    y0, V = pool[j % POOL]
    pde.V_dict = V
    pde.nfe = 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    h0 = time.perf_counter()
    e0.record()
    sol = SH.odeint_adjoint(pde, y0, t, DT, method=method)
    e1.record()
    e1.synchronize()
    host = time.perf_counter() - h0
    return e0.elapsed_time(e1), host * 1e3, pde.nfe, sol


variants = [(m, r) for m in methods for r in ("1", "0")]
res = {v: [] for v in variants}
last = {}
for rnd in range(reps + 1):                                  # round 0 warms every variant up
    for v in variants:
        ev, host, nfe, sol = one(v[0], v[1], rnd)
        if rnd:
            res[v].append((ev, host, nfe))
        if rnd == reps:
            last[v] = sol[-1].clone()
        del sol

print("odeint_adjoint at %d^3, nt = %d, state %s, V_multiplier %d, %d rounds, cold" % (N, NT, P0.dtype, VMULT, reps))
summary = {}
for v in variants:
    ev = np.array([r[0] for r in res[v]]); host = np.array([r[1] for r in res[v]])
    nfe = int(np.median([r[2] for r in res[v]]))
    b = algorithmic_bytes(v[0], nfe)
    med = float(np.median(ev))
    summary[v] = med
    fin = bool(torch.isfinite(last[v]).all())
    print("  %-8s %-8s median %8.3f ms (min %8.3f, max %8.3f; host clock median %8.3f)  nfe %4d  algorithmic %6.2f GB  "
          "%5.2f TB/s = %.3f of the 8 TB/s HBM peak  final state finite: %s"
          % (v[0], "fused" if v[1] == "1" else "unfused", med, ev.min(), ev.max(), float(np.median(host)), nfe, b / 1e9,
             b / med / 1e9, b / med / 1e9 / 8.0, fin))
for m in methods:
    same = torch.equal(last[(m, "1")], last[(m, "0")])
    print("  %-8s fused / unfused time %.3f; final rows equal bit for bit: %s" % (m, summary[(m, "1")] / summary[(m, "0")], same))
if "dopri5" in methods:
    for m in methods:
        if m != "dopri5":
            print("  %-8s fused over dopri5 fused: %.3f of its time" % (m, summary[(m, "1")] / summary[("dopri5", "1")]))

if with_item:
    import config5_lib as C5
    from brainfm_amd import generator as G
    os.environ["BFM_ODE_DEVICE"] = "1"
    del pool, last
    torch.cuda.empty_cache()
    case = C5.voronoi_case(7, pathology_prob=True)
    for m in ["dopri5"] + [m for m in methods if m != "dopri5"]:
        np.random.seed(100)
        torch.manual_seed(100)
        ga = C5.gen_args(160, random_shape_prob=0.0)
        ga.pathology_shape_generator.integ_method = m
        ds = G.build_datasets(ga, str(dev), cases=[case])["all"]
        for _ in range(2):
            ds[0]
        torch.cuda.synchronize()
        ts = []
        for _ in range(6):
            t0 = time.perf_counter()
            ds[0]
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        print("  generator item with the PDE inside (bench.py item_with_pde_ms workload), integ_method %-8s median %.2f ms "
              "(min %.2f) over %d items" % (m, 1e3 * float(np.median(ts)), 1e3 * min(ts), len(ts)))
        del ds
