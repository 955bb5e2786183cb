"""Cold kernel times of interpol grid_hess / grid_pushgrad and of one grid_grad forward + backward at 160^3 with one
channel, spline orders 1, 2 and 3, bound dct2, extrapolate.  Cold, the two grids and the timing of
scripts/bench_spline_grid.py: a 1 GiB buffer is overwritten before every timed launch, one call between two HIP events,
median of 9; `smooth` is the identity plus 1.5 voxels times a sine of period 40 voxels, `jitter` the identity plus a
uniform +-1.5 voxels per voxel.

Two comparisons are the yardsticks.  The contracted backward (the Hessian times the incoming gradient, formed in the
kernel) against materialising the Hessian with the same kernel and reducing it in torch, which is the reference's
algorithm (pushpull.py:322-324).  grid_pushgrad against grid_push at the same order and grid (spline_grid.hip,
which this file's kernels do not touch): the same atomics, 8 more bytes read per voxel.

usage: python scripts/bench_grid_hess.py [output file]   (profiles/grid_hess.txt holds a run)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from brainfm_amd import interpol as IP

dev = torch.device("cuda:0")
N = 160
nv = N ** 3
PEAK = 8e12                                                  # HBM bytes per second
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)


def cold(fn, reps=9):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        flush.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


g = torch.Generator(device="cpu").manual_seed(0)
vol = torch.randn((1, 1, N, N, N), generator=g).to(dev)
cot = torch.randn((1, 1, N, N, N, 3), generator=g).to(dev)
ident = torch.stack(torch.meshgrid(*[torch.arange(N, dtype=torch.float32)] * 3, indexing="ij"), dim=-1)
phase = (ident.sum(-1, keepdim=True) * (6.283185307 / 40.0)) + torch.tensor([0.0, 2.1, 4.2])
grids = {"smooth": (ident + 1.5 * torch.sin(phase))[None].contiguous().to(dev),
         "jitter": (ident + (torch.rand((N, N, N, 3), generator=g) * 3.0 - 1.5))[None].contiguous().to(dev)}
bnd, ext = IP._opts(1, "dct2", True)[0], 1

# compulsory HBM bytes per voxel: grid 12, volume 4, Hessian 36, cotangent 12, gradient of the grid 12, output volume 4
BYTES = {"hess": 12 + 4 + 36, "contracted": 12 + 4 + 12 + 12, "reduce": 12 + 4 + 36 + 36 + 12 + 12,
         "pushgrad": 12 + 12 + 4 + 4, "push": 12 + 4 + 4 + 4,
         "fwdbwd": (12 + 4 + 12) + (12 + 12 + 4 + 4) + (12 + 4 + 12 + 12) + 12 + 12}

say("interpol grid_hess / grid_pushgrad, %d^3, one channel, bound dct2, extrapolate; cold, median (min .. max) of 9, "
    "microseconds" % N)
say("compulsory HBM bytes per voxel: hess %d, contracted backward %d, materialise + reduce in torch %d (the Hessian written,"
    " read again with the cotangent), pushgrad %d (with zeroing the output), push %d, grid_grad forward + backward %d"
    % (BYTES["hess"], BYTES["contracted"], BYTES["reduce"], BYTES["pushgrad"], BYTES["push"], BYTES["fwdbwd"]))
say("%% of peak: those bytes over the median time, against %.0f TB/s" % (PEAK / 1e12))
say()


def row(name, key, t, extra=""):
    med, lo, hi = t
    say("%-44s %10.1f %22s %9.1f %%  %s" % (name, med, "(%.1f .. %.1f)" % (lo, hi), 100 * nv * BYTES[key] / (med * 1e-6) / PEAK,
                                           extra))


for gname, grid in grids.items():
    say("grid: identity + %s displacement" % gname)
    say("%-44s %10s %22s %11s" % ("call", "median us", "(min .. max)", "of HBM peak"))
    for order in (1, 2, 3):
        o = IP._order_list(order)
        tag = "order %d" % order
        row("grid_hess materialised, " + tag, "hess", cold(lambda: IP._hess_raw(vol, grid, bnd, o, ext)))
        tc = cold(lambda: IP._hess_raw(vol, grid, bnd, o, ext, cot=cot))
        tr = cold(lambda: (IP._hess_raw(vol, grid, bnd, o, ext) * cot.unsqueeze(-1)).sum(dim=[1, -2]))
        row("contracted backward, " + tag, "contracted", tc)
        row("materialise + reduce in torch, " + tag, "reduce", tr, "%.2f x the contracted one" % (tr[0] / tc[0]))
        tp = cold(lambda: IP._pushgrad_raw(cot, grid, (N, N, N), bnd, o, ext))
        tq = cold(lambda: IP._push_raw(vol, grid, (N, N, N), bnd, o, ext))
        row("grid_pushgrad, " + tag, "pushgrad", tp, "%.2f x grid_push" % (tp[0] / tq[0]))
        row("grid_push, " + tag, "push", tq)
        x, gr = vol.clone().requires_grad_(True), grid.clone().requires_grad_(True)

        def fwdbwd():
            x.grad = gr.grad = None
            IP.grid_grad(x, gr, order, "dct2", True).backward(cot)

        row("grid_grad forward + backward, " + tag, "fwdbwd", cold(fwdbwd))
    say()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
