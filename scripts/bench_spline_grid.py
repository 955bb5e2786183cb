"""Cold kernel times of interpol grid_pull / grid_push / grid_grad at 160^3 with one channel, spline orders 0, 2 and 3
beside the linear kernels, and of the spline prefilter per family of boundary conditions.  Cold: before every timed
launch a 1 GiB buffer is overwritten, so neither the L2 nor the 256 MB memory-side cache holds the operands; one launch
between two HIP events, median of 9.  Two grids: the identity plus a smooth displacement (1.5 voxels times a sine of
period 40 voxels: neighbouring lanes touch neighbouring texels, what a registration field looks like), and the identity
plus a uniform jitter of +-1.5 voxels per voxel (neighbouring lanes land in different rows: the worst case for the scatter
of push, whose atomics then go out one row per lane).

usage: python scripts/bench_spline_grid.py [output file]   (profiles/spline_grid.txt holds a run)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from brainfm_amd import interpol as IP

dev = torch.device("cuda:0")
N = 160
nv = N ** 3
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)


def cold(fn, before=None, reps=9):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        if before is not None:
            before()
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
ident = torch.stack(torch.meshgrid(*[torch.arange(N, dtype=torch.float32)] * 3, indexing="ij"), dim=-1)
phase = (ident.sum(-1, keepdim=True) * (6.283185307 / 40.0)) + torch.tensor([0.0, 2.1, 4.2])
grids = {"smooth": (ident + 1.5 * torch.sin(phase))[None].contiguous().to(dev),
         "jitter": (ident + (torch.rand((N, N, N, 3), generator=g) * 3.0 - 1.5))[None].contiguous().to(dev)}
bnd, ext = IP._opts(1, "dct2", True)[0], 1

say("interpol grid kernels, %d^3, one channel, bound dct2, extrapolate; cold, median (min .. max) of 9, microseconds" % N)
say("compulsory HBM bytes per voxel: pull 12 (grid) + 4 (out) + 4 (volume) = 20 -> %.1f MB; grad 28 -> %.1f MB"
    % (nv * 20 / 1e6, nv * 28 / 1e6))
say("taps per voxel: order 0: 1, order 1: 8, order 2: 27, order 3: 64; a cubic pull is 64 4-byte L2-served loads per voxel"
    " = %.2f GB of L2 traffic" % (nv * 256 / 1e9))
say("a cubic push is 64 fp32 atomics per voxel = %.2f GB of added bytes; at the chip-wide rate of ~1.3 TB/s of added bytes"
    " that alone is %.0f us (order 2: %.0f us, order 1: %.0f us, order 0: %.0f us)"
    % (nv * 256 / 1e9, nv * 256 / 1.3e6, nv * 108 / 1.3e6, nv * 32 / 1.3e6, nv * 4 / 1.3e6))
say()
for gname, grid in grids.items():
    say("grid: identity + %s displacement" % gname)
    say("%-34s %10s %22s %12s %14s" % ("kernel", "median us", "(min .. max)", "taps*4B GB/s", "atomic floor us"))
    for what in ("pull", "push", "grad"):
        for order in (1, 0, 2, 3):
            o = IP._order_list(order)
            taps = (order + 1) ** 3
            if what == "pull":
                fn = lambda: IP._pull_raw(vol, grid, bnd, o, ext)
            elif what == "grad":
                fn = lambda: IP._grad_raw(vol, grid, bnd, o, ext)
            else:
                fn = lambda: IP._push_raw(vol, grid, (N, N, N), bnd, o, ext)     # includes zeroing the 16 MB output
            med, lo, hi = cold(fn)
            name = "grid_%s3d %s" % (what, "linear (order 1)" if order == 1 else "spline order %d" % order)
            say("%-34s %10.1f %22s %12.0f %14s" % (name, med, "(%.1f .. %.1f)" % (lo, hi), nv * taps * 4 / med / 1e3,
                                                   "%.0f" % (nv * taps * 4 / 1.3e6) if what == "push" else "-"))
    say()
say("spline prefilter, three axes in place (spline_coeff_nd, inplace): 6 passes over %.1f MB = %.1f MB" %
    (nv * 4 / 1e6, nv * 24 / 1e6))
work = vol[0, 0].clone()
for order, bound in ((3, "dct2"), (3, "zero"), (3, "dft"), (2, "dct2"), (2, "zero"), (2, "dft")):
    med, lo, hi = cold(lambda: IP.spline_coeff_nd(work, order, bound, 3, inplace=True), before=lambda: work.copy_(vol[0, 0]))
    say("%-34s %10.1f %22s %12.0f" % ("prefilter order %d %s" % (order, bound), med, "(%.1f .. %.1f)" % (lo, hi),
                                      nv * 24 / med / 1e3))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
