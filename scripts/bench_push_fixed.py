"""Cold times of interpol grid_push and grid_pushgrad in the two push modes, "atomic" (fp32 atomics) against "fixed" (int64
fixed-point atomics, bit-reproducible), in one process: 160^3 points into a 160^3 volume and 2048^2
points into a 2048^2 image, one channel, bound dct2, extrapolate, spline orders 0 to 3 and the mixed orders {3,1,2}
({3,1} in 2-D).  Cold, the two grids and the timing of scripts/bench_spline_grid.py: a 1 GiB buffer is overwritten before
every timed launch, one call between two HIP events, median of 9; `smooth` is the identity plus 1.5 voxels times a sine
of period 40 voxels, `jitter` the identity plus a uniform +-1.5 voxels per voxel.

A timed call is the whole route at the level the public functions use it (interpol._push_raw / _pushgrad_raw): "atomic"
zeroes the output and runs the kernel; "fixed" allocates the workspace, zeroes the accumulators, takes the maxima and the
exponents of the slices, runs the kernel and converts the accumulators.

With --parent-lib PATH the "atomic" exports of another build of the library (the parent commit's) are timed against this
build's in the same process, export against export on one zeroed output, interleaved case by case: the check that the
accumulation policies left the float kernels as fast as they were.

usage: python scripts/bench_push_fixed.py [--parent-lib libbrainfm_hip.so] [output file]
(profiles/push_fixed.txt holds a run)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from brainfm_amd import _lib as L
from brainfm_amd import interpol as IP

args = sys.argv[1:]
parent = None
if "--parent-lib" in args:
    i = args.index("--parent-lib")
    parent = C.CDLL(args[i + 1])
    del args[i:i + 2]
dev = torch.device("cuda:0")
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


def fmt(t):
    return "%9.1f (%.1f .. %.1f)" % t


def in_mode(mode, fn):
    def run():
        IP.set_push_mode(mode)
        try:
            return fn()
        finally:
            IP.set_push_mode(None)
    return run


def make_grids(shape, gen):
    D = len(shape)
    ident = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float32) for n in shape], indexing="ij"), dim=-1)
    phase = (ident.sum(-1, keepdim=True) * (6.283185307 / 40.0)) + torch.tensor([0.0, 2.1, 4.2][:D])
    return {"smooth": (ident + 1.5 * torch.sin(phase))[None].contiguous().to(dev),
            "jitter": (ident + (torch.rand(shape + (D,), generator=gen) * 3.0 - 1.5))[None].contiguous().to(dev)}


def export_call(lib, name, x, g, shape, b, o, ext, out):
    """One atomic export of `lib` on the zeroed `out`, as interpol._export calls it"""
    fn = getattr(lib, "bfm_" + name)
    fn.restype, fn.argtypes = L.SIGNATURES["bfm_" + name]
    dim = g.shape[-1]
    a = [L.ptr(x), x.shape[0], x.shape[1], *x.shape[2:2 + dim], L.ptr(g), g.shape[0], *shape, b]
    a += [] if o is None else [(C.c_int * 3)(*o)]

    def run():
        out.zero_()
        L.check(fn(*a, ext, L.ptr(out), L.stream_ptr()), name)
    return run


gen = torch.Generator(device="cpu").manual_seed(0)
bnd, ext = IP._opts(1, "dct2", True)[0], 1
say("interpol grid_push / grid_pushgrad, push mode 'atomic' (fp32 atomics) against 'fixed' (int64 fixed-point atomics), one "
    "channel, bound dct2, extrapolate")
say("cold, median (min .. max) of 9, microseconds; a call is the whole route: zeroing, [maxima, exponents,] kernel[, "
    "conversion]")
say()
worst = 0.0
for shape, orders in (((160, 160, 160), (0, 1, 2, 3, [3, 1, 2])), ((2048, 2048), (0, 1, 2, 3, [3, 1]))):
    D = len(shape)
    x = torch.randn((1, 1) + shape, generator=gen).to(dev)
    t = torch.randn((1, 1) + shape + (3,), generator=gen).to(dev) if D == 3 else None
    out = torch.empty((1, 1) + shape, device=dev)
    for gname, grid in make_grids(shape, gen).items():
        say("%s points into %s, grid: identity + %s displacement" % ("x".join(map(str, shape)), "x".join(map(str, shape)), gname))
        say("%-22s %-34s %-34s %s" % ("call", "atomic", "fixed", "fixed / atomic"))
        for order in orders:
            o = IP._order_list(order)
            calls = [("grid_push", lambda: IP._push_raw(x, grid, shape, bnd, o, ext))]
            if D == 3:
                calls.append(("grid_pushgrad", lambda: IP._pushgrad_raw(t, grid, shape, bnd, o, ext)))
            for name, fn in calls:
                ta, tf = cold(in_mode("atomic", fn)), cold(in_mode("fixed", fn))
                say("%-22s %-34s %-34s %.2f" % ("%s %s" % (name, order), fmt(ta), fmt(tf), tf[0] / ta[0]))
                worst = max(worst, tf[0] / ta[0])
            if parent is not None:
                ename, eo = IP._linear_or_spline("push", o, D)
                pairs = [("grid_push", ename, eo, x)] + ([("grid_pushgrad", "grid_pushgrad3d", o, t)] if D == 3 else [])
                for name, ename, eo, inp in pairs:
                    tn = cold(export_call(L.load(), ename, inp, grid, shape, bnd, eo, ext, out))
                    tp = cold(export_call(parent, ename, inp, grid, shape, bnd, eo, ext, out))
                    tn2 = cold(export_call(L.load(), ename, inp, grid, shape, bnd, eo, ext, out))
                    say("  atomic export %-18s this build %s, parent %s, this build again %s: this / parent %.3f, run to run "
                        "%.3f" % (ename, fmt(tn), fmt(tp), fmt(tn2), 0.5 * (tn[0] + tn2[0]) / tp[0], tn2[0] / tn[0]))
        say()
say("largest fixed / atomic ratio: %.2f" % worst)
if args:
    with open(args[0], "w") as f:
        f.write("\n".join(lines) + "\n")
