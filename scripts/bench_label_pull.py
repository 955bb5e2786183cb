"""Cold times of interpol.grid_pull on a label image at 160^3: the fused kernel of label_pull.hip against the reference's
formulation run on this library (a loop over unique() of the float grid_pull on the label's indicator with a running
maximum, utils/interpol/api.py:182-193 -- what a commit without the fused kernel would need), and the float grid_pull of
one channel at the same order as the floor.  All-nearest, all-linear and all-cubic (and all-quadratic).

Image: about 100 labels, a blocky ellipsoid with structures (tests/label_pull_refs.py: blocky_labels), int32 unless
said otherwise.  Grid: the identity plus a uniform jitter of +-1.5 voxels per voxel.  Bound dct2, extrapolate.  Cold:
before every timed launch a 1 GiB buffer is overwritten, so neither the L2 nor the 256 MB memory-side cache holds the
operands; device events around the launches, median (min .. max) of 9 (3 for the loop, which takes ~100 pulls).

The ways the fused kernel can keep its per-thread (label, sum) table are timed side by side: that measurement is
what BFM_LABEL_PULL_AUTO's choice rests on.  The fused result is also compared with the loop's at this size.

usage: python scripts/bench_label_pull.py [output file]   (profiles/label_pull.txt holds a run)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from brainfm_amd import interpol as IP
import label_pull_refs as LR

dev = torch.device("cuda:0")
N = 160
nv = N ** 3
HBM_PEAK = 8.0e12
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


def loop_of_pulls(seg, grid, b, o, ext):
    """api.py:182-193 on this library's float kernels"""
    out = torch.zeros((1, 1) + tuple(grid.shape[1:4]), dtype=seg.dtype, device=seg.device)
    pmax = torch.zeros(out.shape, dtype=torch.float32, device=seg.device)
    for label in seg.unique():
        soft = IP._pull_raw((seg == label).to(torch.float32), grid, b, o, ext)
        out[soft > pmax] = label
        pmax = torch.max(pmax, soft)
    return out


g = torch.Generator(device="cpu").manual_seed(0)
lab = LR.blocky_labels((N, N, N), 100, 0)
seg = torch.from_numpy(lab)[None, None].contiguous().to(dev)
nlab = int(seg.unique().numel())
vol = torch.randn((1, 1, N, N, N), generator=g).to(dev)
ident = torch.stack(torch.meshgrid(*[torch.arange(N, dtype=torch.float32)] * 3, indexing="ij"), dim=-1)
grid = (ident + (torch.rand((N, N, N, 3), generator=g) * 3.0 - 1.5))[None].contiguous().to(dev)
bnd, ext = IP._opts(1, "dct2", True)[0], 1
VARIANTS = (("auto", IP.LABEL_PULL_AUTO), ("lds table", IP.LABEL_PULL_LDS), ("register rescan", IP.LABEL_PULL_REGS),
            ("4 slots + passes", IP.LABEL_PULL_PASSES))

say("interpol.grid_pull on a label image, %d^3, %d labels (blocky ellipsoid with structures), int32, grid = identity + "
    "uniform jitter of +-1.5 voxels, bound dct2, extrapolate; cold, median (min .. max), microseconds" % (N, nlab))
say("algorithmic HBM bytes per voxel: 12 (grid in) + 4 (labels gathered: the image once) + 4 (labels out) = 20 -> %.1f MB;"
    " share of the HBM peak = these bytes over the time over %.1f TB/s" % (nv * 20 / 1e6, HBM_PEAK / 1e12))
say()
say("%-10s %-44s %10s %22s %10s %8s" % ("order", "what", "median us", "(min .. max)", "x fused", "of peak"))
for order in (0, 1, 2, 3):
    o = IP._order_list(order)
    fused = {}
    for vname, v in VARIANTS:
        fused[vname] = cold(lambda: IP._label_pull_raw(seg, grid, bnd, o, ext, v))
    base = fused["auto"][0]
    for vname, _ in VARIANTS:
        med, lo, hi = fused[vname]
        say("%-10s %-44s %10.1f %22s %10.2f %7.1f%%" % ("all-%d" % order, "fused label kernel, table: " + vname, med,
                                                        "(%.1f .. %.1f)" % (lo, hi), med / base,
                                                        100.0 * nv * 20 / (med * 1e-6) / HBM_PEAK))
    med, lo, hi = cold(lambda: IP._pull_raw(vol, grid, bnd, o, ext))
    say("%-10s %-44s %10.1f %22s %10.2f %7.1f%%" % ("all-%d" % order, "float grid_pull, one channel (floor)", med,
                                                    "(%.1f .. %.1f)" % (lo, hi), med / base,
                                                    100.0 * nv * 20 / (med * 1e-6) / HBM_PEAK))
    med, lo, hi = cold(lambda: loop_of_pulls(seg, grid, bnd, o, ext), reps=3)
    say("%-10s %-44s %10.1f %22s %10.2f %8s" % ("all-%d" % order, "loop over unique() of float pulls (%d)" % nlab, med,
                                                "(%.1f .. %.1f)" % (lo, hi), med / base, "-"))
    a, b_ = IP._label_pull_raw(seg, grid, bnd, o, ext), loop_of_pulls(seg, grid, bnd, o, ext)
    same = [torch.equal(a, IP._label_pull_raw(seg, grid, bnd, o, ext, v)) for _, v in VARIANTS]
    say("%-10s fused vs loop: %d of %d voxels differ (near-ties: the loop sums a label's taps in another order); the "
        "tables give the same bits: %s" % ("all-%d" % order, int((a != b_).sum()), nv, all(same)))
    say()
say("the worst case for the passes: one label per voxel drawn at random from %d (no segmentation looks like this; a cubic "
    "footprint then holds about 45 distinct labels, 12 passes of 4):" % nlab)
noise = torch.randint(0, nlab, (1, 1, N, N, N), generator=g, dtype=torch.int32).to(dev)
for order in (1, 2, 3):
    o = IP._order_list(order)
    for vname, v in VARIANTS[:2] + VARIANTS[3:]:
        med, lo, hi = cold(lambda: IP._label_pull_raw(noise, grid, bnd, o, ext, v))
        say("%-10s %-44s %10.1f %22s" % ("all-%d" % order, "random labels, table: " + vname, med, "(%.1f .. %.1f)" % (lo, hi)))
say()
say("other label dtypes, all-linear and all-cubic (auto):")
for dt in (torch.uint8, torch.int16, torch.int64):
    s2 = seg.to(dt)
    for order in (1, 3):
        o = IP._order_list(order)
        med, lo, hi = cold(lambda: IP._label_pull_raw(s2, grid, bnd, o, ext))
        say("%-10s %-44s %10.1f %22s" % ("all-%d" % order, "fused label kernel, %s" % str(dt).replace("torch.", ""), med,
                                         "(%.1f .. %.1f)" % (lo, hi)))
say()
say("grid builders at %d^3, fp32 (bytes written: %.1f MB; add_identity_grid_ reads and writes them):" % (N, nv * 12 / 1e6))
mat = torch.tensor([[1.0, 0.02, 0.0, 0.5], [-0.02, 1.0, 0.01, -1.0], [0.0, -0.01, 1.0, 2.0]], device=dev)
disp = torch.zeros((N, N, N, 3), device=dev)
for name, fn, nbytes in (("identity_grid", lambda: IP.identity_grid((N, N, N), torch.float32, dev), nv * 12),
                         ("affine_grid", lambda: IP.affine_grid(mat, (N, N, N)), nv * 12),
                         ("add_identity_grid_", lambda: IP.add_identity_grid_(disp), nv * 24),
                         ("torch: stack(meshgrid)", lambda: torch.stack(torch.meshgrid(
                             *[torch.arange(N, dtype=torch.float32, device=dev)] * 3, indexing="ij"), dim=-1), nv * 12)):
    med, lo, hi = cold(fn)
    say("%-10s %-44s %10.1f %22s %10s %7.1f%%" % ("", name, med, "(%.1f .. %.1f)" % (lo, hi), "",
                                                  100.0 * nbytes / (med * 1e-6) / HBM_PEAK))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
