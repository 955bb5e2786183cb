"""Cold times of brainfm_amd.native at processed 256^3 (1 mm) -> native 320 x 320 x 256 (0.8 x 0.8 x 1 mm):

  resample_maps at K = 1 and K = 17 (one launch of bfm_affine_pull_multi) against the route a caller had before,
    K x (interpol.affine_grid + interpol.grid_pull order 1, bound zero, extrapolate: the same zero padding) on this
    library;
  resample_labels at C = the full label list and the left-hemisphere one (bfm_affine_pull_argmax on the channels-last
    posteriors, at the lane width the library picks and at every width that can be forced) against
    materialising C native volumes with bfm_affine_pull_multi (after the transpose to planes it needs) + torch.argmax + lut;
  each as a share of the 8 TB/s HBM peak over the algorithmic bytes (sources read once, outputs written once).

The scan is axis-aligned (the common case: lanes along native z read along processed z); a second K = 17 row turns it by
3 degrees about x.  Cold: before every timed launch a 1 GiB buffer is overwritten, so neither the L2 nor the 256 MB
memory-side cache holds the operands; device events around the launches, median (min .. max) of 9 (5 for the composed
routes).  The fused results are compared with the composed ones at this size.

usage: python scripts/bench_native.py [output file]   (profiles/native.txt holds a run)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from brainfm_amd import interpol as IP
from brainfm_amd import native as N
from brainfm_amd.engine import LABELS_FULL, LABELS_LEFT

dev = torch.device("cuda:0")
SRC, DST = (256, 256, 256), (320, 320, 256)
ns, nd = int(np.prod(SRC)), int(np.prod(DST))
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


def row(what, t, nbytes, base=None):
    med, lo, hi = t
    say("%-74s %10.1f %22s %8s %7.1f%%" % (what, med, "(%.1f .. %.1f)" % (lo, hi),
                                           "" if base is None else "%.2f" % (med / base),
                                           100.0 * nbytes / (med * 1e-6) / HBM_PEAK))


def affines(tilt_deg=0.0):
    """native: 0.8 x 0.8 x 1 mm; processed: 1 mm, the same centre."""
    aff_n = np.diag([0.8, 0.8, 1.0, 1.0])
    t = np.deg2rad(tilt_deg)
    R = np.array([[1, 0, 0], [0, np.cos(t), -np.sin(t)], [0, np.sin(t), np.cos(t)]])
    aff_n[:3, :3] = R @ aff_n[:3, :3]
    aff_n[:3, 3] = -aff_n[:3, :3] @ ((np.array(DST) - 1) / 2.0)
    aff_p = np.eye(4)
    aff_p[:3, 3] = -(np.array(SRC) - 1) / 2.0
    return aff_p, aff_n


def composed_maps(maps, M):
    """K x (affine_grid + grid_pull order 1): 12 bytes per voxel written and read again, per map"""
    out = []
    for m in maps:
        grid = IP.affine_grid(M, DST)
        out.append(IP.grid_pull(m[None, None], grid[None], interpolation=1, bound="zero", extrapolate=True)[0, 0])
    return out


g = torch.Generator(device="cpu").manual_seed(0)
say("brainfm_amd.native, processed %s (1 mm) -> native %s (0.8 x 0.8 x 1 mm); cold, median (min .. max), microseconds; "
    "share of the HBM peak = algorithmic bytes (sources read once, outputs written once) over the time over %.1f TB/s"
    % ("x".join(map(str, SRC)), "x".join(map(str, DST)), HBM_PEAK / 1e12))
say()
say("%-74s %10s %22s %8s %8s" % ("what", "median us", "(min .. max)", "x fused", "of peak"))
for tilt in (0.0, 3.0):
    aff_p, aff_n = affines(tilt)
    M = torch.tensor(N.vox2vox(aff_p, aff_n)[:3], dtype=torch.float32, device=dev)
    for K in ((1, 17) if tilt == 0.0 else (17,)):
        buf = torch.randn((K,) + SRC, generator=g).to(dev)
        maps = {"m%d" % j: buf[j] for j in range(K)}
        nbytes = K * (ns + nd) * 4
        tag = "K = %2d%s" % (K, "" if tilt == 0.0 else ", scan turned by %g degrees about x" % tilt)
        fused = cold(lambda: N.resample_maps(maps, aff_p, DST, aff_n, nearest=()))
        row("resample_maps, %s (%.0f MB)" % (tag, nbytes / 1e6), fused, nbytes)
        row("  all maps by nearest neighbour", cold(lambda: N.resample_maps(buf, aff_p, DST, aff_n,
                                                                             nearest=tuple(range(K)))), nbytes, fused[0])
        row("  composed: K x (affine_grid + grid_pull order 1)", cold(lambda: composed_maps(list(maps.values()), M), 5),
            nbytes, fused[0])
        a = N.resample_maps(maps, aff_p, DST, aff_n, nearest=())["m%d" % (K - 1)]
        b = composed_maps([buf[K - 1]], M)[0]
        say("  fused vs composed, last map: max |difference| %.3g (the composed route has fp32 coordinates)"
            % float((a - b).abs().max()))
        del buf, maps, a, b
    say()

aff_p, aff_n = affines(0.0)
for labels, name in ((LABELS_FULL, "the full label list"), (LABELS_LEFT, "the left-hemisphere list")):
    C = len(labels)
    post = torch.softmax(torch.randn(SRC + (C,), generator=g).to(dev), -1).permute(3, 0, 1, 2)[None]
    lut = torch.tensor(labels, dtype=torch.int32, device=dev)       # post: (1,C,D,H,W) over channels-last memory
    nbytes = C * ns * 4 + nd * 4

    def composed_labels():
        planes = post[0].contiguous()                                # (C,D,H,W): what bfm_affine_pull_multi reads
        vols = N.resample_maps(planes, aff_p, DST, aff_n, nearest=())
        top, arg = vols.max(0), torch.argmax(vols, 0)
        return torch.where(top.values > 0, lut[arg], torch.zeros_like(lut[arg]))

    fused = cold(lambda: N.resample_labels(post, lut, aff_p, DST, aff_n))
    row("resample_labels, C = %d, %s (%.0f MB), %d lanes per voxel" % (C, name, nbytes / 1e6,
                                                                       N.L.load().bfm_affine_pull_route(C)), fused, nbytes)
    for lanes in (1, 4, 8, 16, 32, 64):
        row("  forced to %2d lanes per voxel%s" % (lanes, " (one thread per voxel, a loop over the channels)"
                                                  if lanes == 1 else ""),
            cold(lambda: N.resample_labels(post, lut, aff_p, DST, aff_n, lanes=lanes), 5), nbytes, fused[0])
    row("  with return_max", cold(lambda: N.resample_labels(post, lut, aff_p, DST, aff_n, return_max=True)),
        nbytes + nd * 4, fused[0])
    row("  composed: transpose + C native volumes (%.0f MB more) + argmax + lut" % (C * nd * 4 / 1e6),
        cold(composed_labels, 5), nbytes, fused[0])
    a, b = N.resample_labels(post, lut, aff_p, DST, aff_n), composed_labels()
    say("  fused vs composed: %d of %d labels differ" % (int((a != b).sum()), nd))
    say()
    del post, a, b
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
