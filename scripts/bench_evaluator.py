"""The evaluator's kernels (csrc/eval_metrics.hip) at N^3, N = 256 (the bench volume) and 160 (a tile), one (1,1,N,N,N)
pair, candidates alternated in one process:

  SSIM        the fused kernel (bfm_eval_ssim3d) against the composed route (bfm_conv1d_axis + element-wise kernels + crop +
              reduction: only kernels older than the evaluator), both reading min / max from device memory
  MS-SSIM     five scales of the fused kernel + bfm_eval_avgpool2_pair (and the composed route at every scale)
  pair stats  bfm_eval_pair_stats: two volumes read once = 8 N^3 bytes; time over that as a share of the 8.0 TB/s HBM peak
  label Dice  bfm_eval_label_counts (two int32 volumes of 8^3 single-label blocks, half of them background, read once =
              8 N^3 bytes) against the one-hot route: two bfm_onehot_lut launches (2 x 33 N^3 floats written) + torch sums

Cold: the inputs rotate over SETS buffer sets, together larger than the 256 MiB Infinity Cache.  Reports min / median / max
of device-event times over the repeats, the better of two alternated passes per candidate, and says which SSIM route wins
by more than the spread (max - min) at each size.

usage: python scripts/bench_evaluator.py [--sizes 256 160] [--reps 9] [--out profiles/evaluator_bench.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from brainfm_amd import _lib as L
from brainfm_amd import evaluator as E

HBM_PEAK = 8.0e12
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, reps, warm=2):
    for i in range(warm):
        fn(i)
    ts = []
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(warm + i)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return min(ts), statistics.median(ts), max(ts)


def bench_size(N, reps, dev):
    lib = L.load()
    sets = max(3, -(-(300 << 20) // (8 * N ** 3)))          # float pairs: > 256 MiB in rotation
    g = torch.Generator().manual_seed(N)
    pairs = []
    for _ in range(sets):
        t = torch.rand((1, 1, N, N, N), generator=g)
        o = (t + 0.1 * torch.randn((1, 1, N, N, N), generator=g)).to(dev)
        pairs.append((o, t.to(dev)))
    labs = np.array(E.label_list_segmentation, dtype=np.int32)
    lsets = []
    for k in range(sets):
        # structures, not noise: 8^3 blocks of one label, half of them background, and a prediction shifted by 3 voxels
        rs = np.random.RandomState(k)
        coarse = labs[rs.randint(0, len(labs), size=(N // 8,) * 3)] * (rs.rand(*(N // 8,) * 3) < 0.5)
        T = torch.from_numpy(coarse.astype(np.int32)).to(dev)
        T = T.repeat_interleave(8, 0).repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()
        P = torch.roll(T, 3, dims=1).contiguous()
        lsets.append((P.reshape(-1), T.reshape(-1)))
    win = E.gaussian_window(1.5)
    stats = [E.pair_stats_dev(o, t) for o, t in pairs]
    lut = E._lut(dev)
    counts = torch.empty(3 * E.n_labels + 1, dtype=torch.int64, device=dev)
    hot = [torch.empty((N ** 3, E.n_labels), device=dev) for _ in range(2)]
    big = N > 160

    def ssim_fused(i):
        o, t = pairs[i % sets]
        E.ssim_planes_dev(o, t, win, stats[i % sets][5:9], fused=True)

    def ssim_composed(i):
        o, t = pairs[i % sets]
        E.ssim_planes_dev(o, t, win, stats[i % sets][5:9], fused=False)

    def ms_fused(i):
        o, t = pairs[i % sets]
        E.ms_ssim_levels_dev(o, t, win, stats[i % sets][5:9], fused=True)

    def ms_composed(i):
        o, t = pairs[i % sets]
        E.ms_ssim_levels_dev(o, t, win, stats[i % sets][5:9], fused=False)

    def pair_stats(i):
        o, t = pairs[i % sets]
        E.pair_stats_dev(o, t)

    def label_counts(i):
        P, T = lsets[i % sets]
        L.check(lib.bfm_eval_label_counts(L.ptr(P), L.ptr(T), P.numel(), L.ptr(lut), E.N_LUT, E.n_labels, L.ptr(counts),
                                          L.stream_ptr()), "eval_label_counts")

    def onehot_dice(i):
        P, T = lsets[i % sets]
        for S, h in ((P, hot[0]), (T, hot[1])):
            L.check(lib.bfm_onehot_lut(L.ptr(S), L.ptr(lut), E.N_LUT, E.n_labels, S.numel(), L.ptr(h), L.stream_ptr()),
                    "onehot_lut")
        torch.mean(2.0 * (hot[0] * hot[1]).sum(dim=0) / torch.clamp((hot[0] + hot[1]).sum(dim=0), min=1e-5))

    cands = [("ssim fused", ssim_fused), ("ssim composed", ssim_composed), ("pair stats", pair_stats),
             ("label counts", label_counts), ("one-hot dice", onehot_dice)]
    if big:
        cands += [("ms-ssim fused", ms_fused), ("ms-ssim composed", ms_composed)]
    res = {}
    for _ in range(2):                                     # alternate, keep the better pass of each
        for name, fn in cands:
            r = timed(fn, reps)
            if name not in res or r[1] < res[name][1]:
                res[name] = r
    a, b = float(E.ssim_planes_dev(*pairs[0], win, stats[0][5:9], fused=True)[0, 0]), \
        float(E.ssim_planes_dev(*pairs[0], win, stats[0][5:9], fused=False)[0, 0])
    say("%d^3 (ms: min / median / max over %d, %d buffer sets of %.0f MB)" % (N, reps, sets, 8.0 * N ** 3 / 1e6))
    for name, _ in cands:
        say("  %-18s %9.3f / %9.3f / %9.3f" % ((name,) + res[name]))
    say("  ssim value fused %.9f, composed %.9f (difference %.2e)" % (a, b, abs(a - b)))
    nbytes = 8.0 * N ** 3
    for name in ("pair stats", "label counts"):
        bw = nbytes / (res[name][1] * 1e-3)
        say("  %-18s %.2f TB/s over %.0f MB read = %.0f %% of the 8.0 TB/s HBM peak" % (name, bw / 1e12, nbytes / 1e6,
                                                                                        100.0 * bw / HBM_PEAK))
    say("  label counts vs one-hot dice: %.1f x" % (res["one-hot dice"][1] / res["label counts"][1]))
    spread = max(res[k][2] - res[k][0] for k in ("ssim fused", "ssim composed"))
    gain = res["ssim composed"][1] - res["ssim fused"][1]
    wins = gain > spread
    say("  ssim composed - fused = %+.3f ms (%.1f x), spread (max - min) %.3f ms: fused %s" %
        (gain, res["ssim composed"][1] / res["ssim fused"][1], spread,
         "beats the composed route by more than the spread" if wins else "does NOT beat the composed route by more than the spread"))
    if big:
        say("  ms-ssim composed / fused = %.1f x" % (res["ms-ssim composed"][1] / res["ms-ssim fused"][1]))
    return wins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 160])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_evaluator.py needs a HIP device")
    dev = torch.device("cuda:0")
    wins = [bench_size(N, a.reps, dev) for N in a.sizes]
    say("fused SSIM kernel as the default: %s" % ("justified at every size measured" if all(wins) else
                                                  "NOT justified: the composed route should be the default"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
