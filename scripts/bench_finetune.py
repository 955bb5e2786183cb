"""Head-only fine-tuning on a frozen backbone (TrainStep(trainable="head")) against the full iteration, on the shipped
64-wide 6-level net with the demo head set (69 head channels), one sample per iteration:

  iteration   forward (backbone + heads) | losses | backward | clip + AdamW (+ repack), device-event times per phase, and
              torch.cuda.max_memory_allocated of each kind of step, at 128^3 and 160^3.  The full iteration is this tree's
              TrainStep(trainable='all'), the default path, measured in the same process -- not a run of an earlier commit.
  kernel      bfm_head_wgrad_rows against bfm_head_bwd_rows (which also writes the [nvox][64] feature gradient) on the same
              buffers at 160^3, in microseconds and as a share of the 8.0 TB/s HBM peak over the algorithmic bytes
              nvox * (64 + n_out) * 4 of the weight gradient alone.

Cold by size: every phase streams several times the 256 MiB Infinity Cache, and the kernel comparison rotates over SETS
buffer sets.  min / median / max over the repeats; the two kinds are alternated and the better pass of each is kept.

usage: python scripts/bench_finetune.py [--reps 7] [--sets 2] [--sizes 128,160] [--out profiles/finetune.txt]"""
import argparse
import gc
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from brainfm_amd import _lib as L
from brainfm_amd import test_utils as TU
from brainfm_amd import train as TR

HBM_PEAK = 8.0e12
NAMES = ["T1", "T1_grad", "T2", "T2_grad", "FLAIR", "FLAIR_grad", "CT", "CT_grad", "seg_ce", "seg_dice", "distance",
         "bias_field_log", "registration", "registration_grad", "SR", "SR_grad"]
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def ev():
    return torch.cuda.Event(enable_timing=True)


def mmm(ts):
    return min(ts), statistics.median(ts), max(ts)


def fmt(r):
    return "%8.2f / %8.2f / %8.2f" % r


def data(n, ns, dev):
    g = torch.Generator().manual_seed(0)
    dims = (n, n, n)
    x = torch.rand((1, 1) + dims, generator=g).to(dev)
    lab = torch.randint(0, ns, (1,) + dims, generator=g)
    target = {"segmentation": torch.nn.functional.one_hot(lab, ns).permute(0, 4, 1, 2, 3).float().contiguous().to(dev)}
    for k in ("T1", "T2", "FLAIR", "CT"):
        target[k] = torch.rand((1, 1) + dims, generator=g).to(dev)
    target["distance"] = torch.randn((1, 4) + dims, generator=g).to(dev)
    target["registration"] = torch.randn((1, 3) + dims, generator=g).to(dev)
    sample = {"bias_field_log": torch.randn((1, 1) + dims, generator=g).to(dev) * 0.3,
              "high_res_residual": torch.randn((1, 1) + dims, generator=g).to(dev) * 0.2}
    return x, target, sample


def iteration(trainable, n, reps, dev):
    """Per-phase times (ms) and the peak memory of `reps` iterations of one kind of step on a fresh session."""
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    ga, ta = TU.default_inference_args(f_maps=64, num_levels=6)
    torch.manual_seed(1)                       # default nn init under seed 1, as bench.py
    s = TU.InferenceSession(ga, ta, dev, passes=3)
    tail = s.model.head.tail(s.engine)
    ns = tail.desc.n_seg
    step = TR.TrainStep(s.engine, tail, NAMES, {"loss_" + k: 1.0 for k in NAMES}, torch.full((ns,), 1.0 / ns), 1, lr=1e-4,
                        trainable=trainable)
    x, target, sample = data(n, ns, dev)
    scale = step.scaler.scale
    phases = {k: [] for k in ("forward", "losses", "backward", "optimiser", "iteration")}
    total = None
    for r in range(reps + 2):                  # two warm passes: tuning and packs, then optimiser state and dgrad packs
        e = [ev() for _ in range(5)]
        step._touched_heads = set()
        e[0].record()
        ctx = step._sample_forward(x)
        e[1].record()
        step._sample_criterion(ctx, target, sample, scale)
        e[2].record()
        grads, slots, vals = step._sample_backward(ctx, target, scale)
        e[3].record()
        ok, _ = step.apply(grads)
        e[4].record()
        torch.cuda.synchronize()
        ld = step._finish_losses([(slots, vals)], n ** 3)
        total = sum(ld.values())
        del ctx, grads
        if r < 2:
            continue
        for k, i in (("forward", 0), ("losses", 1), ("backward", 2), ("optimiser", 3)):
            phases[k].append(e[i].elapsed_time(e[i + 1]))
        phases["iteration"].append(e[0].elapsed_time(e[4]))
    peak = torch.cuda.max_memory_allocated(dev) / 2 ** 30
    n_train = sum(v.numel() for k, v in step.parameters().items() if k in TR.trainable_names(list(step.parameters()), trainable))
    del step, s, tail
    return {k: mmm(v) for k, v in phases.items()}, peak, total, ok, n_train


def kernels(n, n_out, reps, nsets, dev):
    lib = L.load()
    nvox, cf = n ** 3, 64
    g = torch.Generator(device=dev).manual_seed(3)
    sets = []
    for _ in range(nsets):
        rows = torch.randn((n_out, nvox), generator=g, device=dev)
        fn = torch.randn((nvox, cf), generator=g, device=dev)
        sets.append((rows, fn, torch.empty((nvox, cf), device=dev)))
    w = torch.randn((n_out, cf), generator=g, device=dev)
    dW, db = torch.empty((n_out, cf), device=dev), torch.empty(n_out, device=dev)
    ws = torch.empty(max(lib.bfm_head_bwd_workspace(n_out, cf, nvox), lib.bfm_head_wgrad_workspace(n_out, cf, nvox)),
                     dtype=torch.uint8, device=dev)

    def wgrad(i):
        rows, fn, _ = sets[i % nsets]
        L.check(lib.bfm_head_wgrad_rows(L.ptr(rows), nvox, L.ptr(fn), n_out, cf, nvox, L.ptr(dW), L.ptr(db), L.ptr(ws),
                                        ws.numel(), L.stream_ptr()), "head_wgrad_rows")

    def bwd(i):
        rows, fn, dfn = sets[i % nsets]
        L.check(lib.bfm_head_bwd_rows(L.ptr(rows), nvox, L.ptr(fn), L.ptr(w), n_out, cf, nvox, L.ptr(dW), L.ptr(db),
                                      L.ptr(dfn), L.ptr(ws), ws.numel(), L.stream_ptr()), "head_bwd_rows")

    res = {}
    for _ in range(2):
        for name, f in (("bfm_head_wgrad_rows", wgrad), ("bfm_head_bwd_rows", bwd)):
            for i in range(2):
                f(i)
            ts = []
            for i in range(reps):
                e0, e1 = ev(), ev()
                e0.record()
                f(2 + i)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            r = mmm(ts)
            if name not in res or r[1] < res[name][1]:
                res[name] = r
    return res, nvox * (cf + n_out) * 4.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--sizes", default="128,160")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune.py needs a HIP device")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    say("64-wide 6-level net, demo head set, one sample per iteration; ms: min / median / max over %d iterations after two "
        "warm ones" % a.reps)
    say("the full iteration is TrainStep(trainable='all') of THIS tree, run in this process; it is not a separate run of an "
        "earlier commit")
    for n in (int(v) for v in a.sizes.split(",") if v):
        res = {}
        for kind in ("all", "head"):
            res[kind] = iteration(kind, n, a.reps, dev)
        say("crop %d^3" % n)
        for kind, label in (("all", "full iteration  (trainable='all') "), ("head", "frozen backbone (trainable='head')")):
            ph, peak, total, ok, n_train = res[kind]
            say("  %s  %d trained parameters, loss %.4f stepped=%s, peak memory %.2f GiB" % (label, n_train, total, ok, peak))
            for k in ("forward", "losses", "backward", "optimiser", "iteration"):
                say("      %-10s %s" % (k, fmt(ph[k])))
        full, froz = res["all"][0]["iteration"], res["head"][0]["iteration"]
        say("  frozen / full iteration (medians): %.2f / %.2f ms = %.2f x; peak memory %.2f / %.2f GiB"
            % (froz[1], full[1], froz[1] / full[1], res["head"][1], res["all"][1]))
    n, n_out = 160, 69
    res, nbytes = kernels(n, n_out, max(a.reps, 9), max(1, a.sets), dev)
    say("heads' weight gradient at %d^3, n_out %d, C 64, dRaw in rows; us: min / median / max, %d buffer sets, better of two "
        "alternated passes; algorithmic bytes nvox * (64 + n_out) * 4 = %.3f GB" % (n, n_out, max(1, a.sets), nbytes / 1e9))
    for name in ("bfm_head_wgrad_rows", "bfm_head_bwd_rows"):
        r = res[name]
        say("  %-22s %s   %.2f TB/s = %2.0f %% of the 8.0 TB/s HBM peak over those bytes%s"
            % (name, fmt(r), nbytes / (r[1] * 1e-6) / 1e12, 100.0 * nbytes / (r[1] * 1e-6) / HBM_PEAK,
               "" if name == "bfm_head_wgrad_rows" else " (it also writes dFn, nvox * 64 * 4 more)"))
    wg, bw = res["bfm_head_wgrad_rows"], res["bfm_head_bwd_rows"]
    spread = max(wg[2] - wg[0], bw[2] - bw[0])
    if wg[1] < bw[1] and bw[1] - wg[1] > spread:
        verdict = "bfm_head_wgrad_rows is faster beyond the spread: the frozen step calls it"
    elif wg[1] <= bw[1]:
        verdict = "bfm_head_wgrad_rows is no slower, within the spread"
    else:
        verdict = "bfm_head_wgrad_rows is NOT faster than bfm_head_bwd_rows writing a scratch dFn"
    say("  wgrad / bwd = %.2f x (medians), spread (max - min) %.1f us: %s" % (wg[1] / bw[1], spread, verdict))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
