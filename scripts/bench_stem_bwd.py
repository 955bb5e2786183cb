"""Backward of the first layer of a conditioned network (2 -> 32 and 3 -> 32 at 128^3 and 160^3): the one-correlation
route (bfm_stem_mc_bwd) against the generic one (weight gradient by columns + 32 -> 64 data-gradient conv + slice +
bfm_gn_bwd; what runs without BFM_STEM_MC_BWD=1), alternated in one process.  What is timed is backward.backward_single_conv(...,
need_input_grad=False) between two HIP events -- bfm_lrelu_bwd, which both routes run first, included -- and the fused
kernels alone.  Cold by size: the dP of one case (268 MB at 128^3) exceeds the 256 MiB Infinity Cache and is rewritten in
front of every launch.  Reports min / median / max over the repeats and the fraction of the HBM peak over the algorithmic
nvox * (Cout + Cin) * 4 bytes.  With --iteration: one 128^3 training iteration of the full-width 'mask'-conditioned net,
forward / losses + backward / optimiser, with the fused route on and off.

usage: python scripts/bench_stem_bwd.py [--sizes 128 160] [--reps 5] [--iteration] [--out profiles/stem_bwd.txt]"""
import argparse
import os
import statistics
import sys
from argparse import Namespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from brainfm_amd import _lib as L
from brainfm_amd import backward as BW
from brainfm_amd import train as TR

HBM_PEAK = 8.0e12          # bytes/s, MI355X
LINES = []
DEFAULT = BW.STEM_MC_BWD


def say(s):
    print(s, flush=True)
    LINES.append(s)


def ev():
    return torch.cuda.Event(enable_timing=True)


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = ev(), ev()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return min(ts), statistics.median(ts), max(ts)


def layer_case(cin, cout, N, reps, dev):
    from brainfm_amd.engine import UNetEngine
    from oracle import unet_ref as O
    eng = UNetEngine(O.random_state_dict(cin, 2 * cout, 2, out_channels={}, seed=1), cin, 2 * cout, 2, device=dev)
    ly = eng.enc[0][0]
    dims = (N, N, N)
    g = torch.Generator().manual_seed(N + cin)
    x = torch.rand(dims + (cin,), generator=g).to(dev)
    _, t = BW.train_single_conv(eng, ly, x, dims)
    dY = torch.randn(dims + (cout,), generator=g).to(dev)
    lib = eng.lib
    out = {}

    def run(fused):
        def fn():
            BW.STEM_MC_BWD = fused
            out[fused] = BW.backward_single_conv(eng, t, dY, need_input_grad=False)[2]
        return fn

    dP = torch.empty_like(dY)
    ws = torch.empty(lib.bfm_stem_mc_bwd_workspace(cin, cout, N, N, N), dtype=torch.uint8, device=dev)
    dW = torch.empty((cout, cin, 27), device=dev)
    dg, db = torch.empty(cin, device=dev), torch.empty(cin, device=dev)

    def lrelu():
        L.check(lib.bfm_lrelu_bwd_ex(L.ptr(dY), L.ptr(t.out), dY.numel(), eng.slope, L.ptr(dP), None, L.stream_ptr()), "lrelu_bwd")

    def lrelu_and_kernel():
        lrelu()
        L.check(lib.bfm_stem_mc_bwd(L.ptr(dP), cout, L.ptr(x), cin, N, N, N, L.ptr(ly.w_raw), L.ptr(t.scale), L.ptr(t.shift),
                                    L.ptr(t.mean), L.ptr(t.rstd), L.ptr(dW), L.ptr(dg), L.ptr(db), L.ptr(ws), ws.numel(),
                                    L.stream_ptr()), "stem_mc_bwd")

    res = {}
    for _ in range(2):                                   # alternate, keep the better pass of each
        for name, fn in (("fused", run(True)), ("generic", run(False)), ("lrelu", lrelu), ("lrelu+kernel", lrelu_and_kernel)):
            r = timed(fn, reps)
            if name not in res or r[1] < res[name][1]:
                res[name] = r
    BW.STEM_MC_BWD = DEFAULT
    err = max(float((out[True][k] - out[False][k]).abs().max() / out[False][k].abs().max()) for k in out[True])
    nbytes = float(N) ** 3 * (cout + cin) * 4
    kern = res["lrelu+kernel"][1] - res["lrelu"][1]
    say("%d -> %d @ %d^3   (ms: min / median / max over %d)" % (cin, cout, N, reps))
    for name in ("fused", "generic", "lrelu", "lrelu+kernel"):
        say("  %-13s %8.3f / %8.3f / %8.3f" % ((name,) + res[name]))
    say("  fused kernels alone (median difference) %.3f ms = %.3f of the HBM peak over %.0f MB; generic / fused = %.2fx; "
        "fused against generic max|a-b|/max|b| = %.1e" % (kern, nbytes / (kern * 1e-3) / HBM_PEAK, nbytes / 1e6,
                                                           res["generic"][1] / res["fused"][1], err))
    return res


def iteration(N, reps, dev):
    from brainfm_amd import models as M
    from brainfm_amd import test_utils as TU
    ga, ta = TU.default_inference_args(f_maps=64, num_levels=6, tasks=dict(
        T1=True, T2=True, FLAIR=True, CT=True, segmentation=True, distance=True, bias_field=True, registration=True,
        super_resolution=True, surface=False, pathology=True, contrastive=False))
    ta.condition = "mask"
    ta.losses = Namespace(uncertainty=None, implicit_pathol=False, image_grad=True, registration_grad=True)
    ta.weights = Namespace(image=1.0, image_grad=1.0, seg_ce=1.0, seg_dice=1.0, bias_field_log=1.0, distance=1.0,
                           registration=1.0, registration_grad=1.0)
    torch.manual_seed(1)
    ga, ta, model, _, _, _ = M.build_conditioned_model(ga, ta, dev)
    eng = model.backbone.engine(model.head)
    ns = model.head.tail(eng).desc.n_seg
    step = TR.conditioned_train_step(ga, ta, model, torch.full((ns,), 1.0 / ns), 4, lr=1e-4)
    g = torch.Generator().manual_seed(0)
    dims = (N, N, N)
    lab = torch.randint(0, ns, (1,) + dims, generator=g)
    target = {"segmentation": torch.nn.functional.one_hot(lab, ns).permute(0, 4, 1, 2, 3).float().contiguous().to(dev)}
    for k in ("T1", "T2", "FLAIR", "CT"):
        target[k] = torch.rand((1, 1) + dims, generator=g).to(dev)
    target["distance"] = torch.randn((1, 4) + dims, generator=g).to(dev)
    target["registration"] = torch.randn((1, 3) + dims, generator=g).to(dev)
    target["pathology"] = (torch.rand((1, 1) + dims, generator=g) > 0.9).float().to(dev)
    x = torch.rand((1, 1) + dims, generator=g).to(dev)
    extra = {"bias_field_log": torch.randn((1, 1) + dims, generator=g).to(dev) * 0.3,
             "high_res_residual": torch.randn((1, 1) + dims, generator=g).to(dev) * 0.2}

    def one(fused):
        BW.STEM_MC_BWD = fused
        samples = [dict(extra, input=x.clone())]
        e = [ev() for _ in range(4)]
        e[0].record()
        cond = TR.condition_inputs(samples, target, ta.condition, in_channels=eng.in_channels)
        e[1].record()
        loss_dict, total, grads = step.loss_and_grads([x], target, samples, cond=cond)
        e[2].record()
        ok, _ = step.apply(grads)
        e[3].record()
        torch.cuda.synchronize()
        return [e[i].elapsed_time(e[i + 1]) for i in range(3)], total, ok

    one(True)                                            # tunes the conv variants, packs, allocates the optimiser state
    one(False)
    acc = {True: [], False: []}
    for _ in range(reps):
        for fused in (True, False):
            acc[fused].append(one(fused))
    BW.STEM_MC_BWD = DEFAULT
    say("one 'mask'-conditioned iteration, f_maps 64, 6 levels, %d^3, 1 sample (ms, median of %d)" % (N, reps))
    for fused in (True, False):
        ph = [statistics.median(r[0][i] for r in acc[fused]) for i in range(3)]
        say("  %-8s condition_inputs %.3f | forward + losses + backward %.1f | clip + AdamW %.1f | iteration %.1f   (loss %.4f, "
            "stepped %s)" % ("fused" if fused else "generic", ph[0], ph[1], ph[2], sum(ph), acc[fused][-1][1], acc[fused][-1][2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[128, 160])
    ap.add_argument("--cins", type=int, nargs="*", default=[2, 3])
    ap.add_argument("--cout", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iteration", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stem_bwd.py needs a HIP device")
    dev = torch.device("cuda:0")
    for N in a.sizes:
        for cin in a.cins:
            layer_case(cin, a.cout, N, a.reps, dev)
            torch.cuda.empty_cache()
    if a.iteration:
        iteration(128, max(2, a.reps // 2), dev)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
