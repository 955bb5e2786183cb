"""Backward of the first layer of the two-stage model's stage 1 WITH the input gradient through the mask (2 -> 32 at 128^3
and 160^3): the fused pair (bfm_stem_mc_bwd + bfm_stem_mc_dgrad; BFM_STEM_MC_DGRAD=1) against the generic route (weight
gradient by columns + 32 -> 64 data-gradient conv + slice + bfm_gn_bwd + bfm_mask_chain_bwd), alternated in one process.
What is timed is backward.backward_single_conv(..., input_grad=...) between two HIP events -- bfm_lrelu_bwd, which both
routes run first, included -- and the fused kernels alone.  Cold: the operands rotate over SETS buffer sets, and the dP of
one case (268 MB at 128^3) already exceeds the 256 MiB Infinity Cache.  Reports min / median / max over the repeats and the
fraction of the HBM peak over the algorithmic nvox * (Cout + 4) * 4 bytes (dP, x_cl's channel, x_raw, p, dRaw).  With
--iteration: one joint 128^3 training iteration of the full-width two-stage net with the switch on and off.

usage: python scripts/bench_stem_dgrad.py [--sizes 128 160] [--reps 7] [--iteration] [--out profiles/stem_dgrad.txt]"""
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
SETS = 3
LINES = []
DEFAULT = BW.STEM_MC_DGRAD


def say(s):
    print(s, flush=True)
    LINES.append(s)


def ev():
    return torch.cuda.Event(enable_timing=True)


def timed(fn, reps, warm=2):
    for i in range(warm):
        fn(i)
    ts = []
    for i in range(reps):
        e0, e1 = ev(), ev()
        e0.record()
        fn(warm + i)
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
    x_raw = torch.rand(dims, generator=g).to(dev)
    p = torch.sigmoid(3.0 * torch.randn(dims, generator=g)).to(dev)
    x = torch.rand(dims + (cin,), generator=g).to(dev)
    x[..., 0] = x_raw * (1 - p)
    x[..., cin - 1] = (x[..., cin - 1] > 0.6).float()
    _, t = BW.train_single_conv(eng, ly, x, dims)
    dYs = [torch.randn(dims + (cout,), generator=g).to(dev) for _ in range(SETS)]
    dRaws = [torch.zeros(dims, device=dev) for _ in range(SETS)]
    lib = eng.lib
    out = {}

    def run(fused):
        def fn(i):
            BW.STEM_MC_DGRAD = fused
            k = i % SETS
            if i == 0:
                dRaws[0].zero_()
            ig = BW.InputGrad(0, x_raw, p, dRaws[k], 0, 1)
            gr = BW.backward_single_conv(eng, t, dYs[k], need_input_grad=True, input_grad=ig)[2]
            if i == 0:
                torch.cuda.synchronize()
                out[fused] = dict(gr, dRaw=dRaws[0].clone())
        return fn

    dP = torch.empty_like(dYs[0])
    ws = torch.empty(lib.bfm_stem_mc_bwd_workspace(cin, cout, N, N, N), dtype=torch.uint8, device=dev)
    dW = torch.empty((cout, cin, 27), device=dev)
    dg, db = torch.empty(cin, device=dev), torch.empty(cin, device=dev)

    def lrelu(i):
        L.check(lib.bfm_lrelu_bwd_ex(L.ptr(dYs[i % SETS]), L.ptr(t.out), dP.numel(), eng.slope, L.ptr(dP), None, L.stream_ptr()),
                "lrelu_bwd")

    def lrelu_and_pair(i):
        lrelu(i)
        L.check(lib.bfm_stem_mc_bwd(L.ptr(dP), cout, L.ptr(x), cin, N, N, N, L.ptr(ly.w_raw), L.ptr(t.scale), L.ptr(t.shift),
                                    L.ptr(t.mean), L.ptr(t.rstd), L.ptr(dW), L.ptr(dg), L.ptr(db), L.ptr(ws), ws.numel(),
                                    L.stream_ptr()), "stem_mc_bwd")
        L.check(lib.bfm_stem_mc_dgrad(L.ptr(dP), cout, L.ptr(x), cin, N, N, N, L.ptr(ly.w_raw), L.ptr(ly.gamma), L.ptr(t.mean),
                                      L.ptr(t.rstd), L.ptr(dg), L.ptr(db), 0, None, L.ptr(x_raw), L.ptr(p),
                                      L.ptr(dRaws[i % SETS]), 0, 1, L.stream_ptr()), "stem_mc_dgrad")

    def lrelu_and_dgrad(i):
        lrelu(i)
        L.check(lib.bfm_stem_mc_dgrad(L.ptr(dP), cout, L.ptr(x), cin, N, N, N, L.ptr(ly.w_raw), L.ptr(ly.gamma), L.ptr(t.mean),
                                      L.ptr(t.rstd), L.ptr(dg), L.ptr(db), 0, None, L.ptr(x_raw), L.ptr(p),
                                      L.ptr(dRaws[i % SETS]), 0, 1, L.stream_ptr()), "stem_mc_dgrad")

    res = {}
    for _ in range(2):                                   # alternate, keep the better pass of each
        for name, fn in (("fused", run(True)), ("generic", run(False)), ("lrelu", lrelu), ("lrelu+pair", lrelu_and_pair),
                         ("lrelu+dgrad", lrelu_and_dgrad)):
            r = timed(fn, reps)
            if name not in res or r[1] < res[name][1]:
                res[name] = r
    BW.STEM_MC_DGRAD = DEFAULT
    err = max(float((out[True][k] - out[False][k]).abs().max() / out[False][k].abs().max()) for k in out[True])
    nbytes = float(N) ** 3 * (cout + 4) * 4
    pair = res["lrelu+pair"][1] - res["lrelu"][1]
    dgr = res["lrelu+dgrad"][1] - res["lrelu"][1]
    spread = max(res[k][2] - res[k][0] for k in ("fused", "generic"))
    say("%d -> %d @ %d^3   (ms: min / median / max over %d, %d buffer sets)" % (cin, cout, N, reps, SETS))
    for name in ("fused", "generic", "lrelu", "lrelu+pair", "lrelu+dgrad"):
        say("  %-13s %8.3f / %8.3f / %8.3f" % ((name,) + res[name]))
    say("  bfm_stem_mc_dgrad alone (median difference) %.3f ms = %.3f of the HBM peak over %.0f MB; the pair alone %.3f ms"
        % (dgr, nbytes / (dgr * 1e-3) / HBM_PEAK, nbytes / 1e6, pair))
    say("  generic - fused = %.3f ms (generic / fused = %.2fx), spread (max - min) %.3f ms; fused against generic "
        "max|a-b|/max|b| = %.1e" % (res["generic"][1] - res["fused"][1], res["generic"][1] / res["fused"][1], spread, err))
    return res["generic"][1] - res["fused"][1] > spread


def iteration(N, reps, dev):
    from brainfm_amd import models as M
    from brainfm_amd import test_utils as TU
    ga, ta = TU.default_inference_args(f_maps=64, num_levels=6, tasks=dict(
        T1=True, T2=True, FLAIR=True, CT=True, segmentation=True, distance=True, bias_field=True, registration=True,
        super_resolution=True, surface=False, pathology=True, contrastive=False))
    ta.backbone = "unet3d+unet3d"
    ta.condition = None
    ta.losses = Namespace(uncertainty=None, implicit_pathol=False, image_grad=True, registration_grad=True)
    ta.weights = Namespace(image=1.0, image_grad=1.0, seg_ce=1.0, seg_dice=1.0, bias_field_log=1.0, distance=1.0,
                           registration=1.0, registration_grad=1.0, pathol_ce=1.0, pathol_dice=1.0)
    torch.manual_seed(1)
    ga, ta, pm, tm = M.build_inpaint_model(ga, ta, dev)[:4]
    eng1 = tm.backbone.engine(tm.head)
    ns = tm.head.tail(eng1).desc.n_seg
    step = TR.twostage_train_step(ga, ta, pm, tm, torch.full((ns,), 1.0 / ns), 4, lr=1e-4)
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
        BW.STEM_MC_DGRAD = fused
        samples = [dict(extra, input=x)]
        e = [ev() for _ in range(2)]
        e[0].record()
        loss_dict, total, stepped = step.step([x], target, samples)
        e[1].record()
        torch.cuda.synchronize()
        return e[0].elapsed_time(e[1]), total, stepped

    one(True)                                            # tunes the conv variants, packs, allocates the optimiser state
    one(False)
    acc = {True: [], False: []}
    for _ in range(reps):
        for fused in (True, False):
            acc[fused].append(one(fused))
    BW.STEM_MC_DGRAD = DEFAULT
    say("one joint two-stage iteration (step()), f_maps 64, 6 levels, %d^3, 1 sample (ms: min / median / max over %d)" % (N, reps))
    for fused in (True, False):
        ts = [r[0] for r in acc[fused]]
        say("  %-8s %.1f / %.1f / %.1f   (loss %.4f, stepped %s)" % ("fused" if fused else "generic", min(ts),
                                                                      statistics.median(ts), max(ts), acc[fused][-1][1],
                                                                      acc[fused][-1][2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[128, 160])
    ap.add_argument("--cin", type=int, default=2)
    ap.add_argument("--cout", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iteration", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stem_dgrad.py needs a HIP device")
    dev = torch.device("cuda:0")
    wins = []
    for N in a.sizes:
        wins.append(layer_case(a.cin, a.cout, N, a.reps, dev))
        torch.cuda.empty_cache()
    if wins:
        say("the fused pair beats the generic route by more than the spread at %s: BFM_STEM_MC_DGRAD %s"
            % ("every size" if all(wins) else "%d of %d sizes" % (sum(wins), len(wins)),
               "may default to 1" if all(wins) else "stays opt-in"))
    if a.iteration:
        iteration(128, max(2, a.reps // 2), dev)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
