"""Timing of the surface task's hot path at 160^3 (profiles/svf_surface.txt):

  fused     : bfm_svf_integrate, n = 8, both directions (8 launches)
  composed  : the same integration from existing calls -- torch elementwise adds for the coordinates and the add,
              fast_3D_interp_torch (bfm_interp3d_linear, C = 3) for the gather -- the chain the fused kernel replaces
  item      : one BrainIDGen item (two samples) with task.surface off and on, same seeds

    python scripts/bench_svf.py [--reps 20]
Wall times from CUDA events around each call, median of --reps after warm-up; one JSON line at the end.
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from brainfm_amd import generator as G  # noqa: E402
from brainfm_amd import generator_utils as GU  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def composed(F, n, grids):
    xx, yy, zz = grids
    s = 1.0 / 2 ** n
    res = []
    for Fs in (F * s, -F * s):
        for _ in range(n):
            Fs = Fs + GU.fast_3D_interp_torch(Fs, xx + Fs[..., 0], yy + Fs[..., 1], zz + Fs[..., 2], "linear")
        res.append(Fs)
    return res


def item_dataset(surface, size):
    cfg = json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", "svf_surface_item.npz"))["C/cfg_json"]))
    cfg["generator"]["size"] = list(size)
    cfg["task"]["surface"] = surface
    cfg["dataset_option"] = "brain_id"

    def ns(v):
        from argparse import Namespace
        return Namespace(**{k: ns(x) for k, x in v.items()}) if isinstance(v, dict) else v
    rs = np.random.RandomState(0)
    shp = [s + 16 for s in size]
    lab = (rs.rand(*shp) * 6).astype(np.int32) * 2 + 2
    case = {"Gen": lab.astype(np.float32), "T1": rs.rand(*shp).astype(np.float32), "name": "b", "dataset": "MEM"}
    return G.build_datasets(ns(cfg), DEV, cases=[case])["all"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=160)
    ap.add_argument("--n", type=int, default=8)
    a = ap.parse_args()
    size = (a.size,) * 3
    g = torch.Generator().manual_seed(0)
    small = [max(2, round(0.05 * v)) for v in size]
    F = GU.myzoom_torch((torch.randn(*small, 3, generator=g) * 4).to(DEV), np.array(size) / np.array(small))
    grids = torch.meshgrid(*[torch.arange(v, dtype=torch.float32, device=DEV) for v in size], indexing="ij")
    Fo, Fn = GU.svf_integrate(F, a.n)
    Ro, Rn = composed(F, a.n, grids)
    same = bool(torch.equal(Fo, Ro) and torch.equal(Fn, Rn))
    t_fused = timed(lambda: GU.svf_integrate(F, a.n), a.reps)
    t_comp = timed(lambda: composed(F, a.n, grids), a.reps)
    res = {"size": list(size), "n": a.n, "fused_ms": t_fused[0], "fused_min_ms": t_fused[1], "composed_ms": t_comp[0],
           "composed_min_ms": t_comp[1], "speedup": t_comp[0] / t_fused[0], "bitwise_equal": same}
    # the algorithmic traffic: per step and direction read 12 B of the field + write 12 B, 2 x n steps
    nvox = float(np.prod(size))
    res["fused_GBps_algorithmic"] = 2 * a.n * 24 * nvox / (t_fused[0] * 1e-3) / 1e9
    item = {}
    for surface in (False, True):
        ds = item_dataset(surface, size)
        ts = []
        for r in range(max(4, a.reps // 4) + 2):
            np.random.seed(r)
            random.seed(r)
            torch.manual_seed(r)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds[0]
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        item[surface] = float(np.median(ts[2:]))
    res["item_surface_off_ms"], res["item_surface_on_ms"] = item[False], item[True]
    res["item_delta_ms"] = item[True] - item[False]
    for k, v in res.items():
        print("%-26s %s" % (k, v))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
