"""Generate tests/golden/infer_deep_{a,b,c}.npz by RUNNING the reference on the shipped architecture (64 maps, 6 levels).

Run in the build container only (needs the reference tree, about 10 minutes on 8 threads):
    python tests/golden/make_golden_deep.py

The weights are the reference's default initialisation under torch.manual_seed(1), the same draw the product's
build_model makes (bench.py: BASELINE.md section 4), so the fixture stores their sha256 hashes instead of 1 GB of
weights; the inputs are regenerated too (bench.make_volume, bench.make_atlas, a seeded generator) and stored as hashes.

Case A: the bench flow, scripts/demo_test.py:66-119 over bench.make_volume(256) (27 tiles of win 160 / stride 80) with
  the deformed atlas of bench.make_atlas(); the 17 stitched keys at 32 768 sampled voxels (the first 32 768 of the
  bench's --dump-outputs permutation, sorted), their float64 whole-volume moments, and per sampled voxel the smallest
  fp32 relative top-2 gap of the segmentation over the tiles that cover it.
Case B: the one 160^3 tile of that run, (0:160)^3 (axis intervals of 256 are (0,160), (160,240), (176,256)), unstitched.
Case C: a seeded 64 x 80 x 96 input with a zero slab (pooling 5 -> 2, upsampling 2 -> 5).
For B and C: the 15 float maps at 4 096 seeded voxels and the 56 segmentation channels at every fourth of them (1 024),
per-channel float64 moments and
4 096 sampled entries of each of the 6 features, labels on the 1/8 sublattice, the label histogram, and every voxel whose
fp32 relative top-2 gap is below 1e-4, with its gap and label.

One file per case keeps every fixture under 1 MiB: infer_deep_a.npz (the hashes, the configuration and case A),
infer_deep_b.npz, infer_deep_c.npz.  tests/test_oracle_infer.py:load_deep() reads the three as one dict.
"""
import hashlib
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

R = ref_import.setup()
import torch  # noqa: E402

sys.path.insert(0, ROOT)
import bench  # noqa: E402
from make_golden_infer import load_ref_functions, run  # noqa: E402

torch.set_num_threads(8)

F_MAPS, LEVELS = 64, 6
N, STRIDE, WIN = 256, 80, 160
N_SAMPLE_A = 32768
N_SAMPLE_BC = 4096
N_FEAT_SAMPLE = 4096
TIE = 1e-4
C_SHAPE = (64, 80, 96)
C_SEED = 21


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def build():
    import utils.misc as um
    from Trainer.models import build_model
    gen_args = um.preprocess_cfg([R + "/cfgs/generator/default.yaml", R + "/cfgs/generator/test/demo_test.yaml"],
                                 cfg_dir="")
    train_args = um.preprocess_cfg([R + "/cfgs/trainer/default_train.yaml", R + "/cfgs/trainer/default_val.yaml",
                                    R + "/cfgs/trainer/test/demo_test.yaml"], cfg_dir="")
    train_args.f_maps = F_MAPS
    train_args.num_levels = LEVELS
    train_args.task_f_maps = [F_MAPS]
    torch.manual_seed(1)
    gen_args, train_args, model, processors, criterion, post = build_model(gen_args, train_args, "cpu")
    model.eval()
    return gen_args, train_args, model, processors, post


def top2_gap(seg):
    """fp32 relative gap of the two largest probabilities, (D,H,W)."""
    t = torch.topk(seg[0], 2, dim=0).values
    return (t[0] - t[1]) / t[0]


def case_input():
    g = torch.Generator().manual_seed(C_SEED)
    x = torch.rand((1, 1) + C_SHAPE, generator=g)
    x[:, :, :, :, :9] = 0                                  # a zero slab on the last axis
    return x


def single(o, prefix, d, seed):
    """Samples and moments of one unstitched output dict (case B / C)."""
    shape = tuple(o["segmentation"].shape[2:])
    nv = int(np.prod(shape))
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(nv, generator=g)[:N_SAMPLE_BC].sort().values
    d[prefix + "idx"] = idx.numpy().astype(np.int64)
    fkeys = [k for k in o if k not in ("feat", "segmentation", "label")]
    assert len(fkeys) == 15, fkeys
    d[prefix + "float_keys"] = np.array(fkeys)
    d[prefix + "floats"] = np.stack([o[k].reshape(-1)[idx].numpy() for k in fkeys])
    seg_idx = idx[::4]
    d[prefix + "seg_idx"] = seg_idx.numpy().astype(np.int64)
    d[prefix + "seg"] = o["segmentation"][0].reshape(56, -1)[:, seg_idx].numpy()
    for i, f in enumerate(o["feat"]):
        f64 = f[0].double().reshape(f.shape[1], -1)
        d[prefix + "feat%d_mean" % i] = f64.mean(1).numpy()
        d[prefix + "feat%d_sumsq" % i] = (f64 * f64).sum(1).numpy()
        d[prefix + "feat%d_min" % i] = f64.min(1).values.numpy()
        d[prefix + "feat%d_max" % i] = f64.max(1).values.numpy()
        fi = torch.randperm(f.numel(), generator=g)[:N_FEAT_SAMPLE].sort().values    # flat (channel, voxel) entries
        d[prefix + "feat%d_idx" % i] = fi.numpy().astype(np.int64)
        d[prefix + "feat%d_vals" % i] = f.reshape(-1)[fi].numpy()
    lab = o["label"][0, 0]
    assert int(lab.max()) <= 255
    d[prefix + "label_sub"] = lab[::2, ::2, ::2].numpy().astype(np.uint8)
    d[prefix + "label_hist"] = np.bincount(lab.reshape(-1).numpy(), minlength=256)[:int(lab.max()) + 1]
    gap = top2_gap(o["segmentation"]).reshape(-1)
    tie = torch.nonzero(gap < TIE)[:, 0]
    d[prefix + "tie_idx"] = tie.numpy().astype(np.int64)
    d[prefix + "tie_gap"] = gap[tie].numpy()
    d[prefix + "tie_label"] = lab.reshape(-1)[tie].numpy().astype(np.uint8)
    d[prefix + "shape"] = np.array(shape)
    print("%s: %d voxels with gap < 1e-4, %d < 1e-5 (smallest %.2e)" %
          (prefix, tie.numel(), int((gap < 1e-5).sum()), float(gap.min())))


@torch.no_grad()
def main():
    t0 = time.time()
    gen_args, train_args, model, processors, post = build()
    d = {}
    sd = model.state_dict()
    d["sd_names"] = np.array(list(sd.keys()))
    d["sd_sha256"] = np.array([sha(v) for v in sd.values()])
    print("%d state-dict tensors hashed" % len(sd))

    # ---- case C: the odd shape
    x = case_input()
    d["sha_C_input"] = np.array(sha(x))
    o = run(gen_args, train_args, model, processors, post, x.clone())
    single(o, "C/", d, seed=32)

    # ---- case A: the bench flow
    tiling, get_deformed_atlas = load_ref_functions(R + "/utils/test_utils.py", ["tiling", "get_deformed_atlas"])
    from Generator.utils import fast_3D_interp_torch
    full = bench.make_volume(N, "cpu")
    atlas, aff = bench.make_atlas()
    d["sha_volume"] = np.array(sha(full))
    d["sha_atlas"] = np.array(sha(atlas))
    d["atlas_aff"] = aff
    get_deformed_atlas.__globals__.update(MNI=atlas.to(torch.float32), fast_3D_interp_torch=fast_3D_interp_torch,
                                          A=torch.tensor(np.linalg.inv(aff), dtype=torch.float32))
    im_list, cnt = tiling(full, stride=[STRIDE] * 3, win_size=[WIN] * 3)
    assert len(im_list) == 27
    gap_min = torch.full((N, N, N), float("inf"))
    keys, acc = None, {}
    for i, (im, rng) in enumerate(im_list):
        o = run(gen_args, train_args, model, processors, post, im.clone())
        mask = im.clone()
        mask[im != 0.] = 1.
        (x0, x1), (y0, y1), (z0, z1) = rng
        if (x1 - x0, y1 - y0, z1 - z0) == (WIN,) * 3:
            assert (x0, y0, z0) == (0, 0, 0)
            single(o, "B/", d, seed=31)
            d["B/range"] = np.array(rng)
        o["deformed_atlas"] = get_deformed_atlas(torch.squeeze(mask), torch.squeeze(o["regx"]), torch.squeeze(o["regy"]),
                                                 torch.squeeze(o["regz"]))
        gap = top2_gap(o["segmentation"])
        m = torch.squeeze(mask) > 0
        sub = gap_min[x0:x1, y0:y1, z0:z1]
        sub[m] = torch.minimum(sub[m], gap[m])
        if keys is None:
            keys = [k for k in o if "feat" not in k and "segmentation" not in k]
            acc = {k: torch.zeros_like(torch.squeeze(full)) for k in keys}
        for k in keys:
            v = torch.squeeze(o[k] * mask)
            if "label" in k:
                v = v.to(torch.int)
            acc[k][x0:x1, y0:y1, z0:z1] += v
        del o
        print("tile %d/%d %s  %.0f s" % (i + 1, len(im_list), rng, time.time() - t0), flush=True)
    assert len(keys) == 17 and keys[-1] == "deformed_atlas"
    idx = torch.randperm(N ** 3, generator=torch.Generator().manual_seed(bench.DUMP_SEED))[:N_SAMPLE_A].sort().values
    d["A/idx"] = idx.numpy().astype(np.int64)
    d["A/keys"] = np.array(keys)
    vals, mom = [], []
    for k in keys:
        st = (acc[k] / cnt).reshape(-1)
        vals.append(st[idx].numpy())
        s64 = st.double()
        mom.append([float(s64.sum()), float((s64 * s64).sum()), float(s64.min()), float(s64.max())])
    d["A/vals"] = np.stack(vals)
    d["A/moments"] = np.array(mom)
    d["A/gap"] = gap_min.reshape(-1)[idx].numpy()
    ga = d["A/gap"]
    print("A: sampled voxels with gap < 1e-4: %d, < 1e-5: %d" % (int((ga < 1e-4).sum()), int((ga < 1e-5).sum())))

    d["cfg"] = np.array([F_MAPS, LEVELS, 8, STRIDE, WIN, C_SEED] + list(C_SHAPE))
    for case in "abc":
        part = {k: v for k, v in d.items() if k.startswith(case.upper() + "/")}
        if case == "a":
            part.update({k: v for k, v in d.items() if "/" not in k and k != "sha_C_input"})
        if case == "c":
            part["sha_C_input"] = d["sha_C_input"]
        path = os.path.join(HERE, "infer_deep_%s.npz" % case)
        np.savez_compressed(path, **part)
        size = os.path.getsize(path)
        print("infer_deep_%s.npz: %d bytes" % (case, size))
        assert size < 1 << 20, "a committed file must stay under 1 MiB"
    print("%.0f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
