"""Golden vectors for hidden task-head layers (task_f_maps longer than one) by RUNNING the reference.

Run in the build container only (needs the reference tree, a few minutes on 8 threads):
    python tests/golden/make_golden_headlayers.py

With task_f_maps = [c0, ..., cn] the reference's TaskHead (Trainer/models/head.py:27-31,52-55,152-167) puts
ConvBlock(c_i, c_i+1) = Conv3d(3, padding 1, bias) + LeakyReLU(0.2) between the backbone's last feature map and the 1x1x1
heads.  Written here (every file under 1 MiB; the parts of one fixture are read together by twostage_weights.load):

  head_layers.npz (+ _b)        f_maps 8, 3 levels, task_f_maps [8, 16], all nine heads, 24 x 32 x 40 input
  head_layers_wide.npz (+ _b)   f_maps 64, 2 levels, task_f_maps [64, 64], 16 x 24 x 20 input
  head_layers_tiled.npz (+ _b)  the narrow net through the reference's tile loop (scripts/demo_test.py:75-119 in memory,
                                without the atlas) on a 48 x 40 x 56 volume, window 32, stride 16
  head_layers_train.npz (+ _b, _c)  one training iteration of the narrow net (left hemisphere heads, 12 x 16 x 10, two
                                samples): every loss, every gradient in float64 (_b) and in float32 (_c)

Weights are drawn by tests/twostage_weights.py and kept as names, shapes, seed and sha256 (the training fixture stores
them).  Per forward case: the input; the label map in full; every float map at N_VOX seeded voxels, the segmentation at
every fourth of them, N_FEAT seeded entries of every feature map -- from the fp32 model and, under ref64/, from
model.double() (the make_golden_twostage.py layout).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_twostage as G2  # noqa: E402  (sets up the reference import harness)
import make_golden_infer as GI  # noqa: E402

R = G2.R
import torch  # noqa: E402

import twostage_weights as TW  # noqa: E402

N_TILE_VOX = 2048


def configs(f_maps, levels, task_f_maps, left_hemis=False):
    import utils.misc as um
    gen_args = um.preprocess_cfg([R + "/cfgs/generator/default.yaml", R + "/cfgs/generator/test/demo_test.yaml"], cfg_dir="")
    train_args = um.preprocess_cfg([R + "/cfgs/trainer/default_train.yaml", R + "/cfgs/trainer/default_val.yaml",
                                    R + "/cfgs/trainer/test/demo_test.yaml"], cfg_dir="")
    train_args.f_maps = f_maps
    train_args.num_levels = levels
    train_args.task_f_maps = list(task_f_maps)
    if left_hemis:
        gen_args.generator.left_hemis_only = True
    return gen_args, train_args


def build(f_maps, levels, task_f_maps, seed):
    from Trainer.models import build_model
    gen_args, train_args = configs(f_maps, levels, task_f_maps)
    torch.manual_seed(seed)
    gen_args, train_args, model, processors, criterion, post = build_model(gen_args, train_args, "cpu")
    sd = model.state_dict()
    new = TW.draw_state_dict(list(sd.keys()), [tuple(v.shape) for v in sd.values()], seed + 1)
    model.load_state_dict(new)
    model.eval()
    return gen_args, train_args, model, processors, post, new


@torch.no_grad()
def run(gen_args, train_args, model, processors, post, x):
    samples = [{"input": x}]
    outs, _ = model(samples)
    for p in processors:
        outs = p(outs, samples)
    outs, _, _ = post(gen_args, train_args, outs, samples, target=None, feats=None, tasks=gen_args.tasks)
    return outs[0]


def forward_case(stem, f_maps, levels, task_f_maps, shape, seed):
    print(stem)
    gen_args, train_args, model, processors, post, sd = build(f_maps, levels, task_f_maps, seed)
    assert len(model.head.layers) == len(task_f_maps) - 1
    d = {"cfg": np.array([f_maps, levels, 8]), "task_f_maps": np.array(task_f_maps)}
    G2.sd_meta(d, "model", sd, seed + 1)
    x = G2.make_input(shape, seed + 3)
    o = run(gen_args, train_args, model, processors, post, x.clone())
    o64 = run(gen_args, train_args, model.double(), processors, post, x.double())
    model.float()
    d["x"] = x.numpy()
    G2.record(d, o, o64, seed + 4)
    G2.save(stem, d)
    return gen_args, train_args, model, processors, post


@torch.no_grad()
def tiled_case(stem, net, seed):
    """scripts/demo_test.py:75-119 in memory: tiles, outputs * (tile != 0), labels as int, summed and divided by cnt."""
    print(stem)
    gen_args, train_args, model, processors, post = net
    (tiling,) = GI.load_ref_functions(R + "/utils/test_utils.py", ["tiling"])
    (zero_crop,) = GI.load_ref_functions(R + "/utils/test_utils.py", ["zero_crop"])
    tiling.__globals__["zero_crop"] = zero_crop
    D, H, W = 48, 40, 56
    zz, yy, xx = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
    ell = (((zz - D / 2 + .5) / 21.) ** 2 + ((yy - H / 2 + .5) / 17.) ** 2 + ((xx - W / 2 + .5) / 25.) ** 2) <= 1
    g = torch.Generator().manual_seed(seed)
    full = torch.rand((1, 1, D, H, W), generator=g) * ell[None, None]
    im_list, cnt = tiling(full, stride=[16, 16, 16], win_size=[32, 32, 32])
    stitched = {}
    for tag, dt in (("", torch.float32), ("ref64/", torch.float64)):
        m = model.to(dt)
        keys, acc = None, {}
        for im, rng in im_list:
            o = run(gen_args, train_args, m, processors, post, im.clone().to(dt))
            mask = im.clone().to(dt)
            mask[im != 0.] = 1.
            if keys is None:
                keys = [k for k in o if "feat" not in k and "segmentation" not in k]
                acc = {k: torch.zeros((D, H, W), dtype=dt) for k in keys}
            (x0, x1), (y0, y1), (z0, z1) = rng
            for k in keys:
                v = torch.squeeze(o[k] * mask)
                if "label" in k:
                    v = v.to(torch.int)
                acc[k][x0:x1, y0:y1, z0:z1] += v
        stitched[tag] = {k: (acc[k] / cnt.to(dt)) for k in keys}
    model.float()
    idx = torch.randperm(D * H * W, generator=g)[:N_TILE_VOX].sort().values
    d = {"full": full.numpy(), "idx": idx.numpy().astype(np.int64), "keys": np.array(keys),
         "cfg": np.array([16, 32]), "n_tiles": np.array(len(im_list))}
    for tag, st in stitched.items():
        d[tag + "stitched"] = np.stack([st[k].reshape(-1)[idx].numpy() for k in keys])
    d["label_full"] = stitched[""]["label"].numpy().astype(np.float32)
    print("  %d tiles, keys %s" % (len(im_list), keys))
    G2.save(stem, d)


def train_case(stem, seed):
    """One iteration of Trainer/engine.py:96-147 (model -> processors -> criterion -> weighted sum -> backward) without
    autocast / GradScaler, the make_golden_train.py recipe, with task_f_maps [8, 16]; in float64 and again in float32."""
    print(stem)
    from Trainer.models import build_model
    f_maps, levels, tfm = 8, 3, [8, 16]
    gen_args, train_args = configs(f_maps, levels, tfm, left_hemis=True)
    torch.manual_seed(seed)
    gen_args, train_args, model, processors, criterion, post = build_model(gen_args, train_args, "cpu")
    g = torch.Generator().manual_seed(seed + 1)
    TW.move_groupnorm(model.state_dict(), seed + 2)
    with torch.no_grad():
        model.head.final_conv_distance.weight.mul_(8.0)       # the DistProcessor clamp is active on part of the volume
        for lyr in model.head.layers:                          # biases at the scale of the layer's outputs
            lyr.main.bias.copy_(0.5 * (torch.rand(lyr.main.bias.shape, generator=g) - 0.5))
    sd32 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.train()
    criterion.train()
    wd = criterion.weight_dict
    for i, k in enumerate(sorted(wd)):
        wd[k] = float(0.5 + 0.25 * (i % 5))
    dims = (12, 16, 10)
    n_seg, n_dist = gen_args.n_labels, 2
    d = {}
    samples = []
    for i in range(2):
        x = torch.rand((1, 1) + dims, generator=g)
        bf = 0.3 * torch.randn((1, 1) + dims, generator=g)
        hr = 0.2 * torch.randn((1, 1) + dims, generator=g)
        samples.append({"input": x, "bias_field_log": bf, "high_res_residual": hr})
        d["x%d" % i], d["bias_field_log%d" % i], d["high_res_residual%d" % i] = x.numpy(), bf.numpy(), hr.numpy()
    lab = torch.randint(0, n_seg, (1,) + dims, generator=g)
    target = {"segmentation": torch.nn.functional.one_hot(lab, n_seg).permute(0, 4, 1, 2, 3).float().contiguous()}
    for k in ("T1", "T2", "FLAIR", "CT"):
        target[k] = torch.rand((1, 1) + dims, generator=g)
    target["T1_DM"] = (torch.rand((1, 1) + dims, generator=g) > 0.8).float()
    target["distance"] = torch.clamp(2.5 * torch.randn((1, n_dist) + dims, generator=g), -3, 3)
    target["registration"] = torch.randn((1, 3) + dims, generator=g)
    for k, v in target.items():
        d["target/" + k] = v.numpy()
    names = [n for n, _ in model.named_parameters()]
    for tag, dt in (("ref64/", torch.float64), ("ref32/", torch.float32)):
        model.to(dt)
        criterion.weights_ce = criterion.weights_ce.to(dt)
        criterion.weights_dice = criterion.weights_dice.to(dt)
        model.zero_grad()
        smp = [{k: v.to(dt) for k, v in s.items()} for s in samples]
        tgt = {k: v.to(dt) for k, v in target.items()}
        outputs, _ = model(smp)
        for p in processors:
            outputs = p(outputs, tgt, "synth")
        loss_dict = criterion(outputs, tgt, smp)
        losses = sum(loss_dict[k] * wd[k] for k in loss_dict.keys() if k in wd)
        losses.backward()
        for n, p in model.named_parameters():
            d[tag + "grad/" + n] = p.grad.detach().numpy().copy()
        for k, v in loss_dict.items():
            d[tag + "loss/" + k] = np.float64(float(v.detach()))
        d[tag + "loss_total"] = np.float64(float(losses.detach()))
        print("  %s total %.6f" % (tag, float(losses)))
    d["loss_weight_names"] = np.array(sorted(wd))
    d["loss_weights"] = np.array([wd[k] for k in sorted(wd)], dtype=np.float64)
    d["loss_names"] = np.array(list(criterion.loss_names))
    d["param_names"] = np.array(names)
    d["hyper"] = np.array([float(gen_args.generator.all_samples), float(gen_args.max_surf_distance)], dtype=np.float64)
    d["bias_field_log_type"] = np.array(str(train_args.losses.bias_field_log_type))
    d["weights_ce"] = criterion.weights_ce.double().reshape(-1).numpy()
    d["cfg"] = np.array([f_maps, levels, 8])
    d["task_f_maps"] = np.array(tfm)
    for k, v in sd32.items():
        d["sd/" + k] = v.numpy()
    parts = {"": {k: v for k, v in d.items() if not k.startswith("ref")},
             "_b": {k: v for k, v in d.items() if k.startswith("ref64/")},
             "_c": {k: v for k, v in d.items() if k.startswith("ref32/")}}
    for suffix, part in parts.items():
        path = os.path.join(HERE, stem + suffix + ".npz")
        np.savez_compressed(path, **part)
        print("  %s%s.npz: %d bytes" % (stem, suffix, os.path.getsize(path)))
        assert os.path.getsize(path) < 1 << 20, "a committed file must stay under 1 MiB"


if __name__ == "__main__":
    narrow = forward_case("head_layers", 8, 3, [8, 16], (24, 32, 40), 31)
    forward_case("head_layers_wide", 64, 2, [64, 64], (16, 24, 20), 41)
    tiled_case("head_layers_tiled", narrow, 51)
    train_case("head_layers_train", 61)
