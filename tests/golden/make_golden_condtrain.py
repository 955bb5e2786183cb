"""Generate the fixtures of one training iteration of the mask-conditioned model by RUNNING the reference.

Run in the build container only (needs the reference tree, under a minute on 8 threads):
    python tests/golden/make_golden_condtrain.py

The reference's own build_conditioned_model (Trainer/models/__init__.py:423-437) gives model, processors and criterion;
one iteration follows Trainer/engine.py:99-121 -- condition the inputs, model(samples, cond=cond), processors,
criterion, weighted sum -- then backward, without autocast / GradScaler.  It runs with model.double() (the truth,
keys ref64/...) and in float32 (torch's own distance from that truth, keys ref32/...).

  train_cond_mask.npz       condition 'mask',      (8,12,40),  binary mask
  train_cond_maskflip.npz   condition 'mask+flip', (7,10,36) (odd D: one slice maps to itself), soft mask in [0,1]

Both: f_maps 64, 2 levels (first conv 2 -> 32 / 3 -> 32), two samples, the hemisphere head set, weights drawn by
tests/twostage_weights.py and stored as hashes.  Per run: the loss dictionary, the full gradients of the first layer's
three parameters and of the heads, N_GRAD seeded entries plus the L2 norm and the maximum of every other parameter's
gradient.  Every file stays under 1 MiB.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import  # noqa: E402

R = ref_import.setup()
import torch  # noqa: E402

import twostage_weights as TW  # noqa: E402

torch.set_num_threads(8)
N_GRAD = 512
STEM = "backbone.encoders.0.basic_module.SingleConv1."


def is_full(name):
    return name.startswith(STEM) or name.startswith("head.")


def build(condition):
    import utils.misc as um
    import Trainer.models as TM
    gen_args = um.preprocess_cfg([R + "/cfgs/generator/default.yaml", R + "/cfgs/generator/test/demo_test.yaml"],
                                 cfg_dir="")
    train_args = um.preprocess_cfg([R + "/cfgs/trainer/default_train.yaml", R + "/cfgs/trainer/default_val.yaml",
                                    R + "/cfgs/trainer/test/demo_test.yaml"], cfg_dir="")
    train_args.f_maps = 64
    train_args.num_levels = 2
    train_args.task_f_maps = [64]
    train_args.condition = condition
    gen_args.task.pathology = True                       # the head's exclude_keys needs the key present
    gen_args.generator.left_hemis_only = True
    return TM.build_conditioned_model(gen_args, train_args, "cpu")


def condition(samples, target, cond_name):
    """What Trainer/engine.py:102-112 does to the samples, and the condition channels it hands to the model."""
    names = cond_name.split("+")
    cond = []
    for s in samples:
        chans = []
        if "mask" in names:
            s["input"] *= 1 - target["pathology"]
            chans.append(target["pathology"].to(s["input"].dtype))
        if "flip" in names:
            s["input_flip"] = torch.flip(s["input"], dims=[2])
            chans.insert(0, s["input_flip"])
        cond.append(torch.concat(chans, dim=1))
    return cond


def iteration(model, processors, criterion, samples, target, cond_name):
    model.zero_grad()
    cond = condition(samples, target, cond_name)
    outputs, _ = model(samples, cond=cond)
    for p in processors:
        outputs = p(outputs, target, "synth")
    loss_dict = criterion(outputs, target, samples)
    wd = criterion.weight_dict
    total = sum(loss_dict[k] * wd[k] for k in loss_dict.keys() if k in wd)
    total.backward()
    return loss_dict, total, cond


def record(d, prefix, model, loss_dict, total, idx):
    for k, v in loss_dict.items():
        d["%sloss/%s" % (prefix, k)] = np.float64(float(v.detach()))
    d[prefix + "loss_total"] = np.float64(float(total.detach()))
    for n, p in model.named_parameters():
        g = p.grad.detach().double()
        if is_full(n):
            d["%sgrad/%s" % (prefix, n)] = g.numpy().copy()
        else:
            d["%sgrad_at/%s" % (prefix, n)] = g.reshape(-1)[idx[n]].numpy().copy()
            d["%sgrad_l2/%s" % (prefix, n)] = np.float64(float(g.norm()))
            d["%sgrad_max/%s" % (prefix, n)] = np.float64(float(g.abs().max()))


def case(stem, cond_name, dims, soft, seed):
    print(stem)
    torch.manual_seed(seed)
    gen_args, train_args, model, processors, criterion, _ = build(cond_name)
    sd = model.state_dict()
    new = TW.draw_state_dict(list(sd.keys()), [tuple(v.shape) for v in sd.values()], seed + 1)
    model.load_state_dict(new)
    model.train()
    criterion.train()
    wd = criterion.weight_dict
    for i, k in enumerate(sorted(wd)):                   # unequal loss weights so that a swapped weight shows
        wd[k] = float(0.5 + 0.25 * (i % 5))
    d = {"cfg": np.array([64, 2, 8]), "condition": np.array(cond_name), "dims": np.array(dims)}
    d["model/names"] = np.array(list(new.keys()))
    d["model/shapes"] = np.array([",".join(str(s) for s in v.shape) for v in new.values()])
    d["model/sha256"] = np.array([TW.sha(v) for v in new.values()])
    d["model/seed"] = np.array(seed + 1)

    g = torch.Generator().manual_seed(seed + 2)
    n_seg, n_samples = gen_args.n_labels, 2
    samples = []
    for i in range(n_samples):
        s = {"input": torch.rand((1, 1) + dims, generator=g),
             "bias_field_log": 0.3 * torch.randn((1, 1) + dims, generator=g),
             "high_res_residual": 0.2 * torch.randn((1, 1) + dims, generator=g)}
        samples.append(s)
        for k, v in s.items():
            d["sample%d/%s" % (i, k)] = v.numpy().copy()
    lab = torch.randint(0, n_seg, (1,) + dims, generator=g)
    d["target_label"] = lab.numpy().astype(np.uint8)      # target['segmentation'] = its one-hot
    target = {"segmentation": torch.nn.functional.one_hot(lab, n_seg).permute(0, 4, 1, 2, 3).float().contiguous()}
    for k in ("T1", "T2", "FLAIR", "CT"):
        target[k] = torch.rand((1, 1) + dims, generator=g)
    target["distance"] = torch.clamp(2.5 * torch.randn((1, 2) + dims, generator=g), -3, 3)
    target["registration"] = torch.randn((1, 3) + dims, generator=g)
    p = torch.rand((1, 1) + dims, generator=g)
    target["pathology"] = p if soft else (p > 0.7).float()
    for k, v in target.items():
        if k != "segmentation":
            d["target/" + k] = v.numpy()

    idx = {}
    for n, prm in model.named_parameters():
        if not is_full(n):
            idx[n] = torch.randperm(prm.numel(), generator=g)[:N_GRAD].sort().values
            d["grad_idx/" + n] = idx[n].numpy().astype(np.int64)

    def copies(dtype):
        return ([{k: v.clone().to(dtype) for k, v in s.items()} for s in samples],
                {k: v.clone().to(dtype) for k, v in target.items()})

    s32, t32 = copies(torch.float32)
    ld32, tot32, cond32 = iteration(model, processors, criterion, s32, t32, cond_name)
    record(d, "ref32/", model, ld32, tot32, idx)
    for i, c in enumerate(cond32):                         # what the device path must reproduce bit for bit
        d["cond%d" % i] = c.numpy().copy()
        d["masked%d" % i] = s32[i]["input"].numpy().copy()
    model.double()
    criterion.weights_ce = criterion.weights_ce.double()
    criterion.weights_dice = criterion.weights_dice.double()
    s64, t64 = copies(torch.float64)
    ld64, tot64, _ = iteration(model, processors, criterion, s64, t64, cond_name)
    record(d, "ref64/", model, ld64, tot64, idx)

    d["loss_names"] = np.array(list(criterion.loss_names))
    d["loss_weight_names"] = np.array(sorted(wd))
    d["loss_weights"] = np.array([wd[k] for k in sorted(wd)], dtype=np.float64)
    d["param_names"] = np.array([n for n, _ in model.named_parameters()])
    d["hyper"] = np.array([float(gen_args.generator.all_samples), float(gen_args.max_surf_distance)], dtype=np.float64)
    d["bias_field_log_type"] = np.array(str(train_args.losses.bias_field_log_type))
    d["weights_ce"] = criterion.weights_ce.reshape(-1).numpy()
    path = os.path.join(HERE, stem + ".npz")
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    print("  %s: %d bytes, %d parameters, losses %s" % (stem, size, len(d["param_names"]),
                                                        {k: round(float(v), 5) for k, v in ld64.items()}))
    worst = max(abs(float(ld32[k]) - float(ld64[k])) / max(abs(float(ld64[k])), 1e-3) for k in ld64)
    print("  fp32 losses within %.1e of float64" % worst)
    assert size < 1 << 20, "a committed file must stay under 1 MiB"


if __name__ == "__main__":
    case("train_cond_mask", "mask", (8, 12, 40), False, 31)
    case("train_cond_maskflip", "mask+flip", (7, 10, 36), True, 41)
