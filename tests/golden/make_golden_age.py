"""Generate golden vectors for the pooled scalar (brain-age) head by RUNNING the reference.

Run in the build container only (needs the reference tree):
    python tests/golden/make_golden_age.py
Writes tests/golden/train_age.npz: the reference's build_model with tasks {T1, age}, f_maps 8, 3 levels, size 48^3
(final_linear1_age takes 4*48//16*48//16*48//16 = 108 features), all_samples = 2, run in float64: the state dict, the
inputs, the per-sample age after AgeProcessor, the dense T1 outputs (every third voxel per axis), the loss dictionary of SetMultiCriterion, every
parameter gradient of the weighted total and each head parameter's move in one torch.optim.AdamW step (no clipping).
The age target and a shift of final_linear3_age.bias are chosen from a first forward so that one sample has |p| > age,
the other |p| < age, and one raw p is negative: both sign terms of loss_age's gradient are exercised.
Inputs are stored as bytes (x = q / 255 in float32, constant on 2^3 blocks) to keep the file small.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_infer as M  # noqa: E402  (sets up the reference import harness)

R = M.R
import torch  # noqa: E402


def blocky(g, dims, k=2):
    """Random bytes on a grid k times coarser, each value repeated over a k^3 block (compresses well)."""
    q = (torch.rand((1, 1) + tuple(n // k for n in dims), generator=g) * 255).round().to(torch.uint8)
    for ax in (2, 3, 4):
        q = q.repeat_interleave(k, dim=ax)
    return q


def main():
    import utils.misc as um
    from Trainer.models import build_model
    gen_args = um.preprocess_cfg([R + "/cfgs/generator/default.yaml", R + "/cfgs/generator/test/demo_test.yaml"],
                                 cfg_dir="")
    train_args = um.preprocess_cfg([R + "/cfgs/trainer/default_train.yaml", R + "/cfgs/trainer/default_val.yaml",
                                    R + "/cfgs/trainer/test/demo_test.yaml"], cfg_dir="")
    f_maps, levels, size = 8, 3, 48
    train_args.f_maps = f_maps
    train_args.num_levels = levels
    train_args.task_f_maps = [f_maps]
    for k in list(vars(gen_args.task).keys()):
        setattr(gen_args.task, k, False)
    gen_args.task.T1 = True
    gen_args.task.age = True
    gen_args.generator.size = [size, size, size]
    gen_args.generator.all_samples = 2
    torch.manual_seed(31)
    gen_args, train_args, model, processors, criterion, post = build_model(gen_args, train_args, "cpu")
    assert list(train_args.out_channels.keys()) == ["T1", "age"], train_args.out_channels
    g = torch.Generator().manual_seed(32)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if "groupnorm.weight" in k:
                v.copy_(1.0 + 0.4 * (torch.rand(v.shape, generator=g) - 0.5))
            if "groupnorm.bias" in k:
                v.copy_(0.4 * (torch.rand(v.shape, generator=g) - 0.5))
    model.double()
    model.train()
    criterion.train()
    wd = criterion.weight_dict
    for i, k in enumerate(sorted(wd)):
        wd[k] = float(0.5 + 0.25 * (i % 5))

    dims = (size, size, size)
    n_samples = 2
    d = {}
    samples = []
    for i in range(n_samples):
        q = blocky(g, dims)
        if i == 1:                                            # a different-looking second sample: brighter half volume
            q[..., : size // 2, :, :] = (q[..., : size // 2, :, :].float() * 0.3).round().to(torch.uint8)
        d["xq%d" % i] = q.numpy()
        x = torch.from_numpy(q.numpy().astype(np.float32) / np.float32(255))
        samples.append({"input": x.double()})
    tq = blocky(g, dims)
    d["target_T1q"] = tq.numpy()
    t1 = torch.from_numpy(tq.numpy().astype(np.float32) / np.float32(255))

    # first forward: raw ages of the two samples, then rescale / shift the last layer so that p0 and p1 lie at
    # -0.25 * s and 0.75 * s (or the mirror image) and age = 0.5 * s
    with torch.no_grad():
        outs, _ = model(samples)
        p = [float(o["age"]) for o in outs]
        s = 4.0
        lin3 = model.head.final_linear3_age
        k = s / max(abs(p[1] - p[0]), 1e-12)
        lin3.weight.mul_(k)
        lin3.bias.mul_(k)
        p = [v * k for v in p]
        lo = min(p)
        lin3.bias.add_(-lo - 0.25 * s)
        outs, _ = model(samples)
        p = [float(o["age"]) for o in outs]
    age = 0.5 * s
    assert min(p) < 0 < max(p) and min(abs(v) for v in p) < age < max(abs(v) for v in p), (p, age)
    d["raw_age"] = np.array(p, dtype=np.float64)
    sd32 = {k: v.detach().float().clone() for k, v in model.state_dict().items()}
    target64 = {"T1": t1.double(), "age": torch.tensor([age], dtype=torch.float64)}
    d["target_age"] = np.float64(age)

    lr, wdecay = 1e-3, 0.04
    opt = torch.optim.AdamW([{"params": [p_ for p_ in model.parameters() if p_.requires_grad]}])
    for gr in opt.param_groups:
        gr["lr"] = lr
        gr["weight_decay"] = wdecay
    opt.zero_grad()
    outputs, _ = model(samples)
    for i, o in enumerate(outputs):
        d["out_T1_%d" % i] = o["T1"].detach()[..., ::3, ::3, ::3].numpy()          # every third voxel per axis: size
    for pr in processors:
        outputs = pr(outputs, target64, "synth")
    for i, o in enumerate(outputs):
        d["age_%d" % i] = o["age"].detach().numpy()
    loss_dict = criterion(outputs, target64, samples)
    losses = sum(loss_dict[k] * wd[k] for k in loss_dict.keys() if k in wd)
    losses.backward()
    names = [n for n, _ in model.named_parameters()]
    # gradients and AdamW moves in float32 (the fixture stays under 1 MiB; both are compared at fp32-level tolerances)
    before = {n: p_.detach().clone() for n, p_ in model.named_parameters()}
    for n, p_ in model.named_parameters():
        d["grad/" + n] = p_.grad.detach().float().numpy().copy()
    opt.step()
    for n, p_ in model.named_parameters():
        if n.startswith("head."):        # the backbone's moves follow from sd/ and grad/ (torch.optim.AdamW in the test)
            d["delta/" + n] = (p_.detach() - before[n]).float().numpy().copy()
    for k, v in loss_dict.items():
        d["loss/" + k] = np.float64(float(v.detach()))
    d["loss_total"] = np.float64(float(losses.detach()))
    d["loss_weight_names"] = np.array(sorted(wd))
    d["loss_weights"] = np.array([wd[k] for k in sorted(wd)], dtype=np.float64)
    d["loss_names"] = np.array(list(criterion.loss_names))
    d["param_names"] = np.array(names)
    d["param_shapes"] = np.array([str(tuple(v.shape)) for v in sd32.values()])
    d["sd_names"] = np.array(list(sd32.keys()))
    d["hyper"] = np.array([lr, wdecay, 0.9, 0.999, 1e-8, float(gen_args.generator.all_samples)], dtype=np.float64)
    d["cfg"] = np.array([f_maps, levels, 8, size])
    for k, v in sd32.items():
        d["sd/" + k] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "train_age.npz"), **d)
    print("train_age:", {k: float(v) for k, v in loss_dict.items()}, "raw ages", p, "age", age)
    print("params", len(names), "bytes", os.path.getsize(os.path.join(HERE, "train_age.npz")))


if __name__ == "__main__":
    main()
