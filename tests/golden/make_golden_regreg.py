"""Generate golden vectors for the registration regularisers by RUNNING the reference.

Run in the build container only (needs the reference tree):
    python tests/golden/make_golden_regreg.py
Writes tests/golden/regreg.npz:
  * unit/<case>/...: SmoothnessLoss('l2') and HessianLoss('l2') of Trainer/models/losses.py on two odd-shaped
    (1, 3, D, H, W) fields, in float64 on float32-rounded inputs, with their autograd gradients.  Case "slab" has constant
    slabs at the boundary (the last two x slices, the first two y rows, the last two z slices), where the zeroed last
    index and the adjoints' edge terms meet.
  * everything else: one training iteration in the form of train_step.npz (make_golden_train.py) for a net whose only
    task is registration, with losses.registration_grad / _smooth / _hessian switched on: the reference's build_model,
    processors, SetMultiCriterion, backward, clip_gradients and one torch.optim.AdamW step, model in float64.  Gradients
    are stored in float32, the AdamW moves (delta/) for the head only.  The registration head is scaled so that the
    Hessian term's gradient is of the same order as the others' (det^2 grows with the sixth power of the head).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_infer as M  # noqa: E402  (sets up the reference import harness)

R = M.R
import torch  # noqa: E402


def unit_cases(d):
    from Trainer.models.losses import HessianLoss, SmoothnessLoss
    g = torch.Generator().manual_seed(41)
    rand = torch.randn((1, 3, 13, 17, 19), generator=g)
    slab = 0.7 * torch.randn((1, 3, 11, 9, 14), generator=g) + 0.3
    slab[..., -2:] = 0.25                                   # x: last two slices constant
    slab[..., :2, :] = -0.5                                 # y: first two rows constant
    slab[:, :, -2:] = 1.5                                   # z: last two slices constant
    for name, u32 in (("rand", rand), ("slab", slab)):
        u32 = u32.float()
        d["unit/%s/u" % name] = u32.numpy()
        for lname, mod in (("smooth", SmoothnessLoss("l2")), ("hessian", HessianLoss("l2"))):
            u = u32.double().requires_grad_(True)
            v = mod(u)
            v.backward()
            d["unit/%s/%s" % (name, lname)] = np.float64(float(v.detach()))
            d["unit/%s/%s_grad" % (name, lname)] = u.grad.float().numpy().copy()     # fp32: the file stays small
            print(name, lname, float(v.detach()), float(u.grad.abs().max()))


def train_case(d):
    import utils.misc as um
    from Trainer.models import build_model
    gen_args = um.preprocess_cfg([R + "/cfgs/generator/default.yaml", R + "/cfgs/generator/test/demo_test.yaml"],
                                 cfg_dir="")
    train_args = um.preprocess_cfg([R + "/cfgs/trainer/default_train.yaml", R + "/cfgs/trainer/default_val.yaml",
                                    R + "/cfgs/trainer/test/demo_test.yaml"], cfg_dir="")
    f_maps, levels = 8, 3
    train_args.f_maps = f_maps
    train_args.num_levels = levels
    train_args.task_f_maps = [f_maps]
    for k in list(vars(gen_args.task).keys()):
        setattr(gen_args.task, k, False)
    gen_args.task.registration = True
    train_args.losses.registration_grad = True
    train_args.losses.registration_smooth = True
    train_args.losses.registration_hessian = True
    torch.manual_seed(42)
    gen_args, train_args, model, processors, criterion, post = build_model(gen_args, train_args, "cpu")
    assert list(train_args.out_channels.keys()) == ["registration"], train_args.out_channels
    assert list(criterion.loss_names) == ["registration", "registration_grad", "registration_smooth",
                                          "registration_hessian"], criterion.loss_names
    g = torch.Generator().manual_seed(43)
    reg_scale = 0.5
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if "groupnorm.weight" in k:
                v.copy_(1.0 + 0.4 * (torch.rand(v.shape, generator=g) - 0.5))
            if "groupnorm.bias" in k:
                v.copy_(0.4 * (torch.rand(v.shape, generator=g) - 0.5))
        model.head.final_conv_registration.weight.mul_(reg_scale)
    sd32 = {k: v.detach().float().clone() for k, v in model.state_dict().items()}
    model.double()
    model.train()
    criterion.train()
    wd = criterion.weight_dict
    for i, k in enumerate(sorted(wd)):
        wd[k] = float(0.5 + 0.25 * (i % 5))

    dims = (12, 16, 10)
    n_samples = 2
    samples = []
    for i in range(n_samples):
        x = torch.rand((1, 1) + dims, generator=g)
        samples.append({"input": x.double()})
        d["x%d" % i] = x.numpy()
    target = {"registration": torch.randn((1, 3) + dims, generator=g)}
    for k, v in target.items():
        d["target/" + k] = v.numpy()
    target64 = {k: v.double() for k, v in target.items()}

    lr, wdecay, clip = 1e-3, 0.04, 0.05
    opt = torch.optim.AdamW([{"params": [p for p in model.parameters() if p.requires_grad]}])
    for gr in opt.param_groups:
        gr["lr"] = lr
        gr["weight_decay"] = wdecay
    opt.zero_grad()
    outputs, _ = model(samples)
    for p in processors:
        outputs = p(outputs, target64, "synth")
    loss_dict = criterion(outputs, target64, samples)
    losses = sum(loss_dict[k] * wd[k] for k in loss_dict.keys() if k in wd)
    losses.backward()
    names = [n for n, _ in model.named_parameters()]
    # gradients and AdamW moves in float32 (the file stays under 1 MiB; both are compared at fp32-level tolerances); the
    # clipped gradients follow from grad/ and clip_norms
    for n, p in model.named_parameters():
        d["grad/" + n] = p.grad.detach().float().numpy().copy()
    norms = um.clip_gradients(model, clip)
    d["clip_norms"] = np.array(norms, dtype=np.float64)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt.step()
    for n, p in model.named_parameters():
        if n.startswith("head."):        # the backbone's moves follow from sd/ and grad/ (the oracle's AdamW in the test)
            d["delta/" + n] = (p.detach() - before[n]).float().numpy().copy()
    for k, v in loss_dict.items():
        d["loss/" + k] = np.float64(float(v.detach()))
    d["loss_total"] = np.float64(float(losses.detach()))
    d["loss_weight_names"] = np.array(sorted(wd))
    d["loss_weights"] = np.array([wd[k] for k in sorted(wd)], dtype=np.float64)
    d["loss_names"] = np.array(list(criterion.loss_names))
    d["param_names"] = np.array(names)
    d["hyper"] = np.array([lr, wdecay, clip, 0.9, 0.999, 1e-8, float(gen_args.generator.all_samples),
                           float(gen_args.max_surf_distance)], dtype=np.float64)
    d["bias_field_log_type"] = np.array(str(train_args.losses.bias_field_log_type))
    d["weights_ce"] = np.ones(1, dtype=np.float32)
    d["cfg"] = np.array([f_maps, levels, 8])
    for k, v in sd32.items():
        d["sd/" + k] = v.numpy()
    # how much of the registration head's gradient each regulariser carries (printed: the scale above is chosen by it)
    print("train:", {k: float(v.detach()) for k, v in loss_dict.items()}, "total", float(losses.detach()))
    for lname in ("registration", "registration_grad", "registration_smooth", "registration_hessian"):
        model.zero_grad()
        outputs, _ = model(samples)
        v = criterion(outputs, target64, samples)["loss_" + lname] * wd["loss_" + lname]
        v.backward()
        print("  |d %s / d head.weight| = %.3e" % (lname, float(model.head.final_conv_registration.weight.grad.norm())))


def main():
    d = {}
    unit_cases(d)
    train_case(d)
    path = os.path.join(HERE, "regreg.npz")
    np.savez_compressed(path, **d)
    print("bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
