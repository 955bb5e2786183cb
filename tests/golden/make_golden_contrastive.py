"""Generate golden vectors for the head-less contrastive pre-training mode by RUNNING the reference.

Run in the build container only (needs the reference tree):
    python tests/golden/make_golden_contrastive.py
Writes tests/golden/train_contrastive.npz: the reference's build_model with tasks {T1, contrastive} (T1 must be ignored:
out_channels stays empty), f_maps 8, 3 levels, size 48^3, all_samples = 2, run in float64 with temperatures
(0.1, 0.1, 0.1) and weight 0.75: the state dict, the inputs, feat[-1] of both samples after ContrastiveProcessor at every
fourth voxel per axis with the reference's loss of each of those voxels (loss_feat_contrastive called on that voxel
alone: the mean over one voxel), the loss of the whole volume, every parameter gradient of the weighted total, the
hyper-parameters of the torch.optim.AdamW step the test repeats, the processor class names and the signatures of
ContrastiveProcessor.forward and SetCriterion.loss_feat_contrastive.  The GroupNorm affine parameters are perturbed as in
the other generators, plus a bias of about 3 in front of the last convolution: it keeps the feature vectors away from zero,
where the loss's gradient (~ 1 / |feature|) would hang on the sign of single LeakyReLU inputs (see main()).
Inputs are stored as bytes (x = q / 255 in float32, constant on 2^3 blocks); the second is the first plus a small
perturbation, so that the two feature maps are related as two augmentations of one case are.
"""
import inspect
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_infer as M  # noqa: E402  (sets up the reference import harness)

R = M.R
import torch  # noqa: E402

from make_golden_age import blocky  # noqa: E402

STRIDE = 4
# see main(): keeps the feature norms away from zero (1.0 leaves a worst case of 8e-3 below, 3.0 one of 7e-4)
LAST_BIAS = 3.0
KINK = 5e-6
SLOPE = 0.01                                              # nn.LeakyReLU(negative_slope=0.01) of the 'l' in layer_order


def main():
    import utils.misc as um
    from Trainer.models import build_model
    from Trainer.models.joiner import ContrastiveProcessor
    gen_args = um.preprocess_cfg([R + "/cfgs/generator/default.yaml", R + "/cfgs/generator/test/demo_test.yaml"],
                                 cfg_dir="")
    train_args = um.preprocess_cfg([R + "/cfgs/trainer/default_train.yaml", R + "/cfgs/trainer/default_val.yaml",
                                    R + "/cfgs/trainer/test/demo_test.yaml"], cfg_dir="")
    f_maps, levels, size = 8, 3, 48
    temps = (0.1, 0.1, 0.1)
    weight = 0.75
    train_args.f_maps = f_maps
    train_args.num_levels = levels
    train_args.task_f_maps = [f_maps]
    train_args.contrastive_temperatures = type(train_args.weights)()
    train_args.contrastive_temperatures.alpha, train_args.contrastive_temperatures.beta, \
        train_args.contrastive_temperatures.gamma = temps
    for k in list(vars(gen_args.task).keys()):
        setattr(gen_args.task, k, False)
    gen_args.task.T1 = True
    gen_args.task.contrastive = True
    gen_args.generator.size = [size, size, size]
    gen_args.generator.all_samples = 2
    torch.manual_seed(41)
    gen_args, train_args, model, processors, criterion, post = build_model(gen_args, train_args, "cpu")
    assert dict(train_args.out_channels) == {}, train_args.out_channels
    assert type(criterion).__name__ == "SetCriterion" and list(criterion.loss_names) == ["contrastive"]
    assert not [n for n, _ in model.named_parameters() if n.startswith("head.")]
    g = torch.Generator().manual_seed(42)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if "groupnorm.weight" in k:
                v.copy_(1.0 + 0.4 * (torch.rand(v.shape, generator=g) - 0.5))
            if "groupnorm.bias" in k:
                v.copy_(0.4 * (torch.rand(v.shape, generator=g) - 0.5))
        # The loss reads the DIRECTION of a feature vector, so its gradient grows like 1 / |raw feature|; the raw feature is
        # a LeakyReLU output, and where its norm is tiny every channel sits at the activation's kink, where the sign of one
        # channel -- which a float32 forward pass cannot pin -- decides whether that voxel's (large) gradient passes or is
        # multiplied by the slope.  With the perturbation above alone one such voxel carried 6 % of the last layer's weight
        # gradient.  A larger GroupNorm bias in front of the last convolution acts as a bias of its outputs (the convolution
        # has none) and keeps the feature norms away from zero; main() checks the result below (kink_risk).
        last = [k for k in model.state_dict() if k.endswith("SingleConv2.groupnorm.bias")][-1]
        v = model.state_dict()[last]
        v.copy_(LAST_BIAS * (1.0 + 0.4 * (torch.rand(v.shape, generator=g) - 0.5)))
    model.double()
    model.train()
    raw, gn_out = [], []
    last_conv = model.backbone.decoders[-1].basic_module.SingleConv2

    def keep_raw(mod, inp, out):
        out.retain_grad()
        raw.append(out)
    last_conv.register_forward_hook(keep_raw)
    last_conv.groupnorm.register_forward_hook(lambda mod, inp, out: gn_out.append(float(out.detach().abs().max())))
    criterion.train()
    wd = criterion.weight_dict
    wd["loss_contrastive"] = weight

    dims = (size, size, size)
    d = {}
    q0 = blocky(g, dims)
    noise = blocky(g, dims).to(torch.int32) - 128
    q1 = (q0.to(torch.int32) + noise // 6).clamp(0, 255).to(torch.uint8)
    samples = []
    for i, q in enumerate((q0, q1)):
        d["xq%d" % i] = q.numpy()
        x = torch.from_numpy(q.numpy().astype(np.float32) / np.float32(255))
        samples.append({"input": x.double()})
    sd32 = {k: v.detach().float().clone() for k, v in model.state_dict().items()}

    lr, wdecay = 1e-3, 0.04
    opt = torch.optim.AdamW([{"params": [p_ for p_ in model.parameters() if p_.requires_grad]}])
    for gr in opt.param_groups:
        gr["lr"] = lr
        gr["weight_decay"] = wdecay
    opt.zero_grad()
    outputs, _ = model(samples)
    assert list(outputs[0].keys()) == ["feat"]
    for pr in processors:
        outputs = pr(outputs, None, "synth")
    sub = [o["feat"][-1].detach()[..., ::STRIDE, ::STRIDE, ::STRIDE] for o in outputs]
    for i, f in enumerate(sub):
        d["feat_%d" % i] = f.numpy()                                # (1, C, n, n, n) float64
    n = sub[0].shape[-1]
    vox = np.zeros((n, n, n), dtype=np.float64)
    with torch.no_grad():
        for a in range(n):
            for b in range(n):
                for c in range(n):
                    one = [{"feat": [f[..., a:a + 1, b:b + 1, c:c + 1]]} for f in sub]
                    vox[a, b, c] = float(criterion.loss_feat_contrastive(one)["loss_contrastive"])
    d["voxel_loss"] = vox
    loss_dict = criterion(outputs, None, samples)
    losses = sum(loss_dict[k] * wd[k] for k in loss_dict.keys() if k in wd)
    losses.backward()
    # conditioning of the fixture against a float32 forward pass: the share of the last layer's weight gradient that the
    # elements within KINK of the activation's kink could move if every one of them changed sign (KINK = twice the largest
    # error the split-fp16 forward pass shows at this size, 2.5e-6 of the largest feature)
    last_w = model.state_dict()[last.replace("groupnorm.bias", "conv.weight")]
    dw_max = float(dict(model.named_parameters())[last.replace("groupnorm.bias", "conv.weight")].grad.abs().max())
    risk = 0.0
    for r_ in raw:
        pre = torch.where(r_.detach() > 0, r_.detach(), r_.detach() / SLOPE)     # what the activation saw
        near = pre.abs() < KINK * float(r_.detach().abs().max())
        risk += float(r_.grad.abs()[near].sum()) * max(gn_out) / dw_max
        print("raw feature norm min %.3e median %.3e; |d raw| max %.3e median %.3e; elements near the kink %d" %
              (float(r_.detach().norm(dim=1).min()), float(r_.detach().norm(dim=1).median()), float(r_.grad.abs().max()),
               float(r_.grad.abs().median()), int(near.sum())))
    print("kink_risk %.3e of the last conv weight gradient (max %.3e, %s)" % (risk, dw_max, tuple(last_w.shape)))
    assert risk < 1e-3, risk                              # half of the 2e-3 the gradients are compared at
    names = [n_ for n_, _ in model.named_parameters()]
    assert all(p_.grad is not None and float(p_.grad.abs().sum()) > 0 for p_ in model.parameters())
    for n_, p_ in model.named_parameters():
        d["grad/" + n_] = p_.grad.detach().float().numpy().copy()
    for k, v in loss_dict.items():
        d["loss/" + k] = np.float64(float(v.detach()))
    d["loss_total"] = np.float64(float(losses.detach()))
    d["loss_weight_names"] = np.array(sorted(wd))
    d["loss_weights"] = np.array([wd[k] for k in sorted(wd)], dtype=np.float64)
    d["loss_names"] = np.array(list(criterion.loss_names))
    d["temperatures"] = np.array(temps, dtype=np.float64)
    d["processor_names"] = np.array([type(p_).__name__ for p_ in processors])
    d["sig_processor_forward"] = np.array(str(inspect.signature(ContrastiveProcessor.forward)))
    d["sig_loss_feat_contrastive"] = np.array(str(inspect.signature(type(criterion).loss_feat_contrastive)))
    d["tasks"] = np.array(list(gen_args.tasks))
    d["param_names"] = np.array(names)
    d["param_shapes"] = np.array([str(tuple(v.shape)) for v in sd32.values()])
    d["sd_names"] = np.array(list(sd32.keys()))
    d["hyper"] = np.array([lr, wdecay, 0.9, 0.999, 1e-8, float(gen_args.generator.all_samples)], dtype=np.float64)
    d["cfg"] = np.array([f_maps, levels, 8, size, STRIDE])
    for k, v in sd32.items():
        d["sd/" + k] = v.numpy()
    out = os.path.join(HERE, "train_contrastive.npz")
    np.savez_compressed(out, **d)
    print("train_contrastive:", {k: float(v.detach()) for k, v in loss_dict.items()}, "mean of the stored voxels", vox.mean())
    print("params", len(names), "bytes", os.path.getsize(out))


if __name__ == "__main__":
    main()
