"""Generate the fixture of one JOINT training iteration of the two-stage model by RUNNING the reference's own pieces.

Run in the build container only (needs the reference tree, about a minute on 8 threads):
    python tests/golden/make_golden_twostage_train.py

The reference's build_inpaint_model raises a TypeError (Trainer/models/__init__.py:448), so both models, their processors
and the criterion are assembled from the functions it calls, as tests/golden/make_golden_twostage.py does; one iteration
follows train_one_epoch_twostage, Trainer/engine.py:230-253 -- stage 0, PatholProcessor, input_masked, cond =
target['pathology'], stage 1, processors, merge_list_of_dict, criterion, weighted sum -- then backward(), without autocast /
GradScaler.  It runs in float32 (keys ref32/...), with .double() (the truth, ref64/...), and a third time in float64 with
the coupling cut -- input_masked from p.detach() -- for stage 0's fully stored gradients (ref64/grad_cut/...).

  train_twostage.npz   f_maps 64, 2 levels, two samples, (8,12,40), the hemisphere head set plus pathology, a binary
                       target mask, unequal loss weights, weights drawn by tests/twostage_weights.py and stored as hashes

Per run: the loss dictionary, p and input_masked of each sample, the full gradients of both stems, of stage 0's head and of
stage 1's heads, N_GRAD seeded entries plus the L2 norm and the maximum of every other parameter's gradient.  Parameter
names carry the model: pathol/<name>, task/<name>.

The script asserts that cutting the coupling moves stage 0's stem weight and head weight gradients by at least MARGIN of
their maximum (25 x the gradient tolerance of the GPU test): a build that drops the gradient through the mask then fails
that test.  The stage-1 loss weights are multiplied by 4 until it holds; the gain used is stored (task_gain).
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
N_GRAD = 256
MARGIN = 0.05
STEM = "backbone.encoders.0.basic_module.SingleConv1."
MARGIN_KEYS = ("pathol/" + STEM + "conv.weight", "pathol/head.final_conv_pathology.weight")
MODELS = ("pathol", "task")


def is_full(name):
    name = name.split("/", 1)[1]
    return name.startswith(STEM) or name.startswith("head.")


def build():
    """build_inpaint_model's own steps (make_golden_twostage.py:62-79) plus its criterion."""
    import utils.misc as um
    from Trainer.models import process_args, get_criterion
    from Trainer.models.backbone import build_backbone
    from Trainer.models.head import get_head
    from Trainer.models.joiner import get_joiner, get_processors
    gen_args = um.preprocess_cfg([R + "/cfgs/generator/default.yaml", R + "/cfgs/generator/test/demo_test.yaml"], cfg_dir="")
    train_args = um.preprocess_cfg([R + "/cfgs/trainer/default_train.yaml", R + "/cfgs/trainer/default_val.yaml",
                                    R + "/cfgs/trainer/test/demo_test.yaml"], cfg_dir="")
    train_args.f_maps = 64
    train_args.num_levels = 2
    train_args.task_f_maps = [64]
    train_args.backbone = "unet3d+unet3d"
    train_args.condition = None
    gen_args.task.pathology = True
    gen_args.generator.left_hemis_only = True
    gen_args, train_args = process_args(gen_args, train_args, task=gen_args.task)
    names = train_args.backbone.split("+")
    pb = build_backbone(train_args, names[0], num_cond=0)
    ph = get_head(train_args, train_args.task_f_maps, train_args.out_channels, True, -1, stage=0)
    pm = get_joiner(gen_args.tasks, pb, ph, "cpu", postfix="_pathol")
    pp = get_processors(gen_args, train_args, ["pathology"], "cpu")
    tb = build_backbone(train_args, names[1], num_cond=1)
    th = get_head(train_args, train_args.task_f_maps, train_args.out_channels, True, -1, stage=1)
    tm = get_joiner(gen_args.tasks, tb, th, "cpu", postfix="_task")
    tp = get_processors(gen_args, train_args, gen_args.tasks, "cpu", exclude_keys=["pathology"])
    criterion = get_criterion(gen_args, train_args, gen_args.tasks, "cpu")
    return gen_args, train_args, pm, tm, pp, tp, criterion


def iteration(pm, tm, pp, tp, criterion, samples, target, cut=False):
    """Trainer/engine.py:230-253 (condition None: no flip), then backward.  cut: input_masked from p.detach()."""
    import utils.misc as um
    pm.zero_grad()
    tm.zero_grad()
    outputs_pathol, _ = pm(samples)
    for processor in pp:
        outputs_pathol = processor(outputs_pathol, target, "synth")
    cond = []
    for i in range(len(samples)):
        p = outputs_pathol[i]["pathology"]
        samples[i]["input_masked"] = samples[i]["input"] * (1 - (p.detach() if cut else p))
        cond.append(target["pathology"].to(samples[0]["input"].dtype))
    outputs_task, _ = tm(samples, input_name="input_masked", cond=cond)
    for processor in tp:
        outputs_task = processor(outputs_task, target, "synth")
    outputs = um.merge_list_of_dict(outputs_task, outputs_pathol)
    loss_dict = criterion(outputs, target, samples)
    wd = criterion.weight_dict
    total = sum(loss_dict[k] * wd[k] for k in loss_dict.keys() if k in wd)
    total.backward()
    return loss_dict, total, [o["pathology"].detach() for o in outputs_pathol]


def named(pm, tm):
    for pre, m in zip(MODELS, (pm, tm)):
        for n, p in m.named_parameters():
            yield pre + "/" + n, p


def record(d, prefix, pm, tm, loss_dict, total, idx):
    for k, v in loss_dict.items():
        d["%sloss/%s" % (prefix, k)] = np.float64(float(v.detach()))
    d[prefix + "loss_total"] = np.float64(float(total.detach()))
    for n, p in named(pm, tm):
        g = p.grad.detach().double()
        if is_full(n):
            d["%sgrad/%s" % (prefix, n)] = g.numpy().copy()
        else:
            d["%sgrad_at/%s" % (prefix, n)] = g.reshape(-1)[idx[n]].numpy().copy()
            d["%sgrad_l2/%s" % (prefix, n)] = np.float64(float(g.norm()))
            d["%sgrad_max/%s" % (prefix, n)] = np.float64(float(g.abs().max()))


def case(stem, dims, seed):
    print(stem)
    torch.manual_seed(seed)
    gen_args, train_args, pm, tm, pp, tp, criterion = build()
    d = {"cfg": np.array([64, 2, 8]), "dims": np.array(dims)}
    for prefix, m, s in (("pathol", pm, seed + 1), ("task", tm, seed + 2)):
        sd = m.state_dict()
        new = TW.draw_state_dict(list(sd.keys()), [tuple(v.shape) for v in sd.values()], s)
        m.load_state_dict(new)
        d[prefix + "/names"] = np.array(list(new.keys()))
        d[prefix + "/shapes"] = np.array([",".join(str(v_) for v_ in v.shape) for v in new.values()])
        d[prefix + "/sha256"] = np.array([TW.sha(v) for v in new.values()])
        d[prefix + "/seed"] = np.array(s)
        m.train()
    criterion.train()
    wd = criterion.weight_dict
    base = {}
    for i, k in enumerate(sorted(wd)):                   # unequal loss weights so that a swapped weight shows
        base[k] = float(0.5 + 0.25 * (i % 5))

    g = torch.Generator().manual_seed(seed + 3)
    n_seg = gen_args.n_labels
    samples = []
    for i in range(2):
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
    target["pathology"] = (torch.rand((1, 1) + dims, generator=g) > 0.7).float()
    for k, v in target.items():
        if k != "segmentation":
            d["target/" + k] = v.numpy()

    idx = {}
    for n, prm in named(pm, tm):
        if not is_full(n):
            idx[n] = torch.randperm(prm.numel(), generator=g)[:N_GRAD].sort().values
            d["grad_idx/" + n] = idx[n].numpy().astype(np.int32)

    def copies(dtype):
        return ([{k: v.clone().to(dtype) for k, v in s.items()} for s in samples],
                {k: v.clone().to(dtype) for k, v in target.items()})

    def grads_of(keys):
        return {n: p.grad.detach().double().clone() for n, p in named(pm, tm) if n in keys}

    pm.double(), tm.double()
    criterion.weights_ce = criterion.weights_ce.double()
    criterion.weights_dice = criterion.weights_dice.double()
    gain = 1.0
    while True:                                          # raise the stage-1 loss weights until the coupling shows
        for k in wd:
            wd[k] = base[k] * (1.0 if "pathol" in k else gain)
        s64, t64 = copies(torch.float64)
        ld64, tot64, p64 = iteration(pm, tm, pp, tp, criterion, s64, t64)
        coupled = grads_of(MARGIN_KEYS)
        sc, tc = copies(torch.float64)
        iteration(pm, tm, pp, tp, criterion, sc, tc, cut=True)
        cut = grads_of(MARGIN_KEYS)
        margin = {n: float((coupled[n] - cut[n]).abs().max() / coupled[n].abs().max()) for n in MARGIN_KEYS}
        print("  stage-1 weight gain %g: coupled against cut %s" % (gain, {n: "%.3f" % v for n, v in margin.items()}))
        if min(margin.values()) >= MARGIN:
            break
        gain *= 4.0
        assert gain <= 4096.0, "the coupling does not show: raise the image contrast"
    for n, p in named(pm, tm):                           # the cut run is the last backward: store stage 0's full gradients
        if n.startswith("pathol/") and is_full(n):
            d["ref64/grad_cut/" + n] = p.grad.detach().double().numpy().copy()
    ld64, tot64, p64 = iteration(pm, tm, pp, tp, criterion, s64, t64)
    record(d, "ref64/", pm, tm, ld64, tot64, idx)
    for i in range(2):
        d["ref64/p%d" % i] = p64[i].numpy().copy()
        d["ref64/input_masked%d" % i] = s64[i]["input_masked"].detach().numpy().copy()
    pm.float(), tm.float()
    criterion.weights_ce = criterion.weights_ce.float()
    criterion.weights_dice = criterion.weights_dice.float()
    s32, t32 = copies(torch.float32)
    ld32, tot32, p32 = iteration(pm, tm, pp, tp, criterion, s32, t32)
    record(d, "ref32/", pm, tm, ld32, tot32, idx)
    for i in range(2):
        d["ref32/p%d" % i] = p32[i].numpy().copy()
        d["ref32/input_masked%d" % i] = s32[i]["input_masked"].detach().numpy().copy()

    d["task_gain"] = np.float64(gain)
    d["margin"] = np.array([margin[n] for n in MARGIN_KEYS], dtype=np.float64)
    d["margin_keys"] = np.array(MARGIN_KEYS)
    d["loss_names"] = np.array(list(criterion.loss_names))
    d["loss_weight_names"] = np.array(sorted(wd))
    d["loss_weights"] = np.array([wd[k] for k in sorted(wd)], dtype=np.float64)
    d["param_names"] = np.array([n for n, _ in named(pm, tm)])
    d["hyper"] = np.array([float(gen_args.generator.all_samples), float(gen_args.max_surf_distance)], dtype=np.float64)
    d["bias_field_log_type"] = np.array(str(train_args.losses.bias_field_log_type))
    d["weights_ce"] = criterion.weights_ce.reshape(-1).numpy()
    path = os.path.join(HERE, stem + ".npz")
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    print("  %s: %d bytes, %d parameters, losses %s" % (stem, size, len(d["param_names"]),
                                                        {k: round(float(v.detach()), 5) for k, v in ld64.items()}))
    print("  p spans %.3g .. %.3g" % (float(p64[0].min()), float(p64[0].max())))
    assert size < 1 << 20, "a committed file must stay under 1 MiB"


if __name__ == "__main__":
    case("train_twostage", (8, 12, 40), 51)
