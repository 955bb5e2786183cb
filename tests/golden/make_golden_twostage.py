"""Generate the two-stage (pathology-conditioned) and conditioned-model fixtures by RUNNING the reference's own pieces.

Run in the build container only (needs the reference tree, about a minute on 8 threads):
    python tests/golden/make_golden_twostage.py

The reference's build_inpaint_model raises a TypeError (Trainer/models/__init__.py:448 calls get_processors without
gen_args), so the two models are assembled from the functions it calls -- process_args, build_backbone(..., num_cond),
get_head(..., stage=), get_joiner(..., postfix=), get_processors -- and run through the body of
evaluate_image_twostage (utils/test_utils.py:330-345).

  twostage_small.npz (+ _b)   f_maps 8, 3 levels, both state dicts stored, 24 x 20 x 36 input with a zero slab
  twostage_wide.npz (+ _b)    f_maps 64, 2 levels (stage-1 first conv 2 -> 32), weights drawn by tests/twostage_weights.py
                              and stored as hashes, 16 x 12 x 40 input
  conditioned_wide.npz (+ _b) build_conditioned_model, condition 'mask+flip' (3 input channels), f_maps 64, 2 levels
  api_signatures_twostage.json

Per case: x; p and input_masked of stage 0 in full; the label map in full; every float map at N_VOX seeded voxels, the
segmentation at every fourth of them, N_FEAT seeded entries of every feature map -- from the fp32 model and, under ref64/,
from model.double() -- and every voxel whose fp32 relative top-2 gap (t0 - t1) / t0 is below TIE.  Sampling keeps every
file under 1 MiB (the make_golden_deep.py convention).
"""
import inspect
import json
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
from make_golden_infer import load_ref_functions  # noqa: E402

torch.set_num_threads(8)

TIE = 1e-4                  # make_golden_deep.py
TIE_CAP = 1e-3              # most voxels that may be ties
N_VOX = 1024
N_FEAT = 1024


def cfgs(f_maps, levels, backbone, pathology):
    import utils.misc as um
    gen_args = um.preprocess_cfg([R + "/cfgs/generator/default.yaml", R + "/cfgs/generator/test/demo_test.yaml"],
                                 cfg_dir="")
    train_args = um.preprocess_cfg([R + "/cfgs/trainer/default_train.yaml", R + "/cfgs/trainer/default_val.yaml",
                                    R + "/cfgs/trainer/test/demo_test.yaml"], cfg_dir="")
    train_args.f_maps = f_maps
    train_args.num_levels = levels
    train_args.task_f_maps = [f_maps]
    train_args.backbone = backbone
    gen_args.task.pathology = pathology
    return gen_args, train_args


def build_twostage(f_maps, levels):
    """build_inpaint_model's own steps, with the get_processors call it evidently means."""
    from Trainer.models import process_args, get_postprocessor
    from Trainer.models.backbone import build_backbone
    from Trainer.models.head import get_head
    from Trainer.models.joiner import get_joiner, get_processors
    gen_args, train_args = cfgs(f_maps, levels, "unet3d+unet3d", True)
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
    return gen_args, train_args, pm.eval(), tm.eval(), pp, tp, get_postprocessor


@torch.no_grad()
def run_twostage(gen_args, train_args, pm, tm, pp, tp, post, x):
    """utils/test_utils.py:323-345."""
    import utils.misc as um
    samples = [{"input": x}]
    outputs_pathol, _ = pm(samples)
    for processor in pp:
        outputs_pathol = processor(outputs_pathol, samples)
    for i in range(len(samples)):
        samples[i]["input_masked"] = samples[i]["input"] * (1 - outputs_pathol[i]["pathology"])
    outputs_task, _ = tm(samples, input_name="input_masked", cond=[o["pathology"] for o in outputs_pathol])
    for processor in tp:
        outputs_task = processor(outputs_task, samples)
    outputs = um.merge_list_of_dict(outputs_task, outputs_pathol)
    outputs, _, _ = post(gen_args, train_args, outputs, samples, target=None, feats=None, tasks=gen_args.tasks)
    return outputs[0], samples[0]["input_masked"]


def top2_gap(seg):
    t = torch.topk(seg[0], 2, dim=0).values
    return (t[0] - t[1]) / t[0]


def record(d, o, o64, seed):
    """Sampled outputs of one merged output dict (fp32) and of the float64 run."""
    shape = tuple(o["segmentation"].shape[2:])
    nv = int(np.prod(shape))
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(nv, generator=g)[:N_VOX].sort().values
    d["idx"] = idx.numpy().astype(np.int64)
    d["seg_idx"] = idx[::4].numpy().astype(np.int64)
    feat_keys = [k for k in o if k.startswith("feat")]
    fkeys = [k for k in o if k not in feat_keys + ["segmentation", "label"]]
    d["float_keys"] = np.array(fkeys)
    d["feat_keys"] = np.array(feat_keys)
    d["out_keys"] = np.array(list(o.keys()))
    fidx = {}
    for k in feat_keys:
        for i, f in enumerate(o[k]):
            fi = torch.randperm(f.numel(), generator=g)[:N_FEAT].sort().values
            fidx[(k, i)] = fi
            d["%s%d_idx" % (k, i)] = fi.numpy().astype(np.int64)
            d["%s%d_shape" % (k, i)] = np.array(f.shape)
    for prefix, oo in (("", o), ("ref64/", o64)):
        d[prefix + "floats"] = np.stack([oo[k].reshape(-1)[idx].numpy() for k in fkeys])
        d[prefix + "seg"] = oo["segmentation"][0].reshape(oo["segmentation"].shape[1], -1)[:, idx[::4]].numpy()
        for (k, i), fi in fidx.items():
            d[prefix + "%s%d_vals" % (k, i)] = oo[k][i].reshape(-1)[fi].numpy()
    lab = o["label"][0, 0]
    assert o["label"].dtype == torch.int64 and int(lab.max()) <= 255
    d["label"] = lab.numpy().astype(np.uint8)
    gap = top2_gap(o["segmentation"]).reshape(-1)
    tie = torch.nonzero(gap < TIE)[:, 0]
    d["tie_idx"] = tie.numpy().astype(np.int64)
    d["tie_gap"] = gap[tie].numpy()
    d["shape"] = np.array(shape)
    frac = tie.numel() / float(nv)
    print("  %d of %d voxels are ties (%.1e), %d classes present" % (tie.numel(), nv, frac, len(torch.unique(lab))))
    assert frac <= TIE_CAP, "too many near-ties for this seed: pick another"


def save(stem, d):
    """stem.npz: everything but the float64 run; stem_b.npz: the ref64/ arrays.  Each under 1 MiB."""
    parts = {"": {k: v for k, v in d.items() if not k.startswith("ref64/")},
             "_b": {k: v for k, v in d.items() if k.startswith("ref64/")}}
    for suffix, part in parts.items():
        path = os.path.join(HERE, stem + suffix + ".npz")
        np.savez_compressed(path, **part)
        size = os.path.getsize(path)
        print("  %s%s.npz: %d bytes" % (stem, suffix, size))
        assert size < 1 << 20, "a committed file must stay under 1 MiB"


def sd_meta(d, prefix, sd, seed):
    d[prefix + "/names"] = np.array(list(sd.keys()))
    d[prefix + "/shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    d[prefix + "/sha256"] = np.array([TW.sha(v) for v in sd.values()])
    d[prefix + "/seed"] = np.array(seed)


def make_input(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((1, 1) + tuple(shape), generator=g)
    x[..., :4, :, :] = 0                                  # a zero slab
    return x


def twostage(stem, f_maps, levels, shape, seed, stored):
    print(stem)
    torch.manual_seed(seed)
    gen_args, train_args, pm, tm, pp, tp, post = build_twostage(f_maps, levels)
    d = {"cfg": np.array([f_maps, levels, 8])}
    for prefix, m, s in (("pathol", pm, seed + 1), ("task", tm, seed + 2)):
        sd = m.state_dict()
        if stored:
            TW.move_groupnorm(sd, s + 100)
            TW.scale_heads(sd, s + 200)
            d[prefix + "/names"] = np.array(list(sd.keys()))
            for k, v in sd.items():
                d["sd/%s/%s" % (prefix, k)] = v.numpy().copy()
        else:
            new = TW.draw_state_dict(list(sd.keys()), [tuple(v.shape) for v in sd.values()], s)
            m.load_state_dict(new)
            sd_meta(d, prefix, new, s)
    print("  state dicts: %d (stage 0), %d (stage 1) tensors" % (len(pm.state_dict()), len(tm.state_dict())))
    x = make_input(shape, seed + 3)
    o, xm = run_twostage(gen_args, train_args, pm, tm, pp, tp, post, x.clone())
    o64, xm64 = run_twostage(gen_args, train_args, pm.double(), tm.double(), pp, tp, post, x.double())
    pm.float(), tm.float()
    d["x"] = x.numpy()
    d["p"] = o["pathology"].numpy()
    d["input_masked"] = xm.numpy()
    d["ref64/p"] = o64["pathology"].numpy()
    print("  p spans %.3g .. %.3g" % (float(o["pathology"].min()), float(o["pathology"].max())))
    record(d, o, o64, seed + 4)
    save(stem, d)
    return d


@torch.no_grad()
def conditioned(stem, f_maps, levels, shape, seed):
    print(stem)
    import Trainer.models as TM
    gen_args, train_args = cfgs(f_maps, levels, "unet3d", True)       # the head's exclude_keys needs the key present
    train_args.condition = "mask+flip"
    torch.manual_seed(seed)
    try:
        gen_args, train_args, model, processors, _, post = TM.build_conditioned_model(gen_args, train_args, "cpu")
    except Exception as e:                                   # the criterion needs more configuration than inference has
        print("  build_conditioned_model: %s: %s -- assembled from its pieces" % (type(e).__name__, e))
        from Trainer.models.backbone import build_backbone
        from Trainer.models.head import get_head
        from Trainer.models.joiner import get_joiner, get_processors
        gen_args, train_args = TM.process_args(gen_args, train_args, task=gen_args.task)
        backbone = build_backbone(train_args, train_args.backbone, num_cond=len(train_args.condition.split("+")))
        head = get_head(train_args, train_args.task_f_maps, train_args.out_channels, True, -1, stage=1,
                        exclude_keys=["pathology"])
        model = get_joiner(gen_args.tasks, backbone, head, "cpu")
        processors = get_processors(gen_args, train_args, gen_args.tasks, "cpu", exclude_keys=["pathology"])
        post = TM.get_postprocessor
    model.eval()
    sd = model.state_dict()
    new = TW.draw_state_dict(list(sd.keys()), [tuple(v.shape) for v in sd.values()], seed + 1)
    model.load_state_dict(new)
    d = {"cfg": np.array([f_maps, levels, 8])}
    sd_meta(d, "model", new, seed + 1)
    x = make_input(shape, seed + 3)

    def run(m, x):
        cond = [torch.concat([torch.flip(x, dims=[2]), (x != 0).to(x.dtype)], dim=1)]
        samples = [{"input": x}]
        outs, _ = m(samples, cond=cond)
        for p in processors:
            outs = p(outs, samples)
        outs, _, _ = post(gen_args, train_args, outs, samples, target=None, feats=None, tasks=gen_args.tasks)
        return outs[0]
    o = run(model, x.clone())
    o64 = run(model.double(), x.double())
    d["x"] = x.numpy()
    record(d, o, o64, seed + 4)
    save(stem, d)


def signatures():
    import Trainer.models as TM
    import utils.misc as um
    (ev,) = load_ref_functions(R + "/utils/test_utils.py", ["evaluate_image_twostage"])
    ev = getattr(ev, "__wrapped__", ev)
    sig = {"evaluate_image_twostage": str(inspect.signature(ev)),
           "build_inpaint_model": str(inspect.signature(TM.build_inpaint_model)),
           "build_conditioned_model": str(inspect.signature(TM.build_conditioned_model)),
           "merge_list_of_dict": str(inspect.signature(um.merge_list_of_dict))}
    with open(os.path.join(HERE, "api_signatures_twostage.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)
        f.write("\n")
    print(sig)


if __name__ == "__main__":
    signatures()
    twostage("twostage_small", 8, 3, (24, 20, 36), 7, stored=True)
    twostage("twostage_wide", 64, 2, (16, 12, 40), 7, stored=False)
    conditioned("conditioned_wide", 64, 2, (16, 12, 40), 7)
