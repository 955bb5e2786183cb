"""The pathology-robust two-stage ("inpainting") inference harness of the reference (utils/test_utils.py:316-350 and the
tile loop of scripts/demo_test.py:66-119 around it), beside test_utils.py, whose configuration globals
(default_gen_cfg_file, default_train_cfg_file, ...), session cache (_cached_session, _default_cfgs), output assembly
(_tail_outputs) and tiling / stitch helpers it uses:

  TwoStageSession(gen_args, train_args, device, ...)      both models of build_inpaint_model resident
  evaluate_image_twostage(inputs, pathol_ckp_path, task_ckp_path, ...)   :316-350, sessions cached like evaluate_image
  tiled_inference_twostage(full_im, session, stride, win_size)           one GPU, eager

All arithmetic runs in libbrainfm_hip.so."""
from collections import OrderedDict

import torch

from . import _lib as L
from . import misc as MI
from . import models as M
from . import test_utils as TU
from .engine import UNetEngine


class TwoStageSession:
    """The two-stage (pathology-robust, "inpainting") model of build_inpaint_model with both engines resident:
    stage 0 predicts the pathology probability p from the image, stage 1 reads {image * (1 - p), p} as a two-channel
    input and evaluates every other head (utils/test_utils.py:316-350)."""

    def __init__(self, gen_args, train_args, device, pathol_state_dict=None, task_state_dict=None, pathol_ckp_path=None,
                 task_ckp_path=None):
        (self.gen_args, self.train_args, self.pathol_model, self.task_model, self.pathol_processors,
         self.task_processors, _, self.postprocessor) = M.build_inpaint_model(gen_args, train_args, device)
        for model, ckp, sd in ((self.pathol_model, pathol_ckp_path, pathol_state_dict),
                               (self.task_model, task_ckp_path, task_state_dict)):
            if ckp is not None:
                M.load_checkpoint(ckp, [model], model_keys=["model"])
            if sd is not None:
                M.load_state_dict_by_suffix(model, sd)
        self.device = torch.device(device if not isinstance(device, int) else "cuda:%d" % device)
        self.tasks = self.gen_args.tasks

    @property
    def pathol_engine(self):
        return self.pathol_model.backbone.engine(self.pathol_model.head)

    @property
    def task_engine(self):
        return self.task_model.backbone.engine(self.task_model.head)

    engine = task_engine                                     # what the tile loop asks a session for (device, library)

    def stitch_keys(self):
        """The keys tiled_inference_twostage stitches: STITCH_KEYS + ['pathology'], those the two head sets produce."""
        tail = self.task_model.head.tail(self.task_engine)
        return TU.stitch_selection(list(tail.map_names), tail.desc.n_seg > 0)[0] + ["pathology"]

    def run_stages(self, x_cl, dims, want_feat=True, want_seg=True):
        """Both stages of one sample.  x_cl: (D,H,W,1) contiguous fp32.  Returns (stage 0: (feats, maps, fnorm),
        stage 1: (feats, maps, fnorm, seg, label, tail), the stage-1 input (D,H,W,2))."""
        eng0, eng1 = self.pathol_engine, self.task_engine
        D, H, W = dims
        # stage 0: backbone, then the tail with the one pathology head (sigmoid in the tail: PatholProcessor, joiner.py:79-87)
        feats0 = eng0.backbone_cl(x_cl, dims)
        tail0 = self.pathol_model.head.tail(eng0)
        maps0, fnorm0, _, _ = tail0.run(feats0[-1][0], dims, input_cl=x_cl, want_feat=want_feat, want_seg=False)
        p = maps0["pathology"]
        # the stage-1 input {x * (1 - p), p}, channels-last, in one pass
        xin = torch.empty((D, H, W, 2), dtype=torch.float32, device=eng1.device)
        L.check(eng1.lib.bfm_mask_concat2(L.ptr(x_cl), L.ptr(p), D * H * W, L.ptr(xin), L.stream_ptr()), "mask_concat2")
        # stage 1: backbone, then the fused tail (processors and post-processor in one kernel); high_res adds the
        # ORIGINAL input to the residual (Trainer/models/__init__.py:308 reads samples[i]['input'])
        feats1 = eng1.backbone_cl(xin, dims)
        tail1 = self.task_model.head.tail(eng1)
        maps1, fnorm1, seg, label = tail1.run(feats1[-1][0], dims, input_cl=x_cl, want_feat=want_feat, want_seg=want_seg)
        return (feats0, maps0, fnorm0), (feats1, maps1, fnorm1, seg, label, tail1), xin

    @torch.no_grad()
    @L.on_device(lambda self, *a, **k: self.device)
    def evaluate(self, inputs, feature_only=True):
        """inputs: (batch, 1, s, r, c).  feature_only: (feat_pathol[-1], feat_task[-1]); otherwise the merged output dict
        of the reference: 'feat_task' and 'feat_pathol' (lists, deepest first), 'pathology', the float maps,
        'segmentation' and the int64 'label'."""
        if inputs.shape[0] != 1:
            res = [self.evaluate(inputs[b:b + 1], feature_only) for b in range(inputs.shape[0])]
            if feature_only:
                return tuple(torch.cat([r[j] for r in res], 0) for j in range(2))
            return OrderedDict((k, ([torch.cat([r[k][j] for r in res], 0) for j in range(len(res[0][k]))]
                                    if isinstance(res[0][k], list) else torch.cat([r[k] for r in res], 0)))
                               for k in res[0])
        eng1 = self.task_engine
        dims = tuple(inputs.shape[2:])
        x_cl = eng1.to_cl(inputs)
        (feats0, maps0, fnorm0), (feats1, maps1, fnorm1, seg, label, tail1), _ = \
            self.run_stages(x_cl, dims, want_feat=True, want_seg=not feature_only)

        def feat_list(feats, fnorm):
            bufs = [f for f, _ in feats]
            if fnorm is not None:
                bufs[-1] = fnorm
            return [UNetEngine.as_ncdhw(f) for f in bufs]

        task = OrderedDict(feat_task=feat_list(feats1, fnorm1))
        TU._tail_outputs(tail1, maps1, seg, label, task)
        pathol = OrderedDict(feat_pathol=feat_list(feats0, fnorm0), pathology=maps0["pathology"][None, None])
        out = MI.merge_list_of_dict([task], [pathol])[0]
        if feature_only:
            return out["feat_pathol"][-1], out["feat_task"][-1]
        return out


@torch.no_grad()
def evaluate_image_twostage(inputs, pathol_ckp_path, task_ckp_path, feature_only=True, device="cpu", gen_cfg=None,
                            model_cfg=None):
    """utils/test_utils.py:316-350.  inputs: (batch, 1, s, r, c).  Both models stay resident between calls."""
    device = TU._resolve_device(device)
    if torch.device(device).type != "cuda":
        raise L.BfmError("evaluate_image_twostage runs on a HIP device only; there is no CPU fallback in the product path")
    key = ("twostage", pathol_ckp_path, task_ckp_path, (TU._mtime(pathol_ckp_path), TU._mtime(task_ckp_path)), gen_cfg,
           model_cfg, str(device))
    build = lambda: TwoStageSession(*TU._default_cfgs(gen_cfg, model_cfg), device, pathol_ckp_path=pathol_ckp_path,
                                    task_ckp_path=task_ckp_path)
    return TU._cached_session(key, build).evaluate(inputs, feature_only)


@torch.no_grad()
@L.on_device(lambda full_im, session, *a, **k: session.device)
def tiled_inference_twostage(full_im, session, stride=[80, 80, 80], win_size=[160, 160, 160]):
    """The tile loop of scripts/demo_test.py:66-119 around the two-stage model, on one GPU: per tile stage 0 -> mask ->
    stage 1 -> `output * (tile input != 0)` accumulated in tile order through the stitch kernels, then / cnt.
    full_im: (1,1,D,H,W).  session: a TwoStageSession.  Returns ({key: (D,H,W) fp32}, ranges, cnt) with the keys
    STITCH_KEYS + ['pathology'] that the heads produce.
    Every tile runs eagerly, one after the other: no graph capture, no lanes, no batching of same-shape tiles through the
    deep levels and no distribution over ranks (tiled_inference / tiled_inference_distributed have those for the
    one-stage model)."""
    lib = L.load()
    eng = session.task_engine
    full_im = full_im.to(device=eng.device, dtype=torch.float32)
    shape = tuple(full_im.shape[2:])
    ranges = TU.tiling_ranges(shape, stride, win_size)
    cnt = TU.count_volume(shape, ranges, eng.device)
    keys = session.stitch_keys()
    acc_buf = torch.zeros((len(keys),) + shape, dtype=torch.float32, device=eng.device)
    acc = OrderedDict((k, acc_buf[j]) for j, k in enumerate(keys))
    for rng in ranges:
        x_cl = eng.to_cl(TU.tile_window(full_im, rng))
        dims = tuple(b - a for a, b in rng)
        (_, maps0, _), (_, maps1, _, _, label, _), _ = session.run_stages(x_cl, dims, want_feat=False, want_seg=False)
        maps = dict(maps1)
        maps["pathology"] = maps0["pathology"]
        TU._stitch_tile(lib, acc, keys, maps, label, x_cl, rng, shape)
    n = shape[0] * shape[1] * shape[2]
    L.check(lib.bfm_divide_by_count_multi(L.ptr(acc_buf), L.ptr(cnt), n, len(keys), L.stream_ptr()), "divide_by_count")
    return acc, ranges, cnt
