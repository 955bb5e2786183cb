"""torch.autograd through the HIP network for losses written in torch.

``train.TrainStep`` trains with the reference's own criterion; the reference's model, though, is an ordinary nn.Module that
is also fine-tuned on downstream tasks with the user's head and loss (scripts/demo_get_feature.py).  This module is that
path:

    dm = differentiable(model)                       # shares model's nn.Parameter objects and state-dict keys
    procs = differentiable_processors(processors)
    outs, _ = dm(samples)                            # same keys, shapes and layouts as model(samples), with a grad_fn
    for p in procs: outs = p(outs)
    loss = my_loss(outs[0]["feat"][-1], outs[0]["T1"], ...)
    loss.backward()                                  # backbone_backward, bfm_head_bwd, bfm_normalize_bwd on the device
    torch.optim.AdamW(model.parameters()).step()     # the next forward of dm AND of model sees the new weights

One torch.autograd.Function per sample: forward = backward.backbone_forward_train (tape) + Tail.run_raw, backward = the
kernels TrainStep._sample_backward runs.  A frozen backbone (no backbone parameter and no input requires grad) runs without
a tape and ends at bfm_head_wgrad, as TrainStep(trainable='head').  With nothing requiring grad, or under torch.no_grad(),
the call IS model(...): the inference path, the same bits.

After an optimiser step the parameters' version counters have moved; instead of letting UNet3D.engine() build a new
engine (and tune its convolutions again), sync_engine refreshes the engine's tensors from the parameters in place and
rebuilds the packed weight forms, as TrainStep.apply does.  A parameter whose storage or shape changed still rebuilds.

Refused by name: a second-order backward (create_graph=True), hidden head layers (task_f_maps longer than one), the pooled
age head, conditioned and two-stage models, torch.autocast, CPU tensors (no CPU fallback).  Several ranks: all-reduce the
parameters' .grad yourself (or wrap the parameters in your own reducer); nothing here talks to torch.distributed.
"""
import ctypes as C
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib as L
from . import backward as BW
from . import models as M
from .engine import UNetEngine


# --------------------------------------------------------------------------- the engine after an optimiser step
def _ptrs(key):
    return None if key is None else tuple(k[0] for k in key)


def sync_engine(backbone, head=None):
    """backbone.engine(head) without a rebuild where only the parameters' VALUES changed (an optimiser stepped them in
    place): the engine's raw weights / gamma / beta and the tail's head rows are refreshed from the parameters, every packed
    form is rebuilt in place (UNetEngine.repack_all) and the cache keys of UNet3D.engine / TaskHead.tail are moved on, so
    that neither this path nor model(...) builds a new engine or tunes again.  Only the head moved: nothing of the backbone
    is repacked."""
    key = (backbone._version_key(), None if head is None else head._version_key())
    old = backbone._engine_key
    eng = backbone._engine
    if eng is None or old is None or old == key:
        return backbone.engine(head)
    if _ptrs(old[0]) != _ptrs(key[0]) or _ptrs(old[1]) != _ptrs(key[1]):
        return backbone.engine(head)                       # moved or replaced storage: rebuild, as ever
    own = dict(backbone.named_parameters())
    pairs = []
    for pair in eng.enc + eng.dec:
        for ly in pair:
            stem = ly.name[len("backbone."):]
            pairs += [(ly.w_raw, own[stem + ".conv.weight"]), (ly.gamma, own[stem + ".groupnorm.weight"]),
                      (ly.beta, own[stem + ".groupnorm.bias"])]
    tail = head._tail if head is not None else None
    if tail is not None and (head._tail_key is None or head._tail_key[0] != id(eng)):
        tail = None
    hown = dict(head.named_parameters()) if head is not None else {}
    if tail is not None:
        for task, (r0, n) in tail.row_of.items():
            pairs += [(tail.head_w[r0:r0 + n], hown["final_conv_%s.weight" % task].reshape(n, -1)),
                      (tail.head_b[r0:r0 + n], hown["final_conv_%s.bias" % task].reshape(n))]
    if any(tuple(dst.shape) != tuple(src.shape) for dst, src in pairs):
        return backbone.engine(head)
    with torch.no_grad(), torch.cuda.device(eng.device):
        for dst, src in pairs:
            if dst.data_ptr() != src.data_ptr():           # fp32 parameters on the device ARE the engine's tensors
                dst.copy_(src.detach())
        if old[0] != key[0]:
            eng.repack_all(refresh=BW.refresh_dgrad)
        if tail is not None and old[1] != key[1] and tail.n_out:
            hw = torch.zeros(1, dtype=torch.float32, device=eng.device)
            L.check(eng.lib.bfm_absmax_f32(L.ptr(tail.head_w), 1, tail.head_w.numel(), tail.head_w.numel(), L.ptr(hw),
                                           L.stream_ptr()), "absmax head_w")
            tail.desc.head_wmax = float(hw.item())
            eng.weights_epoch += 1
    backbone._engine_key = key
    if tail is not None:
        head._tail_key = (id(eng), key[1]) + tuple(head._tail_key[2:])
    return eng


# --------------------------------------------------------------------------- one sample
def _cl(t):
    """(1,C,D,H,W) cotangent of any layout -> contiguous (D,H,W,C) fp32 (None stays None)."""
    if t is None:
        return None
    return t[0].permute(1, 2, 3, 0).to(torch.float32).contiguous()


class _SampleFn(torch.autograd.Function):
    """Backbone (+ heads) of one (1,Cin,D,H,W) sample.  Inputs: the owner, use_head, fast, x, then the backbone's and the
    head's parameters in named_parameters() order.  Outputs: the decoder feature maps (deepest first, the last one
    unit-normalised when unit_feat) and, with a head, the raw head outputs as one (1,n_out,D,H,W) view."""

    @staticmethod
    def forward(ctx, owner, use_head, fast, x, *params):
        backbone = owner._backbone
        head = owner._head if use_head else None
        eng = sync_engine(backbone, owner._head)              # one engine, with or without the heads in this call
        nb = len(owner._bb_names)
        needs = ctx.needs_input_grad[4:]
        ctx.train_backbone = bool(ctx.needs_input_grad[3] or any(needs[:nb]))
        ctx.owner, ctx.eng, ctx.use_head = owner, eng, use_head
        dims = tuple(x.shape[2:])
        ctx.dims, ctx.x_dtype = dims, x.dtype
        with torch.cuda.device(eng.device):
            x_cl = eng.to_cl(x)
            if ctx.train_backbone:
                feats, tape = BW.backbone_forward_train(eng, x_cl, dims, fast=fast)
            else:
                feats, tape = eng.backbone_cl(x_cl, dims), None      # frozen: the inference path, nothing taped
            bufs = [f for f, _ in feats]
            feat_last = bufs[-1]
            raw, fn, tail = None, None, None
            if use_head:
                tail = head.tail(eng)
                raw, fn = tail.run_raw(feat_last, dims, want_feat=True, apply_hidden=False)
            elif eng.unit_feat:
                fn = eng.normalize(feat_last, dims)
            if fn is not None:
                bufs[-1] = fn
        ctx.tape, ctx.tail = tape, tail
        ctx.feat_last = feat_last if ctx.train_backbone else None
        ctx.fn = bufs[-1]
        ctx.n_feat = len(bufs)
        outs = [UNetEngine.as_ncdhw(f) for f in bufs]
        if raw is not None:
            outs.append(UNetEngine.as_ncdhw(raw))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        if torch.is_grad_enabled():
            raise NotImplementedError("brainfm_amd.autograd: backward(create_graph=True) asks for a second-order graph; the "
                                      "HIP backward kernels are not differentiable again")
        owner, eng, dims = ctx.owner, ctx.eng, ctx.dims
        lib = eng.lib
        nvox = dims[0] * dims[1] * dims[2]
        nb = len(owner._bb_names)
        need_x = ctx.needs_input_grad[3]
        gfeats = [_cl(g) for g in gouts[:ctx.n_feat]]
        graw = _cl(gouts[ctx.n_feat]) if ctx.use_head else None
        grads = OrderedDict()
        dx = None
        with torch.cuda.device(eng.device):
            st = L.stream_ptr()
            dFn = gfeats[-1]                                       # cotangent of the (normalised) last map, (D,H,W,C)
            if graw is not None:
                tail = ctx.tail
                n_out, cf = tail.n_out, tail.c_feat
                dW = torch.empty((n_out, cf), dtype=torch.float32, device=eng.device)
                db = torch.empty(n_out, dtype=torch.float32, device=eng.device)
                if ctx.train_backbone:
                    dF = torch.empty((nvox, cf), dtype=torch.float32, device=eng.device)
                    ws = torch.empty(lib.bfm_head_bwd_workspace(n_out, cf, nvox), dtype=torch.uint8, device=eng.device)
                    L.check(lib.bfm_head_bwd(L.ptr(graw), L.ptr(ctx.fn), L.ptr(tail.head_w), n_out, cf, nvox, L.ptr(dW),
                                             L.ptr(db), L.ptr(dF), L.ptr(ws), ws.numel(), st), "head_bwd")
                    dF = dF.view(dims + (cf,))
                    dFn = dF if dFn is None else BW._add(dF, dFn)
                else:
                    ws = torch.empty(lib.bfm_head_wgrad_workspace(n_out, cf, nvox), dtype=torch.uint8, device=eng.device)
                    L.check(lib.bfm_head_wgrad(L.ptr(graw), L.ptr(ctx.fn), n_out, cf, nvox, L.ptr(dW), L.ptr(db), L.ptr(ws),
                                               ws.numel(), st), "head_wgrad")
                for task, (r0, n) in tail.row_of.items():
                    grads["head.final_conv_%s.weight" % task] = dW[r0:r0 + n]
                    grads["head.final_conv_%s.bias" % task] = db[r0:r0 + n]
            if ctx.train_backbone:
                if dFn is not None and eng.unit_feat:
                    cf = dFn.shape[-1]
                    dfeat = torch.empty_like(dFn)
                    L.check(lib.bfm_normalize_bwd(L.ptr(ctx.feat_last), L.ptr(dFn), cf, nvox, 1e-12, L.ptr(dfeat), st),
                            "normalize_bwd")
                else:
                    dfeat = dFn
                g, dx = BW.backbone_backward(eng, ctx.tape, gfeats[:-1] + [dfeat], want_input_grad=True)
                grads.update(g)
        out = [None, None, None, UNetEngine.as_ncdhw(dx).to(ctx.x_dtype) if (need_x and dx is not None) else None]
        names = owner._bb_names + (owner._head_names if ctx.use_head else [])
        needs = ctx.needs_input_grad[4:]
        shapes = ctx.owner._shapes
        for name, need in zip(names, needs):
            g = grads.get(name) if need else None
            out.append(g.reshape(shapes[name]) if g is not None else None)
        return tuple(out)


# --------------------------------------------------------------------------- the modules
def _refuse_call(x):
    if torch.is_autocast_enabled():
        raise L.BfmError("brainfm_amd.autograd under torch.autocast: the HIP kernels compute in their own precisions; "
                         "leave the autocast region around the model call")
    if x.device.type != "cuda":
        raise L.BfmError("brainfm_amd.autograd needs a HIP device; the product path has no CPU fallback")


class _Owner:
    """What one _SampleFn needs of its model: the modules, the parameters in a fixed order under the reference's names."""

    def __init__(self, backbone, head):
        self._backbone, self._head = backbone, head
        bb = list(backbone.named_parameters())
        hd = list(head.named_parameters()) if head is not None else []
        self._bb_names = ["backbone." + k for k, _ in bb]
        self._head_names = ["head." + k for k, _ in hd]
        self._bb_params = [p for _, p in bb]
        self._head_params = [p for _, p in hd]
        self._shapes = {n: tuple(p.shape) for n, p in zip(self._bb_names + self._head_names,
                                                          self._bb_params + self._head_params)}

    def wants_grad(self, x, use_head):
        ps = self._bb_params + (self._head_params if use_head else [])
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in ps))

    def sample(self, x, use_head, fast):
        """(feature maps, raw head outputs or None) of one (1,Cin,D,H,W) sample, with a grad_fn."""
        ps = self._bb_params + (self._head_params if use_head else [])
        outs = _SampleFn.apply(self, use_head, fast, x, *ps)
        if use_head:
            return list(outs[:-1]), outs[-1]
        return list(outs), None


class DifferentiableBackbone(nn.Module):
    """models.UNet3D with get_feature / forward under autograd.  The encoders / decoders ARE the backbone's modules (same
    parameters, same state-dict keys)."""

    def __init__(self, backbone, fast=None, head=None):
        """head: the TaskHead the backbone's engine is shared with (differentiable(model) passes model.head), so that calls
        with and without the heads run on ONE engine."""
        super().__init__()
        if not isinstance(backbone, M.UNet3D):
            raise L.BfmError("differentiable: expected a models.UNet3D backbone, got %s" % type(backbone).__name__)
        if backbone.in_channels != 1:
            raise NotImplementedError("differentiable: conditioned models (a backbone reading %d input channels) are not "
                                      "built; their stem's backward is the training step's" % backbone.in_channels)
        self.encoders = backbone.encoders
        self.decoders = backbone.decoders
        self.fast = fast
        self.__dict__["_inner"] = backbone                    # not a registered child: the state-dict keys stay the model's
        self.__dict__["_owner"] = _Owner(backbone, head)

    def _inference(self, x1):
        """UNet3D.get_feature of one sample on the shared engine: the same kernels, the same bits."""
        with torch.no_grad():
            eng = sync_engine(self._inner, self._owner._head)
            with torch.cuda.device(eng.device):
                dims = tuple(x1.shape[2:])
                bufs = [f for f, _ in eng.backbone_cl(eng.to_cl(x1), dims)]
                if self._inner.is_unit_vector:
                    bufs[-1] = M.normalize_cl(eng, bufs[-1], dims)
            return [UNetEngine.as_ncdhw(f) for f in bufs]

    def get_feature(self, x):
        """unet3d/model.py:195-209 with a grad_fn: list of decoder features (deepest first), last one unit-normalised."""
        _refuse_call(x)
        if self._owner.wants_grad(x, False):
            outs = [self._owner.sample(x[b:b + 1], False, self.fast)[0] for b in range(x.shape[0])]
        else:
            outs = [self._inference(x[b:b + 1]) for b in range(x.shape[0])]
        if len(outs) == 1:
            return outs[0]
        return [torch.cat([o[i] for o in outs], 0) for i in range(len(outs[0]))]

    def forward(self, x):
        return self.get_feature(x)[-1]


class DifferentiableModel(nn.Module):
    """models.MultiInputIndepJoiner under autograd: dm(input_list, input_name='input', cond=[]) -> (outs, inputs)."""

    def __init__(self, model, fast=None):
        super().__init__()
        if not isinstance(model, M.MultiInputIndepJoiner):
            raise L.BfmError("differentiable: expected the model build_model returns (models.MultiInputIndepJoiner), got %s"
                             % type(model).__name__)
        if model.postfix:
            raise NotImplementedError("differentiable: two-stage models (the '%s' stage of build_inpaint_model) are not "
                                      "built; train them with TwoStageTrainStep" % model.postfix)
        head = model.head
        if head is not None:
            if len(head.layers):
                raise NotImplementedError("differentiable: task_f_maps %s: hidden head layers (task_f_maps longer than one) "
                                          "are not built under autograd" % (head.task_f_maps,))
            if head.age_task is not None:
                raise NotImplementedError("differentiable: the pooled age head ('%s') is not built under autograd"
                                          % head.age_task)
        self.backbone = DifferentiableBackbone(model.backbone, fast, head)
        self.head = head
        self.fast = fast
        self.__dict__["_model"] = model
        self.__dict__["_owner"] = _Owner(model.backbone, head)

    def forward(self, input_list, input_name="input", cond=[]):
        if len(cond) > 0:
            raise NotImplementedError("differentiable: conditioned models (cond inputs) are not built under autograd")
        model, owner = self._model, self._owner
        use_head = model.head is not None and bool(model.head.dense_channels)
        xs = [x[input_name] for x in input_list]
        for x in xs:
            _refuse_call(x)
        if not any(owner.wants_grad(x, use_head) for x in xs):
            sync_engine(model.backbone, model.head)
            return model(input_list, input_name, cond)             # the inference path itself: the same bits
        outs = []
        for xin in xs:
            per_b = []
            for b in range(xin.shape[0]):
                feats, raw = owner.sample(xin[b:b + 1], use_head, self.fast)
                out = OrderedDict()
                out["feat" + model.postfix] = feats
                if raw is not None:
                    # TaskHead.split_raw on the channels-last view, so that the heads' strides are model(...)'s
                    out.update(model.head.split_raw(raw[0].permute(1, 2, 3, 0)))
                per_b.append(out)
            if len(per_b) == 1:
                outs.append(per_b[0])
            else:
                m = OrderedDict()
                for k in per_b[0]:
                    if isinstance(per_b[0][k], list):
                        m[k] = [torch.cat([p[k][j] for p in per_b], 0) for j in range(len(per_b[0][k]))]
                    else:
                        m[k] = torch.cat([p[k] for p in per_b], 0)
                outs.append(m)
        return outs, xs


def differentiable(model, fast=None):
    """The nn.Module counterpart of `model` (what build_model returned) whose outputs carry a grad_fn.  It shares the
    model's nn.Parameter objects: list(dm.parameters()) is list(model.parameters()), dm.state_dict() has the model's keys.
    fast: handed to backward.backbone_forward_train (None: its default, the inference layer path with the tape hook)."""
    return DifferentiableModel(model, fast)


# --------------------------------------------------------------------------- processors
def _need_cuda(t, what):
    if t.device.type != "cuda":
        raise L.BfmError("%s needs a HIP device; the product path has no CPU fallback" % what)


class _SoftmaxFn(torch.autograd.Function):
    """SegProcessor's bfm_softmax_cl; backward bfm_softmax_cl_bwd from the stored posterior."""

    @staticmethod
    def forward(ctx, x):
        lib = L.load()
        t, p, rs, c, n = M._cl_rows(x)
        buf, view = M._new_like_spatial(t, c)
        L.check(lib.bfm_softmax_cl(C.c_void_p(p), rs, c, L.ptr(buf), c, n, L.stream_ptr()), "softmax")
        ctx.post = buf
        return view

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib = L.load()
        g, gp, grs, c, n = M._cl_rows(g)
        buf, view = M._new_like_spatial(g, c)
        with torch.cuda.device(g.device):
            L.check(lib.bfm_softmax_cl_bwd(L.ptr(ctx.post), c, C.c_void_p(gp), grs, c, L.ptr(buf), c, n, L.stream_ptr()),
                    "softmax_bwd")
        return view


class _UnaryFn(torch.autograd.Function):
    """models._unary for EW_SIGMOID / EW_CLAMP; backward bfm_ew_unary_bwd channel by channel, from the output (sigmoid) or
    the input (clamp)."""

    @staticmethod
    def forward(ctx, x, op, a, b):
        y = M._unary(op, x, a, b)
        ctx.op, ctx.a, ctx.b = op, float(a), float(b)
        ctx.save_for_backward(y if op == L.EW_SIGMOID else x)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib = L.load()
        v, vp, vrs, c, n = M._cl_rows(ctx.saved_tensors[0])
        g, gp, grs, _, _ = M._cl_rows(g)
        buf, view = M._new_like_spatial(g, c)
        with torch.cuda.device(g.device):
            for j in range(c):
                L.check(lib.bfm_ew_unary_bwd(ctx.op, C.c_void_p(vp + 4 * j), vrs, C.c_void_p(gp + 4 * j), grs,
                                             C.c_void_p(buf.data_ptr() + 4 * j), c, n, ctx.a, ctx.b, L.stream_ptr()),
                        "ew_unary_bwd")
        return view, None, None, None


class _NormalizeFn(torch.autograd.Function):
    """ContrastiveProcessor's F.normalize(dim=1) of one (1,C,D,H,W) map; backward bfm_normalize_bwd."""

    @staticmethod
    def forward(ctx, f):
        cl = f[0].permute(1, 2, 3, 0).contiguous().to(torch.float32)
        ctx.cl = cl
        return UNetEngine.as_ncdhw(M.normalize_cl(None, cl, tuple(f.shape[2:])))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        cl = ctx.cl
        gcl = _cl(g)
        out = torch.empty_like(cl)
        with torch.cuda.device(cl.device):
            L.check(L.load().bfm_normalize_bwd(L.ptr(cl), L.ptr(gcl), cl.shape[-1], cl.numel() // cl.shape[-1], 1e-12,
                                               L.ptr(out), L.stream_ptr()), "normalize_bwd")
        return UNetEngine.as_ncdhw(out)


class DifferentiableSegProcessor(nn.Module):
    """joiner.py:69-77 under autograd: SegProcessor's kernel, the same bits."""

    @L.on_device(lambda self, outputs, *a, **k: outputs[0]["segmentation"] if outputs else None)
    def forward(self, outputs, *kwargs):
        for output in outputs:
            _need_cuda(output["segmentation"], "DifferentiableSegProcessor")
            output["segmentation"] = _SoftmaxFn.apply(output["segmentation"])
        return outputs


class DifferentiableDistProcessor(nn.Module):
    """joiner.py:149-157 under autograd."""

    def __init__(self, gen_args):
        super().__init__()
        self.gen_args = gen_args

    def forward(self, outputs, *kwargs):
        m = float(self.gen_args.max_surf_distance)
        for output in outputs:
            _need_cuda(output["distance"], "DifferentiableDistProcessor")
            output["distance"] = _UnaryFn.apply(output["distance"], L.EW_CLAMP, -m, m)
        return outputs


class DifferentiablePatholProcessor(nn.Module):
    """joiner.py:79-87 under autograd."""

    def forward(self, outputs, *kwargs):
        for output in outputs:
            _need_cuda(output["pathology"], "DifferentiablePatholProcessor")
            output["pathology"] = _UnaryFn.apply(output["pathology"], L.EW_SIGMOID, 0.0, 0.0)
        return outputs


class DifferentiableContrastiveProcessor(nn.Module):
    """joiner.py:136-147 under autograd."""

    @L.on_device(lambda self, outputs, *a, **k: outputs[0]["feat"][-1] if outputs else None)
    def forward(self, outputs, *kwargs):
        for output in outputs:
            f = output["feat"][-1]
            _need_cuda(f, "DifferentiableContrastiveProcessor")
            per_b = [_NormalizeFn.apply(f[b:b + 1]) for b in range(f.shape[0])]
            output["feat"][-1] = per_b[0] if len(per_b) == 1 else torch.cat(per_b, 0)
        return outputs


def differentiable_processors(processors):
    """Counterparts of what get_processors returned, in the same order: the same forward kernels (bit-identical values), a
    backward on the device.  AgeProcessor and UncertaintyProcessor are plain torch ops and are handed back as they are."""
    out = []
    for p in processors:
        if isinstance(p, M.SegProcessor):
            out.append(DifferentiableSegProcessor())
        elif isinstance(p, M.DistProcessor):
            out.append(DifferentiableDistProcessor(p.gen_args))
        elif isinstance(p, M.PatholProcessor):
            out.append(DifferentiablePatholProcessor())
        elif isinstance(p, M.ContrastiveProcessor):
            out.append(DifferentiableContrastiveProcessor())
        elif isinstance(p, (M.AgeProcessor, M.UncertaintyProcessor)):
            out.append(p)
        else:
            raise L.BfmError("differentiable_processors: no counterpart of %s" % type(p).__name__)
    return out
