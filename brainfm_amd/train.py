"""One training iteration of the multi-task U-Net on the HIP kernels.

Mirrors the reference's iteration -- Trainer/engine.py:96-147:

    outputs, _ = model(samples)                       -> backward.backbone_forward_train + Tail.run_raw   (per sample)
    outputs = processor(outputs, ...)                 -> softmax / clamp folded into the loss kernels
    loss_dict = criterion(outputs, target, samples)   -> bfm_loss_l1_multi / bfm_loss_grad_l1_multi / bfm_loss_seg / ...
    losses = sum(loss_dict[k] * weight_dict[k])
    scaler.scale(losses).backward()                   -> bfm_head_bwd, bfm_normalize_bwd, backward.backbone_backward
    scaler.unscale_(optimizer); clip_gradients(...)   -> bfm_grad_sumsq_multi (+ non-finite flag; LARS: bfm_lars_sums_multi),
                                                         per-parameter coefficient                      (TrainStep._measure)
    scaler.step(optimizer); scaler.update()           -> bfm_adamw_step_multi | bfm_adam_step_multi | bfm_sgd_step_multi |
                                                         bfm_lars_step_multi, LossScaler.update         (TrainStep._update)

With train_args.freeze_feat (TrainStep(trainable='head')) the backbone is frozen: model(samples) runs on the inference kernels
without a tape, backward() ends at the heads (bfm_head_wgrad: dW and db, no feature gradient) and the optimiser sees the
`head.` tensors alone.

The four optimisers share one path: one descriptor per parameter (bfm_optim_tensor_t), one chunk map, one measuring launch and
one update launch over all tensors, whatever the kind.

with the criterion of Trainer/models/criterion.py (SetMultiCriterion: sum over the samples / all_samples) restricted to
the supervised dense heads: T1 T2 FLAIR CT (+_grad, optional <key>_DM weights), SR(+_grad), distance, registration
(+_grad, and the regularisers registration_smooth / registration_hessian of the raw head output), bias_field_log (l1 | l2,
soft mask 1 - seg[:, 0]), seg_ce, seg_dice, and loss_age of the pooled scalar head (| abs(p) - age |, models.AgeHead).
Any other loss name raises.  criterion_losses builds the loss names and weights from train_args as get_criterion does.
The head-less pre-training mode (task 'contrastive': SetCriterion with loss_feat_contrastive alone, criterion.py:96-109)
is ContrastiveStep, which shares the parameter table, optimiser, scaler and checkpoint code with TrainStep.

Everything numeric runs in the HIP library; torch holds buffers, adds the per-sample gradients and runs the RCCL
all-reduce.  There is no CPU path: without the extension or a HIP device construction fails.
"""
import ctypes as C
import math
import os
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib as L
from . import backward as BW
from . import models as M

IMAGE_KEYS = ("T1", "T2", "FLAIR", "CT")
SUPPORTED = set(IMAGE_KEYS) | {k + "_grad" for k in IMAGE_KEYS} | {
    "SR", "SR_grad", "distance", "surface", "registration", "registration_grad", "registration_smooth",
    "registration_hessian", "bias_field_log", "seg_ce", "seg_dice", "pathol_ce", "pathol_dice", "age"}
REG_REGULARISERS = ("registration_smooth", "registration_hessian")
TRAINABLE = ("all", "head")


def trainable_names(names, trainable):
    """The parameter names a step with TrainStep(trainable=...) trains, in the order given: 'all' keeps every name, 'head'
    the task head's (`head.`: the 1x1x1 heads, hidden head layers, the pooled scalar head) -- what scripts/train.py:46-53
    get_params_groups keeps of a model whose backbone has requires_grad = False."""
    if trainable == "all":
        return list(names)
    if trainable == "head":
        return [n for n in names if n.startswith("head.")]
    raise ValueError("trainable=%r: one of %s" % (trainable, ", ".join(repr(t) for t in TRAINABLE)))


def freeze_feat_of(train_args):
    """train_args.freeze_feat (cfgs/trainer/default_train.yaml:77) as a bool; a missing key is False.  The `feat_opt` block
    beside it (default_train.yaml:90-92, always present) is not read: no line of the reference reads it either, every
    trained tensor is in the one parameter group of scripts/train.py:46-53, and a frozen backbone has no group at all."""
    if isinstance(train_args, dict):
        return bool(train_args.get("freeze_feat", False))
    return bool(getattr(train_args, "freeze_feat", False))


def criterion_losses(train_args, tasks, exclude_keys=()):
    """(loss_names, weight_dict) as Trainer/models/__init__.py get_criterion builds them from the task names and
    train_args.losses / train_args.weights, in the reference's order.  A switch missing from train_args.losses is off."""
    lo, w = train_args.losses, train_args.weights
    on = lambda k: bool(getattr(lo, k, False))                         # noqa: E731
    names, wd = [], OrderedDict()
    if "contrastive" in tasks:
        return ["contrastive"], OrderedDict(loss_contrastive=w.contrastive)

    def add(name, weight):
        names.append(name)
        wd["loss_" + name] = weight
    for task in tasks:
        if any(k in task for k in IMAGE_KEYS):
            add(task, w.image)
            if on("image_grad"):
                add(task + "_grad", w.image_grad)
        if "segmentation" in task:
            add("seg_ce", w.seg_ce)
            add("seg_dice", w.seg_dice)
        if "bias_field" in task:
            add("bias_field_log", w.bias_field_log)
        if "super_resolution" in task:
            add("SR", w.image)
            if on("image_grad"):
                add("SR_grad", w.image_grad)
        if "distance" in task:
            add("distance", w.distance)
        if "registration" in task:
            add("registration", w.registration)
            for k in ("registration_grad",) + REG_REGULARISERS:
                if on(k):
                    add(k, getattr(w, k))
        if "surface" in task:
            add("surface", w.surface)
        if "age" in task:
            add("age", w.age)
        if "pathology" in task and "pathology" not in exclude_keys:
            add("pathol_ce", w.pathol_ce)
            add("pathol_dice", w.pathol_dice)
    if on("implicit_pathol"):
        add("implicit_pathol_ce", w.implicit_pathol_ce)
        add("implicit_pathol_dice", w.implicit_pathol_dice)
    return names, wd


class LossScaler:
    """torch.cuda.amp.GradScaler's state machine (scripts/train.py:164, Trainer/engine.py:139-147): the loss is
    multiplied by `scale`, gradients are divided by it before clipping, a step with a non-finite gradient is skipped and
    halves the scale, `growth_interval` clean steps in a row double it."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        self.scale = float(init_scale) if enabled else 1.0
        self.growth_factor, self.backoff_factor = float(growth_factor), float(backoff_factor)
        self.growth_interval = int(growth_interval)
        self.enabled = bool(enabled)
        self._good = 0

    def update(self, found_inf):
        if not self.enabled:
            return
        if found_inf:
            self.scale *= self.backoff_factor
            self._good = 0
        else:
            self._good += 1
            if self._good == self.growth_interval:
                self.scale *= self.growth_factor
                self._good = 0


def cosine_scheduler(base_value, final_value, epochs, niter_per_ep, warmup_epochs=0, start_warmup_value=0.0):
    """utils/misc.py:1265-1276: linear warm-up then half a cosine, one value per iteration."""
    import numpy as np
    warm_iters = warmup_epochs * niter_per_ep
    warm = np.linspace(start_warmup_value, base_value, warm_iters) if warmup_epochs > 0 else np.array([])
    it = np.arange(epochs * niter_per_ep - warm_iters)
    sched = final_value + 0.5 * (base_value - final_value) * (1 + np.cos(np.pi * it / len(it)))
    return np.concatenate((warm, sched))


def multistep_scheduler(base_value, lr_drops, epochs, niter_per_ep, warmup_epochs=0, start_warmup_value=0.0, gamma=0.1):
    """utils/misc.py:1251-1262 (the default lr schedule of cfgs/trainer/default_train.yaml).  Kept quirk: the milestones
    index the array WITHOUT its warm-up part, so every drop lands warmup_epochs later than lr_drops says."""
    import numpy as np
    warm_iters = warmup_epochs * niter_per_ep
    warm = np.linspace(start_warmup_value, base_value, warm_iters) if warmup_epochs > 0 else np.array([])
    sched = np.ones(epochs * niter_per_ep - warm_iters) * base_value
    for m in lr_drops:
        sched[m * niter_per_ep:] *= gamma
    return np.concatenate((warm, sched))


def allreduce_mean_(grads, group=None, events=None):
    """DDP's gradient averaging (scripts/train.py:153-158) as ONE flat all-reduce over all parameters: xGMI rings are
    per-link bound, so a single ~100 MB bucket beats many small ones.  In place; no-op without a process group.
    events: a list that receives (start, end) device events around the collective (it is not overlapped with anything: what
    it takes is what it exposes; bench.py's config 5 block reports it)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return grads
    keys = list(grads.keys())
    flat = torch.cat([grads[k].reshape(-1) for k in keys])
    if events is not None and flat.is_cuda:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    if events is not None and flat.is_cuda:
        e1.record()
        del events[:]
        events.extend([e0, e1, flat.numel() * flat.element_size()])
    flat /= dist.get_world_size(group)
    off = 0
    for k in keys:
        n = grads[k].numel()
        grads[k].copy_(flat[off:off + n].view_as(grads[k]))
        off += n
    return grads


def reduce_losses_(loss_dict, touched, loss_names, tasks, loss_weights, device, group=None):
    """utils.reduce_dict of the loss dictionary over the ranks (Trainer/engine.py:124-130) and, in the same collective, the
    union of the heads some rank's loss reached (DDP's find_unused_parameters=True).  loss_names / tasks give the fixed
    layout: a rank may lack a loss another one has.  Returns (loss_dict, total, touched) as every rank now sees them."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    keys = list(loss_names)
    # gloo reduces on the host, RCCL on the device
    rdev = device if dist.get_backend(group) == "nccl" else torch.device("cpu")
    t = torch.tensor([loss_dict.get("loss_" + k, 0.0) for k in keys] +
                     [1.0 if ("loss_" + k) in loss_dict else 0.0 for k in keys] +
                     [1.0 if task in touched else 0.0 for task in tasks], dtype=torch.float64, device=rdev)
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    t = t.cpu().tolist()
    nk = len(keys)
    loss_dict = OrderedDict(("loss_" + k, t[i] / world) for i, k in enumerate(keys) if t[nk + i] > 0)
    total = sum(v * loss_weights.get(k, 0.0) for k, v in loss_dict.items() if k in loss_weights)
    return loss_dict, total, {task for j, task in enumerate(tasks) if t[2 * nk + j] > 0}


class _Sink:
    """What the backward pass sees of a GradStore (engine.grad_sink): `out` hands a kernel its slot, `done` adds the
    earlier samples' sum for that slot and counts its bucket down."""

    def __init__(self, store, partial, row_of):
        self.store, self.partial, self.row_of = store, partial, row_of

    def out(self, name, shape):
        return self.store.out(name, shape)

    def done(self, name):
        if self.partial is not None:
            v = self.store.views[name]
            if name in ("head.weight_all", "head.bias_all"):
                kind = "weight" if name == "head.weight_all" else "bias"
                for task, (r0, n) in self.row_of.items():
                    v[r0:r0 + n].add_(self.partial["head.final_conv_%s.%s" % (task, kind)])
            else:
                v.add_(self.partial[name])
        self.store.done(name)


class GradStore:
    """All parameter gradients of one iteration in ONE persistent flat fp32 buffer, laid out in the order the backward pass
    completes them (heads, decoders last to first, encoders last to first), cut into a few buckets of about equal bytes.
    The weight-gradient kernels write straight into their slot (`out`), `done` counts a bucket down, and a bucket whose last
    tensor is complete is all-reduced on a communication stream while the backward pass goes on -- DDP's bucketed overlap
    (scripts/train.py:153-158) without DDP's copies: no torch.cat of 252 tensors in front of the collective and no 252
    copy_ launches behind it.  The optimiser reads the slots in place; the mean's 1 / world is folded into
    its gradient scale.  xGMI rings are per-link bound, so buckets are large (default 6 of ~180 MB for the 264 M-parameter
    net; BFM_GRAD_BUCKETS).  Every rank issues the same collectives in the same order whatever its loss turns out to be; an
    iteration that is skipped afterwards only wastes them."""

    def __init__(self, named_shapes, device, n_buckets=None):
        self.device = device
        nb = int(os.environ.get("BFM_GRAD_BUCKETS", "6")) if n_buckets is None else int(n_buckets)
        self.names = [n for n, _ in named_shapes]
        sizes = [int(np.prod(s)) for _, s in named_shapes]
        offs = np.concatenate([[0], np.cumsum([(n + 3) // 4 * 4 for n in sizes])])      # 16-byte aligned slots
        self.total = int(offs[-1])
        self.flat = torch.zeros(self.total, dtype=torch.float32, device=device)
        self.views = OrderedDict()
        for (name, shape), o, n in zip(named_shapes, offs[:-1], sizes):
            self.views[name] = self.flat[int(o):int(o) + n].view(tuple(shape))
        # bucket b = tensors [first[b], first[b + 1]): cut where the running byte count passes b / nb of the total
        nb = max(1, min(nb, len(self.names)))
        self.first = [0]
        for i in range(1, len(self.names)):
            if len(self.first) < nb and offs[i] >= self.total * len(self.first) / nb:
                self.first.append(i)
        self.first.append(len(self.names))
        self.range = [(int(offs[self.first[b]]), int(offs[self.first[b + 1]])) for b in range(len(self.first) - 1)]
        self.bucket_of = {}
        for b in range(len(self.first) - 1):
            for i in range(self.first[b], self.first[b + 1]):
                self.bucket_of[self.names[i]] = b
        self.comm = torch.cuda.Stream(device=device) if torch.device(device).type == "cuda" else None
        self.group = None
        self.works = []
        self.pending = []
        self.launched = []
        self.events = None
        self.active = False

    def begin(self, group=None):
        import torch.distributed as dist
        self.group = group
        self.world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
        self.pending = [self.first[b + 1] - self.first[b] for b in range(len(self.range))]
        self.launched = [False] * len(self.range)
        self.works = []
        self.events = None
        self.active = True

    def out(self, name, shape):
        v = self.views[name]
        if tuple(v.shape) != tuple(shape):
            raise L.BfmError("gradient slot %s has shape %s, the kernel writes %s" % (name, tuple(v.shape), tuple(shape)))
        return v

    def done(self, name):
        """The kernel that completes `name` has been enqueued on the current stream."""
        b = self.bucket_of[name]
        self.pending[b] -= 1
        if self.pending[b] == 0:
            self._launch(b)

    def _launch(self, b):
        if self.launched[b]:
            return
        self.launched[b] = True
        if self.world <= 1:
            return
        import torch.distributed as dist
        lo, hi = self.range[b]
        seg = self.flat[lo:hi]
        if self.comm is None:
            self.works.append(dist.all_reduce(seg, op=dist.ReduceOp.SUM, group=self.group, async_op=True))
            return
        ev = torch.cuda.Event()
        ev.record()                                                   # the bucket's last producer, on the compute stream
        with torch.cuda.stream(self.comm):
            self.comm.wait_event(ev)
            self.works.append(dist.all_reduce(seg, op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def finish(self):
        """Backward is over: launch what is left (a slot nobody wrote is all-reduced as the zeros it holds), then make the
        compute stream wait for the collectives.  events = (backward end, collectives end, bytes): the time between the two
        is what the all-reduce EXPOSES (bench.py: config5.allreduce_exposed_ms)."""
        for b in range(len(self.range)):
            if not self.launched[b]:
                self._launch(b)
        self.active = False
        if self.world <= 1:
            return
        if self.comm is None:
            for w in self.works:
                w.wait()
            return
        main = torch.cuda.current_stream(self.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(main)
        with torch.cuda.stream(self.comm):
            for w in self.works:
                w.wait()
            e1.record(self.comm)
        main.wait_event(e1)
        self.events = (e0, e1, self.total * 4)
        self.works = []


# bfm_optim_tensor_t (include/brainfm_hip.h), the one descriptor of every multi-tensor launch: s0 = exp_avg | momentum_buffer
# | mu, s1 = exp_avg_sq (Adam and AdamW, else 0); q and wd are LARS' per-tensor trust ratio and decay.
_OPT_DESC = np.dtype([("p", "<u8"), ("g", "<u8"), ("s0", "<u8"), ("s1", "<u8"), ("n", "<i8"), ("grad_scale", "<f4"),
                      ("bias1", "<f4"), ("bias2_sqrt", "<f4"), ("first_chunk", "<i4"), ("q", "<f4"), ("wd", "<f4")])
assert _OPT_DESC.itemsize == 64
# how a checkpoint's optimiser state names its buffers, per kind (torch.optim.Adam / AdamW / SGD, utils.LARS)
_STATE_KEYS = {"adam": ("exp_avg", "exp_avg_sq"), "adamw": ("exp_avg", "exp_avg_sq"), "sgd": ("momentum_buffer",),
               "lars": ("mu",)}


def lars_trust_ratio(sum_gg, sum_pp, sum_pg, coef, weight_decay, eta):
    """q of utils/misc.py:1302-1309 from the three sums of bfm_lars_sums_multi, in float64: |dp|^2 of dp = coef g + wd p is
    coef^2 sum g^2 + 2 coef wd sum p g + wd^2 sum p^2.  q = eta |p| / |dp| where both norms are positive, else 1."""
    dp2 = coef * coef * sum_gg + 2.0 * coef * weight_decay * sum_pg + weight_decay * weight_decay * sum_pp
    pn, un = math.sqrt(max(sum_pp, 0.0)), math.sqrt(max(dp2, 0.0))
    return eta * pn / un if (pn > 0.0 and un > 0.0) else 1.0


class TrainStep:
    """Parameters live in the engine (layer .w_raw / .gamma / .beta) and the tail (head_w / head_b); `step` updates
    them in place and drops the packed-weight caches so that the next forward repacks.

    trainable='head' is head-only fine-tuning on a frozen backbone (train_args.freeze_feat; the reference sets
    requires_grad = False on the backbone and get_params_groups, scripts/train.py:46-53, leaves it out of the optimiser):
    the backbone runs on the inference kernels without a tape, the backward pass ends at the heads (bfm_head_wgrad: no
    feature gradient), gradients, optimiser state, clip norms and the scaler's check cover the `head.` tensors alone, and
    nothing of the backbone is touched or repacked.  One rank only."""
    hidden = ()                 # the hidden head layers' records (steps without a task head have none)
    trainable = "all"

    def __init__(self, engine, tail, loss_names, loss_weights, weights_ce, all_samples, max_surf_distance=3.0,
                 bias_field_log_type="l2", lr=1e-4, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, clip_max_norm=0.0,
                 scaler=None, age_head=None, optimizer="adamw", trainable="all"):
        trainable_names((), trainable)                     # an unknown value raises here
        self.trainable = trainable
        if "contrastive" in loss_names:
            # the reference never mixes it with other losses (get_criterion returns early, Trainer/models/__init__.py:169-178)
            raise L.BfmError("loss 'contrastive' is the head-less pre-training mode: use ContrastiveStep, not TrainStep")
        bad = [n for n in loss_names if n not in SUPPORTED]
        if bad:
            raise L.BfmError("losses outside the HIP training path: %s" % bad)
        self.tail = tail
        # hidden head layers (task_f_maps longer than one; engine._HeadLayer records the tail carries): trained in place
        self.hidden = list(getattr(tail, "hidden", ()))
        if self.hidden and age_head is not None:
            raise L.BfmError("task_f_maps with hidden head layers and the pooled scalar head together are not built")
        self._init_optim(engine, loss_names, loss_weights, lr, weight_decay, betas, eps, clip_max_norm, scaler, optimizer)
        self.all_samples = float(all_samples)
        self.max_dist = float(max_surf_distance)
        self.bias_l2 = 1 if bias_field_log_type == "l2" else 0
        self.wce = torch.as_tensor(weights_ce).to(device=self.dev, dtype=torch.float32).contiguous()
        nseg = tail.desc.n_seg
        self._ws_bytes = (self.lib.bfm_loss_workspace(max(nseg, 1)), self.lib.bfm_loss_l1_multi_workspace())
        # the pooled scalar head (models.AgeHead, e.g. TaskHead.age_head()): the step trains its own copy of the parameters
        if age_head is not None:
            prm = OrderedDict((k, v.detach().to(device=self.dev, dtype=torch.float32).clone().contiguous())
                              for k, v in age_head.params.items())
            self.age = M.AgeHead(prm, age_head.c_feat, age_head.n_flat, self.dev)
        if "age" in self.loss_names and self.age is None:
            raise L.BfmError("loss 'age' needs the pooled scalar head (TrainStep(..., age_head=model.head.age_head()))")
        if any(n in REG_REGULARISERS for n in self.loss_names) and "registration" not in tail.row_of:
            raise L.BfmError("losses %s need the registration head" % [n for n in self.loss_names if n in REG_REGULARISERS])

    def _init_optim(self, engine, loss_names, loss_weights, lr, weight_decay, betas, eps, clip_max_norm, scaler,
                    optimizer="adamw"):
        """What every kind of step holds: the engine, the loss table, the optimiser's and the scaler's state, the lanes.
        optimizer: 'adam', 'adamw', 'sgd', 'lars' (Trainer/models/__init__.py:360-372), or what models.build_optimizer
        returned -- its betas / eps / momentum / eta then hold, and apply() / step() read lr and weight_decay from its
        param_groups[0] (the dictionary the loop of Trainer/engine.py:95-97 writes every iteration) when theirs are None."""
        spec = M.optimizer_spec(optimizer)
        self.opt_kind = spec.kind
        self.opt_spec = spec if spec is optimizer else None
        if self.opt_spec is not None:
            betas, eps = tuple(spec.betas), spec.eps
        self.momentum, self.eta = float(spec.momentum), float(spec.eta)
        self.eng = engine
        self.lib = engine.lib
        self.dev = engine.device
        self.loss_names = list(loss_names)
        self.loss_weights = dict(loss_weights)
        self.lr, self.wd, self.betas, self.eps, self.clip = float(lr), float(weight_decay), betas, float(eps), float(clip_max_norm)
        self.scaler = scaler if scaler is not None else LossScaler(enabled=False)
        self.t = 0                                          # iterations stepped so far
        self.steps = {}                                     # per-parameter AdamW step counts (a head without an active
                                                            # loss is not stepped: its .grad is None in the reference)
        self._touched_heads = set()
        self._active_rows = set()
        self.state = {}                                   # name -> (m, v) | (momentum buffer,) | (mu,)
        self.age = None
        self.sample_lanes = max(1, int(os.environ.get("BFM_TRAIN_LANES", "2")))
        self._lane_streams = []
        self._lane = 0
        self._ws_lane = {}

    @property
    def _ws(self):
        return self._lane_ws()[0]

    @property
    def _ws_multi(self):
        return self._lane_ws()[1]

    def _lane_ws(self):
        """Reduction scratch of the loss kernels, one set per sample lane."""
        w = self._ws_lane.get(self._lane)
        if w is None:
            w = self._ws_lane[self._lane] = tuple(torch.empty(b, dtype=torch.uint8, device=self.dev) for b in self._ws_bytes)
        return w

    # ------------------------------------------------------------------ parameters
    def parameters(self):
        """{reference parameter name: device tensor (views for the heads)}."""
        p = OrderedDict()
        for pair in self.eng.enc + self.eng.dec:
            for ly in pair:
                p[ly.name + ".groupnorm.weight"] = ly.gamma
                p[ly.name + ".groupnorm.bias"] = ly.beta
                p[ly.name + ".conv.weight"] = ly.w_raw
        for hl in getattr(self, "hidden", ()):                     # registered in front of the 1x1x1 heads (head.py:27-31)
            p[hl.name + ".weight"] = hl.w_raw
            p[hl.name + ".bias"] = hl.bias
        for task, (r0, n) in self.tail.row_of.items():
            p["head.final_conv_%s.weight" % task] = self.tail.head_w[r0:r0 + n]
            p["head.final_conv_%s.bias" % task] = self.tail.head_b[r0:r0 + n]
        if self.age is not None:                                   # registered after the dense heads (head.py:38-48)
            for k, v in self.age.params.items():
                p["head." + k] = v
        return p

    def grad_store(self):
        """The persistent gradient buffer (GradStore), slots in the order the backward pass completes them."""
        if self.trainable != "all":
            raise L.BfmError("TrainStep(trainable=%r) runs on one rank: it has no bucketed gradient all-reduce" % self.trainable)
        st = self.__dict__.get("_grad_store")
        if st is None:
            named = [("head.weight_all", (self.tail.n_out, self.tail.c_feat)), ("head.bias_all", (self.tail.n_out,))]
            if self.age is not None:                               # the pooled head's backward ends before the backbone's
                named += [("head." + k, tuple(v.shape)) for k, v in self.age.params.items()]
            for hl in reversed(getattr(self, "hidden", ())):      # backward.backward_head_layer: the bias first
                named.append((hl.name + ".bias", tuple(hl.bias.shape)))
                named.append((hl.name + ".weight", tuple(hl.w_raw.shape)))
            for pair in list(reversed(self.eng.dec)) + list(reversed(self.eng.enc)):
                for ly in reversed(pair):
                    named.append((ly.name + ".conv.weight", tuple(ly.w_raw.shape)))
                    named.append((ly.name + ".groupnorm.weight", tuple(ly.gamma.shape)))
                    named.append((ly.name + ".groupnorm.bias", tuple(ly.beta.shape)))
            st = self._grad_store = GradStore(named, self.dev)
        return st

    def _weights_changed(self):
        """Right after the optimiser: every packed form a layer holds (forward variants, skip half, up-folded, transposed
        data-gradient layer) is rebuilt in place, so the next pass packs nothing lazily.  A step on a frozen backbone
        rebuilds the hidden head layers' forms alone and leaves every backbone layer as it is: its optimiser cannot have
        moved one."""
        self.eng.repack_all(refresh=BW.refresh_dgrad, backbone=self.trainable == "all")
        hw = torch.zeros(1, dtype=torch.float32, device=self.dev)
        L.check(self.lib.bfm_absmax_f32(L.ptr(self.tail.head_w), 1, self.tail.head_w.numel(), self.tail.head_w.numel(),
                                        L.ptr(hw), L.stream_ptr()), "absmax head_w")
        self.tail.desc.head_wmax = float(hw.item())

    # ------------------------------------------------------------------ checkpoints (scripts/train.py:205-214)
    def _ref_shape(self, name, t):
        if name.startswith("head.final_conv_") and name.endswith(".weight"):
            return tuple(t.shape) + (1, 1, 1)                      # nn.Conv3d(C, n, 1) weight
        return tuple(t.shape)

    def state_dict(self):
        """The model's state_dict under the reference's names and shapes (CPU copies)."""
        return OrderedDict((k, v.detach().reshape(self._ref_shape(k, v)).cpu().clone()) for k, v in self.parameters().items())

    def optimizer_state_dict(self, lr=None, weight_decay=None):
        """state_dict() layout of this step's optimiser (torch.optim.AdamW / Adam / SGD, utils.LARS) for the single parameter
        group of scripts/train.py:46-53 (parameters in model.named_parameters() order == self.parameters() order).  On a
        frozen backbone the group indexes the trainable tensors alone, in that order: get_params_groups skips a parameter
        with requires_grad = False, so torch numbers what is left."""
        lr, wd = self._hyper(lr, weight_decay)
        params = self.parameters()
        params = OrderedDict((k, params[k]) for k in trainable_names(list(params), self.trainable))
        state = {}
        for i, (k, p) in enumerate(params.items()):
            if k in self.state:
                shp = self._ref_shape(k, p)
                st = {key: buf.reshape(shp).cpu().clone() for key, buf in zip(_STATE_KEYS[self.opt_kind], self.state[k])}
                if self.opt_kind in ("adam", "adamw"):
                    st = dict(step=torch.tensor(float(self.steps.get(k, self.t))), **st)
                state[i] = st
        group = self._param_group(lr, wd)
        group["params"] = list(range(len(params)))
        return {"state": state, "param_groups": [group]}

    def _hyper(self, lr=None, weight_decay=None):
        """(lr, weight_decay) of this call: the arguments, else the spec's param group, else the constructor's."""
        group = self.opt_spec.param_groups[0] if self.opt_spec is not None else {}
        lr = group.get("lr", self.lr) if lr is None else lr
        wd = group.get("weight_decay", self.wd) if weight_decay is None else weight_decay
        return float(lr), float(wd)

    def _param_group(self, lr, wd):
        """The optimiser's param group without 'params'.  AdamW's is spelled out (the checkpoints written so far hold these
        keys, whatever the installed torch writes); Adam's and SGD's keys are read off a throw-away instance of the installed
        torch; LARS' are those of utils/misc.py:1283-1289."""
        if self.opt_kind == "adamw":
            return {"lr": lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": wd, "amsgrad": False,
                    "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None}
        if self.opt_kind == "lars":
            return {"lr": lr, "weight_decay": wd, "momentum": self.momentum, "eta": self.eta, "weight_decay_filter": None,
                    "lars_adaptation_filter": None}
        dummy = [torch.nn.Parameter(torch.zeros(1))]
        opt = torch.optim.Adam(dummy) if self.opt_kind == "adam" else torch.optim.SGD(dummy, lr=0.0, momentum=self.momentum)
        group = dict(opt.state_dict()["param_groups"][0])
        group.update(lr=lr, weight_decay=wd)
        if self.opt_kind == "adam":
            group.update(betas=tuple(self.betas), eps=self.eps)
        return group

    def save_checkpoint(self, path, epoch=0, **extra):
        """torch.save of {'model', 'optimizer', 'epoch', ...}: what utils.save_on_master writes in scripts/train.py, and
        what brainfm_amd.models.load_checkpoint / the reference's load_checkpoint read back."""
        ckp = {"model": self.state_dict(), "optimizer": self.optimizer_state_dict(), "epoch": int(epoch),
               "scaler_scale": self.scaler.scale, "optimizer_kind": self.opt_kind, "trainable": self.trainable}
        ckp.update(extra)
        torch.save(ckp, path)

    def load_checkpoint(self, path):
        """Parameters (matched by name suffix, as utils/checkpoint.py:558-571) and the optimiser's buffers back into the
        engine.  Optimiser state of another kind than this step's raises: 'optimizer_kind' decides, or the state's keys for a
        checkpoint the reference wrote (exp_avg is never read as a momentum buffer).  So does a checkpoint whose 'trainable'
        entry (absent: 'all') is not this step's: its optimiser state numbers another list of tensors."""
        ckp = M.read_checkpoint_file(path)
        wrote = ckp.get("trainable", "all") if isinstance(ckp, dict) else "all"
        if wrote != self.trainable:
            raise L.BfmError("checkpoint %s was written by a step with trainable=%r; this step has trainable=%r and does not "
                             "renumber its optimiser state" % (path, wrote, self.trainable))
        opt = ckp.get("optimizer")
        if opt and opt.get("state"):
            keys = set().union(*(set(st.keys()) for st in opt["state"].values()))
            found = ckp.get("optimizer_kind")
            if found is None:
                found = next((k_ for k_ in ("adamw", "sgd", "lars") if set(_STATE_KEYS[k_]) <= keys), None)
                same = found is not None and _STATE_KEYS[found] == _STATE_KEYS[self.opt_kind]
                found = "adam or adamw" if found == "adamw" else found      # their states look alike
            else:
                same = found == self.opt_kind and set(_STATE_KEYS[self.opt_kind]) <= keys
            if not same:
                raise L.BfmError("checkpoint %s holds the state of optimiser %r (keys %s); this step runs %r and does not "
                                 "reinterpret it" % (path, found, sorted(keys), self.opt_kind))
            if self.opt_kind != "adamw":
                for g in opt.get("param_groups", ()):
                    for k_, inert in M._OPTIMIZER_UNBUILT.items():
                        if g.get(k_) not in (inert, None):
                            raise L.BfmError("checkpoint %s was written with %s=%r, which the HIP %s step does not build"
                                             % (path, k_, g.get(k_), self.opt_kind))
        key = next((k for k in ckp if "model" in k), None)
        sd = ckp[key] if key is not None else ckp
        params = self.parameters()
        for k, p in params.items():
            cands = [lk for lk in sd if lk == k or lk.endswith("." + k) or k.endswith("." + lk)]
            if not cands:
                raise KeyError("checkpoint has no tensor matching '%s'" % k)
            src = sd[max(cands, key=len)]
            if src.numel() != p.numel():
                raise ValueError("shape mismatch for %s: %s vs %s" % (k, tuple(src.shape), tuple(p.shape)))
            p.copy_(src.reshape(p.shape).to(device=self.dev, dtype=torch.float32))
        if self.trainable != "all":
            self.eng.repack_all(refresh=BW.refresh_dgrad)      # the file's backbone replaced the frozen one, this once
        self._weights_changed()
        if opt and opt.get("state"):
            names = trainable_names(list(params.keys()), self.trainable)
            self.state = {}
            for i, st in opt["state"].items():
                k = names[int(i)]
                self.state[k] = tuple(st[key].reshape(-1).to(device=self.dev, dtype=torch.float32).contiguous()
                                      for key in _STATE_KEYS[self.opt_kind])
                # SGD and LARS keep no step count: a buffer means at least one step
                self.steps[k] = int(float(st["step"])) if "step" in st else 1
            self.t = max(self.steps.values()) if self.steps else 0
        if "scaler_scale" in ckp and self.scaler.enabled:
            self.scaler.scale = float(ckp["scaler_scale"])
        return ckp

    # ------------------------------------------------------------------ losses
    def _col(self, task, j=0):
        r0, n = self.tail.row_of[task]
        if j >= n:
            raise L.BfmError("head '%s' has %d channels" % (task, n))
        return r0 + j

    def _t(self, x, shape_tail):
        x = torch.as_tensor(x).to(device=self.dev, dtype=torch.float32).contiguous()
        if tuple(x.shape[-3:]) != tuple(shape_tail):
            raise L.BfmError("target of shape %s does not match the volume %s" % (tuple(x.shape), tuple(shape_tail)))
        return x

    def _coef(self, name, scale):
        """What multiplies d loss_<name> / d raw: loss scale * weight / all_samples (0 without a weight)."""
        return scale * self.loss_weights.get("loss_" + name, 0.0) / self.all_samples

    def _issue_entries(self, entries, launch, what, vals, keep, distinct_cols=False):
        """Issue per-column loss entries (slot, col, target, weight, mask, clamp, l2, coef) in groups of at most 32, in order.
        launch(n, a, stage) calls the export on the group's ctypes arrays a.cols / l2 / clamp / coef / tg / wt / mk and the
        device pointer of an fp64 staging row, whose n values then go to the entries' slots of `vals`.
        distinct_cols: an entry whose column is already in the group waits for the next launch."""
        pending = list(entries)
        while pending:
            batch, rest, seen = [], [], set()
            for e in pending:
                if len(batch) == 32 or (distinct_cols and e[1] in seen):
                    rest.append(e)
                else:
                    seen.add(e[1])
                    batch.append(e)
            pending = rest
            n = len(batch)
            ptrs = lambda j: (C.c_void_p * n)(*[(e[j].data_ptr() if e[j] is not None else None) for e in batch])  # noqa: E731
            a = SimpleNamespace(
                cols=(C.c_int32 * n)(*[e[1] for e in batch]), tg=ptrs(2), wt=ptrs(3), mk=ptrs(4),
                clamp=(C.c_float * n)(*[e[5] for e in batch]), l2=(C.c_int32 * n)(*[e[6] for e in batch]),
                coef=(C.c_float * n)(*[e[7] for e in batch]))
            keep.extend(e[j] for j in (2, 3, 4) for e in batch)
            stage = torch.empty(n, dtype=torch.float64, device=self.dev)
            L.check(launch(n, a, L.ptr(stage)), what)
            idx = torch.tensor([e[0] for e in batch], dtype=torch.int64, device=self.dev)
            vals.index_copy_(0, idx, stage)

    def _sample_losses(self, raw, dims, target, sample, dRaw, vals, scale, rows=False):
        """Launch every loss of one sample; values land in `vals` (device fp64, one slot list per loss name).
        rows: raw / dRaw are (n_out, nvox) rows instead of channels-last (nvox, n_out)."""
        lib, st = self.lib, L.stream_ptr()
        D, H, W = dims
        nvox = D * H * W
        n_out = self.tail.n_out
        # element (column c, voxel v) of raw and dRaw at c * cs + v * vs: all a loss entry needs to know of the layout
        cs, vs = (raw.stride(0), 1) if rows else (1, n_out)
        pr, pd = L.ptr(raw), L.ptr(dRaw)
        ws, wsn = L.ptr(self._ws), self._ws.numel()
        wsm, wsmn = L.ptr(self._ws_multi), self._ws_multi.numel()
        slots = {}
        k = 0
        dense = []                                        # l1 / l2 entries (slot, col, target, weight, mask, clamp, l2, coef)
        grads_l1 = []                                     # gradient-L1 entries, the same tuple (no mask, clamp or l2)
        keep = []                                         # tensors the deferred launch reads
        active = set()                                    # head rows some loss of this sample differentiates
        pathol_done = False

        def slot(name, n=1):
            nonlocal k
            slots.setdefault(name, []).append((k, n))
            k += n
            return C.c_void_p(vals.data_ptr() + 8 * (k - n))

        def entry(name, co, tgt, wt=None, mask=None, clampv=0.0, l2=0, coef=0.0):
            slot(name)
            active.add(co)
            (grads_l1 if name.endswith("_grad") else dense).append((k - 1, co, tgt, wt, mask, clampv, l2, coef))

        for name in self.loss_names:
            coef = self._coef(name, scale)
            if name in IMAGE_KEYS or (name.endswith("_grad") and name[:-5] in IMAGE_KEYS) or name in ("SR", "SR_grad"):
                key = name[:-5] if name.endswith("_grad") else name
                if key == "SR":
                    head, tgt, wt = "high_res_residual", sample.get("high_res_residual"), None
                else:
                    head, tgt = key, target.get(key)
                    wt = (1.0 - self._t(target[key + "_DM"], dims)) if (key + "_DM") in target else None
                if tgt is None or head not in self.tail.row_of:
                    continue                                          # criterion.py:274-281: shape mismatch -> 0
                entry(name, self._col(head), self._t(tgt, dims), wt, coef=coef)
            elif name in ("distance", "surface", "registration", "registration_grad"):
                # criterion.py:175-185: loss_image / loss_image_grad of the whole multi-channel map (surface: 8 channels,
                # Trainer/models/__init__.py:103-106; its head has no processor, so no clamp)
                head = "registration" if name.startswith("registration") else name
                if head not in target or head not in self.tail.row_of:
                    continue
                nch = self.tail.row_of[head][1]
                tgt = self._t(target[head], dims).reshape(-1, D, H, W)
                if tgt.shape[0] != nch:
                    continue
                for j in range(nch):
                    entry(name, self._col(head, j), tgt[j], clampv=self.max_dist if name == "distance" else 0.0,
                          coef=coef / nch)
            elif name in REG_REGULARISERS:
                # criterion.py:187-191: SmoothnessLoss('l2') / HessianLoss('l2') of the raw registration output (no processor,
                # no target); value and coef * d/d(raw) in one launch pair, added into the registration rows of dRaw
                r0, nch = self.tail.row_of["registration"]
                active.update(range(r0, r0 + nch))
                wsr = torch.empty(lib.bfm_loss_reg_workspace(nch, D, H, W), dtype=torch.uint8, device=self.dev)
                keep.append(wsr)
                fn = lib.bfm_loss_reg_smooth if name == "registration_smooth" else lib.bfm_loss_reg_hessian
                L.check(fn(pr, r0 * cs, cs, vs, nch, D, H, W, coef, pd, slot(name), L.ptr(wsr), wsr.numel(), st),
                        "loss_" + name)
            elif name in ("pathol_ce", "pathol_dice"):
                # criterion.py:193-212 on sigmoid(raw) (PatholProcessor): both names of a sample in ONE bfm_loss_pathol call,
                # issued when the first of them comes up
                if pathol_done:
                    continue
                pathol_done = True
                if "pathology" not in target or "pathology" not in self.tail.row_of:
                    continue                                          # shape mismatch / no head -> 0, as the reference
                tgt = self._t(target["pathology"], dims).reshape(-1)
                if tgt.numel() != nvox:
                    continue
                co = self._col("pathology")
                active.add(co)
                on = [n_ for n_ in ("pathol_ce", "pathol_dice") if n_ in self.loss_names]
                p_ce, p_di = (slot(n_) if n_ in on else None for n_ in ("pathol_ce", "pathol_dice"))
                c_ce, c_di = (self._coef(n_, scale) if n_ in on else 0.0 for n_ in ("pathol_ce", "pathol_dice"))
                wsp = torch.empty(lib.bfm_loss_pathol_workspace(), dtype=torch.uint8, device=self.dev)
                keep.extend([tgt, wsp])
                L.check(lib.bfm_loss_pathol(pr, co * cs, vs, L.ptr(tgt), nvox, c_ce, c_di, pd, p_ce, p_di, L.ptr(wsp),
                                            wsp.numel(), st), "loss_pathol")
            elif name == "bias_field_log":
                if "bias_field_log" not in sample or "bias_field_log" not in self.tail.row_of:
                    continue
                mask = 1.0 - self._t(target["segmentation"], dims).reshape(-1, D, H, W)[0]
                entry(name, self._col("bias_field_log"), self._t(sample["bias_field_log"], dims), mask=mask, l2=self.bias_l2,
                      coef=coef)
            elif name in ("seg_ce", "seg_dice"):
                # CE and Dice share the softmax: one launch covers both names, at seg_ce's place in the order where it is on
                if name == "seg_dice" and "seg_ce" in self.loss_names:
                    continue
                r0, ns = self.tail.row_of["segmentation"]
                active.update(range(r0, r0 + ns))
                tgt = self._t(target["segmentation"], dims).reshape(ns, D, H, W)
                c_ce, c_di = (self._coef(n_, scale) if n_ in self.loss_names else 0.0 for n_ in ("seg_ce", "seg_dice"))
                P = torch.empty(nvox * ns, dtype=torch.float32, device=self.dev)     # in the layout of raw
                L.check(lib.bfm_loss_seg(pr, cs, vs, n_out, r0, ns, L.ptr(tgt), L.ptr(self.wce), L.ptr(self.wce), nvox, c_ce,
                                         c_di, L.ptr(P), pd, slot("seg", 1 + 2 * ns), ws, wsn, st), "loss_seg")
        # every l1 / l2 entry in one pass over raw per 32, then every gradient-L1 entry (distinct columns per launch: two
        # entries on one column would race on dRaw)
        self._issue_entries(dense, lambda n, a, stage: lib.bfm_loss_l1_multi(
            pr, cs, vs, n_out, nvox, n, a.cols, a.l2, a.clamp, a.coef, a.tg, a.wt, a.mk, pd, stage, wsm, wsmn, st),
            "loss_l1_multi", vals, keep)
        self._issue_entries(grads_l1, lambda n, a, stage: lib.bfm_loss_grad_l1_multi(
            pr, cs, vs, n_out, n, a.cols, a.coef, a.tg, a.wt, D, H, W, pd, stage, wsm, wsmn, st),
            "loss_grad_l1_multi", vals, keep, distinct_cols=True)
        self._keep = keep
        self._active_rows = active
        return slots, k

    def _finish_losses(self, per_sample, nvox):
        """Host side of SetMultiCriterion: fold channels / samples of the fp64 slots into {loss_<name>: value}."""
        out = OrderedDict()
        wdice = self.wce.double().cpu()
        for slots, vals in per_sample:
            v = vals.cpu()
            for name, lst in slots.items():
                if name == "seg":
                    (k0, n), = lst
                    ns = (n - 1) // 2
                    ce = float(v[k0]) / nvox
                    num, den = v[k0 + 1:k0 + 1 + ns], v[k0 + 1 + ns:k0 + 1 + 2 * ns]
                    dice = float((wdice * (1.0 - 2.0 * num / torch.clamp(den, min=1e-5))).sum())
                    if "seg_ce" in self.loss_names:
                        out["loss_seg_ce"] = out.get("loss_seg_ce", 0.0) + ce / self.all_samples
                    if "seg_dice" in self.loss_names:
                        out["loss_seg_dice"] = out.get("loss_seg_dice", 0.0) + dice / self.all_samples
                else:
                    val = sum(float(v[k0]) for k0, _ in lst) / len(lst)
                    out["loss_" + name] = out.get("loss_" + name, 0.0) + val / self.all_samples
        # keep the criterion's loss order
        return OrderedDict((("loss_" + n), out["loss_" + n]) for n in self.loss_names if ("loss_" + n) in out)

    # ------------------------------------------------------------------ forward + backward
    def _one_sample(self, x, target, sample, scale, x_cl=None):
        """Forward, losses and backward of one augmented sample on the current stream.  Returns (grads, slots, vals).
        x_cl: the network's channels-last input where it is not x itself (condition_inputs)."""
        ctx = self._sample_forward(x, x_cl)
        self._sample_criterion(ctx, target, sample, scale)
        return self._sample_backward(ctx, target, scale)

    def _sample_forward(self, x, x_cl=None):
        """Backbone and heads of one sample in training mode.  Returns the sample's context: tape, head outputs `raw`, the
        zeroed head-gradient buffer `dRaw` (rows: both are (n_out, nvox) rows, otherwise channels-last)."""
        eng, tail = self.eng, self.tail
        dims = tuple(x.shape[-3:])
        if x_cl is None:
            x_cl = eng.to_cl(x)
        elif tuple(x_cl.shape) != dims + (eng.in_channels,) or x_cl.dtype != torch.float32 or not x_cl.is_contiguous():
            raise L.BfmError("conditioned input %s %s: the network reads contiguous fp32 %s"
                             % (tuple(x_cl.shape), x_cl.dtype, dims + (eng.in_channels,)))
        if self.trainable == "head":
            feats, tape = eng.backbone_cl(x_cl, dims), None        # frozen: the inference path, nothing taped or kept
        else:
            feats, tape = BW.backbone_forward_train(eng, x_cl, dims)
        feat_last = feats[-1][0]
        head_in, hid_tape = feat_last, None
        if self.hidden:
            # F.normalize runs before the hidden layers (unet3d/model.py:207-208, head.py:53-55); the 1x1x1 heads then read
            # the last layer's output as it is
            hid_tape = []
            head_in, _ = eng.run_head_layers(self.hidden, feat_last, dims, tape=hid_tape)
        n_out, cf = tail.n_out, tail.c_feat
        # head outputs as rows of nvox values wherever the one-pass heads backward exists (64 features, <= 96 outputs,
        # <= 64 classes: every shipped head set); BFM_TRAIN_ROWS=0 keeps channels-last
        rows = (os.environ.get("BFM_TRAIN_ROWS", "1") != "0" and cf == 64 and n_out <= 96 and
                tail.row_of.get("segmentation", (0, 0))[1] <= 64)
        raw, fn = tail.run_raw(head_in, dims, want_feat=True, rows=rows, apply_hidden=False)
        if fn is None:
            fn = head_in
        dRaw = torch.zeros_like(raw)
        if tape is None:
            feats = feat_last = None                       # frozen: only fn (and the hidden layers' tape) is read again
        return dict(dims=dims, feats=feats, tape=tape, feat_last=feat_last, rows=rows, raw=raw, fn=fn, dRaw=dRaw,
                    hid_tape=hid_tape)

    def _sample_criterion(self, ctx, target, sample, scale):
        """Every loss of the sample: values into the context's fp64 slots, gradients added into its dRaw."""
        vals = torch.zeros(4 * len(self.loss_names) + 2 * self.tail.n_out + 8, dtype=torch.float64, device=self.dev)
        ctx["slots"], ctx["k_used"] = self._sample_losses(ctx["raw"], ctx["dims"], target, sample, ctx["dRaw"], vals, scale,
                                                          rows=ctx["rows"])
        ctx["vals"], ctx["active"], ctx["keep"] = vals, self._active_rows, self._keep

    def _sample_backward(self, ctx, target, scale, pre_heads=None, input_grad=None):
        """Backward of one sample from its head-gradient buffer.  Returns (grads, slots, vals).
        pre_heads: called with the context first; it may add into ctx['dRaw'] before the heads' backward reads it, and may
        run the sample's criterion itself (two-stage training: the stage-1 gradient through the mask).
        input_grad: a backward.InputGrad for the first layer."""
        if self.trainable == "head":
            if pre_heads is not None or input_grad is not None:
                raise L.BfmError("a step on a frozen backbone has no gradient in front of its heads to hand on (two-stage "
                                 "training is not built with freeze_feat)")
            return self._sample_backward_heads(ctx, target, scale)
        if pre_heads is not None:
            pre_heads(ctx)
        eng, tail, lib = self.eng, self.tail, self.lib
        dims, feats, tape, feat_last, rows = ctx["dims"], ctx["feats"], ctx["tape"], ctx["feat_last"], ctx["rows"]
        fn, dRaw, slots, k_used, vals = ctx["fn"], ctx["dRaw"], ctx["slots"], ctx["k_used"], ctx["vals"]
        nvox = dims[0] * dims[1] * dims[2]
        n_out, cf = tail.n_out, tail.c_feat
        st = L.stream_ptr()
        age_tape = None
        if self.age is not None:
            _, age_tape = self.age.forward(fn, dims)
        sink = getattr(eng, "grad_sink", None)
        dW = sink.out("head.weight_all", (n_out, cf)) if sink is not None else torch.empty((n_out, cf), dtype=torch.float32, device=self.dev)
        db = sink.out("head.bias_all", (n_out,)) if sink is not None else torch.empty(n_out, dtype=torch.float32, device=self.dev)
        dFn = torch.empty((nvox, cf), dtype=torch.float32, device=self.dev)
        wsb = torch.empty(lib.bfm_head_bwd_workspace(n_out, cf, nvox), dtype=torch.uint8, device=self.dev)
        if rows:
            L.check(lib.bfm_head_bwd_rows(L.ptr(dRaw), nvox, L.ptr(fn), L.ptr(tail.head_w), n_out, cf, nvox, L.ptr(dW),
                                          L.ptr(db), L.ptr(dFn), L.ptr(wsb), wsb.numel(), st), "head_bwd_rows")
        else:
            L.check(lib.bfm_head_bwd(L.ptr(dRaw), L.ptr(fn), L.ptr(tail.head_w), n_out, cf, nvox, L.ptr(dW), L.ptr(db),
                                     L.ptr(dFn), L.ptr(wsb), wsb.numel(), st), "head_bwd")
        if sink is not None:
            sink.done("head.weight_all")
            sink.done("head.bias_all")
        age_grads = None
        if age_tape is not None:
            # its pooled gradient joins dFn after the dense heads' and before normalize_bwd
            age_grads = self._age_backward(age_tape, target, scale, slots, k_used, vals, dFn, sink)
        hid_grads = OrderedDict()
        for hl, x_in, x_bound, y in reversed(ctx.get("hid_tape") or []):
            # the hidden layers, last to first: dFn is the gradient of the layer's output on the way in, of its input after
            dX, gr = BW.backward_head_layer(eng, hl, x_in, x_bound, y, dFn.view(dims + (hl.cout,)), dims)
            hid_grads.update(gr)
            dFn, cf = dX.reshape(nvox, hl.cin), hl.cin
        if eng.unit_feat:
            dfeat = torch.empty_like(dFn)
            L.check(lib.bfm_normalize_bwd(L.ptr(feat_last), L.ptr(dFn), cf, nvox, 1e-12, L.ptr(dfeat), st), "normalize_bwd")
        else:
            dfeat = dFn
        g = BW.backbone_backward(eng, tape, [None] * (len(feats) - 1) + [dfeat.view(dims + (cf,))], input_grad=input_grad)
        for task, (r0, n) in tail.row_of.items():
            g["head.final_conv_%s.weight" % task] = dW[r0:r0 + n]
            g["head.final_conv_%s.bias" % task] = db[r0:r0 + n]
        if age_grads is not None:
            g.update(age_grads)
        g.update(hid_grads)
        # heads no loss of this sample reached: the reference leaves their .grad None (the all-zero rows above only keep
        # the gradient dictionary's layout fixed for the flat all-reduce); loss_and_grads collects who was reached
        self._touched_heads.update(task for task, (r0, n) in tail.row_of.items()
                                   if any(r in ctx["active"] for r in range(r0, r0 + n)))
        return g, slots, vals

    def _age_backward(self, age_tape, target, scale, slots, k_used, vals, dFn, sink=None):
        """criterion.py loss_age of one sample and the pooled head's backward: the loss value into the sample's next fp64
        slot, the parameter gradients returned as {name: tensor}, the gradient of the normalised feature ADDED into dFn."""
        age_t = self._age_target(target)
        on = "age" in self.loss_names and age_t is not None
        coef = self._coef("age", scale) if on else 0.0
        loss_ptr = None
        if on:
            slots["age"] = [(k_used, 1)]
            loss_ptr = C.c_void_p(vals.data_ptr() + 8 * k_used)
            self._touched_heads.add("age")
        age_grads = OrderedDict()
        for k_, v_ in self.age.params.items():
            name = "head." + k_
            age_grads[name] = (sink.out(name, tuple(v_.shape)) if sink is not None else
                               torch.empty(v_.shape, dtype=torch.float32, device=self.dev))
        self.age.backward(age_tape, age_t if on else 0.0, coef, loss_ptr,
                          {k_[5:]: v_ for k_, v_ in age_grads.items()}, dFn)
        if sink is not None:
            for name in age_grads:
                sink.done(name)
        return age_grads

    def _sample_backward_heads(self, ctx, target, scale):
        """Backward of one sample on a frozen backbone: it ends where the last trainable tensor is reached.  Without hidden
        head layers that is the 1x1x1 heads themselves, whose dW / db come from bfm_head_wgrad[_rows] with no feature
        gradient formed; with hidden layers bfm_head_bwd[_rows] hands dFn down to the first of them, which forms no input
        gradient.  The pooled scalar head's backward adds into a scratch feature gradient nobody reads (hidden layers and the
        pooled head together never get here: __init__ refuses the pair)."""
        eng, tail, lib = self.eng, self.tail, self.lib
        dims, rows, fn, dRaw = ctx["dims"], ctx["rows"], ctx["fn"], ctx["dRaw"]
        slots, k_used, vals = ctx["slots"], ctx["k_used"], ctx["vals"]
        nvox = dims[0] * dims[1] * dims[2]
        n_out, cf = tail.n_out, tail.c_feat
        st = L.stream_ptr()
        dW = torch.empty((n_out, cf), dtype=torch.float32, device=self.dev)
        db = torch.empty(n_out, dtype=torch.float32, device=self.dev)
        hid_tape = ctx.get("hid_tape") or []
        g = OrderedDict()
        if hid_tape:
            dFn = torch.empty((nvox, cf), dtype=torch.float32, device=self.dev)
            wsb = torch.empty(lib.bfm_head_bwd_workspace(n_out, cf, nvox), dtype=torch.uint8, device=self.dev)
            if rows:
                L.check(lib.bfm_head_bwd_rows(L.ptr(dRaw), nvox, L.ptr(fn), L.ptr(tail.head_w), n_out, cf, nvox, L.ptr(dW),
                                              L.ptr(db), L.ptr(dFn), L.ptr(wsb), wsb.numel(), st), "head_bwd_rows")
            else:
                L.check(lib.bfm_head_bwd(L.ptr(dRaw), L.ptr(fn), L.ptr(tail.head_w), n_out, cf, nvox, L.ptr(dW), L.ptr(db),
                                         L.ptr(dFn), L.ptr(wsb), wsb.numel(), st), "head_bwd")
            for i, (hl, x_in, x_bound, y) in enumerate(reversed(hid_tape)):
                first = i + 1 == len(hid_tape)                 # the first hidden layer: nothing trainable in front of it
                dX, gr = BW.backward_head_layer(eng, hl, x_in, x_bound, y, dFn.view(dims + (hl.cout,)), dims,
                                                need_input_grad=not first)
                g.update(gr)
                if not first:
                    dFn = dX.reshape(nvox, hl.cin)
        else:
            wsb = torch.empty(lib.bfm_head_wgrad_workspace(n_out, cf, nvox), dtype=torch.uint8, device=self.dev)
            if rows:
                L.check(lib.bfm_head_wgrad_rows(L.ptr(dRaw), nvox, L.ptr(fn), n_out, cf, nvox, L.ptr(dW), L.ptr(db),
                                                L.ptr(wsb), wsb.numel(), st), "head_wgrad_rows")
            else:
                L.check(lib.bfm_head_wgrad(L.ptr(dRaw), L.ptr(fn), n_out, cf, nvox, L.ptr(dW), L.ptr(db), L.ptr(wsb),
                                           wsb.numel(), st), "head_wgrad")
        heads = OrderedDict()
        for task, (r0, n) in tail.row_of.items():
            heads["head.final_conv_%s.weight" % task] = dW[r0:r0 + n]
            heads["head.final_conv_%s.bias" % task] = db[r0:r0 + n]
        if self.age is not None:
            _, age_tape = self.age.forward(fn, dims)
            scratch = torch.zeros((nvox, cf), dtype=torch.float32, device=self.dev)
            heads.update(self._age_backward(age_tape, target, scale, slots, k_used, vals, scratch))
        heads.update(g)
        self._touched_heads.update(task for task, (r0, n) in tail.row_of.items()
                                   if any(r in ctx["active"] for r in range(r0, r0 + n)))
        return heads, slots, vals

    @staticmethod
    def _age_target(target):
        """target['age'] as a float (a float, a 0-d or a one-element tensor; datasets.py:678-679), or None."""
        a = target.get("age") if target is not None else None
        if a is None:
            return None
        if isinstance(a, torch.Tensor) or isinstance(a, np.ndarray):
            if (a.numel() if isinstance(a, torch.Tensor) else a.size) != 1:
                raise L.BfmError("target['age'] holds %d values; one training sample takes one age" % int(np.prod(a.shape)))
            return float(a.reshape(-1)[0])
        return float(a)

    @L.on_device(lambda self, *a, **k: self.dev)
    def loss_and_grads(self, xs, target, samples, cond=None):
        """xs: list of (1,C,D,H,W) inputs (one per augmented sample); target / samples as the reference's dicts
        (NCDHW tensors).  cond: what condition_inputs returned for these samples -- the network then reads those
        channels-last inputs (xs gives the sizes only; no permute of xs is made).  Returns (loss_dict, total, grads) with grads = d(scale * total)/d(parameter) summed over the
        samples in sample order (scale = the loss scaler's).
        With sample_lanes > 1 (default 2, BFM_TRAIN_LANES) consecutive samples run on separate streams from the second
        iteration on -- the packed weights are all in place by then (apply() rebuilds them eagerly) and the conv variants
        are tuned -- so that one sample's small kernels and launch tails hide under the other's convolutions, as the two
        tiles in flight of the inference path do; the gradients are still added on the caller's stream in sample order,
        so the result is the same bits."""
        eng = self.eng
        scale = self.scaler.scale
        n = len(xs)
        if cond is not None and len(cond) != n:
            raise L.BfmError("%d conditioned inputs for %d samples" % (len(cond), n))
        cls = list(cond) if cond is not None else [None] * n
        self._touched_heads = set()
        lanes = self.sample_lanes if (n > 1 and self.t >= 1) else 1
        nvox = None
        results = []
        # Where the gradients of the iteration are collected.  With more than one rank -- or with one sample lane -- the LAST
        # sample's kernels write straight into the persistent GradStore and start its buckets' all-reduces as each bucket
        # completes, i.e. under that sample's own backward pass; the earlier samples' sum (in sample order; a + b == b + a
        # bit for bit) is added slot by slot in front of each `done`.  That is DDP with gradient accumulation: no_sync for
        # all samples but the last.  The last sample then runs on the caller's stream after the lanes have joined.  One
        # rank with two lanes keeps every sample on the lanes (nothing to all-reduce).
        import torch.distributed as dist
        group = getattr(self, "_group", None)
        world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
        # only inside step(): a bare loss_and_grads() call must neither start collectives nor hand out views of a buffer the
        # next call overwrites
        use_store = (self.__dict__.pop("_store_next", False) and os.environ.get("BFM_GRAD_STORE", "1") != "0" and
                     (lanes <= 1 or world > 1))
        n_head = n - 1 if use_store else n                 # samples that go the ordinary way
        store = None
        if lanes <= 1 or n_head <= 1:
            for x, sample, x_cl in zip(xs[:n_head], samples[:n_head], cls):
                results.append(self._one_sample(x, target, sample, scale, x_cl) + (None,))
        else:
            main = torch.cuda.current_stream(self.dev)
            while len(self._lane_streams) < lanes:
                self._lane_streams.append(torch.cuda.Stream(device=self.dev))
            start = torch.cuda.Event()
            start.record(main)
            seen = eng.pack_count
            for i, (x, sample) in enumerate(zip(xs[:n_head], samples[:n_head])):
                k = i % lanes
                st = self._lane_streams[k]
                st.wait_event(start)
                if eng.pack_count != seen:                 # a packed form was created lazily while issuing an earlier
                    for r in results:                      # sample (new shape): later samples must see it finished
                        st.wait_event(r[3])
                    seen = eng.pack_count
                eng.lane, self._lane = k, k
                try:
                    with torch.cuda.stream(st):
                        g, slots, vals = self._one_sample(x, target, sample, scale, cls[i])
                        ev = torch.cuda.Event()
                        ev.record(st)
                finally:
                    eng.lane, self._lane = 0, 0
                results.append((g, slots, vals, ev))
            for g, slots, vals, ev in results:
                main.wait_event(ev)
                vals.record_stream(main)
                for t_ in g.values():
                    t_.record_stream(main)
        if use_store:
            store = self.grad_store()
            store.begin(group)
            part = None
            for r in results:
                part = r[0] if part is None else OrderedDict((k_, part[k_] + v_) for k_, v_ in r[0].items())
            eng.grad_sink = _Sink(store, part, self.tail.row_of)
            try:
                results.append(self._one_sample(xs[-1], target, samples[-1], scale, cls[-1]) + (None,))
            finally:
                eng.grad_sink = None
        grads = None
        per_sample = []
        self._store_live = store
        for x, (g, slots, vals, _) in zip(xs, results):
            nvox = x.shape[-3] * x.shape[-2] * x.shape[-1]
            per_sample.append((slots, vals))
            if store is not None:
                continue                                   # the last sample's slots already hold the sum
            if grads is None:
                grads = g
            else:
                for k_, v_ in g.items():
                    grads[k_] = grads[k_] + v_
        if store is not None:
            grads = results[-1][0]
        loss_dict = self._finish_losses(per_sample, nvox)
        total = sum(v * self.loss_weights.get(k, 0.0) for k, v in loss_dict.items() if k in self.loss_weights)
        return loss_dict, total, grads

    # ------------------------------------------------------------------ optimiser
    @L.on_device(lambda self, *a, **k: self.dev)
    def apply(self, grads, lr=None, weight_decay=None, grad_div=1.0):
        """unscale -> per-parameter clip (utils/misc.py:1329-1338) -> AdamW -> scaler.update.  Returns
        (stepped, norms): stepped is False when a non-finite gradient made the scaler skip the step.
        grad_div: the gradients hold a SUM over that many ranks (GradStore); the mean's division is folded into the unscale."""
        plan = self._measure(grads, grad_div)
        if plan["found_inf"]:
            self.scaler.update(True)
            return False, plan["norms"]
        self._update(plan, lr, weight_decay)
        self.scaler.update(False)
        return True, plan["norms"]

    def _measure(self, grads, grad_div=1.0):
        """First half of apply: the optimiser state of every parameter with a gradient, each gradient's norm (unscaled) and
        whether any is non-finite, from one launch over all tensors: bfm_grad_sumsq_multi, or for LARS bfm_lars_sums_multi,
        whose sum p^2 and sum p g the update's trust ratio needs.  Nothing is updated; the scaler is not touched."""
        lib, st = self.lib, L.stream_ptr()
        params = self.parameters()
        names = [k for k in params if k in grads]
        if self.trainable != "all":
            frozen = sorted(set(names) - set(trainable_names(names, self.trainable)))
            if frozen:
                raise L.BfmError("gradients for %d tensors a step with trainable=%r keeps frozen (%s, ...)"
                                 % (len(frozen), self.trainable, frozen[0]))
        for k in names:
            grads[k] = grads[k].contiguous()
            if not params[k].is_contiguous():
                raise L.BfmError("parameter %s is not contiguous" % k)
            if k not in self.state:
                self.state[k] = tuple(torch.zeros(params[k].numel(), dtype=torch.float32, device=self.dev)
                                      for _ in _STATE_KEYS[self.opt_kind])
        CH = 65536
        firsts, nchunks = self._chunks(names, params, CH)
        desc = np.zeros(len(names), dtype=_OPT_DESC)
        for i, k in enumerate(names):
            bufs = self.state[k]
            desc[i] = (params[k].data_ptr(), grads[k].data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr() if len(bufs) > 1 else 0,
                       params[k].numel(), 0.0, 1.0, 1.0, firsts[i], 1.0, 0.0)
        tdev = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(self.dev)
        lars = self.opt_kind == "lars"
        width = 3 if lars else 1
        sums = torch.zeros(len(names) * width, dtype=torch.float64, device=self.dev)
        flag = torch.zeros(1, dtype=torch.int32, device=self.dev)
        ws = torch.empty(nchunks * 3, dtype=torch.float64, device=self.dev) if lars else self._chunk_ws
        fn = lib.bfm_lars_sums_multi if lars else lib.bfm_grad_sumsq_multi
        L.check(fn(L.ptr(tdev), len(names), L.ptr(self._chunk_map), nchunks, CH, L.ptr(sums), L.ptr(flag), L.ptr(ws),
                   ws.numel() * 8, st), "lars_sums_multi" if lars else "grad_sumsq_multi")
        sums = sums.cpu().reshape(-1, width)
        inv = 1.0 / (self.scaler.scale * grad_div)
        found_inf = bool(flag.item())
        norms = [math.sqrt(v) * inv if math.isfinite(v) else float("inf") for v in sums[:, 0].tolist()]
        found_inf = found_inf or any(not math.isfinite(v) for v in norms)
        return dict(grads=grads, params=params, names=names, norms=norms, inv=inv, found_inf=found_inf, desc=desc, CH=CH,
                    sums3=sums if lars else None)

    def _chunks(self, names, params, CH):
        """The chunk map (device) of these tensors and each one's first chunk; kept while the sizes stay the same."""
        first, firsts, cmap = 0, [], []
        for i, k in enumerate(names):
            nch = (params[k].numel() + CH - 1) // CH
            firsts.append(first)
            cmap.extend([i] * nch)
            first += nch
        key = tuple(params[k].numel() for k in names)
        if getattr(self, "_chunk_key", None) != key:
            self._chunk_key = key
            self._chunk_map = torch.tensor(cmap, dtype=torch.int32, device=self.dev)
            self._chunk_ws = torch.empty(len(cmap), dtype=torch.float64, device=self.dev)
        return firsts, len(cmap)

    def _update(self, plan, lr=None, weight_decay=None):
        """Second half of apply: the per-tensor numbers (clip coefficient, bias corrections, LARS' decay and trust ratio) into
        the descriptors _measure prepared, one launch of the optimiser over all tensors, then the packed weights."""
        lr, wd = self._hyper(lr, weight_decay)
        params, names, norms, inv, desc, CH = (plan[k] for k in ("params", "names", "norms", "inv", "desc", "CH"))
        self.t += 1
        for i, (k, nrm) in enumerate(zip(names, norms)):
            self.steps[k] = self.steps.get(k, 0) + 1        # one step count per parameter, as torch's optimisers keep
            coef = inv
            if self.clip > 0:
                c = self.clip / (nrm + 1e-6)
                if c < 1:
                    coef *= c
            desc[i]["grad_scale"] = coef
            if self.opt_kind in ("adam", "adamw"):
                # bias corrections in float32 as bfm_adamw_step forms them (powf, sqrtf)
                desc[i]["bias1"] = np.float32(1.0) - np.power(np.float32(self.betas[0]), np.float32(self.steps[k]), dtype=np.float32)
                desc[i]["bias2_sqrt"] = np.sqrt(np.float32(1.0) - np.power(np.float32(self.betas[1]), np.float32(self.steps[k]),
                                                                          dtype=np.float32), dtype=np.float32)
            elif self.opt_kind == "lars" and len(self._ref_shape(k, params[k])) != 1:
                # utils/misc.py:1299-1310: decay and trust ratio for everything but the reference's 1-D parameters
                sgg, spp, spg = (float(v) for v in plan["sums3"][i])
                desc[i]["wd"] = wd
                desc[i]["q"] = lars_trust_ratio(sgg, spp, spg, float(np.float32(coef)), float(np.float32(wd)), self.eta)
        tdev = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(self.dev)
        fn, tail = {"adamw": (self.lib.bfm_adamw_step_multi, (lr, self.betas[0], self.betas[1], self.eps, wd)),
                    "adam": (self.lib.bfm_adam_step_multi, (lr, self.betas[0], self.betas[1], self.eps, wd)),
                    "sgd": (self.lib.bfm_sgd_step_multi, (lr, self.momentum, wd)),
                    "lars": (self.lib.bfm_lars_step_multi, (lr, self.momentum))}[self.opt_kind]
        L.check(fn(L.ptr(tdev), len(names), L.ptr(self._chunk_map), int(self._chunk_map.numel()), CH, *tail, L.stream_ptr()),
                self.opt_kind + "_step_multi")
        self._keep_desc = tdev
        self._weights_changed()

    @L.on_device(lambda self, *a, **k: self.dev)
    def step(self, xs, target, samples, lr=None, weight_decay=None, group=None, cond=None):
        """One full iteration (Trainer/engine.py:96-147; cond as loss_and_grads takes it).  Returns (loss_dict, total, stepped).  With more than one rank
        the loss dictionary is averaged over the ranks first (utils.reduce_dict, engine.py:124-130) and the skip decision
        is taken on that reduced value, so every rank skips -- or enters the gradient all-reduce -- together."""
        import torch.distributed as dist
        if self.trainable != "all":
            world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
            if group is not None or world > 1:
                raise L.BfmError("TrainStep(trainable=%r) is single-rank in this version: the step on a frozen backbone has "
                                 "no gradient all-reduce (group given or world size %d)" % (self.trainable, world))
        self._group = group
        self._store_next = self.trainable == "all"         # a frozen step never touches the GradStore
        loss_dict, total, grads = self.loss_and_grads(xs, target, samples, cond=cond)
        store = self.__dict__.pop("_store_live", None)
        touched = set(self._touched_heads)
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
        if store is not None:
            store.finish()                                     # every rank, whatever its loss: the collectives are in flight
            self.allreduce_events = list(store.events) if store.events else []
        if multi:
            tasks = list(self.tail.row_of.keys()) + (["age"] if self.age is not None else [])
            loss_dict, total, touched = reduce_losses_(loss_dict, touched, self.loss_names, tasks, self.loss_weights, self.dev,
                                                       group)
        if not math.isfinite(total):
            return loss_dict, total, False                     # engine.py:129-136: non-finite loss -> skip the iteration
        grad_div = 1.0
        if store is not None:
            grad_div = float(store.world)                      # the buckets hold the SUM over the ranks; the mean's 1 / world
        else:                                                  # goes into the optimiser's gradient scale
            allreduce_mean_(grads, group, self.__dict__.setdefault("allreduce_events", []))
        for task in self.tail.row_of:                          # heads nobody's loss reached: no gradient, no step
            if task not in touched:
                grads.pop("head.final_conv_%s.weight" % task, None)
                grads.pop("head.final_conv_%s.bias" % task, None)
        if self.age is not None and "age" not in touched:
            for k_ in self.age.params:
                grads.pop("head." + k_, None)
        stepped, _ = self.apply(grads, lr, weight_decay, grad_div=grad_div)
        return loss_dict, total, stepped


CONDITION_MODES = {frozenset(["mask"]): 0, frozenset(["flip"]): 1, frozenset(["mask", "flip"]): 2}


def condition_inputs(samples, target, condition, device=None, in_channels=None):
    """Trainer/engine.py:102-112 on the device, with the concat of joiner.py:178 and the channels-last repack, one
    bfm_condition_input launch per sample.  condition: 'mask', 'flip' or 'mask+flip' (train_args.condition).  Returns the
    per-sample (D,H,W,Cin) inputs of the conditioned network (channels: image, flipped image, mask) and leaves in
    samples[i]['input'] the masked image and in samples[i]['input_flip'] its flip, as the reference does.
    A target['pathology'] that is not a tensor (the generator stores 0. for a case without pathology) is an all-zero mask.
    in_channels: the engine's input channels; a condition that gives another count raises."""
    parts = frozenset(str(condition).split("+")) if condition else frozenset()
    if parts not in CONDITION_MODES:
        raise L.BfmError("unknown condition %r: 'mask', 'flip' or 'mask+flip'" % (condition,))
    mode = CONDITION_MODES[parts]
    cin = 3 if mode == 2 else 2
    if in_channels is not None and int(in_channels) != cin:
        raise L.BfmError("condition %r gives %d input channels, the network reads %d" % (condition, cin, in_channels))
    lib = L.load()
    out = []
    for sample in samples:
        x = sample["input"]
        dev = torch.device(device) if device is not None else x.device
        if dev.type != "cuda":
            raise L.BfmError("condition_inputs runs on a HIP device only; there is no CPU fallback in the product path")
        if x.dim() != 5 or x.shape[0] != 1 or x.shape[1] != 1:
            raise L.BfmError("expected a (1,1,D,H,W) input, got %s" % (tuple(x.shape),))
        D, H, W = (int(v) for v in x.shape[2:])
        with torch.cuda.device(dev):
            xd = x.to(device=dev, dtype=torch.float32).contiguous()
            p = None
            if mode != 1:
                p = target.get("pathology") if target is not None else None
                if isinstance(p, torch.Tensor):
                    if p.numel() != D * H * W:
                        raise L.BfmError("target['pathology'] %s does not match the input %s" % (tuple(p.shape), tuple(x.shape)))
                    p = p.to(device=dev, dtype=torch.float32).contiguous()
                else:
                    p = torch.zeros((D, H, W), dtype=torch.float32, device=dev)
            x_cl = torch.empty((D, H, W, cin), dtype=torch.float32, device=dev)
            masked = torch.empty_like(xd) if mode != 1 else None
            flipped = torch.empty_like(xd) if mode != 0 else None
            L.check(lib.bfm_condition_input(L.ptr(xd), L.ptr(p), mode, D, H, W, L.ptr(x_cl), L.ptr(masked), L.ptr(flipped),
                                            L.stream_ptr()), "condition_input")
        if masked is not None:
            sample["input"] = masked
        if flipped is not None:
            sample["input_flip"] = flipped
        out.append(x_cl)
    return out


def conditioned_train_step(gen_args, train_args, model, weights_ce, all_samples, **kw):
    """The TrainStep of a mask-conditioned model: (gen_args, train_args, model) as build_conditioned_model returns them
    (Trainer/models/__init__.py:423-437), losses as its get_criterion(..., exclude_keys=['pathology']) call builds them."""
    eng = model.backbone.engine(model.head)
    names, weights = criterion_losses(train_args, gen_args.tasks, exclude_keys=("pathology",))
    n_cond = len(str(train_args.condition).split("+"))
    if eng.in_channels != 1 + n_cond:
        raise L.BfmError("condition %r needs %d input channels, the backbone has %d"
                         % (train_args.condition, 1 + n_cond, eng.in_channels))
    kw.setdefault("max_surf_distance", float(gen_args.max_surf_distance))
    kw.setdefault("trainable", "head" if freeze_feat_of(train_args) else "all")
    return TrainStep(eng, model.head.tail(eng), names, weights, weights_ce, all_samples, **kw)


def train_step(gen_args, train_args, model, weights_ce, all_samples, **kw):
    """The TrainStep of the plain model: (gen_args, train_args, model) as build_model returns them, losses as its
    get_criterion(gen_args, train_args, gen_args.tasks) builds them.  train_args.freeze_feat (cfgs/trainer/default_train.yaml)
    gives trainable='head': the reference's requires_grad = False on the backbone."""
    eng = model.backbone.engine(model.head)
    names, weights = criterion_losses(train_args, gen_args.tasks)
    kw.setdefault("max_surf_distance", float(gen_args.max_surf_distance))
    kw.setdefault("trainable", "head" if freeze_feat_of(train_args) else "all")
    if model.head.age_task is not None:
        kw.setdefault("age_head", model.head.age_head())
    return TrainStep(eng, model.head.tail(eng), names, weights, weights_ce, all_samples, **kw)


class TwoStageTrainStep:
    """One joint iteration of the two-stage (pathology-robust, "inpainting") model: Trainer/engine.py:193-318,
    train_one_epoch_twostage, the loop that produces the two checkpoints evaluate_image_twostage loads.  Per sample
    (engine.py:230-253, without autocast as TrainStep):

        outputs_pathol = pathol_model(samples); PatholProcessor       stage-0 forward (tape kept), p = sigmoid(raw0)
        samples[i]['input_masked'] = input * (1 - p)                  bfm_twostage_train_input, with cond = target['pathology']
        outputs_task = task_model(samples, 'input_masked', cond)      stage-1 forward, its losses, its backward; the first
                                                                      layer's input gradient goes through the mask into
                                                                      stage 0's head gradient (backward.InputGrad)
        criterion(merge(outputs_task, outputs_pathol), ...)           pathol_ce / pathol_dice on stage 0's output
        backward                                                      stage-0 backward

    pathol_step / task_step: the TrainStep of each model (loss names pathol_* and all the others).  One LossScaler is shared;
    `step` takes one skip decision for both models and hands the same lr / weight decay / clip to both AdamW states, which
    is the arithmetic of the reference's single optimiser over both models' parameters.  The samples run one after the
    other on the caller's stream (no sample lanes, no GradStore overlap).  A target['pathology'] that is not a tensor is an
    all-zero mask, and the pathology losses are then absent (condition_inputs has the same rule)."""

    PREFIX = ("pathol.", "task.")

    def __init__(self, pathol_step, task_step, loss_names=None):
        s0, s1 = pathol_step, task_step
        for s_ in (s0, s1):
            if s_.trainable != "all":
                raise L.BfmError("TwoStageTrainStep takes steps with trainable='all': a frozen backbone (freeze_feat) is not "
                                 "built for the two coupled models")
            if torch.device(s_.dev).type != "cuda":
                raise L.BfmError("TwoStageTrainStep runs on a HIP device only; there is no CPU fallback in the product path")
        if torch.device(s0.dev) != torch.device(s1.dev):
            raise L.BfmError("the two stages live on %s and %s: one device trains both" % (s0.dev, s1.dev))
        if s0.eng.in_channels != 1 or s1.eng.in_channels != 2:
            raise L.BfmError("two-stage training reads a 1-channel image (stage 0) and {masked image, mask} (stage 1); "
                             "the backbones read %d and %d channels" % (s0.eng.in_channels, s1.eng.in_channels))
        if "pathology" not in s0.tail.row_of or s0.tail.row_of["pathology"][1] != 1:
            raise L.BfmError("stage 0 needs the one-channel pathology head")
        bad = [n for n in s0.loss_names if not n.startswith("pathol_")] + [n for n in s1.loss_names if n.startswith("pathol_")]
        if bad:
            raise L.BfmError("losses on the wrong stage: %s (pathol_* act on stage 0, every other name on stage 1)" % bad)
        self.pathol_step, self.task_step = s0, s1
        self.dev, self.lib = s0.dev, s0.lib
        self.scaler = s0.scaler
        s1.scaler = self.scaler                            # ONE GradScaler (engine.py:280-287)
        self.loss_names = list(loss_names) if loss_names is not None else list(s1.loss_names) + list(s0.loss_names)
        if sorted(self.loss_names) != sorted(list(s0.loss_names) + list(s1.loss_names)):
            raise L.BfmError("loss names %s are not those of the two steps" % (self.loss_names,))
        self.loss_weights = dict(s1.loss_weights)
        self.loss_weights.update(s0.loss_weights)

    def parameters(self):
        """{'pathol.' / 'task.' + reference parameter name: device tensor} of both models."""
        out = OrderedDict()
        for pre, s_ in zip(self.PREFIX, (self.pathol_step, self.task_step)):
            out.update((pre + k, v) for k, v in s_.parameters().items())
        return out

    def _split(self, grads):
        return tuple(OrderedDict((k[len(pre):], v) for k, v in grads.items() if k.startswith(pre)) for pre in self.PREFIX)

    def _sample(self, x, target, sample, scale):
        """engine.py:230-253 and the backward of one sample.  Returns the results of _sample_backward of stage 0 and of
        stage 1, and (stage-0 logits as a strided view of the head outputs, p)."""
        s0, s1, lib = self.pathol_step, self.task_step, self.lib
        if x.dim() != 5 or x.shape[0] != 1 or x.shape[1] != 1:
            raise L.BfmError("expected a (1,1,D,H,W) input, got %s" % (tuple(x.shape),))
        dims = tuple(int(v) for v in x.shape[2:])
        nvox = dims[0] * dims[1] * dims[2]
        xd = x.to(device=self.dev, dtype=torch.float32).contiguous()
        t = target.get("pathology") if target is not None else None
        target0 = target
        if isinstance(t, torch.Tensor):
            if t.numel() != nvox:
                raise L.BfmError("target['pathology'] %s does not match the input %s" % (tuple(t.shape), tuple(x.shape)))
            t = t.to(device=self.dev, dtype=torch.float32).contiguous()
        else:
            t = None                                       # the generator's 0.: a zero mask and no pathology loss
            target0 = {k: v for k, v in (target or {}).items() if k != "pathology"}
        ctx0 = s0._sample_forward(xd)
        raw0 = ctx0["raw"]
        co = s0._col("pathology")
        off, vs = (co * raw0.stride(0), 1) if ctx0["rows"] else (co, s0.tail.n_out)
        xin = torch.empty(dims + (2,), dtype=torch.float32, device=self.dev)
        p = torch.empty(dims, dtype=torch.float32, device=self.dev)
        masked = torch.empty_like(xd)
        L.check(lib.bfm_twostage_train_input(L.ptr(xd), L.ptr(raw0), off, vs, L.ptr(t), nvox, L.ptr(xin), L.ptr(p),
                                             L.ptr(masked), L.stream_ptr()), "twostage_train_input")
        sample["input_masked"] = masked
        res = {}

        def stage1_then_pathol_losses(ctx):
            ctx1 = s1._sample_forward(xd, xin)
            s1._sample_criterion(ctx1, target, sample, scale)
            ig = BW.InputGrad(0, xd, p, ctx["dRaw"], off, vs)
            res[1] = s1._sample_backward(ctx1, target, scale, input_grad=ig)
            s0._sample_criterion(ctx, target0, sample, scale)

        res[0] = s0._sample_backward(ctx0, target0, scale, pre_heads=stage1_then_pathol_losses)
        return res[0], res[1], (raw0.reshape(-1)[off:off + (nvox - 1) * vs + 1:vs], p)

    @L.on_device(lambda self, *a, **k: self.dev)
    def loss_and_grads(self, xs, target, samples, masks=None):
        """xs: list of (1,1,D,H,W) inputs; target / samples as the reference's dicts.  Leaves samples[i]['input_masked'].
        masks: a list that receives each sample's (stage-0 logits, p = their sigmoid) as the mask was built from them.
        Returns (loss_dict, total, grads): the merged loss dictionary in the criterion's order, and grads =
        d(scale * total)/d(parameter) of both models under parameters()' names, summed over the samples in sample order."""
        s0, s1 = self.pathol_step, self.task_step
        scale = self.scaler.scale
        s0._touched_heads, s1._touched_heads = set(), set()
        for s_ in (s0, s1):
            s_.__dict__.pop("_store_next", None)
        sums = [None, None]
        per = ([], [])
        nvox = None
        for x, sample in zip(xs, samples):
            nvox = x.shape[-3] * x.shape[-2] * x.shape[-1]
            r0, r1, mask = self._sample(x, target, sample, scale)
            if masks is not None:
                masks.append(mask)
            for j, (g, slots, vals) in enumerate((r0, r1)):
                per[j].append((slots, vals))
                if sums[j] is None:
                    sums[j] = g
                else:
                    for k_, v_ in g.items():
                        sums[j][k_] = sums[j][k_] + v_
        s0._touched_heads.add("pathology")                 # reached through the mask whatever the pathology losses do
        found = OrderedDict()
        found.update(s1._finish_losses(per[1], nvox))
        found.update(s0._finish_losses(per[0], nvox))
        loss_dict = OrderedDict(("loss_" + n, found["loss_" + n]) for n in self.loss_names if "loss_" + n in found)
        total = sum(v * self.loss_weights.get(k, 0.0) for k, v in loss_dict.items() if k in self.loss_weights)
        grads = OrderedDict()
        for pre, g in zip(self.PREFIX, sums):
            grads.update((pre + k, v) for k, v in g.items())
        return loss_dict, total, grads

    @L.on_device(lambda self, *a, **k: self.dev)
    def step(self, xs, target, samples, lr=None, weight_decay=None, group=None):
        """One full joint iteration (engine.py:217-287).  Returns (loss_dict, total, stepped).  A non-finite gradient in
        either model skips both and backs the shared scale off once; with more than one rank the loss dictionary is averaged
        first and the merged gradient dictionary goes through allreduce_mean_."""
        import torch.distributed as dist
        s0, s1 = self.pathol_step, self.task_step
        loss_dict, total, grads = self.loss_and_grads(xs, target, samples)
        touched = set(s1._touched_heads)
        heads = list(s1.tail.row_of.keys())
        tasks = heads + (["age"] if s1.age is not None else [])
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            loss_dict, total, touched = reduce_losses_(loss_dict, touched, self.loss_names, tasks, self.loss_weights, self.dev,
                                                       group)
        if not math.isfinite(total):
            return loss_dict, total, False
        allreduce_mean_(grads, group)
        g0, g1 = self._split(grads)
        for task in heads:                                 # stage-1 heads nobody's loss reached: no gradient, no step
            if task not in touched:
                g1.pop("head.final_conv_%s.weight" % task, None)
                g1.pop("head.final_conv_%s.bias" % task, None)
        if s1.age is not None and "age" not in touched:
            for k_ in s1.age.params:
                g1.pop("head." + k_, None)
        plans = (s0._measure(g0), s1._measure(g1))
        if plans[0]["found_inf"] or plans[1]["found_inf"]:
            self.scaler.update(True)
            return loss_dict, total, False
        s0._update(plans[0], lr, weight_decay)
        s1._update(plans[1], lr, weight_decay)
        self.scaler.update(False)
        return loss_dict, total, True

    def save_checkpoint(self, pathol_path, task_path, epoch=0, **extra):
        """The two checkpoints TwoStageSession / evaluate_image_twostage load (scripts/train.py:205-214 per model)."""
        self.pathol_step.save_checkpoint(pathol_path, epoch=epoch, **extra)
        self.task_step.save_checkpoint(task_path, epoch=epoch, **extra)


def twostage_train_step(gen_args, train_args, pathol_model, task_model, weights_ce, all_samples, **kw):
    """The TwoStageTrainStep of the two models build_inpaint_model returns (Trainer/models/__init__.py:441-463), losses as
    its get_criterion(gen_args, train_args, gen_args.tasks) builds them: pathol_ce / pathol_dice go to stage 0, every other
    name to stage 1, and the merged dictionary keeps the criterion's order.  train_args.condition None or 'mask' is the
    loop's runnable path; with 'flip' the reference concatenates three channels into a backbone built with num_cond=1
    (engine.py:240-242 against models/__init__.py:451), which cannot run, so it is refused here."""
    if freeze_feat_of(train_args) or kw.get("trainable", "all") != "all":
        raise L.BfmError("freeze_feat: two-stage training couples two backbones through the predicted mask (stage 0 learns "
                         "from stage 1's input gradient); a frozen backbone is not built for twostage_train_step")
    cond = getattr(train_args, "condition", None)
    if cond and "flip" in str(cond):
        raise L.BfmError("condition %r: the reference's two-stage loop builds a 3-channel input with 'flip' for a stage-1 "
                         "backbone of 2 channels (num_cond=1) and cannot run; two-stage training takes None or 'mask'" % (cond,))
    if cond and str(cond) != "mask":
        raise L.BfmError("unknown condition %r for two-stage training: None or 'mask'" % (cond,))
    eng0 = pathol_model.backbone.engine(pathol_model.head)
    eng1 = task_model.backbone.engine(task_model.head)
    for e_ in (eng0, eng1):
        if torch.device(e_.device).type != "cuda":
            raise L.BfmError("two-stage training runs on a HIP device only; there is no CPU fallback in the product path")
    if eng0.in_channels != 1 or eng1.in_channels != 2:
        raise L.BfmError("two-stage training reads a 1-channel image (stage 0) and {masked image, mask} (stage 1); the "
                         "backbones read %d and %d channels" % (eng0.in_channels, eng1.in_channels))
    names, weights = criterion_losses(train_args, gen_args.tasks)
    n0 = [n for n in names if n.startswith("pathol_")]
    n1 = [n for n in names if not n.startswith("pathol_")]
    kw.setdefault("max_surf_distance", float(gen_args.max_surf_distance))
    scaler = kw.pop("scaler", None)
    if scaler is None:
        scaler = LossScaler(enabled=False)
    age_head = kw.pop("age_head", None)                    # the pooled scalar head belongs to stage 1 (every head but pathology)
    s0 = TrainStep(eng0, pathol_model.head.tail(eng0), n0, weights, weights_ce, all_samples, scaler=scaler, **kw)
    s1 = TrainStep(eng1, task_model.head.tail(eng1), n1, weights, weights_ce, all_samples, scaler=scaler, age_head=age_head,
                   **kw)
    return TwoStageTrainStep(s0, s1, loss_names=names)


class _NoHead:
    """What TrainStep's shared code reads of a tail when the model has no head (process_args leaves out_channels empty
    for task 'contrastive', Trainer/models/__init__.py:57)."""
    row_of = {}
    n_out = 0


class ContrastiveStep(TrainStep):
    """One iteration of the reference's feature pre-training (gen_args.task.contrastive): the backbone alone, trained with
    loss_feat_contrastive (criterion.py:96-109) on the last feature maps of the FIRST TWO augmented samples after
    ContrastiveProcessor (joiner.py:136-147).  The criterion is SetCriterion, not SetMultiCriterion: no loop over the
    samples and no division by all_samples.  Parameters, apply / step, checkpoints and the scaler are TrainStep's; the
    parameter table holds the backbone alone.

    Samples after the second are not run.  The reference pushes every sample through the model (engine.py:114) and then
    reads outputs[0] and outputs[1] only, so the others cost a forward pass and change neither the loss nor a gradient.

    temperatures: (alpha, beta, gamma) = train_args.contrastive_temperatures.{alpha, beta, gamma} (criterion.py:45-48); no
    shipped yaml sets them, so they are plain arguments here.

    More than one rank is refused (BfmError): the gradient all-reduce of this step is not built."""

    def __init__(self, engine, loss_weights, temperatures, lr=1e-4, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8,
                 clip_max_norm=0.0, scaler=None, optimizer="adamw"):
        self.tail = _NoHead()
        self._init_optim(engine, ["contrastive"], loss_weights, lr, weight_decay, betas, eps, clip_max_norm, scaler, optimizer)
        self.alpha, self.beta, self.gamma = (float(t) for t in temperatures)
        if not (self.alpha > 0 and self.beta > 0 and self.gamma > 0):
            raise L.BfmError("contrastive temperatures must be positive, got %s" % (tuple(temperatures),))
        cf = engine.fm[0]
        if not 2 <= cf <= 64:
            raise L.BfmError("the contrastive loss kernel takes 2..64 feature channels, the backbone has %d" % cf)
        self.c_feat = cf
        self.n_norm = (1 if engine.unit_feat else 0) + 1   # the backbone's unit_feat (unet3d/model.py:205-207) + the processor
        self._ws_bytes = (max(self.lib.bfm_loss_contrastive_workspace(), self.lib.bfm_loss_workspace(1)),)   # + apply()'s sums

    def grad_store(self):
        raise L.BfmError("ContrastiveStep runs on one rank: it has no bucketed gradient all-reduce")

    def _weights_changed(self):
        self.eng.repack_all(refresh=BW.refresh_dgrad)

    def _forward(self, x):
        dims = tuple(x.shape[-3:])
        feats, tape = BW.backbone_forward_train(self.eng, self.eng.to_cl(x), dims)
        return feats, tape, dims

    def _backward(self, feats, tape, dims, dfeat):
        return BW.backbone_backward(self.eng, tape, [None] * (len(feats) - 1) + [dfeat.view(dims + (self.c_feat,))])

    @L.on_device(lambda self, *a, **k: self.dev)
    def loss_and_grads(self, xs, target=None, samples=None, cond=None):
        """xs: the augmented samples' inputs, (1,C,D,H,W) each, at least two; target / samples are not read (the loss has no
        target); cond must be None: the contrastive backbone is not mask-conditioned.  Returns ({'loss_contrastive': v}, weight * v, grads) with grads = d(scale * weight * v)/d(parameter)
        under the backbone's parameter names: sample 0's gradient + sample 1's, added on the caller's stream.
        With sample_lanes > 1 (from the second iteration on, as TrainStep) the two forwards run on two streams, the loss
        kernel on the caller's stream after both, and the two backward passes on the two streams again; every kernel sees
        the same inputs as with one lane, so the result is the same bits."""
        self.__dict__.pop("_store_next", None)
        if cond is not None:
            raise L.BfmError("ContrastiveStep takes no conditioned inputs: its backbone reads the one-channel samples")
        if len(xs) < 2:
            raise L.BfmError("the contrastive loss compares two augmented samples; got %d" % len(xs))
        if any(x.shape[0] != 1 for x in xs[:2]) or tuple(xs[0].shape) != tuple(xs[1].shape):
            raise L.BfmError("ContrastiveStep takes two (1,C,D,H,W) inputs of one shape, got %s and %s"
                             % (tuple(xs[0].shape), tuple(xs[1].shape)))
        eng, lib = self.eng, self.lib
        w = float(self.loss_weights.get("loss_contrastive", 0.0))
        coef = self.scaler.scale * w
        lanes = min(2, self.sample_lanes) if self.t >= 1 else 1
        main = torch.cuda.current_stream(self.dev)
        while len(self._lane_streams) < lanes:
            self._lane_streams.append(torch.cuda.Stream(device=self.dev))

        def on_lanes(fn):
            """fn(i) for i = 0, 1: in turn on the caller's stream, or one per lane stream between two joins."""
            if lanes <= 1:
                return [fn(0), fn(1)]
            start = torch.cuda.Event()
            start.record(main)
            seen = eng.pack_count
            out, evs = [], []
            for i in range(2):
                st = self._lane_streams[i]
                st.wait_event(start)
                if eng.pack_count != seen:                 # a packed form was created lazily while issuing sample 0
                    for e in evs:
                        st.wait_event(e)
                    seen = eng.pack_count
                eng.lane, self._lane = i, i
                try:
                    with torch.cuda.stream(st):
                        out.append(fn(i))
                        ev = torch.cuda.Event()
                        ev.record(st)
                finally:
                    eng.lane, self._lane = 0, 0
                evs.append(ev)
            for ev in evs:
                main.wait_event(ev)
            return out

        def keep(t_):                                      # allocated on a lane, used on the caller's stream (or back)
            if lanes > 1:
                for st in [main] + self._lane_streams[:2]:
                    t_.record_stream(st)
            return t_

        fwd = on_lanes(lambda i: self._forward(xs[i]))
        dims = fwd[0][2]
        nvox = dims[0] * dims[1] * dims[2]
        f0, f1 = keep(fwd[0][0][-1][0]), keep(fwd[1][0][-1][0])
        d0, d1 = keep(torch.empty_like(f0)), keep(torch.empty_like(f1))
        val = torch.zeros(1, dtype=torch.float64, device=self.dev)
        ws = self._lane_ws()[0]
        L.check(lib.bfm_loss_contrastive(L.ptr(f0), L.ptr(f1), self.c_feat, nvox, self.n_norm, 1e-12, self.alpha, self.beta,
                                         self.gamma, coef, L.ptr(d0), L.ptr(d1), None, None, L.ptr(val), L.ptr(ws),
                                         ws.numel(), L.stream_ptr()), "loss_contrastive")
        dfs = (d0, d1)
        gs = on_lanes(lambda i: self._backward(fwd[i][0], fwd[i][1], dims, dfs[i]))
        if lanes > 1:
            for g in gs:
                for t_ in g.values():
                    t_.record_stream(main)
        grads = OrderedDict((k_, gs[0][k_] + gs[1][k_]) for k_ in gs[0])
        v = float(val.item())
        return OrderedDict(loss_contrastive=v), w * v, grads

    def step(self, xs, target=None, samples=None, lr=None, weight_decay=None, group=None):
        """One full iteration (Trainer/engine.py:96-147) on one rank.  Returns (loss_dict, total, stepped)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            raise L.BfmError("ContrastiveStep runs on one rank: the gradient all-reduce of the contrastive step is not "
                             "built (world size %d)" % dist.get_world_size(group))
        return super().step(xs, target, samples, lr=lr, weight_decay=weight_decay, group=group)


def contrastive_train_step(gen_args, train_args, model, **kw):
    """The ContrastiveStep of the head-less model: (gen_args, train_args, model) as build_model returns them for
    gen_args.task.contrastive, the loss weight as get_criterion reads it (train_args.weights.contrastive) and the temperatures
    from train_args.contrastive_temperatures.{alpha, beta, gamma} (criterion.py:45-48).  train_args.freeze_feat is refused by
    name: the backbone is all this model trains."""
    if freeze_feat_of(train_args):
        raise L.BfmError("freeze_feat: ContrastiveStep trains the backbone alone (the contrastive model has no head); with a "
                         "frozen backbone nothing is left to train")
    names, weights = criterion_losses(train_args, gen_args.tasks)
    if names != ["contrastive"]:
        raise L.BfmError("contrastive_train_step builds the step of task 'contrastive'; the tasks are %s" % (list(gen_args.tasks),))
    t = train_args.contrastive_temperatures
    return ContrastiveStep(model.backbone.engine(model.head), weights, (t.alpha, t.beta, t.gamma), **kw)
