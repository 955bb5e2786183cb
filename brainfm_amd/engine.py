"""Device driver for the BrainFM inference path on MI355X.

Owns the packed weights and drives the HIP kernels of libbrainfm_hip.so for
``AbstractUNet.get_feature`` (Trainer/models/unet3d/model.py:195-209) and the
fused tail (head.py:52-59, joiner.py:69-77,149-157,
Trainer/models/__init__.py:272-354).  torch is used for device memory and
streams only -- every arithmetic step is a kernel from brainfm_amd/csrc.

Activations live in HBM as fp32 channels-last-3D (D,H,W,C) buffers; the
tensors handed back to callers are NCDHW *views* of those buffers
(torch.channels_last_3d strides), so shapes and values match the reference.
"""
import ctypes as C
import os
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import _lib as L

LABELS_LEFT = [0, 1, 2, 3, 4, 7, 8, 9, 10, 14, 15, 17, 31, 34, 36, 38, 40, 42]
LABELS_FULL = [0, 11, 12, 13, 16, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 46,
               1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 15, 17, 47, 49, 51, 53, 55,
               18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 48, 50, 52, 54, 56]


def features_per_level(f_maps, num_levels):
    """number_of_features_per_level, Trainer/models/unet3d/utils.py:109-110."""
    return [f_maps * 2 ** k for k in range(num_levels)]


def nearest_index_map(n_in, n_out):
    """F.interpolate(mode='nearest') source index per destination index:
    min(floor(dst * float32(in/out)), in-1) -- ATen's nearest_neighbor_compute_source_index."""
    scale = np.float32(n_in) / np.float32(n_out)
    idx = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, n_in - 1).astype(np.int32)


def tap_row_table(lo, hi):
    """(output voxel, tap) -> row of the low-res tensor that a 3x3x3 zero-padded conv over nearest_up(lo -> hi) reads
    there, -1 where the tap leaves the hi-res volume: int32 [prod(hi)][27], taps kd, kh, kw ascending.  lo == hi is the
    identity map, a plain conv (conv3d_tap.hip: bfm_tap_sum_batch)."""
    maps = [nearest_index_map(lo[a], hi[a]).astype(np.int64) for a in range(3)]
    z, y, x = np.meshgrid(*[np.arange(hi[a]) for a in range(3)], indexing="ij")
    tab = np.full(tuple(hi) + (27,), -1, dtype=np.int32)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                zz, yy, xx = z + kd - 1, y + kh - 1, x + kw - 1
                ok = (zz >= 0) & (zz < hi[0]) & (yy >= 0) & (yy < hi[1]) & (xx >= 0) & (xx < hi[2])
                row = (maps[0][zz.clip(0, hi[0] - 1)] * lo[1] + maps[1][yy.clip(0, hi[1] - 1)]) * lo[2] \
                    + maps[2][xx.clip(0, hi[2] - 1)]
                tab[..., (kd * 3 + kh) * 3 + kw] = np.where(ok, row, -1)
    return np.ascontiguousarray(tab.reshape(-1, 27))


_TUNE_CHOICES = {}          # (device, passes, shape key) -> conv variant that won UNetEngine._autotune in this process

# The conv variants (cfg[6]): 0 conv_mfma, 1 conv_mfma_ws, 2 conv_mfma16, 3 conv_wino F(2,3), 4 conv_wino4 F(4,3),
# 5 conv_wino_b5 (F(2,3) on 5 x 5 x 10 boxes, split K; the batched levels only).  Per variant
# the packed-weight layout and its packer; for the two Winograd families also the entry points that exist once per family
# with one C signature (_lib.SIGNATURES).  Names here; UNetEngine._variant binds them to the library once per engine.
_Variant = namedtuple("_Variant", "layout pack_bytes pack rows box dense masked_workspace masked uniform_scratch uniform",
                      defaults=(None,) * 7)
_MFMA = _Variant("mfma", "bfm_pack_conv_weights_mfma_bytes", "bfm_pack_conv_weights_mfma")
_CONV_VARIANTS = (
    _MFMA,
    _MFMA,
    _Variant("mfma16", "bfm_pack_conv_weights_mfma16_bytes", "bfm_pack_conv_weights_mfma16"),
    _Variant("wino", "bfm_pack_conv_weights_wino_bytes", "bfm_pack_conv_weights_wino", "bfm_conv3x3x3_wino_rows",
             "bfm_conv3x3x3_wino_box", "bfm_conv3x3x3_wino_ex", "bfm_conv3x3x3_wino_masked_workspace",
             "bfm_conv3x3x3_wino_masked", "bfm_conv3x3x3_wino_uniform_scratch", "bfm_conv3x3x3_wino_uniform"),
    _Variant("wino4", "bfm_pack_conv_weights_wino4_bytes", "bfm_pack_conv_weights_wino4", "bfm_conv3x3x3_wino4_rows",
             "bfm_conv3x3x3_wino4_box", "bfm_conv3x3x3_wino4", "bfm_conv3x3x3_wino4_masked_workspace",
             "bfm_conv3x3x3_wino4_masked", "bfm_conv3x3x3_wino4_uniform_scratch", "bfm_conv3x3x3_wino4_uniform"),
    # 5: conv_wino_b5, F(2,3) on 5 x 5 x 10 boxes with a split K loop -- conv_wino's pack; the batched levels only
    # (UNetEngine._batch_launch), one moment row per box
    _Variant("wino", "bfm_pack_conv_weights_wino_bytes", "bfm_pack_conv_weights_wino", "bfm_conv3x3x3_wino_b5_rows"),
)
_VARIANT_OF = {}                                        # packed-weight layout -> the first variant that reads it
for _ver, _v in enumerate(_CONV_VARIANTS):
    _VARIANT_OF.setdefault(_v.layout, _ver)

# The persisted tune table: the variants agree to ~1e-6, not bit for bit, so a choice made by timing would let two
# processes flip different argmax ties of the same volume.  brainfm_amd/conv_tune_gfx950.json (next to the .so, tracked)
# holds the winners for the shapes of the BASELINE configurations, keyed by architecture, MFMA passes and layer shape;
# a shape found there is never timed.  Shapes outside it are timed in-process as before and written back only under
# BFM_CONV_TUNE_SAVE=1 (scripts/make_tune_table.py).  BFM_CONV_TUNE=0: the planner's static choice, no table;
# BFM_CONV_TUNE=retune: ignore the table and time everything again.  BFM_CONV_TUNE_FILE: another path.
TUNE_FILE = os.environ.get("BFM_CONV_TUNE_FILE") or os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                  "conv_tune_gfx950.json")
_TUNE_TABLE = None          # {"<arch>/<passes>": {"cin,cout,d,h,w,two,acc": variant}}
_ARCH = {}


def _tune_key_str(key):
    cin, cout, dims, two, acc = key[:5]
    return ",".join(str(int(v)) for v in (cin, cout) + tuple(dims) + (two, acc) + tuple(key[5:]))


def _arch_of(dev_index):
    if dev_index not in _ARCH:
        name = getattr(torch.cuda.get_device_properties(dev_index), "gcnArchName", "") or "gpu"
        _ARCH[dev_index] = name.split(":")[0]
    return _ARCH[dev_index]


def _tune_table():
    global _TUNE_TABLE
    if _TUNE_TABLE is None:
        _TUNE_TABLE = {}
        mode = os.environ.get("BFM_CONV_TUNE", "1")
        if mode not in ("0", "retune") and os.path.exists(TUNE_FILE):
            import json
            try:
                _TUNE_TABLE = json.load(open(TUNE_FILE)).get("choices", {})
            except Exception as e:                               # a damaged table must not change results silently
                raise L.BfmError("cannot read the conv tune table %s: %r" % (TUNE_FILE, e))
    return _TUNE_TABLE


def _tune_lookup(dev_index, passes, key):
    return _tune_table().get("%s/%s" % (_arch_of(dev_index), passes), {}).get(_tune_key_str(key))


def _tune_store(dev_index, passes, key, ver):
    """Remember a timed winner; with BFM_CONV_TUNE_SAVE=1 also merge it into the file (read-merge-rename, so that
    several ranks saving at once leave a valid table)."""
    sect = "%s/%s" % (_arch_of(dev_index), passes)
    _tune_table().setdefault(sect, {})[_tune_key_str(key)] = int(ver)
    if os.environ.get("BFM_CONV_TUNE_SAVE") == "1":
        import json
        disk = {}
        if os.path.exists(TUNE_FILE) and os.environ.get("BFM_CONV_TUNE", "1") != "retune":
            try:
                disk = json.load(open(TUNE_FILE)).get("choices", {})
            except Exception:
                disk = {}
        for sct, tab in _tune_table().items():
            disk.setdefault(sct, {}).update(tab)
        doc = {"about": "conv variant per layer shape (0 conv_mfma, 1 conv_mfma_ws, 2 conv_mfma16, 3 conv_wino, 4 conv_wino4, "
                        "5 conv_wino_b5); key = cin,cout,D,H,W,two_sources,accumulate[,1 = batched levels[,5 = with "
                        "conv_wino_b5 admitted]]; written by UNetEngine._autotune under "
                        "BFM_CONV_TUNE_SAVE=1 (scripts/make_tune_table.py)",
               "choices": {k: dict(sorted(v.items())) for k, v in sorted(disk.items())}}
        tmp = "%s.%d.tmp" % (TUNE_FILE, os.getpid())
        with open(tmp, "w") as f:
            json.dump(doc, f, indent=0, sort_keys=False)
        os.replace(tmp, TUNE_FILE)


TRAIN_F43 = os.environ.get("BFM_TRAIN_F43", "1") != "0"     # F(4,3) (conv_wino4d) in the training forward / data gradients


class _Layer:
    __slots__ = ("name", "cin", "cout", "groups", "gamma", "beta", "kind", "wpacked", "wexp", "w_raw", "packs", "skip",
                 "used")

    def touch(self, layout):
        """Remember which packed forms the current pass really launches (autotune trials leave the others behind)."""
        u = getattr(self, "used", None)
        if u is None:
            u = self.used = set()
        u.add(layout)


HEAD_SLOPE = 0.2            # nn.LeakyReLU(0.2) of a hidden head layer (head.py:162)


class _HeadLayer(_Layer):
    """One hidden task-head layer (head.py:152-167, `head.layers.{i}.main`): a conv layer without GroupNorm (gamma and
    beta stay None, one group) that has a bias."""
    __slots__ = ("bias",)


class UNetEngine:
    """Weights + kernels for UNet3D('gcl') inference.

    state_dict uses the reference's key names
    (``backbone.encoders.{i}.basic_module.SingleConv{j}.{groupnorm.weight,groupnorm.bias,conv.weight}``,
    ``head.final_conv_{task}.{weight,bias}``); a ``backbone.``-less or ``module.``-prefixed dict is accepted
    the way utils/checkpoint.py:558-571 suffix-matches names.
    """
    prof = None
    lane = 0
    weights_epoch = 0           # bumped when the weights change in place: captured graphs bake in the packing exponents
    pack_count = 0              # packed weight forms created so far (train.py: lazily created ones order the sample lanes)
    _ws_lanes = None
    _variants = None            # _CONV_VARIANTS bound to self.lib (_variant)
    _f23_ids = None             # caches made on first use: _needs_f23, _same_boxes, uniform_flags (one pass), _region_ok
    _same_box_cache = None
    _uf_cache = None
    _deep_ok = None
    _tap_cache = None           # (lo, hi) -> device table of _tap_table
    _head_layers = None         # (task_f_maps, [_HeadLayer]) once a head with hidden layers asked for them (head_layers)
    _unit_bound = None
    _no_heads = None
    dense_last = False
    tape = None                # training (backward.py): list that single_conv / maxpool append their records to
    grad_sink = None            # training (train.GradStore through train._Sink): where the backward kernels put gradients
    prof_reps = 1
    use_upfold = False
    upfold_min = 250
    fuse_stats = False

    def __init__(self, state_dict, in_channels=1, f_maps=64, num_levels=6, num_groups=8, unit_feat=True,
                 device="cuda", passes=3, eps=1e-5, slope=0.01):
        self.lib = L.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.BfmError("UNetEngine needs a HIP device; the product path has no CPU fallback")
        self.fm = features_per_level(f_maps, num_levels) if isinstance(f_maps, int) else list(f_maps)
        self.in_channels = in_channels
        self.num_groups = num_groups
        self.unit_feat = bool(unit_feat)
        self.passes = int(passes)
        self.eps = float(eps)
        self.slope = float(slope)
        self._up_cache = {}
        self._ws_lanes = {}
        self._ws_retired = []
        self.lane = 0
        # arrival counters of the one-launch GroupNorm rows form, made here -- outside any graph capture -- for the lanes a
        # session may use (zero on first use, left zero by every call)
        self._gn_tickets = {ln: torch.zeros(16, dtype=torch.int32, device=self.device) for ln in range(4)}
        self._uf_tickets = {ln: torch.zeros(1, dtype=torch.int32, device=self.device) for ln in range(4)}
        self.gn_one_launch = os.environ.get("BFM_GN_ONE_LAUNCH", "1") != "0"
        self._plan_cache = {}
        self._tuned = set()
        self.force_direct = False
        # decoder first convs with an exact 2x upsample: fold the upsample into the weights (conv3d_upfold.hip)
        self.use_upfold = os.environ.get("BFM_UPFOLD", "1") != "0"
        self.upfold_min = int(os.environ.get("BFM_UPFOLD_MIN", "250"))    # fewest low-res voxels worth it (split-K below ~4000)
        # GroupNorm moments from rows the producing conv wrote in its epilogue instead of a pass over the activation
        self.fuse_stats = os.environ.get("BFM_FUSE_STATS", "1") != "0"
        # MaxPool3d(2) in the epilogue of the F(2,3) layers that feed it (round 5; 0: the separate launch, same bits)
        self.fuse_pool = os.environ.get("BFM_FUSE_POOL", "1") != "0"
        # the 2..4-channel stem of a conditioned network on the matrix core (0: the exact-fp32 direct kernel)
        self.stem_mc = os.environ.get("BFM_STEM_MC", "1") != "0"
        self.prof_reps = 1
        self.prof = None            # bench.py: list collecting (start_event, end_event, flops, bytes) per MFMA conv launch
        sd = self._normalise_keys(state_dict)
        self.enc = []
        for i, co in enumerate(self.fm):
            ci = in_channels if i == 0 else self.fm[i - 1]
            c1 = max(co // 2, ci)                       # DoubleConv encoder rule, buildingblocks.py:131-137
            self.enc.append([self._make_layer(sd, "backbone.encoders.%d.basic_module.SingleConv1" % i, ci, c1),
                             self._make_layer(sd, "backbone.encoders.%d.basic_module.SingleConv2" % i, c1, co)])
        rev = list(reversed(self.fm))
        self.dec = []
        for i in range(len(rev) - 1):
            ci, co = rev[i] + rev[i + 1], rev[i + 1]    # decoder rule, buildingblocks.py:139-141,313-319
            self.dec.append([self._make_layer(sd, "backbone.decoders.%d.basic_module.SingleConv1" % i, ci, co),
                             self._make_layer(sd, "backbone.decoders.%d.basic_module.SingleConv2" % i, co, co)])
        self.sd = sd
        # a head with hidden layers (task_f_maps longer than one) reads a one-voxel halo around every box it computes:
        # the backbone's last convolution then never leaves boxes out (backbone_cl(mask_last=True) runs dense)
        self.dense_last = any(k.startswith("head.layers.") for k in sd)

    # ------------------------------------------------------------------ weights
    @staticmethod
    def _normalise_keys(state_dict):
        out = {}
        for k, v in state_dict.items():
            for marker in ("backbone.", "head."):
                j = k.find(marker)
                if j >= 0:
                    out[k[j:]] = v
                    break
            else:
                out[k] = v
        return out

    def _dev(self, t, dtype=torch.float32):
        return torch.as_tensor(t).to(device=self.device, dtype=dtype).contiguous()

    def _make_layer(self, sd, name, cin, cout):
        ly = _Layer()
        ly.name, ly.cin, ly.cout = name, cin, cout
        ly.groups = self.num_groups if cin >= self.num_groups else 1      # buildingblocks.py:56-57
        ly.gamma = self._dev(sd[name + ".groupnorm.weight"])
        ly.beta = self._dev(sd[name + ".groupnorm.bias"])
        w = self._dev(sd[name + ".conv.weight"])
        if tuple(w.shape) != (cout, cin, 3, 3, 3):
            raise L.BfmError("%s.conv.weight has shape %s, expected %s" % (name, tuple(w.shape), (cout, cin, 3, 3, 3)))
        ly.w_raw = w
        ly.kind = None
        ly.wpacked = None
        ly.wexp = 0
        ly.packs = {}
        ly.skip = None
        return ly

    def _mfma_ok(self, ly, ca, cb):
        return (not self.force_direct) and ca % 16 == 0 and cb % 16 == 0 and ly.cout % 64 == 0

    def _variant(self, ver):
        """_CONV_VARIANTS[ver] with the entry points as functions of self.lib (looked up once per engine).  A number
        outside the table (a BFM_CONV_VER nobody defined) is conv_mfma, as the library's own launcher takes it."""
        if self._variants is None:
            self._variants = tuple(_Variant(v.layout, *[fn and getattr(self.lib, fn) for fn in v[1:]])
                                   for v in _CONV_VARIANTS)
        return self._variants[ver if 0 <= ver < len(self._variants) else 0]

    def _make_pack(self, ly, layout, wmax=None):
        """Create ly.packs[layout] from ly.w_raw (reusing the buffer of `prev` when repacking in place); wmax: max |w|
        when the caller already has it on the host (saves a device round trip per layer)."""
        st = L.stream_ptr()
        prev = ly.packs.get(layout)
        self.pack_count += 1
        if layout in _VARIANT_OF:
            v = self._variant(_VARIANT_OF[layout])
            ps = (self.passes,) if v.dense is not None else ()     # the Winograd packers take the passes too
            nbytes = v.pack_bytes(ly.cin, ly.cout, *ps)
            buf = prev[0] if prev is not None else torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            wexp = C.c_int(0)
            wmax = float(ly.w_raw.abs().max().item()) if wmax is None else wmax
            L.check(v.pack(L.ptr(ly.w_raw), ly.cin, ly.cout, wmax, *ps, L.ptr(buf), C.byref(wexp), st),
                    "pack_%s %s" % (layout, ly.name))
            ly.packs[layout] = (buf, wexp.value)
        elif layout == "direct":
            buf = prev[0] if prev is not None else torch.empty(27 * ly.cin * ly.cout, dtype=torch.float32, device=self.device)
            L.check(self.lib.bfm_pack_conv_weights_direct(L.ptr(ly.w_raw), ly.cin, ly.cout, L.ptr(buf), st),
                    "pack_direct " + ly.name)
            ly.packs[layout] = (buf, 0)
        else:
            raise L.BfmError("unknown weight layout '%s'" % layout)

    def _pack(self, ly, mfma, ver=0):
        """Pack (once per layout) and select the weights for this launch: 'direct' [27][Cin][Cout] fp32,
        'mfma' 32x32x16 fragments (plan variants 0/1), 'mfma16' 16x16x32 tap-pair fragments (variant 2),
        'wino' F(2,3)-along-x transformed fragments (variant 3, single-source layers only), 'wino4' F(4,3) (variant 4)."""
        layout = self._variant(ver).layout if mfma else "direct"
        if layout not in ly.packs:
            self._make_pack(ly, layout)
        ly.touch(layout)
        ly.wpacked, ly.wexp = ly.packs[layout]
        ly.kind = "mfma" if mfma else "direct"

    def _make_upfold_pack(self, ly, ca, cb, wmax=None):
        st = L.stream_ptr()
        self.pack_count += 1
        prev = ly.packs.get("upfold")
        nbytes = self.lib.bfm_pack_conv_weights_upfold_bytes(cb, ly.cout, self.passes)
        buf = prev[0] if prev is not None else torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        wexp = C.c_int(0)
        wmax = float(ly.w_raw[:, ca:].abs().max().item()) if wmax is None else wmax
        L.check(self.lib.bfm_pack_conv_weights_upfold(L.ptr(ly.w_raw), ca, cb, ly.cout, wmax, self.passes,
                                                      L.ptr(buf), C.byref(wexp), st), "pack_upfold " + ly.name)
        ly.packs["upfold"] = (buf, wexp.value)

    def repack_all(self, refresh=None, backbone=True):
        """The weights changed in place (training): rebuild, into the same buffers, every packed form a layer launched in
        the last pass (forward variants, skip half, up-folded form, the transposed data-gradient layer that backward.py
        hangs on it), so that nothing is packed lazily inside the next pass; forms only the autotune trials used are
        dropped.  All max |w| come to the host in ONE copy.  `refresh(ly, dg)` re-derives a data-gradient layer's weights.
        backbone=False: only the hidden head layers changed (training on a frozen backbone); the encoder and decoder layers
        keep their packed forms and their record of what the last pass used."""
        jobs = []                                          # (layer, layout, max|w| tensor)
        self.weights_epoch += 1

        hidden = self._head_layers[1] if self._head_layers is not None else []
        slots = torch.zeros(4 * (len(self.enc) + len(self.dec) + len(hidden)) * 4 + 16, dtype=torch.float32,
                            device=self.device)
        nslot = [0]

        def absmax(t):                                     # one launch per tensor into its slot of one vector
            i = nslot[0]
            nslot[0] += 1
            if t.is_contiguous():
                rows, ln, stride = 1, t.numel(), t.numel()
            else:                                           # w_raw[:, c0:]: rows of (cin - c0) * 27 floats, cin * 27 apart
                rows, ln, stride = t.shape[0], t[0].numel(), t.stride(0)
                if not t[0].is_contiguous():
                    raise L.BfmError("absmax: unsupported layout")
            L.check(self.lib.bfm_absmax_f32(L.ptr(t), rows, ln, stride, C.c_void_p(slots.data_ptr() + 4 * i),
                                            L.stream_ptr()), "absmax")
            return i

        def visit(ly, wm=None):
            used = getattr(ly, "used", None) or set()
            for layout in list(ly.packs.keys()):
                if layout not in used:
                    del ly.packs[layout]
                elif layout == "dgrad_layer":
                    dg = ly.packs[layout]
                    if refresh is not None:
                        refresh(ly, dg)
                    if wm is None:
                        wm = absmax(ly.w_raw)
                    visit(dg, wm)                          # transposing, mirroring and zero rows keep max |w|
                elif layout == "upfold":
                    jobs.append((ly, layout, absmax(ly.w_raw[:, ly.skip.cin:])))
                elif layout == "direct":
                    jobs.append((ly, layout, None))
                else:
                    if wm is None:
                        wm = absmax(ly.w_raw)
                    jobs.append((ly, layout, wm))
            ly.used = set()
            ly.wpacked, ly.kind = None, None
            if ly.skip is not None:
                ly.skip.w_raw.copy_(ly.w_raw[:, :ly.skip.cin])
                visit(ly.skip)

        for pair in (self.enc + self.dec if backbone else []) + [hidden]:
            for ly in pair:
                visit(ly)
        host = slots[:nslot[0]].cpu().tolist() if nslot[0] else []
        for ly, layout, m in jobs:
            wmax = host[m] if m is not None else None
            if layout == "upfold":
                self._make_upfold_pack(ly, ly.skip.cin, ly.cin - ly.skip.cin, wmax)
            else:
                self._make_pack(ly, layout, wmax)

    # ------------------------------------------------------------------ helpers
    def _upsample_desc(self, lo, hi):
        key = (tuple(lo), tuple(hi))
        if key not in self._up_cache:
            maps = [nearest_index_map(lo[a], hi[a]) for a in range(3)]
            reps = [np.bincount(maps[a], minlength=lo[a]).astype(np.int32) for a in range(3)]
            dev = [torch.from_numpy(m).to(self.device) for m in maps + reps]
            up = L.Upsample(lo[0], lo[1], lo[2], *[t.data_ptr() for t in dev])
            self._up_cache[key] = (up, dev)
        return self._up_cache[key][0]

    def _tap_table(self, lo, hi):
        """tap_row_table(lo, hi) on the device, built once per (lo, hi) shape."""
        key = (tuple(lo), tuple(hi))
        if self._tap_cache is None:
            self._tap_cache = {}
        if key not in self._tap_cache:
            self._tap_cache[key] = torch.from_numpy(tap_row_table(key[0], key[1])).to(self.device)
        return self._tap_cache[key]

    def _workspace(self, nbytes):
        """Scratch of the current lane (tiles of different lanes run concurrently on their own streams)."""
        nbytes = max(int(nbytes), 256)
        if self._ws_lanes is None:
            self._ws_lanes, self._ws_retired = {}, []
        ws = self._ws_lanes.get(self.lane)
        if ws is None or ws.numel() < nbytes:
            if ws is not None:
                self._ws_retired.append(ws)       # captured graphs of smaller shapes keep pointing into it
            ws = self._ws_lanes[self.lane] = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=self.device)
        return ws

    def _uf_ticket(self):
        """The arrival counter of bfm_uniform_boxes_levels, as _gn_ticket: zero before its first use, left zero, one per lane."""
        t = self._uf_tickets
        if self.lane not in t:
            t[self.lane] = torch.zeros(1, dtype=torch.int32, device=self.device)
        return t[self.lane]

    def _gn_ticket(self):
        """The arrival counter of bfm_gn_stats_rows' one-launch form: zero before its first use, left zero by every
        call; one per lane (the lanes' GroupNorm kernels run concurrently)."""
        t = self._gn_tickets
        if self.lane not in t:
            t[self.lane] = torch.zeros(16, dtype=torch.int32, device=self.device)
        return t[self.lane]

    def _plan(self, cin, cout, dims, two_src=False, accum=False):
        key = (cin, cout, tuple(dims), bool(two_src), bool(accum))
        if key not in self._plan_cache:
            cfg = (C.c_int * 8)()
            L.check(self.lib.bfm_conv3x3x3_mfma_plan(cin, cout, dims[0], dims[1], dims[2], cfg), "mfma_plan")
            if two_src and cfg[6] in (3, 4):                        # BFM_CONV_VER=3/4: Winograd takes one source
                cfg[6] = 0
            if cfg[6] == 5:                                         # BFM_CONV_VER=5: conv_wino_b5 runs the batched levels only
                cfg[6] = 0
            self._plan_cache[key] = cfg
        return self._plan_cache[key]

    def _autotune(self, ly, key, launch, vers=None):
        """Pick the fastest conv variant (0 conv_mfma, 1 conv_mfma_ws, 2 conv_mfma16, 3 conv_wino, 4 conv_wino4; 5
        conv_wino_b5 only where _deep_b5 puts it up against a batched layer's present variant) for this
        (Cin, Cout, dims, two-source) by timing them once on the real operands (HIP events on the launch stream).  All variants compute the same result; the chip is
        power-limited on this kernel, so which one wins is shape dependent (profiles/).  BFM_CONV_VER pins one."""
        cfg = self._plan_cache[key]
        if self._variant_pinned(key):
            return cfg
        gkey = (torch.cuda.current_device(), getattr(self, "passes", None), key)
        c = self._settled_variant(key, vers)
        if c is not None:
            if vers is None or c in vers:
                cfg[6] = c
                self._tuned.add(key)
                return cfg
            # a caller that rules F(4,3) out (training, the uniform-box layers) takes F(2,3) on a COPY: the shared plan
            # keeps the table's choice, so a later inference forward on this engine runs what a fresh process would
            narrowed = (C.c_int * 8)(*list(cfg))
            narrowed[6] = 3
            return narrowed
        best, best_ms = cfg[6], None
        # Winograd (3: F(2,3), 4: F(4,3)) takes single-source layers only.  F(4,3) rounds ~2x coarser than F(2,3): it is
        # timed only when the committed table is being made (BFM_CONV_TUNE=retune, scripts/make_tune_table.py) -- a shape
        # outside the table never gets it from an in-process timing
        single = (0, 1, 2, 3, 4) if os.environ.get("BFM_CONV_TUNE", "1") == "retune" else (0, 1, 2, 3)
        if hasattr(self, "enc") and self._needs_f23(ly):
            single = (0, 1, 2, 3)                               # these layers never run F(4,3): do not let it win their entry
        for ver in (vers if vers is not None else ((0, 1, 2) if key[3] else single)):
            if ver == 4 and 4 not in single and cfg[6] != 4:
                continue                                        # F(4,3) is timed when the table is made, never in-process
                                                                # (unless the plan runs it already: _deep_b5's yardstick)
            trial = (C.c_int * 8)(*list(cfg))
            trial[6] = ver
            try:
                self._pack(ly, True, ver)
                launch(trial)                                   # warm (also validates LDS / shape limits)
                ms = None
                for _ in range(2):                              # best of two 3-launch brackets: DVFS noise is large
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record()
                    launch(trial)
                    launch(trial)
                    launch(trial)
                    ev[1].record()
                    ev[1].synchronize()
                    t = ev[0].elapsed_time(ev[1])
                    ms = t if ms is None else min(ms, t)
            except L.BfmError:
                continue
            if ver == 4:
                ms = ms / 0.97                                  # F(4,3) pays in rounding: it must win by 3 % to be taken
            if ver == 5:
                ms = ms / 0.97                                  # conv_wino_b5 displaces a present variant: not on a tie
            if best_ms is None or ms < best_ms:
                best, best_ms = ver, ms
        cfg[6] = best
        self._tuned.add(key)
        _TUNE_CHOICES[gkey] = best
        _tune_store(gkey[0], gkey[1], key, best)
        return cfg

    def _variant_pinned(self, key):
        """The plan's variant stands as it is: timed before on this engine, or pinned (BFM_CONV_VER, BFM_CONV_TUNE=0)."""
        return bool(key in self._tuned or os.environ.get("BFM_CONV_VER") or os.environ.get("BFM_CONV_TUNE", "1") == "0")

    def _settled_variant(self, key, vers=None):
        """The variant _autotune gives this shape without timing anything, or None when it would have to time: the plan's
        when pinned, else this process's earlier choice, else the persisted table's.  _autotune decides by this, and so does
        a producer that must know its reader's kernel before the reader runs (_known_variant)."""
        if self._variant_pinned(key):
            return int(self._plan_cache[key][6])
        # one choice per process, device and shape: a second engine (another session, a resumed run) takes the first
        # one's winner instead of re-timing, so that two sessions in one process compute bit-identical results
        gkey = (torch.cuda.current_device(), getattr(self, "passes", None), key)
        if gkey not in _TUNE_CHOICES:
            saved = _tune_lookup(gkey[0], gkey[1], key)         # the persisted table: same bits in every process
            if saved is not None and not (key[3] and saved in (3, 4)) and (vers is None or saved in vers):
                _TUNE_CHOICES[gkey] = int(saved)
        c = _TUNE_CHOICES.get(gkey)
        if c is not None and (vers is None or c in vers or (c == 4 and 3 in vers)):
            return int(c)
        return None

    def conv_choices(self):
        """{shape key: variant} of every conv shape timed so far in this process on this device (see _autotune)."""
        dev, ps = torch.cuda.current_device(), getattr(self, "passes", None)
        return {k[2]: v for k, v in _TUNE_CHOICES.items() if k[0] == dev and k[1] == ps}

    def adopt_conv_choices(self, table):
        """Take another engine's (another rank's) winners: shapes not timed here yet will use them without timing, and
        shapes already timed switch over (weights are packed per variant on first use).  Returns True when a shape
        already in use changed variant -- captured graphs then hold the old kernels and must be dropped."""
        dev, ps = torch.cuda.current_device(), getattr(self, "passes", None)
        changed = False
        for key, ver in table.items():
            _TUNE_CHOICES[(dev, ps, key)] = ver
            if key in self._tuned and self._plan_cache[key][6] != ver:
                self._plan_cache[key][6] = ver
                changed = True
        return changed

    def _gn_stats(self, ly, A, ca, B, cb, dims, lo_dims, upp, scale, shift, bound, ws_min):
        """GroupNorm scale/shift/bound of cat((A, up(B))).  Uses the producers' moment rows when every source has
        them (and the upsample is an exact 2x, so every low-res voxel weighs 8); otherwise reads the tensors."""
        D, H, W = dims
        st = L.stream_ptr()
        ra = getattr(A, "_bfm_rows", None) if self.fuse_stats else None
        rb = getattr(B, "_bfm_rows", None) if (self.fuse_stats and B is not None) else None
        if self.tape is not None and ((ra is not None and len(ra) > 2) or (rb is not None and len(rb) > 2)):
            ra = rb = None                                   # (slices of a batch's rows: the inference flow only)
        exact2 = B is None or tuple(dims) == tuple(2 * v for v in lo_dims)
        mean = rstd = None
        if self.tape is not None:
            mean = torch.empty(ly.groups, dtype=torch.float32, device=self.device)
            rstd = torch.empty(ly.groups, dtype=torch.float32, device=self.device)
            self._last_moments = (mean, rstd)
        if ra is not None and (B is None or (rb is not None and exact2)):
            need = self.lib.bfm_gn_stats_rows_workspace(ra[1], ca, rb[1] if rb is not None else 0, cb)
            ws = self._workspace(max(need, ws_min))
            if (len(ra) > 2 or (rb is not None and len(rb) > 2)) and self.tape is None:
                # a source that is one sample of a batched producer: its rows are a slice (total, first) of the batch's
                ta, fa = (ra[2], ra[3]) if len(ra) > 2 else (ra[1], 0)
                tb, fb = ((rb[2], rb[3]) if len(rb) > 2 else (rb[1], 0)) if rb is not None else (0, 0)
                L.check(self.lib.bfm_gn_stats_rows_sliced(L.ptr(ra[0]), ta, fa, ra[1], ca,
                                                          L.ptr(rb[0]) if rb is not None else None, tb, fb,
                                                          rb[1] if rb is not None else 0, cb, 8.0, D * H * W, L.ptr(ly.gamma),
                                                          L.ptr(ly.beta), ly.groups, self.eps, L.ptr(scale), L.ptr(shift),
                                                          L.ptr(bound), L.ptr(ws), ws.numel(),
                                                          L.ptr(self._gn_ticket()) if self.gn_one_launch else None, st),
                        "gn_stats_rows(slice) " + ly.name)
                return ws
            L.check(self.lib.bfm_gn_stats_rows_train(L.ptr(ra[0]), ra[1], ca, L.ptr(rb[0]) if rb is not None else None,
                                                     rb[1] if rb is not None else 0, cb, 8.0, D * H * W, L.ptr(ly.gamma),
                                                     L.ptr(ly.beta), ly.groups, self.eps, L.ptr(scale), L.ptr(shift),
                                                     L.ptr(bound), L.ptr(mean), L.ptr(rstd), L.ptr(ws), ws.numel(),
                                                     L.ptr(self._gn_ticket()) if self.gn_one_launch else None, st),
                    "gn_stats_rows " + ly.name)
            return ws
        self._complete(A, dims)                              # this route reads every voxel (B is never stored by need)
        wsb = self.lib.bfm_gn_stats_workspace(ca, cb, D, H, W, upp)
        ws = self._workspace(max(wsb, ws_min))
        L.check(self.lib.bfm_gn_stats_train(L.ptr(A), ca, L.ptr(B), cb, D, H, W, upp, L.ptr(ly.gamma), L.ptr(ly.beta),
                                            ly.groups, self.eps, L.ptr(scale), L.ptr(shift), L.ptr(bound), L.ptr(mean),
                                            L.ptr(rstd), L.ptr(ws), ws.numel(), st), "gn_stats " + ly.name)
        return ws

    def _record(self, ly, A, B, dims, lo_dims, scale, shift, bound, out):
        """Training tape entry of one SingleConv (backward.ConvTape fields)."""
        if self.tape is not None:
            mean, rstd = self._last_moments
            self.tape.append(dict(ly=ly, A=A, B=B, dims=tuple(dims), lo_dims=tuple(lo_dims) if lo_dims is not None else None,
                                  scale=scale, shift=shift, bound=bound, mean=mean, rstd=rstd, out=out))

    def _conv_launch(self, ly, A, ca, B, cb, dims, upp, scale, shift, bound, groups, cfg, out, ws, rows=None, slope=None,
                     mask_img=None, uni_flags=None, pool=None, need=None):
        """One launch of the planned variant of GN-apply + conv + LeakyReLU (cfg[6]: 0/1/2 conv_mfma family,
        3 / 4 Winograd F(2,3) / F(4,3); cfg[7] bit 0: accumulate onto `out`).  mask_img (variants 3 and 4 only): the tile's
        input image; boxes of output voxels where it is all zero are left uncomputed (the family's _masked entry point).
        uni_flags (variants 3 and 4, one source): per-box flags of bfm_uniform_boxes -> the family's _uniform entry point.
        need (with uni_flags): the class mates of `out` are stored by need (bit 1 of the flag argument); an image instead of
        True: the masked convolution with that mask image reads `out` next (bfm_conv3x3x3_wino4_uniform_keep).
        A tensor that was stored by need (_bfm_need) is read by the launch its producer counted on, or not at all."""
        D, H, W = dims
        st = L.stream_ptr()
        slope = self.slope if slope is None else float(slope)
        self._pack(ly, True, cfg[6])
        v = self._variant(cfg[6])
        tag = getattr(A, "_bfm_need", None)
        if B is not None and getattr(B, "_bfm_need", None) is not None:
            raise L.BfmError("%s: an upsampled source that was stored by need" % ly.name)

        def reads(route, ok=False):
            if tag is not None and not ok:
                raise L.BfmError("%s: its input was stored by need for %s, and this launch (%s) would read boxes that were "
                                 "never written" % (ly.name, "the uniform-box pair on its flags" if tag[1] is None else
                                                    "the masked convolution", route))
        fbit = (cfg[7] & 1) | (2 if need is not None else 0)
        if mask_img is not None:
            if v.masked is None or cb or rows is not None:
                raise L.BfmError("a masked launch is a one-source Winograd kernel without moment rows")
            reads("masked", tag is not None and tag[1] is mask_img and (cfg[6] == 3 or self._same_boxes(dims)))
            nws = v.masked_workspace(D, H, W, self.passes)
            mws = torch.empty(nws, dtype=torch.uint8, device=self.device)       # box activity, count, list of boxes
            L.check(v.masked(L.ptr(A), ca, D, H, W, L.ptr(scale), L.ptr(shift), L.ptr(bound), groups, L.ptr(ly.wpacked),
                             ly.wexp, ly.cout, slope, self.passes, cfg[7] & 1, L.ptr(out), L.ptr(mask_img), L.ptr(mws), nws,
                             st), "conv_wino(masked) " + ly.name)
            return
        if pool is not None:
            # (pooled tensor, its moment rows): the F(2,3) kernel writes MaxPool3d(2) of its output too (single_conv(pool=True))
            if cfg[6] != 3 or cb or mask_img is not None:
                raise L.BfmError("the fused pooling is the one-source F(2,3) kernel's")
            pooled, prow = pool
            if uni_flags is not None:
                reads("uniform, pool", tag is not None and tag[1] is None and tag[0] is uni_flags)
                scratch = torch.empty(self.lib.bfm_conv3x3x3_wino_uniform_scratch(ly.cout), dtype=torch.uint8,
                                      device=self.device)
                L.check(self.lib.bfm_conv3x3x3_wino_uniform_pool(
                    L.ptr(A), ca, D, H, W, L.ptr(scale), L.ptr(shift), L.ptr(bound), groups, L.ptr(ly.wpacked), ly.wexp,
                    ly.cout, slope, self.passes, fbit, L.ptr(out), L.ptr(rows[0]) if rows is not None else None,
                    L.ptr(uni_flags), L.ptr(scratch), L.ptr(pooled), L.ptr(prow[0]) if prow is not None else None, st),
                        "conv_wino(uniform, pool) " + ly.name)
            else:
                if need is not None:
                    raise L.BfmError("%s: stores by need without the uniform-box pair" % ly.name)
                reads("pool")
                L.check(self.lib.bfm_conv3x3x3_wino_pool(
                    L.ptr(A), ca, D, H, W, L.ptr(scale), L.ptr(shift), L.ptr(bound), groups, L.ptr(ly.wpacked), ly.wexp,
                    ly.cout, slope, self.passes, cfg[7] & 1, L.ptr(out), L.ptr(rows[0]) if rows is not None else None,
                    L.ptr(pooled), L.ptr(prow[0]) if prow is not None else None, st), "conv_wino(pool) " + ly.name)
            return
        if uni_flags is not None and not self._pair_ok(cfg[6], dims, cb):
            uni_flags = None                                # the flags are per box of conv_wino's grid: dense launch, same bits
        if uni_flags is not None and v.uniform is not None:
            reads("uniform", tag is not None and tag[1] is None and tag[0] is uni_flags)
            scratch = torch.empty(v.uniform_scratch(ly.cout), dtype=torch.uint8, device=self.device)
            if need is not None and need is not True:
                if cfg[6] != 4 or fbit != 3:
                    raise L.BfmError("stores for a masked reader are the accumulating F(4,3) pair's")
                L.check(self.lib.bfm_conv3x3x3_wino4_uniform_keep(
                    L.ptr(A), ca, D, H, W, L.ptr(scale), L.ptr(shift), L.ptr(bound), groups, L.ptr(ly.wpacked), ly.wexp,
                    ly.cout, slope, self.passes, fbit, L.ptr(out), L.ptr(rows[0]) if rows is not None else None,
                    L.ptr(uni_flags), L.ptr(scratch), L.ptr(need), st), "conv_wino4(uniform, keep) " + ly.name)
                return
            L.check(v.uniform(L.ptr(A), ca, D, H, W, L.ptr(scale), L.ptr(shift), L.ptr(bound), groups, L.ptr(ly.wpacked),
                              ly.wexp, ly.cout, slope, self.passes, fbit, L.ptr(out),
                              L.ptr(rows[0]) if rows is not None else None, L.ptr(uni_flags), L.ptr(scratch), st),
                    "conv_wino(uniform) " + ly.name)
            return
        if need is not None:
            raise L.BfmError("%s: stores by need without the uniform-box pair" % ly.name)
        reads("dense")
        if v.dense is not None:
            if cb:
                raise L.BfmError("the Winograd variant takes one source" if cfg[6] == 3 else
                                 "the Winograd variants take one source")
            L.check(v.dense(L.ptr(A), ca, D, H, W, L.ptr(scale), L.ptr(shift), L.ptr(bound), groups, L.ptr(ly.wpacked),
                            ly.wexp, ly.cout, slope, self.passes, cfg[7] & 1, L.ptr(out),
                            L.ptr(rows[0]) if rows is not None else None, st), "conv_%s %s" % (v.layout, ly.name))
            return
        L.check(self.lib.bfm_conv3x3x3_mfma_ex(L.ptr(A), ca, L.ptr(B) if cb else None, cb, D, H, W, upp if cb else None,
                                               L.ptr(scale), L.ptr(shift), L.ptr(bound), groups, L.ptr(ly.wpacked),
                                               ly.wexp, ly.cout, slope, self.passes, cfg, L.ptr(out), L.ptr(ws),
                                               ws.numel(), L.ptr(rows[0]) if rows is not None else None, st),
                "conv_mfma " + ly.name)

    def _needs_f23(self, ly):
        """The uniform-box layers whose OUTPUT another uniform-box layer reads (the second conv of encoders.0, both of
        encoders.1) stay with F(2,3): the shortcut rests on class mates multiplying the same operands, with the flags grown by
        one voxel per layer; a voxel of an F(2,3) output depends numerically on its mathematical support, a voxel of an
        F(4,3) output on its whole quad (conv3d_wino4.hip), which a consumer's flags do not cover.  The two layers at the END
        of those chains -- the skip halves of the last two decoders' first convs -- read F(2,3) outputs and feed no
        uniform-box layer: a box is a whole number of quads, its sums depend on its mathematical halo only, so they may run
        F(4,3) with the same flags (bfm_conv3x3x3_wino4_uniform, round 5).  A layer must compute the same bits with the
        shortcut on and off, so the rule goes by position in the network, never by the state of a switch."""
        if self._f23_ids is None:
            self._f23_ids = {id(self.enc[i][j]) for i, j in ((0, 1), (1, 0), (1, 1)) if i < len(self.enc)}
        return id(ly) in self._f23_ids

    def _same_boxes(self, dims):
        """conv_wino4's box for this volume is conv_wino's (the grid bfm_uniform_boxes flags)."""
        if self._same_box_cache is None:
            self._same_box_cache = {}
        cache, key = self._same_box_cache, tuple(dims)
        if key not in cache:
            b3, b4 = (C.c_int * 3)(), (C.c_int * 3)()
            ok = (self._variant(3).box(dims[0], dims[1], dims[2], self.passes, b3) == 0 and
                  self._variant(4).box(dims[0], dims[1], dims[2], self.passes, b4) == 0)
            cache[key] = ok and list(b3) == list(b4)
        return cache[key]

    def _pair_ok(self, ver, dims, cb=0, mask_img=None):
        """A launch of variant `ver` that is handed uniform flags takes the _rest / _uniform pair: a one-source Winograd
        launch that leaves no box out, F(4,3) only where its boxes are the flags' (single_conv, _single_conv_upfold and
        _conv_launch decide by this, and so does a producer that stores by need for them: _need_reader)."""
        return ver in (3, 4) and not cb and mask_img is None and (ver != 4 or self._same_boxes(dims))

    def _known_variant(self, ly, tune_ly, key):
        """The variant _f23_cfg(ly, _autotune(tune_ly, key, ...)) will return, when that is settled without timing anything
        (pinned, timed before, or in the table); None: not known yet."""
        self._plan(key[0], key[1], key[2], key[3], key[4])
        ver = self._settled_variant(key)
        if ver is None:
            return None
        cfg = (C.c_int * 8)()
        cfg[6] = ver
        return int(self._f23_cfg(ly, cfg)[6])

    def _need_reader(self, reader, flags, dims, ca):
        """Whether the one convolution that reads a (dims, ca) tensor will, in this pass, take the uniform-box pair on
        `flags` -- then the tensor's producer may store its class mates by need.  reader: ("conv", layer, its flags): the next
        SingleConv of the level; ("skip", decoder's first conv, its flags): the skip half of an up-folded decoder conv;
        ("masked", layer, mask image): the network's last convolution, which computes the boxes that hold input."""
        if (reader is None or flags is None or not self.uniform_need or self.tape is not None or not self.fuse_stats
                or self.force_direct):
            return False
        kind, ly, arg = reader
        if kind == "skip":
            cb = ly.cin - ca
            lo = tuple(v // 2 for v in dims)
            if not (arg is flags and self._mfma_ok(ly, ca, cb) and self.use_upfold and all(v % 2 == 0 for v in dims)
                    and lo[0] * lo[1] * lo[2] >= self.upfold_min):
                return False
            return self._pair_ok(self._known_variant(ly, self._skip_layer(ly, ca), (ca, ly.cout, tuple(dims), False, True)),
                                 dims)
        if not (ly.cin == ca and self._mfma_ok(ly, ca, 0)):
            return False
        ver = self._known_variant(ly, ly, (ly.cin, ly.cout, tuple(dims), False, False))
        if kind == "conv":
            return arg is flags and self._pair_ok(ver, dims)
        # the masked form: its boxes must be the flags' (F(2,3)'s are), single_conv's own condition otherwise
        return (arg is not None and self.mask_skip and ver in (3, 4) and (ver == 3 or self._same_boxes(dims))
                and self._variant(ver).masked is not None)

    def _complete(self, t, dims):
        """A tensor stored by need for the pair, for a reader that looks at every voxel: the remaining class mates are
        copied from their classes' first boxes (what the full launch does).  Not for an accumulated tensor.  The one reader
        a producer cannot foresee is the GroupNorm of a decoder whose up-sampled source came without moment rows (a conv
        variant that emits none): it reads the skip tensor in full.  need_completed counts these; the default flows leave
        it at zero."""
        tag = getattr(t, "_bfm_need", None)
        if tag is None:
            return
        if tag[1] is not None:
            raise L.BfmError("a tensor stored by need for the masked convolution cannot be completed")
        L.check(self.lib.bfm_uniform_fill(L.ptr(t), dims[0], dims[1], dims[2], t.shape[-1], self.passes, L.ptr(tag[0]),
                                          L.stream_ptr()), "uniform_fill")
        t._bfm_need = None
        self.need_completed += 1

    def _f23_cfg(self, ly, cfg):
        """A tuned choice of the F(4,3) kernel (variant 4) becomes F(2,3) for the uniform-box layers that feed another one
        (_needs_f23); in training only under BFM_TRAIN_F43=0 (round 5: the training forward and the data gradients take
        F(4,3) where the table says so -- the gradients stay within the float64 tests' bounds, tests/test_gpu_train.py)."""
        if cfg[6] == 4 and ((self.tape is not None and not TRAIN_F43) or self._needs_f23(ly)):
            cfg = (C.c_int * 8)(*list(cfg))
            cfg[6] = 3
        return cfg

    def _rows_for(self, cin, cout, dims, cfg, S=1):
        """(buffer, nrows) for the producer's output-moment rows, or None when this plan cannot emit them."""
        v = self._variant(cfg[6])
        if v.rows is not None:
            return self._rows_buf(cout, S, v.rows, dims[0], dims[1], dims[2], self.passes)
        return self._rows_buf(cout, S, self.lib.bfm_conv3x3x3_mfma_rows, cin, cout, dims[0], dims[1], dims[2], cfg)

    def _rows_buf(self, cout, S, rows_fn, *args):
        """(buffer, n) for the moment rows a producer writes beside its output -- n = rows_fn(*args) rows of cout channels
        per sample, S samples -- or None (BFM_FUSE_STATS=0: rows_fn is not asked; or no rows for this shape)."""
        if not self.fuse_stats:
            return None
        n = rows_fn(*args)
        if n <= 0:
            return None
        return (torch.empty(self.lib.bfm_moment_rows_bytes(S * n, cout), dtype=torch.uint8, device=self.device), n)

    @staticmethod
    def _tag(ly):
        """The layer's name in the records of the instrumented pass."""
        return ly.name.replace("backbone.", "").replace(".basic_module.SingleConv", ".")

    def _bracket(self, launch, record):
        """Issue one conv launch.  In the instrumented pass (bench.py: self.prof is a list) the launch is issued prof_reps
        times back to back inside one HIP event pair, so the bracket holds kernel time, not host submission gaps (the
        result is idempotent except for the accumulating halves of the up-folded layers, "sk" and "x%dsk": their output is
        that of a plain pass with prof_reps == 1 only); record() -> (flops, bytes, tag, cin, cout, dims, cfg) is asked for after the closing event only
        (counting the voxels of a masked or uniform launch synchronises)."""
        if self.prof is None:
            launch()
            return
        reps = max(1, int(self.prof_reps))
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        for _ in range(reps):
            launch()
        ev[1].record()
        flops, nbytes, tag, cin, cout, dims, cfg = record()
        self.prof.append((ev[0], ev[1], flops, nbytes, reps, (tag, cin, cout, tuple(dims), tuple(cfg))))

    # ------------------------------------------------------------------ one SingleConv
    def single_conv(self, ly, A, dims, B=None, lo_dims=None, mask_img=None, uni_flags=None, pool=False, reader=None):
        """GroupNorm -> Conv3d(3,p=1) -> LeakyReLU on cat((A, nearest_up(B))).
        A: (D,H,W,CA) fp32, B: (d,h,w,CB) fp32 or None.  Returns (D,H,W,Cout).
        mask_img: (D,H,W) image; the caller promises to look at the output only where it is non-zero (the tile loop's
        last convolution, see backbone_cl).  Honoured when the layer runs the 4-wave Winograd kernel, ignored otherwise.
        reader: the one convolution that reads the output (_need_reader), when the caller knows it: where that one takes the
        uniform-box pair on the same flags, the output's class mates are stored by need and the tensor is tagged with the
        flags (_bfm_need); any other reader of a tagged tensor raises (_conv_launch) or completes it first (_complete)."""
        D, H, W = dims
        ca = A.shape[-1]
        cb = 0 if B is None else B.shape[-1]
        assert ca + cb == ly.cin, (ly.name, ca, cb, ly.cin)
        st = L.stream_ptr()
        up = self._upsample_desc(lo_dims, dims) if B is not None else None
        upp = C.byref(up) if up is not None else None
        scale = torch.empty(ly.cin, dtype=torch.float32, device=self.device)
        shift = torch.empty(ly.cin, dtype=torch.float32, device=self.device)
        bound = torch.empty(ly.groups, dtype=torch.float32, device=self.device)
        mfma = self._mfma_ok(ly, ca, cb)
        if (mfma and B is not None and self.use_upfold and tuple(dims) == tuple(2 * v for v in lo_dims)
                and lo_dims[0] * lo_dims[1] * lo_dims[2] >= self.upfold_min):
            return self._single_conv_upfold(ly, A, dims, B, lo_dims, upp, scale, shift, bound, uni_flags=uni_flags,
                                            reader=reader)
        cfg = None
        wsc = 0
        if mfma:
            cfg = self._plan(ly.cin, ly.cout, dims, B is not None)
            wsc = self.lib.bfm_conv3x3x3_mfma_workspace(ly.cin, ly.cout, D, H, W, cfg[5])
        ws = self._gn_stats(ly, A, ca, B, cb, dims, lo_dims, upp, scale, shift, bound, wsc)
        out = torch.empty((D, H, W, ly.cout), dtype=torch.float32, device=self.device)
        if mfma:
            def _launch(c):
                self._conv_launch(ly, A, ca, B, cb, dims, upp, scale, shift, bound, ly.groups, c, out, ws)
            cfg = self._f23_cfg(ly, self._autotune(ly, (ly.cin, ly.cout, tuple(dims), B is not None, False), _launch))
        self._pack(ly, mfma, cfg[6] if cfg is not None else 0)
        if mfma:
            if mask_img is not None and not (cfg[6] in (3, 4) and B is None and self.tape is None):
                mask_img = None
            if uni_flags is not None and not self._pair_ok(cfg[6], dims, cb, mask_img):
                uni_flags = None
            rows = self._rows_for(ly.cin, ly.cout, dims, cfg) if mask_img is None else None
            # pool: the caller pools this output next (an encoder level's second conv): where the F(2,3) kernel's box allows
            # it writes MaxPool3d(2) of the output and that tensor's moment rows in its epilogue; maxpool() then returns them
            pl = None
            if (pool and cfg[6] == 3 and B is None and mask_img is None and self.tape is None and self.fuse_pool
                    and min(dims) >= 2 and self.lib.bfm_conv3x3x3_wino_pool_ok(D, H, W, self.passes)):
                pooled = torch.empty((D // 2, H // 2, W // 2, ly.cout), dtype=torch.float32, device=self.device)
                pl = (pooled, self._rows_buf(ly.cout, 1, self.lib.bfm_conv3x3x3_wino_rows, D, H, W, self.passes))

            # by need: the non-accumulating F(2,3) pair (class_fill); a pooling that is not fused would read every voxel
            need = None
            if (uni_flags is not None and cfg[6] == 3 and rows is not None and (pl is not None or not pool)
                    and reader is not None and reader[0] != "masked" and self._need_reader(reader, uni_flags, dims, ly.cout)):
                need = True
                if self.poison_skipped:
                    out.fill_(float("nan"))

            def _record():
                nv = D * H * W
                if mask_img is not None:                    # only the boxes the kernel computes count as work
                    nv = self.masked_voxels(mask_img, dims, cfg[6])
                if uni_flags is not None:                   # a uniform box runs a quarter of its products
                    nv = self.uniform_voxels(uni_flags, dims)
                lo = 0 if B is None else lo_dims[0] * lo_dims[1] * lo_dims[2]
                return (2.0 * 27 * ly.cin * ly.cout * nv, 4.0 * (nv * ca + lo * cb + nv * ly.cout + 27 * ly.cin * ly.cout),
                        self._tag(ly) + ("[masked]" if mask_img is not None else "[uniform]" if uni_flags is not None else ""),
                        ly.cin, ly.cout, dims, cfg)
            self._bracket(lambda: self._conv_launch(ly, A, ca, B, cb, dims, upp, scale, shift, bound, ly.groups, cfg, out, ws,
                                                    rows, mask_img=mask_img, uni_flags=uni_flags, pool=pl, need=need), _record)
            if need is not None:
                out._bfm_need = (uni_flags, None)
            if rows is not None:
                out._bfm_rows = rows
            if pl is not None:
                if pl[1] is not None:
                    pl[0]._bfm_rows = pl[1]
                out._bfm_pooled = (pl[0], (D // 2, H // 2, W // 2))
        elif ca == 1 and cb == 0 and ly.cout in (32, 64) and not self.force_direct:
            rows = self._rows_buf(ly.cout, 1, self.lib.bfm_conv3x3x3_stem_rows, D, H, W)
            L.check(self.lib.bfm_conv3x3x3_stem_ex(L.ptr(A), D, H, W, L.ptr(scale), L.ptr(shift), L.ptr(bound),
                                                   L.ptr(ly.wpacked), ly.cout, self.slope, L.ptr(out),
                                                   L.ptr(rows[0]) if rows is not None else None, st),
                    "conv_stem " + ly.name)
            if rows is not None:
                out._bfm_rows = rows
        elif ca in (2, 3, 4) and cb == 0 and ly.cout in (32, 64) and not self.force_direct and self.stem_mc:
            # the stem of a conditioned / two-stage network (image + condition channels): GroupNorm(1, ca), one bound
            rows = self._rows_buf(ly.cout, 1, self.lib.bfm_conv3x3x3_stem_rows, D, H, W)
            L.check(self.lib.bfm_conv3x3x3_stem_mc_ex(L.ptr(A), ca, D, H, W, L.ptr(scale), L.ptr(shift), L.ptr(bound),
                                                      L.ptr(ly.wpacked), ly.cout, self.slope, L.ptr(out),
                                                      L.ptr(rows[0]) if rows is not None else None, st),
                    "conv_stem_mc " + ly.name)
            ly.kind = "stem_mc"
            if rows is not None:
                out._bfm_rows = rows
        else:
            L.check(self.lib.bfm_conv3x3x3_direct(L.ptr(A), ca, L.ptr(B), cb, D, H, W, upp, L.ptr(scale),
                                                  L.ptr(shift), L.ptr(ly.wpacked), ly.cout, self.slope, L.ptr(out),
                                                  st), "conv_direct " + ly.name)
        self._record(ly, A, B, dims, lo_dims, scale, shift, bound, out)
        return out

    def masked_voxels(self, mask_img, dims, ver=None):
        """Output voxels bfm_conv3x3x3_wino_masked / _wino4_masked computes for this image: those of the kernel's boxes that
        hold a non-zero voxel (host-side count for the instrumented pass; synchronises).  ver: the variant (3 / 4) of the
        launch; None = what the last convolution of the network runs at these dims (the tile loop's masked layer)."""
        D, H, W = dims
        if ver is None:
            ly = self.dec[-1][-1] if self.dec else self.enc[0][-1]
            key = (ly.cin, ly.cout, tuple(dims), False, False)
            ver = _TUNE_CHOICES.get((torch.cuda.current_device(), getattr(self, "passes", None), key))
            if ver is None:
                ver = _tune_lookup(torch.cuda.current_device(), getattr(self, "passes", None), key)
            if os.environ.get("BFM_CONV_VER"):
                ver = int(os.environ["BFM_CONV_VER"])
        box = (C.c_int * 3)()
        L.check(self._variant(4 if ver == 4 else 3).box(D, H, W, self.passes, box), "wino_box")
        td, th, tw = box[0], box[1], box[2]
        m = (mask_img.reshape(D, H, W) != 0)
        m = torch.nn.functional.pad(m, (0, -W % tw, 0, -H % th, 0, -D % td))
        m = m.reshape(m.shape[0] // td, td, m.shape[1] // th, th, m.shape[2] // tw, tw)
        act = m.any(dim=5, keepdim=True).any(dim=3, keepdim=True).any(dim=1, keepdim=True).expand_as(m)
        act = act.reshape(m.shape[0] * td, m.shape[2] * th, m.shape[4] * tw)[:D, :H, :W]
        n = int(act.sum().item())
        self.last_mask_fraction = n / float(D * H * W)
        return n

    def uniform_flags(self, x_cl, dims, radius, level=0):
        """bfm_uniform_boxes_level of the one-channel image x_cl (D,H,W,1), dims = the image's: flags for the Winograd
        kernel's box grid of the tensor `level` poolings down, or None (switched off, more channels, or no such grid)."""
        if not self.uniform_skip or x_cl is None or x_cl.shape[-1] != 1 or self.tape is not None:
            return None
        # one set of flags per (image, level): the largest radius any layer of the level needs is valid for all of them
        # (a box constant within 3 voxels is constant within 2) and flags 1 % fewer boxes than each layer's own radius
        radius = max([radius] + [r for k, r in self.UNIFORM_RADIUS.items() if k[1] == level])
        ckey = (x_cl.data_ptr(), tuple(dims), int(level), int(radius), torch.cuda.current_stream(self.device).cuda_stream)
        if self._uf_cache is None:
            self._uf_cache = {}
        cache = self._uf_cache
        if ckey in cache:
            return cache[ckey]
        D, H, W = dims
        # every level the net will ask for, in one launch (their flags go into the cache under their own keys); a level
        # without a box grid or with boxes shorter than its radius sends each level through its own call below
        lv = sorted({k[1] for k in self.UNIFORM_RADIUS})
        rad = [max(r for k, r in self.UNIFORM_RADIUS.items() if k[1] == l) for l in lv]
        if level in lv and radius == rad[lv.index(level)]:
            nb = [self.lib.bfm_uniform_boxes_bytes(D >> l, H >> l, W >> l, self.passes) for l in lv]
            if min(nb) > 0:
                bufs = [torch.empty(n, dtype=torch.uint8, device=self.device) for n in nb]
                rc = self.lib.bfm_uniform_boxes_levels(L.ptr(x_cl), D, H, W, len(lv), (C.c_int * len(lv))(*lv),
                                                       (C.c_int * len(lv))(*rad), self.passes,
                                                       (C.c_void_p * len(lv))(*[b.data_ptr() for b in bufs]),
                                                       L.ptr(self._uf_ticket()), L.stream_ptr())
                if rc != -2:
                    L.check(rc, "uniform_boxes_levels")
                    for l, r, b in zip(lv, rad, bufs):
                        cache[ckey[:2] + (int(l), int(r)) + ckey[4:]] = b
                    return cache[ckey]
        n = self.lib.bfm_uniform_boxes_bytes(D >> level, H >> level, W >> level, self.passes)
        if n <= 0:
            return None
        flags = torch.empty(n, dtype=torch.uint8, device=self.device)     # one byte per box + the first box of each class
        rc = self.lib.bfm_uniform_boxes_level(L.ptr(x_cl), D, H, W, int(level), int(radius), self.passes, L.ptr(flags),
                                              L.stream_ptr())
        if rc == -2:                                         # BFM_E_SHAPE: a box side shorter than the radius, no classes
            flags = None
        else:
            L.check(rc, "uniform_boxes")
        cache[ckey] = flags
        return flags

    # image-voxel radius within which the input must be constant for the OUTPUT of these layers to be one vector:
    # (encoder level, conv index) and the skip halves of the decoders that end at levels 0 and 1
    UNIFORM_RADIUS = {("enc", 0, 1): 2, ("dec", 0): 3}
    if os.environ.get("BFM_UNIFORM_LEVELS", "1") != "0":   # one pooling level down too (0: full resolution only)
        UNIFORM_RADIUS.update({("enc", 1, 0): 4, ("enc", 1, 1): 6, ("dec", 1): 8})

    def uniform_voxels(self, flags, dims):
        """Voxels' worth of matrix products a bfm_conv3x3x3_wino_uniform launch runs: the boxes not flagged and one flagged
        box per class (host-side, for the instrumented pass; synchronises)."""
        nb = self.lib.bfm_conv3x3x3_wino_rows(dims[0], dims[1], dims[2], self.passes)
        f = flags[:nb]
        k = int((f != 0).sum().item())
        reused = k - int(torch.unique(f[f != 0]).numel())    # all flagged boxes but one per class present
        self.last_uniform_fraction = k / float(nb)
        return int(round(dims[0] * dims[1] * dims[2] * (1.0 - max(reused, 0) / float(nb))))

    def _skip_layer(self, ly, ca):
        """The skip-channel half of a decoder's first conv as a layer of its own (weights w[:, :ca])."""
        if ly.skip is None:
            sk = _Layer()
            sk.name, sk.cin, sk.cout, sk.groups = ly.name + "[skip]", ca, ly.cout, ly.groups
            sk.gamma, sk.beta = ly.gamma, ly.beta
            sk.w_raw = ly.w_raw[:, :ca].contiguous()
            sk.kind, sk.wpacked, sk.wexp, sk.packs, sk.skip = None, None, 0, {}, None
            ly.skip = sk
        return ly.skip

    def _single_conv_upfold(self, ly, A, dims, B, lo_dims, upp, scale, shift, bound, uni_flags=None, reader=None):
        """cat((skip, up2x(x))) -> GN -> conv -> LeakyReLU as: GN stats over the virtual concat, the upsampled
        channels through bfm_conv3x3x3_upfold (8 folded taps on the low-res tensor), the skip channels through
        bfm_conv3x3x3_mfma accumulating onto that."""
        D, H, W = dims
        ca, cb = A.shape[-1], B.shape[-1]
        st = L.stream_ptr()
        sk = self._skip_layer(ly, ca)
        key = (ca, ly.cout, tuple(dims), False, True)           # tuned in accumulate mode (its epilogue differs)
        cfg0 = self._plan(ca, ly.cout, dims, False, True)
        cfg0[7] = 1
        wsc = self.lib.bfm_conv3x3x3_mfma_workspace(ca, ly.cout, D, H, W, cfg0[5])
        wsu = self.lib.bfm_conv3x3x3_upfold_workspace(cb, lo_dims[0], lo_dims[1], lo_dims[2], ly.cout)   # split-K slabs
        ws = self._gn_stats(ly, A, ca, B, cb, dims, lo_dims, upp, scale, shift, bound, max(wsc, wsu))
        out = torch.empty((D, H, W, ly.cout), dtype=torch.float32, device=self.device)
        if "upfold" not in ly.packs:
            self._make_upfold_pack(ly, ca, cb)
        ly.touch("upfold")
        wup, wexp_up = ly.packs["upfold"]

        def _launch_skip(c):
            self._conv_launch(sk, A, ca, None, 0, dims, None, scale, shift, bound, ly.groups, c, out, ws)
        cfg = self._f23_cfg(ly, self._autotune(sk, key, _launch_skip))   # trials accumulate onto garbage; overwritten below
        self._pack(sk, True, cfg[6])
        sc_b, sh_b = scale[ca:], shift[ca:]
        nv = D * H * W
        lo = lo_dims[0] * lo_dims[1] * lo_dims[2]

        def _launch_up():
            L.check(self.lib.bfm_conv3x3x3_upfold_ex(L.ptr(B), cb, lo_dims[0], lo_dims[1], lo_dims[2], L.ptr(sc_b),
                                                     L.ptr(sh_b), L.ptr(bound), ly.groups, L.ptr(wup), wexp_up, ly.cout,
                                                     self.passes, L.ptr(out), L.ptr(ws) if wsu else None, ws.numel(), st),
                    "conv_upfold " + ly.name)
        self._bracket(_launch_up, lambda: (2.0 * 27 * cb * ly.cout * nv, 4.0 * (lo * cb + nv * ly.cout),
                                           self._tag(ly) + "up", cb, ly.cout, dims, (0,) * 8))
        rows = self._rows_for(ca, ly.cout, dims, cfg)
        if uni_flags is not None and not self._pair_ok(cfg[6], dims):
            uni_flags = None
        # by need: the accumulating F(4,3) pair, when the masked last convolution is all that reads the output
        need = None
        if (uni_flags is not None and cfg[6] == 4 and rows is not None and reader is not None and reader[0] == "masked"
                and self._need_reader(reader, uni_flags, dims, ly.cout)):
            need = reader[2]
        self._bracket(lambda: self._conv_launch(sk, A, ca, None, 0, dims, None, scale, shift, bound, ly.groups, cfg, out, ws,
                                                rows, uni_flags=uni_flags, need=need),
                      lambda: (2.0 * 27 * ca * ly.cout * (nv if uni_flags is None else self.uniform_voxels(uni_flags, dims)),
                               4.0 * (nv * ca + 2 * nv * ly.cout),
                               self._tag(ly) + ("sk[uniform]" if uni_flags is not None else "sk"), ca, ly.cout, dims, cfg))
        if need is not None:
            out._bfm_need = (uni_flags, need)
        if rows is not None:
            out._bfm_rows = rows
        self._record(ly, A, B, dims, lo_dims, scale, shift, bound, out)
        return out

    def maxpool(self, X, dims, out=None):
        D, H, W = dims
        c = X.shape[-1]
        fused = getattr(X, "_bfm_pooled", None)
        if fused is not None and out is None and self.tape is None:
            return fused                                     # written by the producing conv's epilogue (single_conv(pool=True))
        if out is None:
            out = torch.empty((D // 2, H // 2, W // 2, c), dtype=torch.float32, device=self.device)
        self._complete(X, dims)
        rows = self._rows_buf(c, 1, self.lib.bfm_maxpool2_rows, c, D, H, W)
        L.check(self.lib.bfm_maxpool2_ex(L.ptr(X), c, D, H, W, L.ptr(out), L.ptr(rows[0]) if rows is not None else None,
                                         L.stream_ptr()), "maxpool2")
        if rows is not None:
            out._bfm_rows = rows
        if self.tape is not None:
            self.tape.append(dict(pool_in=X, pool_dims=tuple(dims)))
        return out, (D // 2, H // 2, W // 2)

    def maxpool_batch(self, X, dims):
        """MaxPool3d(2) of a batch (S,D,H,W,C) in one launch; per sample the bits of bfm_maxpool2."""
        S, (D, H, W), c = X.shape[0], dims, X.shape[-1]
        out = torch.empty((S, D // 2, H // 2, W // 2, c), dtype=torch.float32, device=self.device)
        if c % 4 or self.tape is not None:
            for s_ in range(S):
                self.maxpool(X[s_], dims, out=out[s_])
            return out
        rows = self._rows_buf(c, S, self.lib.bfm_maxpool2_batch_rows, c, D, H, W)
        L.check(self.lib.bfm_maxpool2_batch(L.ptr(X), c, S, D, H, W, L.ptr(out), L.ptr(rows[0]) if rows is not None else None,
                                            L.stream_ptr()), "maxpool2_batch")
        if rows is not None:
            out._bfm_rows = rows
        return out

    # ------------------------------------------------------------------ the deep levels, batched over samples
    # Levels >= deep_from (20^3 voxels and fewer on a 160^3 tile) are bound by their weights: 253 M of the 264 M
    # parameters = 1 GB of packed fragments that every tile re-reads for a few thousand voxels.  Tiles of one shape
    # therefore go through these levels TOGETHER: one launch per layer over S samples (bfm_conv3x3x3_mfma_batch,
    # bfm_gn_stats*_batch; GroupNorm statistics stay per sample), the weights are read once per batch.  A single
    # tile takes the same code with S = 1, so that a tile's result does not depend on what it was batched with.
    deep_from = int(os.environ.get("BFM_DEEP_FROM", "3"))
    deep_batch = os.environ.get("BFM_DEEP_BATCH", "1") != "0"
    DEEP_VERS = (0, 2)                                     # conv_mfma, conv_mfma16: the variants that take a batch
    # round 6: single-source layers of the batched levels may also run conv_wino4d on the batch (bfm_conv3x3x3_wino4_batch:
    # per sample the bits of bfm_conv3x3x3_wino4) where the committed tune table says so -- the level-2 layers of the
    # 160 x 80 x 80-class tiles were 250-workgroup launches at half the kernel's rate, four of them per shape
    DEEP_VERS_1SRC = (0, 2, 4)
    # Volumes that boxes of 5 x 5 x 10 divide (an 80-wide tile from level 2 down: 20 / 10 wide) may also run conv_wino_b5
    # (variant 5: F(2,3), 18 of 27 tap-rows, split K) where the committed tune table says so.  Eligibility goes by the
    # per-sample dims alone (_deep_b5).  It is admitted beside DEEP_VERS_1SRC, not inside it: its choice against the key's
    # present variant is a table entry of its own, so that switching it off finds the entries above as they were.
    # BFM_WINO_B5=0: the routes without it; =force: every eligible layer takes it.
    use_wino_b5 = os.environ.get("BFM_WINO_B5", "1")
    deep_upfold = os.environ.get("BFM_DEEP_UPFOLD", "1") != "0"          # fold exact 2x upsamples inside the region too
    deep_upfold_min = int(os.environ.get("BFM_DEEP_UPFOLD_MIN", "100"))  # fewest low-res voxels per sample worth it
    # The smallest levels (2^3, 5 x 2 x 2, 5 x 5 x 2 voxels per sample) as tap-wise GEMMs over the batch's densely packed
    # rows (conv3d_tap.hip): one source with at most tap_max voxels, or two sources whose low-res tensor has at most
    # tap_max -- at most half of conv_mfma's 128-row tile filled per sample.  Of the shapes alone, never of S.
    # BFM_TAP=0: the conv_mfma route.
    use_tap = os.environ.get("BFM_TAP", "1") != "0"
    tap_max = 64
    # The tile loop multiplies every output of a tile by (tile input != 0) (scripts/demo_test.py:88-100): the last
    # convolution and the per-voxel heads leave out the voxels that product discards (BFM_MASK_SKIP=0: compute them all).
    mask_skip = os.environ.get("BFM_MASK_SKIP", "1") != "0"
    # Where the one-channel input image is constant (a head volume's zero background), the first layers' activations are
    # one vector per layer; the two full-resolution Winograd layers that read them (encoders.0 conv 2, the skip half of the
    # last decoder's conv 1) run a quarter of the matrix products in boxes that see nothing else (bfm_uniform_boxes,
    # bfm_conv3x3x3_wino_uniform; bit-identical).  BFM_UNIFORM_SKIP=0: every box in full.
    uniform_skip = os.environ.get("BFM_UNIFORM_SKIP", "1") != "0"
    # A computed box stages its input with a one-voxel halo, so of a tensor that only a uniform-box layer on the same flags
    # reads, the class mates with no computed box next to them are never read: its producer stores those boxes by need
    # (the `need` table behind the flags; _need_reader).  BFM_UNIFORM_NEED=0: every box is stored; same bits wherever a
    # later kernel looks.  BFM_POISON_SKIPPED=1 (debugging): such an output is filled with NaN before the launch.
    uniform_need = os.environ.get("BFM_UNIFORM_NEED", "1") != "0"
    poison_skipped = os.environ.get("BFM_POISON_SKIPPED", "0") == "1"
    need_completed = 0          # tensors stored by need that a reader of every voxel had to complete (_complete)

    # A small tile's level deep_from - 1 is small too (80^3: 20^3 voxels of 256 channels -- launches of 60-100 us that
    # fill a fifth of the chip; round 6: the 160 x 80 x 80 class too, 40 x 20 x 20 = 16 000 voxels, 250 workgroups per
    # launch): the region starts one level higher for tiles whose level there has at most this many voxels.  A function
    # of the tile shape alone, like everything that decides which kernels a tile runs.
    deep_vox = int(os.environ.get("BFM_DEEP_VOX", "16000"))

    def _region_ok(self, df):
        if self._deep_ok is None:
            self._deep_ok = {}
        cache = self._deep_ok
        if df not in cache:                                  # every layer of the region must be a matrix-core layer
            ndeep = len(self.enc) - 1 - df
            layers = [ly for pair in self.enc[df:] + self.dec[:ndeep] for ly in pair]
            cache[df] = all(ly.cin % 16 == 0 and ly.cout % 64 == 0 for ly in layers) and \
                self.enc[df - 1][1].cout % 16 == 0
        return cache[df]

    def has_deep_region(self):
        if not (self.deep_batch and self.tape is None and not self.force_direct and len(self.fm) > self.deep_from >= 1):
            return False
        return self._region_ok(self.deep_from)

    def region_start(self, dims):
        """First level of the batched region for tiles of this shape: deep_from, or shallower levels (not above 2) while
        they have at most deep_vox voxels."""
        df = self.deep_from
        while df - 1 >= 2:
            lv = [v >> (df - 1) for v in dims]
            if min(lv) < 1 or lv[0] * lv[1] * lv[2] > self.deep_vox or not self._region_ok(df - 1):
                break
            df -= 1
        return df

    def _batch_stats(self, ly, A, ca, B, cb, S, dims, lo_dims, upp, scale, shift, bound):
        """GroupNorm scale / shift / bound [S][..] of cat((A[s], up(B[s]))) for every sample of a batch."""
        D, H, W = dims
        st = L.stream_ptr()
        ra = getattr(A, "_bfm_rows", None) if self.fuse_stats else None
        rb = getattr(B, "_bfm_rows", None) if (self.fuse_stats and B is not None) else None
        exact2 = B is None or tuple(dims) == tuple(2 * v for v in lo_dims)
        if ra is not None and ra[1] <= 128 and (B is None or (rb is not None and exact2 and rb[1] <= 128)):
            L.check(self.lib.bfm_gn_stats_rows_batch(L.ptr(ra[0]), ra[1], ca, L.ptr(rb[0]) if rb is not None else None,
                                                     rb[1] if rb is not None else 0, cb, 8.0, D * H * W, S,
                                                     L.ptr(ly.gamma), L.ptr(ly.beta), ly.groups, self.eps, L.ptr(scale),
                                                     L.ptr(shift), L.ptr(bound), st), "gn_stats_rows_batch " + ly.name)
            return
        need = self.lib.bfm_gn_stats_batch_workspace(ca, cb, S, D, H, W, upp)
        ws = self._workspace(need)
        L.check(self.lib.bfm_gn_stats_batch(L.ptr(A), ca, L.ptr(B), cb, S, D, H, W, upp, L.ptr(ly.gamma), L.ptr(ly.beta),
                                            ly.groups, self.eps, L.ptr(scale), L.ptr(shift), L.ptr(bound), L.ptr(ws),
                                            ws.numel(), st), "gn_stats_batch " + ly.name)

    def batch_conv(self, ly, A, dims, B=None, lo_dims=None, stats=None):
        """SingleConv on a batch: A (S,D,H,W,CA), B (S,d,h,w,CB) or None -> (S,D,H,W,Cout).  `stats`: per-sample
        (scale, shift, bound) already computed (the first layer of the region takes them from the pooling rows)."""
        S = A.shape[0]
        D, H, W = dims
        ca = A.shape[-1]
        cb = 0 if B is None else B.shape[-1]
        assert ca + cb == ly.cin, (ly.name, ca, cb, ly.cin)
        if not self._mfma_ok(ly, ca, cb):
            raise L.BfmError("%s: the batched levels need channel counts that are multiples of 16 / 64" % ly.name)
        up = self._upsample_desc(lo_dims, dims) if B is not None else None
        upp = C.byref(up) if up is not None else None
        if stats is None:
            scale = torch.empty((S, ly.cin), dtype=torch.float32, device=self.device)
            shift = torch.empty((S, ly.cin), dtype=torch.float32, device=self.device)
            bound = torch.empty((S, ly.groups), dtype=torch.float32, device=self.device)
            self._batch_stats(ly, A, ca, B, cb, S, dims, lo_dims, upp, scale, shift, bound)
        else:
            scale, shift, bound = stats
        if self.use_tap and (lo_dims[0] * lo_dims[1] * lo_dims[2] if B is not None else D * H * W) <= self.tap_max:
            return self._batch_conv_tap(ly, A, dims, B, lo_dims, scale, shift, bound)
        if (B is not None and self.use_upfold and self.deep_upfold and tuple(dims) == tuple(2 * v for v in lo_dims)
                and lo_dims[0] * lo_dims[1] * lo_dims[2] >= self.deep_upfold_min):
            return self._batch_conv_upfold(ly, A, dims, B, lo_dims, scale, shift, bound)
        key = (ly.cin, ly.cout, tuple(dims), B is not None, False, 1)       # trailing 1: a layer of the batched levels
        vers = self.DEEP_VERS if B is not None else self.DEEP_VERS_1SRC
        cfg = self._batch_plan(key, vers)
        out = torch.empty((S, D, H, W, ly.cout), dtype=torch.float32, device=self.device)
        if key not in self._tuned:
            # timed on ONE sample (the choice must not depend on the batch size: a tile's bits may not either)
            cfg = self._autotune(ly, key, lambda c: self._batch_launch(ly, c, A[0:1], B[0:1] if B is not None else None, upp, dims,
                                                                       scale[0:1], shift[0:1], bound[0:1], out[0:1]),
                                 vers=vers)
        if B is None:
            cfg = self._deep_b5(ly, key, cfg, A, dims, scale, shift, bound)
        self._pack(ly, True, cfg[6])
        rows = self._rows_for(ly.cin, ly.cout, dims, cfg, S)
        nv = D * H * W
        lo = 0 if B is None else lo_dims[0] * lo_dims[1] * lo_dims[2]
        self._bracket(lambda: self._batch_launch(ly, cfg, A, B, upp, dims, scale, shift, bound, out, rows),
                      lambda: (2.0 * 27 * ly.cin * ly.cout * nv * S,
                               4.0 * (S * (nv * ca + lo * cb + nv * ly.cout) + 27 * ly.cin * ly.cout),
                               self._tag(ly) + ("x%d" % S), ly.cin, ly.cout, dims, cfg))
        if rows is not None:
            out._bfm_rows = rows
        return out

    def _batch_plan(self, key, vers):
        """The cached plan of a layer of the batched levels (key as in batch_conv: cin, cout, dims, two sources,
        accumulate, 1), its variant clamped to `vers` = those that take a batch."""
        if key not in self._plan_cache:
            cfg = (C.c_int * 8)()
            L.check(self.lib.bfm_conv3x3x3_mfma_plan(key[0], key[1], key[2][0], key[2][1], key[2][2], cfg), "mfma_plan")
            if cfg[6] not in vers:
                cfg[6] = 0
            if key[4]:
                cfg[7] = 1
            self._plan_cache[key] = cfg
        return self._plan_cache[key]

    B5_TUNE_S = 4                                          # samples in the batch that times conv_wino_b5 against the present variant

    def _deep_b5(self, ly, key, cfg, A, dims, scale, shift, bound):
        """The plan of a single-source layer of the batched levels once conv_wino_b5 (variant 5) is admitted: `cfg` (the
        variant the layer runs without it, plan key `key`) or a copy with variant 5.  Admitted where boxes of 5 x 5 x 10
        divide the per-sample volume -- by the layer's shape alone, never by S.  The choice between the two is an entry of
        its own in the tune table (key + (5,)), so that BFM_WINO_B5=0 finds the table's earlier entries as they were.  A
        shape outside the table times the two on B5_TUNE_S copies of the first sample, whatever S is: these layers run
        batched (x2 .. x8 in the tile flows), and on one sample both are bound by their launches (two kernels against
        one or two), which says little about the batch."""
        if self.use_wino_b5 == "0" or key[3]:
            return cfg
        trial = []

        def launch(c):
            if not trial:                                   # made only when something is timed
                n = self.B5_TUNE_S
                trial.extend(t[0:1].expand((n,) + tuple(t.shape[1:])).contiguous() for t in (A, scale, shift, bound))
                trial.append(torch.zeros((n,) + tuple(dims) + (ly.cout,), dtype=torch.float32, device=self.device))
            self._batch_launch(ly, c, trial[0], None, None, dims, trial[1], trial[2], trial[3], trial[4])
        key5 = key + (5,)
        if key5 not in self._plan_cache:
            ok = self.lib.bfm_conv3x3x3_wino_b5_splitk(key[0], key[1], key[2][0], key[2][1], key[2][2]) > 0
            self._plan_cache[key5] = (C.c_int * 8)(*list(cfg)) if ok else None
        cfg5 = self._plan_cache[key5]
        if cfg5 is None:
            return cfg
        if self.use_wino_b5 == "force" or os.environ.get("BFM_CONV_VER") == "5":
            cfg5[6] = 5
        elif key5 not in self._tuned:
            cfg5 = self._autotune(ly, key5, launch, vers=(cfg[6], 5))
        return cfg5

    def _batch_launch(self, ly, cfg, A, B, upp, dims, scale, shift, bound, out, rows=None, aff=0):
        """One launch of `ly` on the batch A (S,D,H,W,CA) [+ B]: conv_wino4d on the batch (cfg[6] == 4, one source),
        conv_wino_b5 (cfg[6] == 5, one source) or bfm_conv3x3x3_mfma_batch.  cfg[7] bit 0: accumulate onto `out`; aff: pitch
        of the rows of scale / shift when they are column windows of wider tables (0: ly.cin)."""
        S, (D, H, W), ca = A.shape[0], dims, A.shape[-1]
        cb = 0 if B is None else B.shape[-1]
        st = L.stream_ptr()
        self._pack(ly, True, cfg[6])
        if cfg[6] == 5:
            ws = self._workspace(self.lib.bfm_conv3x3x3_wino_b5_workspace(ca, ly.cout, S, D, H, W))
            L.check(self.lib.bfm_conv3x3x3_wino_b5_batch(L.ptr(A), ca, S, D, H, W, L.ptr(scale), L.ptr(shift), L.ptr(bound),
                                                         ly.groups, L.ptr(ly.wpacked), ly.wexp, ly.cout, self.slope,
                                                         self.passes, cfg[7] & 1, L.ptr(out),
                                                         L.ptr(rows[0]) if rows is not None else None, aff, L.ptr(ws),
                                                         ws.numel(), st), "conv_wino_b5_batch " + ly.name)
            return
        if cfg[6] == 4:
            L.check(self.lib.bfm_conv3x3x3_wino4_batch(L.ptr(A), ca, S, D, H, W, L.ptr(scale), L.ptr(shift), L.ptr(bound),
                                                       ly.groups, L.ptr(ly.wpacked), ly.wexp, ly.cout, self.slope, self.passes,
                                                       cfg[7] & 1, L.ptr(out), L.ptr(rows[0]) if rows is not None else None,
                                                       aff, st), "conv_wino4_batch " + ly.name)
            return
        ws = self._workspace(self.lib.bfm_conv3x3x3_mfma_batch_workspace(ly.cin, ly.cout, S, D, H, W, cfg[5]))
        L.check(self.lib.bfm_conv3x3x3_mfma_batch(L.ptr(A), ca, L.ptr(B) if cb else None, cb, S, D, H, W,
                                                  upp if cb else None, L.ptr(scale), L.ptr(shift), L.ptr(bound), ly.groups,
                                                  L.ptr(ly.wpacked), ly.wexp, ly.cout, self.slope, self.passes, cfg,
                                                  L.ptr(out), L.ptr(ws), ws.numel(),
                                                  L.ptr(rows[0]) if rows is not None else None, aff, st),
                "conv_mfma_batch " + ly.name)

    def _batch_conv_upfold(self, ly, A, dims, B, lo_dims, scale, shift, bound):
        """A decoder's first conv on a batch, with the exact 2x upsample folded into the weights (as _single_conv_upfold
        does per tile): the low-res channels through bfm_conv3x3x3_upfold_batch (8 folded taps instead of 27), the skip
        channels through bfm_conv3x3x3_mfma_batch accumulating onto that.  Which path a layer takes depends on its
        shapes alone, never on S: a tile's bits do not depend on what it is batched with."""
        S = A.shape[0]
        D, H, W = dims
        ca, cb = A.shape[-1], B.shape[-1]
        st = L.stream_ptr()
        sk = self._skip_layer(ly, ca)
        if "upfold" not in ly.packs:
            self._make_upfold_pack(ly, ca, cb)
        ly.touch("upfold")
        wup, wexp_up = ly.packs["upfold"]
        # the two halves' GroupNorm affine: column windows of the concat's [S][ca + cb] tables (rows ca + cb apart)
        sc_a, sh_a = scale[:, :ca], shift[:, :ca]
        sc_b, sh_b = scale[:, ca:], shift[:, ca:]
        aff = ca + cb
        out = torch.empty((S, D, H, W, ly.cout), dtype=torch.float32, device=self.device)
        key = (ca, ly.cout, tuple(dims), False, True, 1)
        cfg = self._batch_plan(key, self.DEEP_VERS_1SRC)
        if key not in self._tuned:                              # on one sample; trials accumulate onto garbage
            cfg = self._autotune(sk, key, lambda c: self._batch_launch(sk, c, A[0:1], None, None, dims, sc_a[0:1], sh_a[0:1],
                                                                       bound[0:1], out[0:1], None, aff),
                                 vers=self.DEEP_VERS_1SRC)
        cfg = self._deep_b5(sk, key, cfg, A, dims, sc_a, sh_a, bound)
        self._pack(sk, True, cfg[6])
        nv = D * H * W
        lo = lo_dims[0] * lo_dims[1] * lo_dims[2]
        wsu = self.lib.bfm_conv3x3x3_upfold_batch_workspace(cb, S, lo_dims[0], lo_dims[1], lo_dims[2], ly.cout)

        def _launch_up():
            ws = self._workspace(wsu)
            L.check(self.lib.bfm_conv3x3x3_upfold_batch(L.ptr(B), cb, S, lo_dims[0], lo_dims[1], lo_dims[2], L.ptr(sc_b),
                                                        L.ptr(sh_b), L.ptr(bound), ly.groups, L.ptr(wup), wexp_up,
                                                        ly.cout, self.passes, L.ptr(out), L.ptr(ws) if wsu else None,
                                                        ws.numel() if wsu else 0, aff, st), "conv_upfold_batch " + ly.name)
        self._bracket(_launch_up, lambda: (2.0 * 27 * cb * ly.cout * nv * S, 4.0 * (S * (lo * cb + nv * ly.cout)),
                                           self._tag(ly) + "x%dup" % S, cb, ly.cout, dims, (0,) * 8))
        rows = self._rows_for(ca, ly.cout, dims, cfg, S)
        self._bracket(lambda: self._batch_launch(sk, cfg, A, None, None, dims, sc_a, sh_a, bound, out, rows, aff),
                      lambda: (2.0 * 27 * ca * ly.cout * nv * S, 4.0 * S * (nv * ca + 2 * nv * ly.cout),
                               self._tag(ly) + "x%dsk" % S, ca, ly.cout, dims, cfg))
        if rows is not None:
            out._bfm_rows = rows
        return out

    def _batch_conv_tap(self, ly, A, dims, B, lo_dims, scale, shift, bound):
        """A layer of the batched levels whose (low-res) tensor has at most tap_max voxels per sample, as tap-wise GEMMs:
        bfm_conv3x3x3_tap_batch multiplies every tap's weights with the S * n_lo densely packed rows of the batch (one pass
        over the packed weights), bfm_tap_sum_batch gathers the 27 products of every output voxel.  One source: the sum
        applies LeakyReLU and writes the moment rows.  Two sources: that is the upsampled half, without activation; the
        skip half then accumulates onto it through conv_mfma as in _batch_conv_upfold."""
        S = A.shape[0]
        D, H, W = dims
        nv = D * H * W
        ca = A.shape[-1]
        st = L.stream_ptr()
        if "mfma" not in ly.packs:
            self._make_pack(ly, "mfma")
        ly.touch("mfma")
        wp, wexp = ly.packs["mfma"]
        out = torch.empty((S, D, H, W, ly.cout), dtype=torch.float32, device=self.device)
        if B is None:
            X, cx, n_lo, kc0, aff = A, ca, nv, 0, 0
            sc_x, sh_x = scale, shift
            tab = self._tap_table(dims, dims)
            rows = self._rows_buf(ly.cout, S, self.lib.bfm_tap_sum_rows, nv, ly.cout)
        else:
            X, cx, n_lo, kc0, aff = B, B.shape[-1], lo_dims[0] * lo_dims[1] * lo_dims[2], ca // 16, ly.cin
            sc_x, sh_x = scale[:, ca:], shift[:, ca:]
            tab = self._tap_table(lo_dims, dims)
            rows = None
        wsb = self.lib.bfm_conv3x3x3_tap_batch_workspace(cx, ly.cout, S, n_lo)

        def _launch_tap():
            ws = self._workspace(wsb)
            L.check(self.lib.bfm_conv3x3x3_tap_batch(L.ptr(X), cx, S, n_lo, L.ptr(sc_x), L.ptr(sh_x), L.ptr(bound), ly.groups,
                                                     L.ptr(wp), wexp, ly.cout, kc0, ly.cin // 16, self.passes, L.ptr(ws),
                                                     ws.numel(), aff, st), "conv_tap_batch " + ly.name)
            L.check(self.lib.bfm_tap_sum_batch(L.ptr(ws), cx, ly.cout, S, n_lo, L.ptr(tab), nv, self.slope,
                                               1 if B is None else 0, 0, L.ptr(out),
                                               L.ptr(rows[0]) if rows is not None else None, st),
                    "tap_sum_batch " + ly.name)
        self._bracket(_launch_tap, lambda: (2.0 * 27 * cx * ly.cout * nv * S,
                                            4.0 * (S * (n_lo * cx + nv * ly.cout) + 27 * cx * ly.cout),
                                            self._tag(ly) + "x%dtap" % S, cx, ly.cout, dims, (0,) * 8))
        if B is not None:
            # the skip half on conv_mfma itself (what decoders.0.2 runs at these shapes by the committed table): a fixed
            # choice, so that no shape of this route is ever timed in-process
            sk = self._skip_layer(ly, ca)
            sc_a, sh_a = scale[:, :ca], shift[:, :ca]
            key = (ca, ly.cout, tuple(dims), False, True, 1, "tap")
            cfg = self._batch_plan(key, (0,))
            self._pack(sk, True, 0)
            rows = self._rows_for(ca, ly.cout, dims, cfg, S)
            self._bracket(lambda: self._batch_launch(sk, cfg, A, None, None, dims, sc_a, sh_a, bound, out, rows, aff),
                          lambda: (2.0 * 27 * ca * ly.cout * nv * S, 4.0 * S * (nv * ca + 2 * nv * ly.cout),
                                   self._tag(ly) + "x%dsk" % S, ca, ly.cout, dims, cfg))
        if rows is not None:
            out._bfm_rows = rows
        return out

    def deep_region(self, tops, df=None):
        """tops: [(x, dims)] = the outputs of encoder level df-1 of S same-shape samples (each (D,H,W,C)); df defaults to
        deep_from.  Runs encoder levels >= df and the decoders that end at those levels on the whole batch.  Returns
        (out (S,d,h,w,C) = the decoder output at level df, its dims, [per-level feature batches, deepest first])."""
        S = len(tops)
        df = self.deep_from if df is None else df
        dims0 = tuple(tops[0][1])
        assert all(tuple(d) == dims0 for _, d in tops)
        c0 = tops[0][0].shape[-1]
        d = tuple(v // 2 for v in dims0)
        if min(dims0) < 2:
            raise L.BfmError("volume too small for %d pooling levels" % (len(self.enc) - 1))
        # level deep_from: pool every sample into its slot of the batch; the first layer's statistics come from the
        # pooling rows of each sample (the same call as the one-sample path)
        l1, l2 = self.enc[df]
        P = torch.empty((S,) + d + (c0,), dtype=torch.float32, device=self.device)
        scale = torch.empty((S, l1.cin), dtype=torch.float32, device=self.device)
        shift = torch.empty((S, l1.cin), dtype=torch.float32, device=self.device)
        bound = torch.empty((S, l1.groups), dtype=torch.float32, device=self.device)
        for s_, (x, dd) in enumerate(tops):
            ps, _ = self.maxpool(x, dd, out=P[s_])
            self._gn_stats(l1, ps, c0, None, 0, d, None, None, scale[s_], shift[s_], bound[s_], 0)
        x = self.batch_conv(l1, P, d, stats=(scale, shift, bound))
        x = self.batch_conv(l2, x, d)
        skips = [(x, d)]
        for i in range(df + 1, len(self.enc)):
            l1, l2 = self.enc[i]
            if min(d) < 2:
                raise L.BfmError("volume too small for %d pooling levels" % (len(self.enc) - 1))
            d2 = tuple(v // 2 for v in d)
            P = self.maxpool_batch(x, d)                     # one launch for the batch; its rows feed the next GroupNorm
            d = d2
            x = self.batch_conv(l1, P, d)
            x = self.batch_conv(l2, x, d)
            skips.insert(0, (x, d))
        feats = [(x, d)]
        skips = skips[1:]
        ndeep = len(self.enc) - 1 - df                      # decoders that end at a level >= deep_from
        for (l1, l2), (skip, sd_) in zip(self.dec[:ndeep], skips):
            y = self.batch_conv(l1, skip, sd_, B=x, lo_dims=d)
            x = self.batch_conv(l2, y, sd_)
            d = sd_
            feats.append((x, d))
        return x, d, feats

    def backbone_cl(self, x_cl, dims, mask_last=False):
        """x_cl: (D,H,W,Cin).  Returns the decoder feature maps as channels-last buffers,
        deepest first, the last one NOT yet L2-normalised (the tail kernel does that).
        mask_last: the caller keeps, of everything computed from the LAST feature map, only the voxels where the
        (one-channel) input is non-zero -- the tile loop, scripts/demo_test.py:88-100.  The last convolution then leaves
        out the boxes of voxels whose input is all zero (its own GroupNorm statistics come from the previous layer's
        full output, so nothing that is kept changes); that map holds unwritten memory there."""
        if self.has_deep_region():
            return self.backbone_batch([x_cl], dims, mask_last=mask_last)[0]
        self._uf_cache = {}                                  # flags live for one pass (keyed by the image's address)
        mask_last = mask_last and not self.dense_last
        mask_img = x_cl if (mask_last and self.mask_skip and x_cl.shape[-1] == 1) else None
        skips = self.encoder_top(x_cl, dims, len(self.enc))  # no batched region: every level, then every decoder
        x, d = skips.pop()
        return [(x, d)] + self.decoder_top(skips, x, d, mask_img=mask_img, df=len(self.enc) - 1, image=x_cl)

    def _layer_flags(self, key, image, dims):
        """uniform_flags of the input image for the layer UNIFORM_RADIUS lists under `key` (key[1]: its level), else None."""
        if key not in self.UNIFORM_RADIUS:
            return None
        return self.uniform_flags(image, dims, self.UNIFORM_RADIUS[key], key[1])

    def encoder_top(self, x_cl, dims, df=None):
        """Encoder levels < df (default deep_from) of one sample: ([(skip, dims)] shallowest first, top = last of them)."""
        skips = []
        x, d = x_cl, tuple(dims)
        nlev = self.deep_from if df is None else df
        for i, (l1, l2) in enumerate(self.enc[:nlev]):
            if i > 0:
                if min(d) < 2:
                    raise L.BfmError("volume %s too small for %d pooling levels" % (dims, len(self.enc) - 1))
                x, d = self.maxpool(x, d)
            f1, f2 = (self._layer_flags(("enc", i, j), x_cl, dims) for j in (0, 1))
            x = self.single_conv(l1, x, d, uni_flags=f1, reader=("conv", l2, f2))
            # read by the next level's pooling (fused: the pooled tensor is complete) and by the skip half of the decoder that
            # ends here; the last level's output goes to the region or the first decoder, which read every voxel
            rd = None
            if i + 1 < nlev and i < len(self.dec):
                rd = ("skip", self.dec[len(self.dec) - 1 - i][0], self._layer_flags(("dec", i), x_cl, dims))
            x = self.single_conv(l2, x, d, uni_flags=f2, pool=i + 1 < nlev, reader=rd)   # (the region pools the last level itself)
            skips.append((x, d))
        return skips

    def decoder_top(self, skips, x, d, mask_img=None, df=None, image=None):
        """Decoders that end above the batched levels, one sample: x (d) = this sample's slice of the region's output.
        mask_img: see backbone_cl(mask_last) -- applies to the last decoder's second convolution."""
        ndeep = len(self.enc) - 1 - (self.deep_from if df is None else df)
        feats = []
        nd = len(self.dec) - ndeep
        for k, ((l1, l2), (skip, sd_)) in enumerate(zip(self.dec[ndeep:], reversed(skips))):
            lvl = nd - 1 - k                                  # the level this decoder ends at
            uf = self._layer_flags(("dec", lvl), image, tuple(image.shape[:3])) if image is not None else None
            mk = mask_img if k == nd - 1 else None
            y = self.single_conv(l1, skip, sd_, B=x, lo_dims=d, uni_flags=uf,
                                 reader=("masked", l2, mk) if (mk is not None and mk is image) else None)
            x = self.single_conv(l2, y, sd_, mask_img=mk)
            d = sd_
            feats.append((x, d))
        return feats

    def backbone_batch(self, xs, dims, mask_last=False):
        """The backbone of S same-shape samples: encoder levels above the region per sample, the region batched, the
        remaining decoders per sample.  Returns one feature list per sample (deepest first, like backbone_cl).
        mask_last: as in backbone_cl."""
        self._uf_cache = {}                                  # flags live for one pass (keyed by the image's address)
        mask_last = mask_last and not self.dense_last
        df = self.region_start(dims)
        tops = [self.encoder_top(x, dims, df) for x in xs]
        out, d, deep_feats = self.deep_region([t[-1] for t in tops], df)
        res = []
        for s_, skips in enumerate(tops):
            feats = [(f[s_], fd) for f, fd in deep_feats]
            mask_img = xs[s_] if (mask_last and self.mask_skip and xs[s_].shape[-1] == 1) else None
            o_s = out[s_]
            rws = getattr(out, "_bfm_rows", None)
            if rws is not None:                               # this sample's rows of the region's last layer
                o_s._bfm_rows = (rws[0], rws[1], len(tops) * rws[1], s_ * rws[1])
            feats += self.decoder_top(skips, o_s, d, mask_img=mask_img, df=df, image=xs[s_])
            res.append(feats)
        return res

    @staticmethod
    def as_ncdhw(buf):
        """(D,H,W,C) buffer -> (1,C,D,H,W) view (channels_last_3d strides)."""
        return buf.permute(3, 0, 1, 2).unsqueeze(0)

    def to_cl(self, x):
        """(1,C,D,H,W) tensor of any layout -> (D,H,W,C) contiguous fp32 device buffer."""
        if x.dim() != 5 or x.shape[0] != 1:
            raise L.BfmError("expected a (1,C,D,H,W) tensor, got %s" % (tuple(x.shape),))
        x = x.to(device=self.device, dtype=torch.float32)
        return x[0].permute(1, 2, 3, 0).contiguous()

    # ------------------------------------------------------------------ hidden task-head layers
    def head_layers(self, widths):
        """The _HeadLayer records of TaskHead.layers (head.py:27-31) for task_f_maps = widths, read from the state dict's
        ``head.layers.{i}.main.{weight,bias}``; made once per engine."""
        key = tuple(int(w) for w in widths)
        if self._head_layers is None or self._head_layers[0] != key:
            layers = []
            for i in range(len(key) - 1):
                name = "head.layers.%d.main" % i
                hl = _HeadLayer()
                hl.name, hl.cin, hl.cout, hl.groups = name, key[i], key[i + 1], 1
                if hl.cin % 4 or hl.cout % 4:
                    raise L.BfmError("task_f_maps %s: the hidden head layers take widths that are multiples of 4" % (list(key),))
                hl.gamma = hl.beta = None
                hl.w_raw = self._dev(self.sd[name + ".weight"])
                hl.bias = self._dev(self.sd[name + ".bias"])
                if tuple(hl.w_raw.shape) != (hl.cout, hl.cin, 3, 3, 3) or tuple(hl.bias.shape) != (hl.cout,):
                    raise L.BfmError("%s has shapes %s / %s, expected %s / %s" % (name, tuple(hl.w_raw.shape), tuple(hl.bias.shape),
                                                                                 (hl.cout, hl.cin, 3, 3, 3), (hl.cout,)))
                hl.kind, hl.wpacked, hl.wexp, hl.packs, hl.skip = None, None, 0, {}, None
                layers.append(hl)
            self._head_layers = (key, layers)
        return self._head_layers[1]

    def _head_cfg(self, hl, dims):
        """The conv variant of a hidden head layer, by a fixed rule from the shape alone (never timed: the variants differ
        in the last bits): F(4,3) conv_wino4d where the volume holds its 8 x 8 x 4 box, conv_mfma elsewhere."""
        key = ("head", hl.cin, hl.cout, tuple(dims))
        if key not in self._plan_cache:
            cfg = (C.c_int * 8)()
            L.check(self.lib.bfm_conv3x3x3_mfma_plan(hl.cin, hl.cout, dims[0], dims[1], dims[2], cfg), "mfma_plan")
            box = (C.c_int * 3)()
            # D, H >= 8 and W >= 4: where bfm_conv3x3x3_wino4 dispatches to conv_wino4d (conv3d_wino4.hip, use_dma_kernel)
            f43 = (dims[0] >= 8 and dims[1] >= 8 and dims[2] >= 4
                   and self.lib.bfm_conv3x3x3_wino4_box(dims[0], dims[1], dims[2], self.passes, box) == 0
                   and list(box) == [8, 8, 4]
                   and self.lib.bfm_pack_conv_weights_wino4_bytes(hl.cin, hl.cout, self.passes) > 0)
            cfg[6], cfg[7] = (4 if f43 else 0), 0
            self._plan_cache[key] = cfg
        return self._plan_cache[key]

    def unit_bound(self):
        """A device float holding 1: the prescale bound of a tensor of unit vectors."""
        if self._unit_bound is None:
            self._unit_bound = torch.ones(1, dtype=torch.float32, device=self.device)
        return self._unit_bound

    def absmax(self, x):
        """max |x| of a contiguous fp32 tensor as a device float (bfm_absmax_f32)."""
        out = torch.zeros(1, dtype=torch.float32, device=self.device)
        L.check(self.lib.bfm_absmax_f32(L.ptr(x), 1, x.numel(), x.numel(), L.ptr(out), L.stream_ptr()), "absmax")
        return out

    def normalize(self, feat_cl, dims):
        """F.normalize(dim=1) of a (D,H,W,C) map alone: the tail kernel with no heads."""
        D, H, W = dims
        c = feat_cl.shape[-1]
        if c > 64 or c % 8:
            raise L.BfmError("unit_feat needs c_feat <= 64 and a multiple of 8 (got %d)" % c)
        if self._no_heads is None:
            self._no_heads = (torch.zeros(1, dtype=torch.float32, device=self.device),
                              torch.zeros(1, dtype=torch.int32, device=self.device))
        z, zi = self._no_heads
        desc = L.TailDesc(0, c, z.data_ptr(), z.data_ptr(), zi.data_ptr(), zi.data_ptr(), 0, 0, zi.data_ptr(), 0, 0, 0.0,
                          1, -1, -1, 0)
        out = torch.empty_like(feat_cl)
        L.check(self.lib.bfm_tail_heads(L.ptr(feat_cl), None, D * H * W, C.byref(desc), L.ptr(out), None, None, None, None,
                                        L.stream_ptr()), "normalize")
        return out

    def run_head_layers(self, layers, feat_cl, dims, mask_img=None, tape=None):
        """The hidden head layers on the backbone's raw last feature map (D,H,W,C): F.normalize first where the backbone
        has unit_feat (unet3d/model.py:207-208 runs before the head), then every layer (head.py:54-55).  Returns (the last
        layer's output, the feature map as the reference's out['feat'][-1] holds it).  mask_img: the caller keeps the
        heads' outputs only where this (D,H,W) image is non-zero (the tile loop); the last layer leaves out what it can.
        tape: a list that receives (layer, input, input bound, output) per layer (training)."""
        if feat_cl.shape[-1] != layers[0].cin:
            raise L.BfmError("task_f_maps starts at %d channels but the backbone's last feature map has %d"
                             % (layers[0].cin, feat_cl.shape[-1]))
        if self.unit_feat:
            fnorm = self.normalize(feat_cl, dims)
            bound = self.unit_bound()                        # unit vectors: every |x| <= 1
        else:
            fnorm = feat_cl
            bound = self.absmax(feat_cl)
        x = fnorm
        for i, hl in enumerate(layers):
            last = i + 1 == len(layers)
            y, nb = self.head_conv(hl, x, dims, bound, mask_img=mask_img if last else None,
                                   want_bound=(not last) or tape is not None)
            if tape is not None:
                tape.append((hl, x, bound, y))
            x, bound = y, nb
        return x, fnorm

    def head_conv(self, hl, x, dims, bound, mask_img=None, want_bound=True):
        """One hidden head layer, Conv3d(3, p=1) + bias + LeakyReLU(0.2) (head.py:161-167), on x (D,H,W,cin) whose
        max |x| the device float `bound` holds: the convolution through the matrix-core kernels with the identity affine
        and slope 1 (widths they do not take: conv_direct), then bfm_head_bias_lrelu in place, which also writes the
        output's own bound.  mask_img: the caller reads the output only where this (D,H,W) image is non-zero; the F(4,3)
        kernel then leaves out the boxes without such a voxel.  Returns (y, bound of y or None)."""
        D, H, W = dims
        st = L.stream_ptr()
        from .backward import _identity_affine
        ones, zeros = _identity_affine(self, hl.cin)
        out = torch.empty((D, H, W, hl.cout), dtype=torch.float32, device=self.device)
        if self._mfma_ok(hl, hl.cin, 0):
            cfg = self._head_cfg(hl, dims)
            ws = self._workspace(self.lib.bfm_conv3x3x3_mfma_workspace(hl.cin, hl.cout, D, H, W, cfg[5]))
            if mask_img is not None and not (cfg[6] == 4 and self.mask_skip and self.tape is None):
                mask_img = None
            self._bracket(lambda: self._conv_launch(hl, x, hl.cin, None, 0, dims, None, ones, zeros, bound, 1, cfg, out, ws,
                                                    None, slope=1.0, mask_img=mask_img),
                          lambda: (2.0 * 27 * hl.cin * hl.cout * D * H * W, 4.0 * D * H * W * (hl.cin + hl.cout),
                                   hl.name.replace("head.", ""), hl.cin, hl.cout, dims, cfg))
        else:
            mask_img = None
            self._pack(hl, False)
            L.check(self.lib.bfm_conv3x3x3_direct(L.ptr(x), hl.cin, None, 0, D, H, W, None, L.ptr(ones), L.ptr(zeros),
                                                  L.ptr(hl.wpacked), hl.cout, 1.0, L.ptr(out), st), "conv_direct " + hl.name)
        nb = torch.empty(1, dtype=torch.float32, device=self.device) if want_bound else None
        L.check(self.lib.bfm_head_bias_lrelu(L.ptr(out), L.ptr(hl.bias), hl.cout, D * H * W, HEAD_SLOPE, L.ptr(mask_img),
                                             L.ptr(nb), st), "head_bias_lrelu " + hl.name)
        return out, nb

    # ------------------------------------------------------------------ tail
    def make_tail(self, out_channels, left_hemis_only=False, max_surf_distance=3.0, uncertainty=False):
        return Tail(self, out_channels, left_hemis_only, max_surf_distance)


class Tail:
    """Head weights + role table for bfm_tail_heads (data-driven head set)."""
    hidden = ()                 # the engine's _HeadLayer records when the head has hidden layers (TaskHead.tail sets it)

    def __init__(self, eng, out_channels, left_hemis_only, max_surf_distance, c_feat=None, unit_feat=None):
        """c_feat / unit_feat: a head with hidden layers (task_f_maps longer than one) applies the 1x1x1 heads to the last
        hidden layer's task_f_maps[-1] channels, which are not normalised again (head.py:53-59); the defaults are the
        backbone's last width and its unit_feat."""
        self.eng = eng
        dev = eng.device
        sd = eng.sd
        self.out_channels = OrderedDict(out_channels)
        c_feat = eng.fm[0] if c_feat is None else int(c_feat)
        self.unit_feat = bool(eng.unit_feat if unit_feat is None else unit_feat)
        rows_w, rows_b, roles, names = [], [], [], []
        self.row_of = {}
        for task, n in self.out_channels.items():
            if n <= 0:
                raise L.BfmError("head '%s' (age-style pooled head) is outside the inference path" % task)
            w = torch.as_tensor(sd["head.final_conv_%s.weight" % task]).reshape(n, c_feat)
            b = torch.as_tensor(sd["head.final_conv_%s.bias" % task]).reshape(n)
            self.row_of[task] = (len(roles), n)
            rows_w.append(w)
            rows_b.append(b)
            for j in range(n):
                # every channel of a head goes through the head's post-processing: with `losses.uncertainty` set the
                # regression heads have a second (sigma) channel that the reference's UncertaintyProcessor never splits
                # off (joiner.py:50-55 looks for 'image' in the output names, none has it), so CT * 1000, exp(bias_field_log)
                # and residual + input see both channels (Trainer/models/__init__.py:307-352)
                if task == "CT":
                    r = L.ROLE_CT
                elif task == "bias_field_log":
                    r = L.ROLE_BIAS_LOG
                elif task == "segmentation":
                    r = L.ROLE_SEG
                elif task == "distance":
                    r = L.ROLE_DIST
                elif task == "high_res_residual":
                    r = L.ROLE_SR
                elif task == "pathology":
                    r = L.ROLE_PATHOL
                else:
                    r = L.ROLE_PLAIN
                roles.append(r)
                names.append((task, j))
        self.n_out = len(roles)
        self.c_feat = c_feat
        self.head_w = torch.cat(rows_w, 0).to(device=dev, dtype=torch.float32).contiguous()
        self.head_b = torch.cat(rows_b, 0).to(device=dev, dtype=torch.float32).contiguous()
        self.roles = torch.tensor(roles, dtype=torch.int32, device=dev)
        # output maps in post-processor order (Trainer/models/__init__.py:307-352)
        self.map_names = []
        slot_of_row = [-1] * self.n_out

        def add(name, row=None):
            self.map_names.append(name)
            if row is not None:
                slot_of_row[row] = len(self.map_names) - 1
            return len(self.map_names) - 1

        self.slot_high_res = -1
        self.slot_fake = -1
        self.channels = OrderedDict()                      # output key -> (first map row, channels): adjacent rows
        for task, (r0, n) in self.row_of.items():
            if task in ("T1", "T2", "FLAIR", "CT", "pathology", "bias_field_log", "high_res_residual"):
                key = "bias_field" if task == "bias_field_log" else task
                self.channels[key] = (add(key, r0), n)
                for j in range(1, n):
                    add("%s#%d" % (key, j), r0 + j)
            elif task == "distance":
                for j, nm in enumerate(["lp", "lw", "rp", "rw"][:n]):
                    add(nm, r0 + j)
            elif task == "registration":
                for j, nm in enumerate(["regx", "regy", "regz"][:n]):
                    add(nm, r0 + j)
            elif task == "segmentation":
                pass
            else:
                self.channels[task] = (add(task, r0), n)
                for j in range(1, n):
                    add("%s#%d" % (task, j), r0 + j)
        if "high_res_residual" in self.row_of:
            n = self.row_of["high_res_residual"][1]
            self.slot_high_res = add("high_res")           # one row per residual channel (slot_high_res + channel)
            self.channels["high_res"] = (self.slot_high_res, n)
            for j in range(1, n):
                add("high_res#%d" % j)
        if "distance" in self.row_of:
            self.slot_fake = add("fake_cortical")
        self.out_slot = torch.tensor(slot_of_row, dtype=torch.int32, device=dev)
        self.lut_list = LABELS_LEFT if left_hemis_only else LABELS_FULL
        seg = self.row_of.get("segmentation", (0, 0))
        if seg[1] and seg[1] != len(self.lut_list):
            raise L.BfmError("segmentation head has %d channels but the label list has %d" % (seg[1], len(self.lut_list)))
        self.seg_lut = torch.tensor(self.lut_list, dtype=torch.int32, device=dev)
        dist = self.row_of.get("distance", (0, 0))
        self.desc = L.TailDesc(self.n_out, c_feat, self.head_w.data_ptr(), self.head_b.data_ptr(),
                               self.roles.data_ptr(), self.out_slot.data_ptr(), seg[0], seg[1],
                               self.seg_lut.data_ptr(), dist[1], dist[0], float(max_surf_distance),
                               1 if self.unit_feat else 0, self.slot_high_res, self.slot_fake, len(self.map_names),
                               float(self.head_w.abs().max().item()) if self.n_out else 0.0, 0)

    def run(self, feat_cl, dims, input_cl=None, want_feat=True, want_seg=True, extra_rows=0, skip_zero_input=False):
        """Fused tail.  feat_cl: (D,H,W,c_feat) raw last decoder output.
        skip_zero_input: runs of 64 voxels whose input_cl is all zero are left unwritten (the tile loop discards them).
        Returns (maps: {name: (D,H,W) fp32}, feat_norm (D,H,W,C)|None, seg (D,H,W,n_seg)|None, label (D,H,W) int64|None).
        extra_rows: spare (D,H,W) rows at the end of the map buffer (self.last_buf) for per-tile maps computed after the
        tail (the deformed atlas), so that the stitcher still packs one buffer."""
        eng = self.eng
        D, H, W = dims
        nvox = D * H * W
        dev = eng.device
        fn_hidden = None
        if self.hidden:
            # hidden head layers: the heads read the last layer's output as it is; the feature map handed back is the
            # backbone's, normalised.  A tile (skip_zero_input) gives its mask to the last hidden layer
            mask = input_cl if (skip_zero_input and eng.mask_skip and input_cl is not None and input_cl.numel() == nvox) else None
            feat_cl, fn_hidden = eng.run_head_layers(self.hidden, feat_cl, dims, mask_img=mask)
            want_feat_out, want_feat = want_feat, False
        maps_buf = torch.empty((len(self.map_names) + int(extra_rows), D, H, W), dtype=torch.float32, device=dev)
        nseg = self.desc.n_seg
        feat_norm = torch.empty_like(feat_cl) if want_feat else None
        seg = torch.empty((D, H, W, nseg), dtype=torch.float32, device=dev) if (want_seg and nseg) else None
        label = torch.empty((D, H, W), dtype=torch.int64, device=dev) if nseg else None
        # the maps are the rows of one buffer (no pointer table to build on the device); skipping is a per-call flag, so
        # the one descriptor -- whose head_wmax the training step refreshes -- serves the tile loop and evaluate_image
        skip = 1 if (skip_zero_input and input_cl is not None and not want_feat and not want_seg) else 0
        L.check(eng.lib.bfm_tail_heads_rows(L.ptr(feat_cl), L.ptr(input_cl), nvox, C.byref(self.desc), L.ptr(feat_norm),
                                            L.ptr(maps_buf), nvox, L.ptr(seg), L.ptr(label), skip, L.stream_ptr()),
                "tail_heads")
        maps = OrderedDict((n, maps_buf[i]) for i, n in enumerate(self.map_names))
        self.last_buf = maps_buf                      # [n_maps][D,H,W]: the stitcher consumes all rows in one launch
        if fn_hidden is not None and want_feat_out:
            feat_norm = fn_hidden
        return maps, feat_norm, seg, label

    def run_raw(self, feat_cl, dims, want_feat=True, rows=False, apply_hidden=True):
        """TaskHead.forward only: raw logits (D,H,W,n_out) -- rows=True: (n_out, D*H*W), the training losses' layout --
        [+ normalised features].  apply_hidden=False: feat_cl is already the last hidden layer's output (the training
        step runs the hidden layers itself, for their tape)."""
        eng = self.eng
        D, H, W = dims
        if self.hidden and apply_hidden:
            hid, fn = eng.run_head_layers(self.hidden, feat_cl, dims)
            raw, _ = self.run_raw(hid, dims, want_feat=False, rows=rows, apply_hidden=False)
            return raw, (fn if want_feat else None)
        feat_norm = torch.empty_like(feat_cl) if (want_feat and self.unit_feat) else None
        if rows:
            raw = torch.empty((self.n_out, D * H * W), dtype=torch.float32, device=eng.device)
            L.check(eng.lib.bfm_tail_raw_rows(L.ptr(feat_cl), D * H * W, C.byref(self.desc), L.ptr(feat_norm), L.ptr(raw),
                                              D * H * W, L.stream_ptr()), "tail_raw_rows")
            return raw, feat_norm
        raw = torch.empty((D, H, W, self.n_out), dtype=torch.float32, device=eng.device)
        L.check(eng.lib.bfm_tail_heads(L.ptr(feat_cl), None, D * H * W, C.byref(self.desc), L.ptr(feat_norm), None,
                                       None, None, L.ptr(raw), L.stream_ptr()), "tail_heads(raw)")
        return raw, feat_norm
