"""Mirror of ``Trainer/models/evaluator.py``: the scores of the reference's test flow, computed on the HIP device.

Same names, arguments and return structures as the reference (``{metric_name: 0-d numpy value}``, a Python float for PSNR);
the arithmetic runs in libbrainfm_hip.so (``csrc/eval_metrics.hip``), there is no CPU fallback:

  get_l1 / get_psnr / get_normalized_l2   one pass over both volumes (bfm_eval_pair_stats), host arithmetic on ten numbers
  get_dice                                per-plane sums (bfm_eval_channel_sums); label maps go through
                                          bfm_eval_label_counts and never become a one-hot
  get_ssim / get_ms_ssim                  pytorch_msssim 1.0's algorithm, fused (bfm_eval_ssim3d, bfm_eval_avgpool2_pair);
                                          BFM_SSIM_FUSED=0 selects the route composed of the older kernels instead

``Evaluator.eval_tensors`` is ``eval`` after the file reads, for tensors that are already on the device.  Scalars stay in
device memory between kernels: a metric call reads back once, at its end.  DESIGN.md section 8 lists the reference's quirks
that are kept (and the one that is fixed).
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib as L
from .volio import MRIread, MRIwrite

#########################################

# some constants
label_list_segmentation = [0, 14, 15, 16, 24, 77, 85, 2, 3, 4, 7, 8, 10, 11, 12, 13, 17, 18, 26, 28, 41,
                           42, 43, 46, 47, 49, 50, 51, 52, 53, 54, 58, 60]  # 33
n_neutral_labels = 7
n_labels = len(label_list_segmentation)
nlat = int((n_labels - n_neutral_labels) / 2.0)
vflip = np.concatenate([np.array(range(n_neutral_labels)),
                        np.array(range(n_neutral_labels + nlat, n_labels)),
                        np.array(range(n_neutral_labels, n_neutral_labels + nlat))])

N_LUT = 10000
WIN_SIZE = 11
MS_WEIGHTS = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]
C1, C2 = 0.01 ** 2, 0.03 ** 2


def _device(device, what):
    d = torch.device(device) if not isinstance(device, torch.device) else device
    if d.type != "cuda" or not torch.cuda.is_available():
        raise L.BfmError("%s runs on a HIP device only; there is no CPU fallback in the product path" % what)
    return d


_LUT = {}


def _lut(device):
    key = str(device)
    if key not in _LUT:
        lut = np.zeros(N_LUT, dtype=np.int32)
        for l in range(n_labels):
            lut[label_list_segmentation[l]] = l
        _LUT[key] = torch.from_numpy(lut).to(device)
    return _LUT[key]


def _check_label_range(label):
    if label.size and (label.min() < 0 or label.max() >= N_LUT):
        bad = label.max() if label.max() >= N_LUT else label.min()
        raise IndexError("index %d is out of bounds for dimension 0 with size %d" % (int(bad), N_LUT))


@L.on_device(lambda label, device: device)
def get_onehot(label, device):
    """evaluator.py:30-40: (n_labels, D, H, W) one-hot of a label volume through the 10 000-entry LUT (bfm_onehot_lut)."""
    device = _device(device, "get_onehot")
    lab = np.squeeze(np.asarray(label)).astype(np.int64)
    _check_label_range(lab)
    S = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).to(device)
    out = torch.empty(tuple(S.shape) + (n_labels,), dtype=torch.float32, device=device)
    if S.numel():
        L.check(L.load().bfm_onehot_lut(L.ptr(S), L.ptr(_lut(device)), N_LUT, n_labels, S.numel(), L.ptr(out),
                                        L.stream_ptr()), "onehot_lut")
    return out.permute([3, 0, 1, 2])


def align_shape(nda1, nda2):
    if nda1.shape != nda2.shape:
        print('pre-align', nda1.shape, nda2.shape)
        s = min(nda1.shape[0], nda2.shape[0])
        r = min(nda1.shape[1], nda2.shape[1])
        c = min(nda1.shape[2], nda2.shape[2])
        nda1 = nda1[:s, :r, :c]
        nda2 = nda2[:s, :r, :c]
        print('post-align', nda1.shape, nda2.shape)
    return nda1, nda2


def gaussian_window(sigma):
    """pytorch_msssim's _fspecial_gauss_1d(11, sigma), built in fp32 as the library builds it."""
    coords = torch.arange(WIN_SIZE, dtype=torch.float)
    coords -= WIN_SIZE // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    g /= g.sum()
    return g


def ssim_fused_default():
    """The fused kernel unless BFM_SSIM_FUSED=0 asks for the route composed of bfm_conv1d_axis, element-wise kernels and
    reductions (the on-device cross-check and the bench baseline)."""
    return os.environ.get("BFM_SSIM_FUSED", "1") != "0"


def _ws(device, nbytes):
    from .generator_utils import workspace
    return workspace(device, max(int(nbytes), 8))


def _as5(t, device, what):
    """(D,H,W) / (C,D,H,W) / (B,C,D,H,W) -> contiguous fp32 (B,C,D,H,W) on the device."""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t))
    if t.dim() == 3:
        t = t[None, None]
    elif t.dim() == 4:
        t = t[None]
    if t.dim() != 5:
        raise ValueError("%s takes (D,H,W), (C,D,H,W) or (B,C,D,H,W) volumes, got %s" % (what, tuple(t.shape)))
    return t.to(device=device, dtype=torch.float32).contiguous()


def _pair(output, target, device, what):
    o, t = _as5(output, device, what), _as5(target, device, what)
    if o.shape != t.shape:
        raise ValueError("%s: output %s and target %s differ in shape" % (what, tuple(o.shape), tuple(t.shape)))
    if o.numel() == 0:
        raise ValueError("%s: empty volume" % what)
    return o, t


def pair_stats_dev(o, t):
    """The ten numbers of bfm_eval_pair_stats as a device fp64 tensor (no host sync): sum|o-t|, sum(o-t)^2, sum(o t),
    sum(o^2), sum(t^2), min o, max o, min t, max t, count(t != 0)."""
    lib = L.load()
    stats = torch.empty(10, dtype=torch.float64, device=o.device)
    ws = _ws(o.device, lib.bfm_eval_pair_stats_workspace())
    L.check(lib.bfm_eval_pair_stats(L.ptr(o), L.ptr(t), o.numel(), L.ptr(stats), L.ptr(ws), ws.numel(), L.stream_ptr()),
            "eval_pair_stats")
    return stats


def label_counts(pred, target, device):
    """(|P_l|, |T_l|, |P_l & T_l|) per class as int64 numpy arrays, from two label volumes (host or device, any integer or
    float dtype); raises the reference's IndexError when a label lies outside the LUT."""
    device = _device(device, "label_counts")
    lib = L.load()

    def dev_i32(x):
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
        return x.to(device).to(torch.int32).contiguous()

    P, T = dev_i32(pred), dev_i32(target)
    if P.numel() != T.numel() or P.numel() == 0:
        raise ValueError("label volumes differ in size: %s, %s" % (tuple(P.shape), tuple(T.shape)))
    counts = torch.empty(3 * n_labels + 1, dtype=torch.int64, device=device)
    L.check(lib.bfm_eval_label_counts(L.ptr(P), L.ptr(T), P.numel(), L.ptr(_lut(device)), N_LUT, n_labels, L.ptr(counts),
                                      L.stream_ptr()), "eval_label_counts")
    c = counts.cpu().numpy()
    if c[3 * n_labels]:
        raise IndexError("%d label(s) out of bounds for dimension 0 with size %d" % (int(c[3 * n_labels]), N_LUT))
    return c[:n_labels], c[n_labels:2 * n_labels], c[2 * n_labels:3 * n_labels]


def _score32(v):
    return np.asarray(v, dtype=np.float32)


class Evaluator:
    """
    This class computes the evaluation scores for BrainID.
    """
    def __init__(self, args, metric_names, device):

        self.args = args
        self.metric_names = metric_names
        self.device = device

        # no shipped config of the reference defines ssim_win_sigma (its constructor raises AttributeError on them):
        # pytorch_msssim's default
        self.win_sigma = getattr(args, 'ssim_win_sigma', 1.5)

        self.metric_map = {
            'seg_dice': self.get_dice,
            'pathol_dice': self.get_dice,

            'feat_l1': self.get_l1,
            'recon_l1': self.get_l1,
            'sr_l1': self.get_l1,

            'bf_normalized_l2': self.get_normalized_l2,
            'bf_corrected_l1': self.get_l1,

            'recon_psnr': self.get_psnr,
            'sr_psnr': self.get_psnr,

            'feat_ssim': self.get_ssim,
            'recon_ssim': self.get_ssim,
            'sr_ssim': self.get_ssim,

            'feat_ms_ssim': self.get_ms_ssim,
            'recon_ms_ssim': self.get_ms_ssim,
            'sr_ms_ssim': self.get_ms_ssim,
        }

    # ------------------------------------------------------------------------- helpers
    def _dev(self, what):
        return _device(self.device, what)

    def _run(self, fn, *a, **k):
        d = self._dev(fn.__name__)
        if d.index is not None and d.index != torch.cuda.current_device():
            with torch.cuda.device(d):
                return fn(d, *a, **k)
        return fn(d, *a, **k)

    # ------------------------------------------------------------------------- metrics
    def get_dice(self, metric_name, output, target, *kwargs):
        """
        Dice of segmentation
        """
        return self._run(self._dice, metric_name, output, target)

    def _dice(self, dev, metric_name, output, target):
        o, t = _pair(output, target, dev, "get_dice")
        lib = L.load()
        planes = o.shape[0] * o.shape[1]
        n_per = o.numel() // planes
        sums = torch.empty((planes, 2), dtype=torch.float64, device=dev)
        ws = _ws(dev, lib.bfm_eval_channel_sums_workspace(planes, n_per))
        L.check(lib.bfm_eval_channel_sums(L.ptr(o), L.ptr(t), planes, n_per, L.ptr(sums), L.ptr(ws), ws.numel(),
                                          L.stream_ptr()), "eval_channel_sums")
        s = sums.cpu().numpy()
        return {metric_name: _score32(np.mean(2.0 * s[:, 0] / np.maximum(s[:, 1], 1e-5)))}

    def get_dice_labels(self, metric_name, pred_labels, target_labels):
        """get_dice(get_onehot(pred), get_onehot(target)) from the label volumes themselves: integer counts per class."""
        p, t, i = self._run(lambda dev: label_counts(pred_labels, target_labels, dev))
        dice = 2.0 * i.astype(np.float64) / np.maximum((p + t).astype(np.float64), 1e-5)
        return {metric_name: _score32(np.mean(dice))}

    def get_normalized_l2(self, metric_name, output, target, *kwargs):
        return self._run(self._normalized_l2, metric_name, output, target)

    def _normalized_l2(self, dev, metric_name, output, target):
        o, t = _pair(output, target, dev, "get_normalized_l2")
        s = pair_stats_dev(o, t).cpu().numpy()
        sot, soo, stt = s[2], s[3], s[4]
        w = sot / (soo + 1e-7)
        # sum (w o - t)^2 expanded; fp64 sums of fp32 products keep 1e-16 * sum(t^2), far below any score that fp32 resolves
        num = max(w * w * soo - 2.0 * w * sot + stt, 0.0)
        return {metric_name: _score32(0. + math.sqrt(num / (stt + 1e-7)))}

    def get_l1(self, metric_name, output, target, nonzero_only=False, *kwargs):
        return self._run(self._l1, metric_name, output, target, nonzero_only)

    def _l1(self, dev, metric_name, output, target, nonzero_only):
        o, t = _pair(output, target, dev, "get_l1")
        if nonzero_only:  # compute only within face_aware_region #
            # the reference sums over dim 0, the batch: the result is a (C,D,H,W) volume, NaN where the target is zero
            lib = L.load()
            out = torch.empty(tuple(o.shape[1:]), dtype=torch.float32, device=dev)
            L.check(lib.bfm_eval_l1_nonzero(L.ptr(o), L.ptr(t), o.shape[0], out.numel(), L.ptr(out), L.stream_ptr()),
                    "eval_l1_nonzero")
            return {metric_name: out.cpu().numpy()}
        s = pair_stats_dev(o, t).cpu().numpy()
        return {metric_name: _score32(s[0] / o.numel())}

    def get_psnr(self, metric_name, output, target, *kwargs):
        return self._run(self._psnr, metric_name, output, target)

    def _psnr(self, dev, metric_name, output, target):
        o, t = _pair(output, target, dev, "get_psnr")
        s = pair_stats_dev(o, t).cpu().numpy()
        mse = s[1] / o.numel()
        if mse == 0:
            psnr = float('inf')
        else:
            psnr = 20 * math.log10(s[8] / math.sqrt(mse))
        return {metric_name: psnr}

    def get_ssim(self, metric_name, output, target, *kwargs):
        '''
        Ref: https://github.com/jorge-pessoa/pytorch-msssim
        '''
        return self._run(self._ssim, metric_name, output, target)

    def _ssim(self, dev, metric_name, output, target):
        o, t = _pair(output, target, dev, "get_ssim")
        _require_3d(o)
        stats = pair_stats_dev(o, t)
        res = ssim_planes_dev(o, t, gaussian_window(self.win_sigma), stats[5:9]).cpu().numpy()
        B, Cc = o.shape[:2]
        return {metric_name: _score32(res[:, 0].reshape(B, Cc).mean(1).mean())}

    def get_ms_ssim(self, metric_name, output, target, *kwargs):
        '''
        Ref: https://github.com/jorge-pessoa/pytorch-msssim
        '''
        return self._run(self._ms_ssim, metric_name, output, target)

    def _ms_ssim(self, dev, metric_name, output, target):
        o, t = _pair(output, target, dev, "get_ms_ssim")
        _require_3d(o)
        sizes = [list(o.shape[2:])]
        for _ in range(len(MS_WEIGHTS) - 1):
            sizes.append([(n + 1) // 2 for n in sizes[-1]])
        # the library's size assertion looks at the last two axes only; a depth that reaches 1 before the last pooling makes
        # F.avg_pool3d raise instead -- the reference's bare except turns both into the same message and nan
        if not min(o.shape[-2:]) > (WIN_SIZE - 1) * 2 ** 4 or min(min(sz) for sz in sizes[:-1]) < 2:
            print('Error in MS-SSIM: Image too small for Multi-scale SSIM computation. Skipping...')
            return {metric_name: float('nan')}
        stats = pair_stats_dev(o, t)
        res = ms_ssim_levels_dev(o, t, gaussian_window(self.win_sigma), stats[5:9]).cpu().numpy()   # (5, planes, 2)
        levels = np.concatenate([res[:-1, :, 1], res[-1:, :, 0]], axis=0)
        levels = np.maximum(levels, 0.0)                                    # relu; NaN stays NaN
        val = np.prod(levels ** np.asarray(MS_WEIGHTS, dtype=np.float64)[:, None], axis=0)
        B, Cc = o.shape[:2]
        return {metric_name: _score32(val.reshape(B, Cc).mean(1).mean())}

    def get_score(self, metric_name, output, target, **kwargs):
        assert metric_name in self.metric_map, f'do you really want to compute {metric_name} metric?'
        return self.metric_map[metric_name](metric_name, output, target, **kwargs)

    # ------------------------------------------------------------------------- flows
    def eval_tensors(self, pred, target, clamp=False, is_seg=False, normalize=False, **kwargs):
        """The part of ``eval`` after the file reads, on tensors (device or host) or arrays: (D,H,W), (C,D,H,W) or
        (B,C,D,H,W); with is_seg, two label volumes.  Label maps go to the Dice through integer counts; any other metric
        asked for with is_seg sees the one-hot maps, as in the reference."""
        dev = self._dev("eval_tensors")
        score = {}
        if is_seg:
            onehots = None
            for metric_name in self.metric_names:
                assert metric_name in self.metric_map, f'do you really want to compute {metric_name} metric?'
                if self.metric_map[metric_name] == self.get_dice:
                    score.update(self.get_dice_labels(metric_name, pred, target))
                    continue
                if onehots is None:
                    onehots = tuple(get_onehot(x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x), dev)[None]
                                    for x in (pred, target))
                score.update(self.get_score(metric_name, onehots[0], onehots[1], **kwargs))
            return score
        p, t = _pair(pred, target, dev, "eval_tensors")
        if normalize:
            p = self._run(_minmax_normalised, p)
        if clamp:
            p = torch.clamp(p, min=0., max=1.)
            t = torch.clamp(t, min=0., max=1.)
        for metric_name in self.metric_names:
            score.update(self.get_score(metric_name, p, t, **kwargs))
        return score

    def eval(self, pred_path, target_path, clamp=False, is_seg=False, normalize=False, add_mask=False, flip=False,
             kill_target_labels=[], **kwargs):
        self._dev("eval")
        pred = MRIread(pred_path, im_only=True, dtype='int' if 'label' in os.path.basename(pred_path) else 'float')
        target, aff = MRIread(target_path, im_only=False,
                              dtype='int' if 'label' in os.path.basename(target_path) else 'float')

        pred, target = align_shape(pred, target)

        if flip:
            pred = np.flip(pred, 0)

        for label in kill_target_labels:
            target[target == label] = 0
            pred[pred == label] = 0

        if add_mask and '_masked' not in pred_path:
            pred[target == 0] = 0
            pred[pred < 0] = 0
            MRIwrite(pred, aff, pred_path.split('.')[0] + '_masked.nii.gz')

        if normalize:
            pred = (pred - np.min(pred)) / (np.max(pred) - np.min(pred))

        if is_seg:
            return self.eval_tensors(np.squeeze(pred).copy(), np.squeeze(target), clamp=clamp, is_seg=True, **kwargs)
        pred = torch.tensor(np.squeeze(pred).copy(), dtype=torch.float32)
        target = torch.tensor(np.squeeze(target), dtype=torch.float32)
        return self.eval_tensors(pred, target, clamp=clamp, is_seg=False, normalize=False, **kwargs)


def _require_3d(o):
    # pytorch_msssim squeezes singleton spatial axes and treats the 4-D result as a batch of 2-D images
    if any(s == 1 for s in o.shape[2:]):
        raise NotImplementedError("SSIM of 2-D images (a spatial axis of length 1) is not implemented: 3-D volumes only")


def _minmax_normalised(dev, p):
    """(p - min) / (max - min) over the whole tensor, scalars on the device (eval's `normalize`)."""
    lib = L.load()
    stats = pair_stats_dev(p, p)
    q = p.clone()
    L.check(lib.bfm_minmax_normalise(L.ptr(q), q.numel(), L.ptr(stats[5:7]), L.stream_ptr()), "minmax_normalise")
    return q


# --------------------------------------------------------------------------------------------- SSIM on the device
def _win_arg(win):
    w = win.to(torch.float32).cpu().numpy()
    assert w.shape == (WIN_SIZE,)
    return (C.c_float * WIN_SIZE)(*[float(v) for v in w])


def ssim_planes_dev(X, Y, win, norm_dev=None, fused=None, out=None):
    """{mean ssim, mean cs} per (b, c) plane of two (B,C,D,H,W) fp32 device tensors as a (B*C, 2) fp64 device tensor.
    norm_dev: 4 device doubles {min X, max X, min Y, max Y} applied on load, or None."""
    if fused is None:
        fused = ssim_fused_default()
    lib = L.load()
    B, Cc, D, H, W = X.shape
    planes = B * Cc
    if out is None:
        out = torch.empty((planes, 2), dtype=torch.float64, device=X.device)
    if not fused:
        return _ssim_composed(X, Y, win, norm_dev, out)
    ws = _ws(X.device, lib.bfm_eval_ssim3d_workspace(planes, D, H, W))
    L.check(lib.bfm_eval_ssim3d(L.ptr(X), L.ptr(Y), planes, D, H, W, _win_arg(win), L.ptr(norm_dev), L.ptr(out), L.ptr(ws),
                                ws.numel(), L.stream_ptr()), "eval_ssim3d")
    return out


def avgpool2_pair_dev(X, Y, norm_dev=None):
    lib = L.load()
    B, Cc, D, H, W = X.shape
    shape = (B, Cc, (D + 1) // 2, (H + 1) // 2, (W + 1) // 2)
    Xo = torch.empty(shape, dtype=torch.float32, device=X.device)
    Yo = torch.empty(shape, dtype=torch.float32, device=X.device)
    L.check(lib.bfm_eval_avgpool2_pair(L.ptr(X), L.ptr(Y), B * Cc, D, H, W, L.ptr(norm_dev), L.ptr(Xo), L.ptr(Yo),
                                       L.stream_ptr()), "eval_avgpool2_pair")
    return Xo, Yo


def ms_ssim_levels_dev(X, Y, win, norm_dev=None, fused=None):
    """The five scales' {mean ssim, mean cs} per plane: a (5, B*C, 2) fp64 device tensor."""
    planes = X.shape[0] * X.shape[1]
    res = torch.empty((len(MS_WEIGHTS), planes, 2), dtype=torch.float64, device=X.device)
    for i in range(len(MS_WEIGHTS)):
        ssim_planes_dev(X, Y, win, norm_dev, fused=fused, out=res[i])
        if i < len(MS_WEIGHTS) - 1:
            X, Y = avgpool2_pair_dev(X, Y, norm_dev)
            norm_dev = None                                  # the pooled volumes are normalised already
    return res


def _ssim_composed(X, Y, win, norm_dev, out):
    """The unfused route: five moment volumes from bfm_conv1d_axis (same-size, zero-padded: its interior is the 'valid'
    result), element-wise kernels for the products and the SSIM expression, bfm_crop3d for the interior and bfm_reduce_f32
    for the means.  Only kernels older than the evaluator; kept as the cross-check of the fused kernel and its baseline."""
    from . import generator_utils as GU
    lib = L.load()
    B, Cc, D, H, W = X.shape
    dev = X.device
    wdev = win.to(device=dev, dtype=torch.float32).contiguous()
    half = WIN_SIZE // 2
    dims = (D, H, W)
    filt = [n >= WIN_SIZE for n in dims]
    lo = [half if f else 0 for f in filt]
    od = [n - 2 * half if f else n for n, f in zip(dims, filt)]
    cnt = float(od[0] * od[1] * od[2])

    def blur(v):
        cur = v
        for ax in range(3):
            if filt[ax]:
                nxt = torch.empty_like(cur)
                L.check(lib.bfm_conv1d_axis(L.ptr(cur), D, H, W, ax, L.ptr(wdev), WIN_SIZE, L.ptr(nxt), L.stream_ptr()),
                        "conv1d_axis")
                cur = nxt
        return cur

    def interior_mean(v, dst):
        c = torch.empty(od, dtype=torch.float32, device=dev)
        L.check(lib.bfm_crop3d(L.ptr(v), D, H, W, lo[0], lo[1], lo[2], od[0], od[1], od[2], L.ptr(c), L.stream_ptr()),
                "crop3d")
        dst.copy_((GU.reduce_dev(2, c) / cnt)[0])

    Xf, Yf = X.reshape(B * Cc, D, H, W), Y.reshape(B * Cc, D, H, W)
    for p in range(B * Cc):
        x, y = Xf[p], Yf[p]
        if norm_dev is not None:
            x, y = x.clone(), y.clone()
            L.check(lib.bfm_minmax_normalise(L.ptr(x), x.numel(), L.ptr(norm_dev[0:2]), L.stream_ptr()), "minmax_normalise")
            L.check(lib.bfm_minmax_normalise(L.ptr(y), y.numel(), L.ptr(norm_dev[2:4]), L.stream_ptr()), "minmax_normalise")
        mu1, mu2 = blur(x), blur(y)
        gxx, gyy, gxy = (blur(GU.ew_binary(L.EW_MUL, a, b)) for a, b in ((x, x), (y, y), (x, y)))
        mu1_sq, mu2_sq, mu12 = GU.ew_binary(L.EW_MUL, mu1, mu1), GU.ew_binary(L.EW_MUL, mu2, mu2), GU.ew_binary(L.EW_MUL, mu1, mu2)
        s1 = GU.ew_binary(L.EW_AXPY, gxx, mu1_sq, -1.0)
        s2 = GU.ew_binary(L.EW_AXPY, gyy, mu2_sq, -1.0)
        s12 = GU.ew_binary(L.EW_AXPY, gxy, mu12, -1.0)
        cs = GU.ew_binary(L.EW_DIV2, GU.ew_unary(L.EW_AFFINE, s12, 2.0, C2),
                          GU.ew_unary(L.EW_AFFINE, GU.ew_binary(L.EW_ADD, s1, s2), 1.0, C2))
        lum = GU.ew_binary(L.EW_DIV2, GU.ew_unary(L.EW_AFFINE, mu12, 2.0, C1),
                           GU.ew_unary(L.EW_AFFINE, GU.ew_binary(L.EW_ADD, mu1_sq, mu2_sq), 1.0, C1))
        ss = GU.ew_binary(L.EW_MUL, lum, cs)
        interior_mean(ss, out[p, 0])
        interior_mean(cs, out[p, 1])
    return out
