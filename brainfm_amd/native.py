"""Inference results on the voxel grid of the scan the user handed in.

prepare_image resamples a scan to 1 mm (torch_resize), reorients `orig` to the identity axes (align_volume_to_ref; the
network's input `final` keeps the scan's axes, see processed_grid) and centre-crops; every map evaluate_image /
tiled_inference / tiled_inference_twostage returns lives on that processed grid.  The steps are affine in voxel
coordinates, so ``vox2vox(aff_processed, aff_native)`` maps a native voxel index to processed-voxel coordinates (the
half-voxel shifts of the zoom included) and two kernels of
csrc/affine_pull.hip bring the results back: K float maps in one launch, and class posteriors straight to labels
without a posterior volume on the native grid.  The reference has no counterpart.

    vox2vox(aff_src, aff_dst)                                        float64 4 x 4
    resample_maps(maps, aff_src, shape_dst, aff_dst, nearest=...)    dict or (K,D,H,W) tensor -> the same on shape_dst
    resample_labels(posteriors, lut, aff_src, shape_dst, aff_dst)    (1,C,D,H,W) -> int32 labels on shape_dst
    to_native(outputs, aff, native_shape, native_aff)                a whole result dict of the flows above

Volumes live on the HIP device, affines stay NumPy float64 on the host.  There is no CPU fallback."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from . import misc as MI
from .engine import LABELS_FULL, LABELS_LEFT

BfmError = L.BfmError

# outputs to_native leaves out: the feature pyramid, the posteriors themselves (they become `label`), scalars
_SKIPPED = ("feat", "segmentation", "age")


def vox2vox(aff_src, aff_dst):
    """inv(aff_src) @ aff_dst in float64: a voxel index of the DESTINATION grid -> voxel coordinates of the SOURCE grid
    (both affines are voxel -> world)."""
    a = np.asarray(aff_src, dtype=np.float64)
    b = np.asarray(aff_dst, dtype=np.float64)
    if a.shape != (4, 4) or b.shape != (4, 4):
        raise BfmError("vox2vox: affines must be 4 x 4, got %s and %s" % (a.shape, b.shape))
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        raise BfmError("vox2vox: non-finite affine")
    for name, m in (("aff_src", a), ("aff_dst", b)):
        lin = m[:3, :3]
        scale = np.abs(lin).max()
        if scale == 0 or abs(np.linalg.det(lin / scale)) < 1e-12:
            raise BfmError("vox2vox: singular affine (%s)" % name)
    return np.linalg.inv(a) @ b


def _m12(aff_src, aff_dst):
    return (C.c_double * 12)(*[float(v) for v in vox2vox(aff_src, aff_dst)[:3, :4].reshape(-1)])


def _shape3(shape, what):
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise BfmError("%s: a 3-D shape is needed, got %s" % (what, (shape,)))
    return shape


def _require_cuda(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise BfmError("%s runs on a HIP device only; there is no CPU fallback in the product path" % what)


def _rows_of_one_buffer(ts):
    """(base tensor, row stride in elements) when the (D,H,W) float32 tensors are contiguous, equally spaced rows of one
    allocation in this order (the stitched buffer of the tile flows), otherwise None."""
    t0 = ts[0]
    n = t0.numel()
    if any(not t.is_contiguous() or t.untyped_storage().data_ptr() != t0.untyped_storage().data_ptr() for t in ts):
        return None
    if len(ts) == 1:
        return t0, n
    stride = ts[1].storage_offset() - t0.storage_offset()
    if stride < n or any(t.storage_offset() != t0.storage_offset() + j * stride for j, t in enumerate(ts)):
        return None
    return t0, stride


def _first_tensor(maps):
    if isinstance(maps, torch.Tensor):
        return maps
    if isinstance(maps, dict):
        for v in maps.values():
            return v
    return None


@L.on_device(lambda maps, *a, **k: _first_tensor(maps))
def resample_maps(maps, aff_src, shape_dst, aff_dst, nearest=("label",)):
    """Pull K maps from the grid (their shape, aff_src) onto the grid (shape_dst, aff_dst) in one launch.

    maps: a dict of (D,H,W) tensors (what a tile flow returns) or a (K,D,H,W) tensor; float32, or int32 for a map pulled
    by nearest neighbour.  Dict entries named in ``nearest`` are pulled by nearest neighbour (bit patterns copied), every
    other one trilinearly with zeros outside the source; for a tensor, ``nearest`` holds row indices.  When the dict's
    tensors are the rows of one contiguous buffer, that buffer is read in place; otherwise they are stacked once.
    Returns the same container on the destination grid; its entries are rows of one (K,X,Y,Z) buffer."""
    is_dict = isinstance(maps, dict)
    if is_dict:
        if not maps:
            raise BfmError("resample_maps: no maps")
        keys, ts = list(maps.keys()), list(maps.values())
    else:
        _require_cuda(maps, "resample_maps")
        if maps.dim() != 4:
            raise BfmError("resample_maps: a (K,D,H,W) tensor or a dict of (D,H,W) tensors is needed, got %s"
                           % (tuple(maps.shape),))
        keys, ts = list(range(maps.shape[0])), list(maps.unbind(0))
    for k, t in zip(keys, ts):
        _require_cuda(t, "resample_maps")
        if t.dim() != 3:
            raise BfmError("resample_maps: map %r is not 3-D (shape %s)" % (k, tuple(t.shape)))
        if tuple(t.shape) != tuple(ts[0].shape):
            raise BfmError("resample_maps: map %r has shape %s, the first one %s" % (k, tuple(t.shape), tuple(ts[0].shape)))
    modes = [1 if k in tuple(nearest) else 0 for k in keys]
    for k, t, m in zip(keys, ts, modes):
        if t.dtype != torch.float32 and not (m == 1 and t.dtype == torch.int32):
            raise BfmError("resample_maps: map %r is %s; float32 (or int32 under nearest) is needed" % (k, t.dtype))
    shape_dst = _shape3(shape_dst, "resample_maps")
    M = _m12(aff_src, aff_dst)
    dtypes = [t.dtype for t in ts]
    ts = [t.view(torch.float32) if t.dtype == torch.int32 else t for t in ts]
    rows = _rows_of_one_buffer(ts)
    if rows is None:
        buf = torch.stack([t for t in ts], 0)
        rows = (buf, ts[0].numel())
    base, stride = rows
    d, h, w = ts[0].shape
    out = torch.empty((len(ts),) + shape_dst, dtype=torch.float32, device=base.device)
    L.check(L.load().bfm_affine_pull_multi(L.ptr(base), stride, len(ts), d, h, w, M, (C.c_int * len(ts))(*modes),
                                           shape_dst[0], shape_dst[1], shape_dst[2], L.ptr(out), L.stream_ptr()),
            "affine_pull_multi")
    if is_dict:
        return type(maps)((k, out[j] if dt == torch.float32 else out[j].view(dt))
                          for j, (k, dt) in enumerate(zip(keys, dtypes)))
    return out if maps.dtype == torch.float32 else out.view(maps.dtype)


def _lut_of(lut, n, dev):
    if hasattr(lut, "gen_args"):                                  # an InferenceSession: its label list
        lut = lut.gen_args.label_list_segmentation
    if lut is None:
        raise BfmError("resample_labels: a label list (or a session) is needed")
    if isinstance(lut, torch.Tensor):
        lut = lut.to(device=dev, dtype=torch.int32).contiguous()
    else:
        lut = torch.tensor([int(v) for v in lut], dtype=torch.int32, device=dev)
    if lut.numel() != n:
        raise BfmError("resample_labels: %d posterior channels but %d labels" % (n, lut.numel()))
    return lut


@L.on_device(lambda posteriors, *a, **k: posteriors)
def resample_labels(posteriors, lut, aff_src, shape_dst, aff_dst, return_max=False, lanes=0):
    """Labels on the grid (shape_dst, aff_dst) from class posteriors (1,C,D,H,W) on the grid aff_src: every posterior is
    interpolated trilinearly (zeros outside) and label = lut[first strict maximum], in one kernel that never writes a
    posterior on the destination grid.  A voxel where no interpolated posterior is positive -- outside the field of view
    included -- gets 0, ties go to the lower channel and a NaN never wins.

    lut: the label list (len C), or an InferenceSession, whose label list is taken.  Channels-last memory (what the
    network tail leaves `segmentation` in) is read in place, anything else is made channels-last once.
    Returns int32 (X,Y,Z), with return_max also the winning interpolated posterior as float32.
    lanes: how many lanes share a voxel (0: the library's choice, bfm_affine_pull_route; 1, 2, 4 .. 64 forces a width, for
    measurements and tests -- every width gives the same bits)."""
    _require_cuda(posteriors, "resample_labels")
    if posteriors.dim() != 5 or posteriors.shape[0] != 1:
        raise BfmError("resample_labels: posteriors must be (1,C,D,H,W), got %s" % (tuple(posteriors.shape),))
    if posteriors.dtype != torch.float32:
        raise BfmError("resample_labels: float32 posteriors are needed, got %s" % posteriors.dtype)
    shape_dst = _shape3(shape_dst, "resample_labels")
    M = _m12(aff_src, aff_dst)
    _, c, d, h, w = posteriors.shape
    cl = posteriors[0].permute(1, 2, 3, 0)                        # (D,H,W,C)
    if not cl.is_contiguous():
        cl = cl.contiguous()
    lut = _lut_of(lut, c, cl.device)
    label = torch.empty(shape_dst, dtype=torch.int32, device=cl.device)
    best = torch.empty(shape_dst, dtype=torch.float32, device=cl.device) if return_max else None
    L.check(L.load().bfm_affine_pull_argmax(L.ptr(cl), c, d, h, w, L.ptr(lut), M, shape_dst[0], shape_dst[1],
                                            shape_dst[2], int(lanes), L.ptr(label), L.ptr(best), L.stream_ptr()),
            "affine_pull_argmax")
    return (label, best) if return_max else label


def processed_grid(native_shape, native_aff, shape=None, aligned=False):
    """(shape, affine) of a grid prepare_image puts a scan (native_shape, native_aff) on, from the host arithmetic it runs:
    resize_plan and the zoom's affine update (half-voxel term included), then -- when ``shape`` is given and smaller --
    center_crop's offset (S - shape) // 2, applied ONCE.

    aligned=False: the grid of `final` and `high_res`, what the network sees and every inference output lies on.
    prepare_image, like the reference, passes them to align_volume_to_ref with the affine of the ALREADY aligned volume,
    which finds nothing to swap or flip: they keep the axes of the scan, resized to 1 mm.
    aligned=True: the grid of `orig`, the one output that is reoriented to the identity axes (align_plan between the
    resize and the crop); the `aff` prepare_image returns is this grid's affine when nothing is cropped."""
    native_shape = _shape3(native_shape, "processed_grid")
    aff = np.array(native_aff, dtype=np.float64)
    vox2vox(aff, aff)                                             # the finiteness and singularity checks
    newsize, _ = MI.resize_plan(native_shape, aff, 1.)
    factors = np.array(newsize) / np.array(native_shape)
    out = aff.copy()                                              # myzoom_torch_anisotropic's update
    for a in range(3):
        out[:-1, a] = out[:-1, a] / factors[a]
    out[:-1, -1] = out[:-1, -1] - aff[:-1, :-1] @ (0.5 - 0.5 / factors)
    full = tuple(int(v) for v in newsize)
    if aligned:
        perm, _, out = MI.align_plan(full, out, np.eye(4), 3)
        full = tuple(full[p] for p in perm)
    if shape is None:
        return full, out
    shape = _shape3(shape, "processed_grid")
    if any(s > f for s, f in zip(shape, full)):
        raise BfmError("processed_grid: %s does not fit in the scan's 1 mm grid %s" % (shape, full))
    start = np.array([(f - s) // 2 for s, f in zip(shape, full)], dtype=np.float64)
    out = out.copy()
    out[:-1, -1] = out[:-1, -1] + out[:-1, :-1] @ start
    return shape, out


def _output_grid_affine(aff, shape, native_shape, native_aff):
    """The affine of the grid the inference outputs of `shape` lie on, with the `aff` prepare_image returned as a check.

    That `aff` cannot be used as it stands.  It is the affine of `orig`, the reoriented volume, while the outputs keep the
    scan's axes (processed_grid), and prepare_image hands ONE array to its three center_crop calls (four with add_bf),
    each of which adds its crop offset in place, as in the reference: under a cropping win_size the offset is counted
    several times, for two different shapes.  The grid is fully determined by the scan and the outputs' shape, so it is
    rebuilt from those; `aff` has to be the aligned affine of this scan up to its offset, and tells a zero_crop_first
    result apart: there the volume shrank by more than a plane while `aff` did not move at all."""
    aff = np.asarray(aff, dtype=np.float64)
    vox2vox(aff, aff)
    full, _ = processed_grid(native_shape, native_aff)
    _, aff_al = processed_grid(native_shape, native_aff, aligned=True)
    lin = aff_al[:3, :3]
    if not np.allclose(aff[:3, :3], lin, rtol=0, atol=1e-6 * np.abs(lin).max()):
        raise BfmError("to_native: aff is not the affine prepare_image gives this scan (its axes differ); "
                       "use resample_maps for any other grid")
    _, aff_out = processed_grid(native_shape, native_aff, shape)
    t = np.linalg.solve(lin, aff[:3, 3] - aff_al[:3, 3])          # the offset aff carries, in voxels
    if any(f - s >= 2 for s, f in zip(shape, full)) and np.abs(t).max() < 1e-4:
        raise BfmError("to_native: the maps are %s, the scan's 1 mm grid is %s and aff carries no crop offset: a "
                       "zero_crop_first=True result.  zero_crop discards its offset (as the reference does), so nothing "
                       "says where the maps lie and they cannot be brought back" % (tuple(shape), full))
    return aff_out


def _spatial(t):
    """(D,H,W) view of a (D,H,W), (1,D,H,W) or (1,1,D,H,W) output; None for anything else."""
    if not isinstance(t, torch.Tensor):
        return None
    while t.dim() > 3 and t.shape[0] == 1:
        t = t[0]
    return t if t.dim() == 3 else None


@L.on_device(lambda outputs, *a, **k: _first_tensor(outputs))
def to_native(outputs, aff, native_shape, native_aff, label_from="auto", lut=None):
    """A result dict of evaluate_image(feature_only=False) / tiled_inference / tiled_inference_twostage on the voxel grid
    (native_shape, native_aff) of the scan prepare_image was given; ``aff`` is the affine prepare_image returned.

    Float maps are pulled trilinearly, all in one launch.  `label` comes from `segmentation` through the argmax kernel
    when the posteriors are present, otherwise from the stitched `label` by nearest neighbour; label_from = 'segmentation'
    or 'label' forces either source ('auto' picks as described); ``lut`` is the label list or the session (default: the
    shipped list with as many classes as there are posteriors).  `feat`, `segmentation` itself and scalar outputs (`age`)
    are left out of the result, not resampled: features are not meant for overlaying, the posteriors would be C volumes
    on the native grid (resample_maps brings single channels back when they are wanted), and a scalar has no grid.
    Entries that are not single-channel 3-D maps are left out as well.

    The outputs' grid is rebuilt from the scan and their shape (processed_grid); `aff` only has to belong to this scan,
    because it describes the reoriented `orig` and counts crop offsets once per center_crop call, like the reference's
    (_output_grid_affine).  A zero_crop_first=True result is refused by name; one that lost a single plane cannot be
    told from center_crop's own crop by one and is taken for that."""
    if not isinstance(outputs, dict) or not outputs:
        raise BfmError("to_native: a dict of outputs is needed")
    if label_from not in ("auto", "segmentation", "label"):
        raise BfmError("to_native: label_from must be 'auto', 'segmentation' or 'label', got %r" % (label_from,))
    native_shape = _shape3(native_shape, "to_native")
    seg = outputs.get("segmentation")
    if label_from == "segmentation" and seg is None:
        raise BfmError("to_native: label_from='segmentation' but the outputs hold no posteriors")
    if label_from == "label" and "label" not in outputs:
        raise BfmError("to_native: label_from='label' but the outputs hold no label map")
    use_seg = seg is not None and label_from in ("auto", "segmentation")
    maps, dtypes = OrderedDict(), {}
    for k, v in outputs.items():
        if k in _SKIPPED or (k == "label" and use_seg):
            continue
        if isinstance(v, torch.Tensor) and v.dim() == 5 and v.shape[1] > 1:
            continue
        t = _spatial(v)
        if t is None:
            if isinstance(v, torch.Tensor) and v.dim() >= 2 and k != "label":
                raise BfmError("to_native: output %r is not a 3-D map (shape %s)" % (k, tuple(v.shape)))
            continue
        _require_cuda(t, "to_native")
        if k == "label" and t.dtype != torch.float32:
            dtypes[k] = t.dtype
            t = t.to(torch.int32)
        maps[k] = t
    shape = tuple(seg.shape[2:]) if use_seg else None
    if maps:
        shape = tuple(next(iter(maps.values())).shape)
    if shape is None:
        raise BfmError("to_native: nothing to resample")
    aff_true = _output_grid_affine(aff, shape, native_shape, native_aff)
    out = OrderedDict()
    if maps:
        res = resample_maps(maps, aff_true, native_shape, native_aff, nearest=("label",))
        for k, v in res.items():
            out[k] = v.to(dtypes[k]) if k in dtypes else v
    if use_seg:
        _require_cuda(seg, "to_native")
        if tuple(seg.shape[2:]) != shape:
            raise BfmError("to_native: segmentation is %s, the maps %s" % (tuple(seg.shape[2:]), shape))
        if lut is None:                                           # the shipped label list with this many classes
            lut = {len(LABELS_LEFT): LABELS_LEFT, len(LABELS_FULL): LABELS_FULL}.get(int(seg.shape[1]))
            if lut is None:
                raise BfmError("to_native: %d posterior channels match no shipped label list; pass lut=" % seg.shape[1])
        out["label"] = resample_labels(seg, lut, aff_true, native_shape, native_aff)
    return out

