"""Seeded parameters and fixture access shared by tests/golden/make_golden_twostage.py and the two-stage tests.

The wide (64-map) nets of the two-stage fixtures are not stored: every parameter is drawn here from
torch.Generator().manual_seed(seed) in state-dict order, and the fixture keeps names, shapes and sha256 of each tensor."""
import hashlib
import os
from collections import OrderedDict

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEAD_GAIN = 30.0            # the pathology / segmentation heads are scaled so that p spans (0, 1) and labels are decisive
SCALED_HEADS = ("head.final_conv_pathology.weight", "head.final_conv_segmentation.weight")


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def draw_state_dict(names, shapes, seed):
    """{name: fp32 tensor} in the order given.  GroupNorm weights around 1, GroupNorm and head biases around 0, conv
    weights uniform within 1/sqrt(fan_in) (nn.Conv3d's default range); the heads of SCALED_HEADS times about HEAD_GAIN."""
    g = torch.Generator().manual_seed(int(seed))
    sd = OrderedDict()
    for name, shape in zip(names, shapes):
        shape = tuple(int(s) for s in shape)
        r = torch.rand(shape, generator=g) - 0.5
        if name.endswith("groupnorm.weight"):
            t = 1.0 + 0.4 * r
        elif name.endswith(".bias"):
            t = 0.4 * r
        else:
            fan_in = int(np.prod(shape[1:]))
            t = 2.0 * r / float(np.sqrt(fan_in))
        if name.endswith(SCALED_HEADS):
            t = t * (HEAD_GAIN * (1.0 + 0.1 * float(torch.rand(1, generator=g) - 0.5)))
        sd[name] = t.to(torch.float32).contiguous()
    return sd


def scale_heads(sd, seed):
    """In place: the SCALED_HEADS entries of a state dict times a seeded factor of about HEAD_GAIN."""
    g = torch.Generator().manual_seed(int(seed))
    for name, t in sd.items():
        if name.endswith(SCALED_HEADS):
            t.mul_(HEAD_GAIN * (1.0 + 0.1 * float(torch.rand(1, generator=g) - 0.5)))
    return sd


def move_groupnorm(sd, seed):
    """In place: GroupNorm affines off (1, 0), as tests/golden/make_golden_infer.py:build does."""
    g = torch.Generator().manual_seed(int(seed))
    for k, v in sd.items():
        if "groupnorm.weight" in k:
            v.copy_(1.0 + 0.4 * (torch.rand(v.shape, generator=g) - 0.5))
        if "groupnorm.bias" in k:
            v.copy_(0.4 * (torch.rand(v.shape, generator=g) - 0.5))
    return sd


def load(stem):
    """All parts of a fixture (stem.npz, stem_b.npz, ...) as one dict."""
    d = {}
    for suffix in ("", "_b", "_c", "_d"):
        path = os.path.join(GOLDEN, stem + suffix + ".npz")
        if os.path.exists(path):
            with np.load(path) as z:
                d.update({k: z[k] for k in z.files})
    if not d:
        raise FileNotFoundError(stem)
    return d


def fixture_state_dict(d, prefix):
    """The stored (sd/<prefix>/name arrays) or drawn (names + shapes + seed, hashes checked) state dict of a fixture."""
    names = [str(s) for s in d[prefix + "/names"]]
    if prefix + "/seed" in d:
        shapes = [tuple(int(v) for v in str(s).split(",") if v) for s in d[prefix + "/shapes"]]
        sd = draw_state_dict(names, shapes, int(d[prefix + "/seed"]))
        got = [sha(v) for v in sd.values()]
        assert got == [str(s) for s in d[prefix + "/sha256"]], "drawn parameters differ from the fixture's hashes"
        return sd
    return OrderedDict((n, torch.from_numpy(np.asarray(d["sd/%s/%s" % (prefix, n)]))) for n in names)
