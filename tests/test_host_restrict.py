"""CPU checks for interpol.restrict and the gradient of the separable cubic resize: the float64 numpy restatement
(tests/restrict_refs.py) against the reference's own results (tests/golden/interpol_restrict*.npz), the conditions the
fixture must meet, the shape / factor / anchor arithmetic of brainfm_amd.interpol.restrict without a device, its
signature and its refusals."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_npz
import restrict_refs as RR

ORDERS = {"o0": 0, "o1": 1, "o2": 2, "o3": 3, "o312": [3, 1, 2]}
FILES = ["interpol_restrict.npz"] + ["interpol_restrict_%s.npz" % t for t in ORDERS]
GEOMS = {"c": dict(anchor="c", shape=[5, 4, 6]),
         "f": dict(anchor="f", factor=[2, 3, 2]),
         "l": dict(anchor="l", factor=2, shape=[5, 4, 7]),
         "e": dict(anchor="e", shape=[5, 4, 6]),
         "eu": dict(anchor="e", shape=[13, 9, 19]),
         "cef": dict(anchor=["c", "e", "f"], shape=[5, 4, 6], factor=[2, 2, 2]),
         "T": dict(anchor="e", shape=[1, 1, 3])}
# arrays per order file: 4 bounds for six geometries, 7 + extrapolate False + 'hist' for 'e'; one reduce_sum each; the
# backward of 'c' and 'e'; prefilter=True at orders 2 and 3
N_ARRAYS = {t: 6 * 4 + 9 + 7 + 2 + (1 if t in ("o2", "o3") else 0) for t in ORDERS}


def sin_weights(shape):
    return torch.sin(torch.arange(int(np.prod(shape)), dtype=torch.float32)).reshape(tuple(shape)).double().numpy()


def restated(base, tag, order, what, bound, ext):
    """the float64 restatement of one array of an order file"""
    x = base["T/vol"] if tag == "T" else base["vol"]
    kw = GEOMS[tag]
    shape, coords, fs = RR.geometry(x.shape, kw.get("factor"), kw.get("shape"), kw["anchor"])
    if what == "dimage":
        return RR.restrict_backward(sin_weights(x.shape[:2] + tuple(shape)), coords, shape, fs, order, bound, ext)
    return RR.restrict(x, coords, shape, fs, order, bound, ext, reduce_sum=what == "sum", prefilter=what == "pf")


@pytest.mark.parametrize("otag", list(ORDERS))
def test_restatement_matches_every_array_of_the_fixture(otag):
    """Bar: max(1e-6, 4 x the stored max|ref32 - ref64| of the reference's own float32 run), forward and backward."""
    base, d = load_npz("interpol_restrict.npz"), load_npz("interpol_restrict_%s.npz" % otag)
    worst, n = {}, 0
    for k in d:
        if k.endswith(".err"):
            continue
        tag, combo, what = k.split("/")
        got = restated(base, tag, ORDERS[otag], what, int(combo[1]), int(combo[4]))
        assert got.shape == d[k].shape, k
        err, stored = float(np.abs(got - d[k]).max()), float(d[k + ".err"])
        worst[what] = max(worst.get(what, (0.0, 0.0)), (err, stored))
        assert err <= max(1e-6, 4 * stored), (k, err, stored)
        n += 1
    assert n == N_ARRAYS[otag] == len(d) // 2
    print(otag, {w: "max|restatement - ref| %.2e (stored max|ref32 - ref64| %.2e)" % v for w, v in worst.items()})


def test_restatement_matches_the_resize_gradients_of_the_fixture():
    base = load_npz("interpol_restrict.npz")
    x = base["vol"]
    coords = RR.resize_coords(x.shape[2:], [10, 9, 11], "e")
    w = sin_weights(x.shape[:2] + (10, 9, 11))
    n = 0
    for key, bound, pf in (("resize/dct2_pf", 3, True), ("resize/nearest_nopf", 1, False)):
        got = RR.resize_backward(w, coords, x.shape[2:], bound, pf)
        ref, stored = base[key + "/dimage"], float(base[key + "/dimage.err"])
        err = float(np.abs(got - ref).max())
        print(key, "max|restatement - ref| %.2e (stored max|ref32 - ref64| %.2e)" % (err, stored))
        assert err <= max(1e-6, 4 * stored), (key, err, stored)
        n += 1
    assert n == 2


def test_fixture_coordinates_keep_their_margin_and_files_stay_small():
    base = load_npz("interpol_restrict.npz")
    assert base["vol"].shape == (2, 3, 11, 9, 14) and base["T/vol"].shape == (1, 2, 1, 2, 5)
    for tag, kw in GEOMS.items():
        x = base["T/vol"] if tag == "T" else base["vol"]
        shape, c64, _ = RR.geometry(x.shape, kw.get("factor"), kw.get("shape"), kw["anchor"])
        assert list(base[tag + "/shape"]) == shape
        exts = (0, 1, 2) if tag == "e" else (1,)
        for a in range(3):
            c32 = base["%s/coord%d" % (tag, a)]
            assert c32.dtype == np.float32 and float(np.abs(c32 - c64[a]).max()) < 4e-6
            exact = c32.astype(np.float64) == c64[a]
            for order in (0, 1):                              # 0: the nearest node; any order: the mask thresholds
                for ext in exts:
                    for c in (c32, c64[a]):
                        assert not RR.near_jumps(c, shape[a], order, ext, 1e-3, exact).any(), (tag, a, order, ext)
    # the upsizing case has nodes that receive nothing at order 0
    shape, c64, _ = RR.geometry(base["vol"].shape, None, [13, 9, 19], "e")
    assert any((RR.axis_matrix(c64[a], shape[a], 0, 1, 1).sum(1) == 0).any() for a in range(3))
    for f in FILES:
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 1 << 20, f


@pytest.mark.parametrize("tag", list(GEOMS))
def test_geometry_of_the_mirror_without_a_device(tag):
    """Output shape, coordinate lists bit-equal to the ones the reference handed to grid_push in float32, fullscale."""
    from brainfm_amd import interpol as IP
    base = load_npz("interpol_restrict.npz")
    x = base["T/vol"] if tag == "T" else base["vol"]
    kw = GEOMS[tag]
    shape, lin, fs = IP._restrict_geometry(x.shape, kw.get("factor"), kw.get("shape"), kw["anchor"])
    assert list(shape) == list(base[tag + "/shape"])
    for a in range(3):
        assert lin[a].dtype == torch.float32 and lin[a].device.type == "cpu"
        assert np.array_equal(lin[a].numpy(), base["%s/coord%d" % (tag, a)]), (tag, a)
    assert abs(fs - float(base[tag + "/fullscale"])) <= 1e-15 * abs(fs)


def test_geometry_rules_and_normalisation():
    from brainfm_amd import interpol as IP
    shape, lin, fs = IP._restrict_geometry((1, 1, 8, 8, 8), [2, 2, 2], None, "e")
    assert shape == (4, 4, 4) and fs == 0.125                 # 'e': prod(out / in): the result is the sum times 8
    shape, lin, fs = IP._restrict_geometry((1, 1, 9, 9, 9), None, [5, 5, 5], "c")
    assert fs == 8.0 and torch.equal(lin[0], torch.linspace(0, 4, 9))
    shape, lin, fs = IP._restrict_geometry((1, 1, 9, 8, 7), [2, 3, 1.5], None, "f")
    assert shape == (4, 2, 4) and abs(fs - 1 / 9) < 1e-15      # int(i / f); prod(1 / f)
    shape, lin, fs = IP._restrict_geometry((8, 8, 8), [2.0] * 3, None, ["l", "f", "e"])
    assert shape == (4, 4, 4) and float(lin[0][-1]) == 3.0     # 'l': the last samples coincide
    with pytest.raises(ZeroDivisionError):                     # 'c' with an output axis of length 1, as the reference
        IP._restrict_geometry((1, 1, 8, 8, 8), None, [4, 1, 4], "c")


def test_signature_matches_the_reference():
    from brainfm_amd import interpol as IP
    with open(os.path.join(GOLDEN, "api_signatures_restrict.json")) as f:
        table = json.load(f)["signatures"]
    entry = table["utils.interpol.restrict:restrict"]
    assert entry["mirror"] == "brainfm_amd.interpol:restrict"
    got = [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
           for p in inspect.signature(IP.restrict).parameters.values()]
    assert got == entry["params"]


def test_refusals():
    from brainfm_amd import interpol as IP
    from brainfm_amd._lib import BfmError
    x = torch.zeros(1, 1, 8, 8, 8)
    for kw in (dict(factor=2, anchor="e"), dict(factor=[2, 2]), dict(shape=[4, 4, 4, 4]), dict(anchor=["c", "e"], factor=2)):
        with pytest.raises(NotImplementedError, match="3-D"):  # nb_dim = the longest of factor / shape / anchor
            IP.restrict(x, **kw)
    with pytest.raises(NotImplementedError, match="3-D"):
        IP.restrict(torch.zeros(1, 1, 8, 8), factor=2, anchor=[])      # no list at all: image.dim() - 2
    for order, n in ((4, 4), (7, 7), ("fifth", 5), ([3, 6, 1], 6)):
        with pytest.raises(NotImplementedError, match=str(n)):
            IP.restrict(x, factor=[2, 2, 2], interpolation=order)
    with pytest.raises(ValueError, match="anchor"):
        IP.restrict(x, factor=[2, 2, 2], anchor="x")
    with pytest.raises(ValueError, match="factor"):
        IP.restrict(x, anchor=["c", "c", "c"])
    with pytest.raises(ValueError):
        IP.restrict(x, factor=[2, 2, 2], bound="nope")
    with pytest.raises(TypeError):
        IP.restrict(x, factor=[2, 2, 2], order=3)
    for bound in ("dst1", "dst2"):                             # the refusal of grid_push(prefilter=True)
        with pytest.raises(NotImplementedError, match="dst"):
            IP.restrict(x, factor=[2, 2, 2], interpolation=3, bound=bound, prefilter=True)
    with pytest.raises(BfmError):                              # everything valid, on the CPU
        IP.restrict(x, factor=[2, 2, 2], interpolation=3, anchor="e")
