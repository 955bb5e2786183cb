"""CPU checks for interpol.grid_pull / grid_push / grid_count on 2-D grids: the float64 numpy restatement
(tests/grid2d_refs.py) against the reference's own results (tests/golden/interpol_grid2d*.npz) and against the 3-D
restatement (tests/spline_grid_refs.py) on the embedded problem, the conditions the fixture must meet, the argument
handling of brainfm_amd.interpol, and the load policy of the kernels' source."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_npz
import grid2d_refs as GR
import spline_grid_refs as SR

ORDERS = {"o0": 0, "o1": 1, "o2": 2, "o3": 3, "o31": [3, 1], "o02": [0, 2]}
FILES = ["interpol_grid2d.npz"] + ["interpol_grid2d_%s.npz" % t for t in ORDERS]
CSRC = os.path.join(os.path.dirname(GOLDEN), os.pardir, "brainfm_amd", "csrc")


def allowed(ref32, stored):
    """The stored max|ref32 - ref64| of the array plus the rounding of the stored value to float32 (half a unit in the last
    place of its largest entry)"""
    return float(stored) + 2.0 ** -24 * max(float(np.abs(ref32).max()), 2.0 ** -126)


@pytest.mark.parametrize("otag", list(ORDERS))
def test_restatement_matches_every_array_of_the_fixture(otag):
    """pull, push, count and the four backward arrays.  The backward arrays follow from the restatement as the reference
    forms them: d/dinput of pull is push of the weights, d/dgrid the channel sum of weights times grad, and the mirror
    for push.  The prefiltered arrays (pull_pf, the coefficients, resize) are left to the device tests: the restatement
    is of pull, push and grad, and the reference's own float64 prefilter truncates its boundary sums at z^2n (2e-6 on
    an axis of 5 samples), so an exact solve of the interpolation conditions is not what it computes."""
    base, d = load_npz("interpol_grid2d.npz"), load_npz("interpol_grid2d_%s.npz" % otag)
    order = ORDERS[otag]
    worst = {}
    n = 0
    for k in d:
        if k.endswith(".err"):
            continue
        tag, combo, what = k.split("/")
        if what.startswith("pull_pf"):
            continue                 # prefiltered: the restatement has no prefilter; held on the device (test_gpu_grid2d.py)
        bound, ext = int(combo[1]), int(combo[4])
        vol, grid, src = (base["%s/%s" % (tag, x)].astype(np.float64) for x in ("vol", "grid", "src"))
        ins = vol.shape[2:]
        w, w2 = base[tag + "/wsin"].astype(np.float64), base[tag + "/wcos"].astype(np.float64)
        if what == "pull":
            got = GR.pull(vol, grid, order, bound, ext)
        elif what == "push":
            got = GR.push(src, grid, ins, order, bound, ext)
        elif what == "count":
            got = GR.count(grid, ins, order, bound, ext)
        elif what == "pull_dinput":
            got = GR.push(w, grid, ins, order, bound, ext)
        elif what == "pull_dgrid":
            got = (GR.grad(vol, grid, order, bound, ext) * w[..., None]).sum(1)
        elif what == "push_dinput":
            got = GR.pull(w2, grid, order, bound, ext)
        elif what == "push_dgrid":
            got = (GR.grad(w2, grid, order, bound, ext) * src[..., None]).sum(1)
        else:
            raise AssertionError(k)
        assert got.shape == d[k].shape, k
        err = float(np.abs(got - d[k]).max())
        stored = float(d[k + ".err"])
        worst[what] = max(worst.get(what, (0.0, 0.0)), (err, stored))
        assert err <= allowed(d[k], stored), (k, err, stored)
        n += 1
    assert n == 2 * (15 * 3 + 4 * 4)                         # both shapes: 15 combinations x 3, 4 of them x 4 backward arrays
    print(otag, {w_: "max|restatement - ref| %.2e (stored max|ref32 - ref64| %.2e)" % v for w_, v in worst.items()})


@pytest.mark.parametrize("otag", list(ORDERS))
def test_restatement_equals_the_3d_restatement_on_the_embedded_problem(otag):
    base = load_npz("interpol_grid2d.npz")
    order = ORDERS[otag]
    for tag in ("A", "T"):
        vol, grid, src = (base["%s/%s" % (tag, x)] for x in ("vol", "grid", "src"))
        ins = vol.shape[2:]
        for bound in range(7):
            for ext in (0, 1, 2):
                v3, g3, o3, b3 = GR.embed(vol, grid, order, bound)
                assert np.abs(GR.pull(vol, grid, order, bound, ext) - SR.pull(v3, g3, o3, b3, ext)[..., 0]).max() <= 1e-12
                s3 = src[..., None]
                assert np.abs(GR.push(src, grid, ins, order, bound, ext) -
                              SR.push(s3, g3, ins + (1,), o3, b3, ext)[..., 0]).max() <= 1e-12
                ones = np.ones((grid.shape[0], 1) + grid.shape[1:-1] + (1,))
                assert np.abs(GR.count(grid, ins, order, bound, ext) -
                              SR.push(ones, g3, ins + (1,), o3, b3, ext)[..., 0]).max() <= 1e-12


def test_fixture_coordinates_keep_their_margin_and_files_stay_small():
    base = load_npz("interpol_grid2d.npz")
    for tag in ("A", "T"):
        g, shape = base[tag + "/grid"], base[tag + "/vol"].shape[2:]
        assert not GR.near_jumps(g, shape, 1e-3).any()
        far = 1.5 if tag == "A" else 0.5                     # spills over every edge (the thin grid has 12 pixels only)
        for a in range(2):
            assert g[..., a].min() < -far and g[..., a].max() > shape[a] - 1 + far
    assert base["A/vol"].shape == (2, 3, 7, 6) and base["A/grid"].shape == (2, 5, 9, 2) and base["A/src"].shape == (2, 3, 5, 9)
    assert base["T/vol"].shape == (1, 2, 1, 5) and base["T/grid"].shape == (1, 3, 4, 2)
    assert base["resize/o3_dct2"].shape == (2, 3, 10, 9) and base["resize/o1_edge"].shape == (2, 3, 14, 9)
    assert base["resize/o2_unbatched"].shape == (9, 8)
    for f in FILES:
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 1 << 20, f
    for otag in ORDERS:
        d = load_npz("interpol_grid2d_%s.npz" % otag)
        assert len({k.split("/")[1] for k in d}) == 15
        assert ("A/b3_e1/pull_pf" in d) == (otag in ("o2", "o3"))


def test_a_2d_float_call_reaches_the_device_check():
    """On CPU tensors every 2-D entry gets as far as the device check: no shape or dimension error before it."""
    from brainfm_amd import interpol as IP
    from brainfm_amd._lib import BfmError
    img, grid, src = torch.zeros(2, 3, 7, 6), torch.zeros(2, 5, 9, 2), torch.zeros(2, 3, 5, 9)
    calls = [lambda: IP.grid_pull(img, grid, 3, "dct2", True),
             lambda: IP.grid_pull(img[0, 0], grid[0], [3, 1], ["zero", "dft"]),
             lambda: IP.grid_pull(img, grid, 2, "dct2", True, prefilter=True),
             lambda: IP.grid_push(src, grid, [7, 6], 1, "zero"),
             lambda: IP.grid_push(src, grid, None, "nearest"),
             lambda: IP.grid_count(grid, [7, 6], [0, 2], "dct1"),
             lambda: IP.spline_coeff_nd(img, 3, "dct2", 2),
             lambda: IP.resize(img, shape=[10, 9], interpolation=3, bound="dct2"),
             lambda: IP.resize(img, factor=[2, 1.5], anchor="e", interpolation="linear"),
             lambda: IP.resize(img[0, 0], shape=[9, 8], interpolation="quadratic")]
    for i, call in enumerate(calls):
        with pytest.raises(BfmError, match="HIP device"):
            call()


def test_what_2d_does_not_take_still_raises():
    from brainfm_amd import interpol as IP
    img, grid, src = torch.zeros(1, 1, 4, 4), torch.zeros(1, 2, 2, 2), torch.zeros(1, 1, 2, 2)
    for dt in (torch.uint8, torch.int16, torch.int32, torch.int64):          # label maps: 3-D only
        with pytest.raises(NotImplementedError, match="only 3-D grids are on the hot path"):
            IP.grid_pull(img.to(dt), grid)
        with pytest.raises(NotImplementedError, match="only 3-D grids are on the hot path"):
            IP.grid_pull(torch.zeros(1, 1, 4, dtype=dt), torch.zeros(1, 2, 1))
    for call in (lambda: IP.grid_grad(img, grid), lambda: IP.grid_hess(img, grid),
                 lambda: IP.grid_pushgrad(torch.zeros(1, 1, 2, 2, 2), grid)):
        with pytest.raises(NotImplementedError, match="3-D"):
            call()
    with pytest.raises(NotImplementedError, match="3-D"):
        IP.restrict(img, factor=[2, 2])
    for name in ("quadratic", "cubic", ["linear", "cubic"]):
        for call in (lambda: IP.grid_pull(img, grid, name), lambda: IP.grid_push(src, grid, None, name),
                     lambda: IP.grid_count(grid, None, name)):
            with pytest.raises(NotImplementedError, match="integer"):
                call()
    for order, n in ((4, 4), (7, 7), ("fifth", 5), ([3, 6], 6)):
        for call in (lambda: IP.grid_pull(img, grid, order), lambda: IP.grid_push(src, grid, None, order),
                     lambda: IP.grid_count(grid, None, order), lambda: IP.spline_coeff_nd(img, order, "dct2", 2),
                     lambda: IP.resize(img, shape=[5, 5], interpolation=order)):
            with pytest.raises(NotImplementedError, match=str(n)):
                call()
    line, g1 = torch.zeros(1, 1, 4), torch.zeros(1, 2, 1)                   # 1-D grids raise everywhere
    for call in (lambda: IP.grid_pull(line, g1), lambda: IP.grid_push(torch.zeros(1, 1, 2), g1),
                 lambda: IP.grid_count(g1), lambda: IP.grid_grad(line, g1)):
        with pytest.raises(NotImplementedError):
            call()
    # resize checks the device before the number of dimensions: on CPU tensors a 1-D resize stops there, as it did (on the
    # device it raises NotImplementedError, tests/test_gpu_grid2d.py)
    for kw in (dict(factor=[2]), dict(factor=2, anchor=["c"]), dict(shape=[8])):
        with pytest.raises(IP.L.BfmError, match="HIP device"):
            IP.resize(line, **kw)
    for bound in ("dst1", "dst2", ["dct2", "dst2"]):                          # the prefilter's refusals, as in 3-D
        with pytest.raises(NotImplementedError):
            IP.spline_coeff_nd(img, 3, bound, 2)
        with pytest.raises(NotImplementedError):
            IP.grid_pull(img, grid, 3, bound, prefilter=True)


def test_opts_keep_three_entries():
    from brainfm_amd import interpol as IP
    b, o, ext = IP._opts([3, 1], ["zero", "dft"], True)
    assert list(b) == [0, 6, 6] and o == (3, 1, 1) and ext == 1
    assert IP._order_list(2) == (2, 2, 2) and IP._bound_list("dct2") == [3, 3, 3]


def test_kernel_source_loads_texels_and_coordinates_through_ld_tex_only():
    """Every read of the image and of the grid in spline_grid.hip -- the three dimension-generic kernels, the three padded 3-D
    ones, the three linear ones and the tap walk -- and in the point prologue of grid_kernels.h is a 4-byte ld_tex: no wider vector
    type, no other load builtin, and no subscript or dereference of the image, row or grid pointers."""
    src = open(os.path.join(CSRC, "spline_grid.hip")).read()
    assert not os.path.exists(os.path.join(CSRC, "spline_grid2d.hip"))
    code = re.sub(r"//[^\n]*", "", src)
    assert "ld_tex(" in code and "ld_tex3" not in code
    for word in ("float2", "float4", "uint2", "uint4", "int2", "int4", "__builtin_nontemporal_load", "__ldg",
                 "buffer_load", "global_load", "asm"):
        assert not re.search(r"\b%s\b" % word, code), word
    kernels = code[:code.index("static int launch_grid")]
    assert 'extern "C"' not in kernels
    assert not re.search(r"\b(src|row|grid)\s*\[", kernels) and not re.search(r"(?<![.\w])g\s*\[", kernels)   # never subscripted
    # nor dereferenced: the image pointer is declared and handed to ld_tex, the grid pointer is a parameter handed to the
    # prologue, and neither appears anywhere else
    assert len(re.findall(r"\bsrc\b", kernels)) == (kernels.count("const float* src = ") + kernels.count("ld_tex(src + ") +
                                                      kernels.count("const float* row = src + "))
    assert len(re.findall(r"\brow\b", kernels)) == (kernels.count("const float* row = ") + kernels.count("ld_tex(row + ") +
                                                      kernels.count("float* row = dst + ") + kernels.count("atomicAdd(row + "))
    assert len(re.findall(r"\bgrid\b", kernels)) == (kernels.count("__restrict__ grid, ") + kernels.count(", grid, Bg, dims, ") +
                                                       kernels.count(", grid, Bg, GridDims<3>{{nx, ny, nz}}, "))
    names = ["spline_pull", "spline_push", "spline_grad", "padded_pull3d", "padded_push3d", "padded_grad3d", "LinearNodes",
             "linear_pull3d", "linear_push3d", "linear_grad3d"]
    at = [kernels.index("void __launch_bounds__(256) " + n if n[:6] in ("spline", "padded") else n) for n in names]
    at.append(len(kernels))
    assert at == sorted(at)
    body = {n: kernels[at[i]:at[i + 1]] for i, n in enumerate(names)}
    assert kernels[:at[0]].count("ld_tex(") == 0                                # the tap walk itself loads nothing
    for n in names:
        loads = 1 if ("pull" in n or "grad" in n) else 0                        # one texel load, in the tap loop; push: none
        assert body[n].count("ld_tex(") == loads, n
        if n != "LinearNodes":
            assert body[n].count("grid_point<") == 1, n
    hdr = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "grid_kernels.h")).read())
    assert "GridPixel" not in hdr and "grid_pixel" not in hdr and "GridVoxel" not in hdr
    point = hdr[hdr.index("grid_point("):hdr.index("grid_check_args")]
    assert point.count("ld_tex(g + a)") == 1 and point.count("ld_tex(") == 1 and not re.search(r"(?<![.\w])g\s*\[", point)
    assert "a < D" in point                                                    # D separate 4-byte loads
