"""CPU checks of tests/golden/grid_family_bits.npz and grid_nd_bits.npz (the stored bits of the interpol grid kernels,
tests/test_gpu_grid_bits.py): their size, that every case of tests/grid_bits_cases.py is there, that the coordinates of
the atomic cases keep every address to two addends, and the 2-D arrays against the float64 restatement."""
import os

import numpy as np

from conftest import GOLDEN, load_npz
import grid_bits_cases as GB
import grid2d_refs as GR


def test_file_stays_small_and_holds_every_case():
    assert os.path.getsize(os.path.join(GOLDEN, "grid_family_bits.npz")) < 1 << 20
    d = load_npz("grid_family_bits.npz")
    cases = GB.det_cases()
    assert list(d["cases"]) == [c[0] for c in cases] and len(cases) == len(GB.ORDERS) * len(GB.CONFIGS) + 2
    B, Cc, gs = GB.GRID[0], GB.VOL[1], GB.GRID[1:]
    assert d["pull"].shape == (len(cases), B, Cc) + gs and d["pull"].dtype == np.float32
    assert d["grad"].shape == (len(cases), B, Cc) + gs + (3,)
    assert d["hess"].shape == (len(cases), B, Cc) + gs + (3, 3)
    assert d["hessc"].shape == (len(cases), B) + gs + (3,)
    for tag, dt in zip(GB.LABEL_DTYPES, (np.uint8, np.int16, np.int32, np.int64)):
        assert d["label/" + tag].shape == (len(cases), len(GB.VARIANTS), B, Cc) + gs and d["label/" + tag].dtype == dt
    tables = GB.table_cases()
    assert list(d["table/names"]) == [c[0] for c in tables] and len(tables) == 4 * 4 * 2 + 4 * 2
    assert d["table/rowptr"].shape == (len(tables), GB.TABLE_M + 1)
    assert d["table/col"].shape == d["table/val"].shape == (len(tables), 4 * GB.TABLE_M)
    atomics = GB.atomic_cases()
    assert list(d["atomic/names"]) == [c[0] for c in atomics] and len(atomics) == 3 * len(GB.ORDERS)
    assert d["atomic/push"].shape == d["atomic/pushgrad"].shape == (len(atomics), 1, 2) + GB.ATOMIC_SHAPE
    assert tuple(d["big/names"]) == GB.BIG_CASES and d["big/sha"].shape == (2, 32)
    for k, v in GB.make_inputs().items():                # the stored inputs are the ones the case module describes
        assert d[k].shape == v.shape and d[k].dtype == v.dtype, k


def test_stored_inputs_hold_the_ties_and_spill_over_every_face():
    d = load_npz("grid_family_bits.npz")
    g = d["in/grid"].astype(np.float64)
    for a in range(3):
        assert g[..., a].min() < -1.5 and g[..., a].max() > GB.VOL[2 + a] + 0.5
        assert (g[..., a] == np.round(g[..., a])).sum() >= 4                    # floor ties of the odd orders
        assert (np.abs(g[..., a] - np.floor(g[..., a]) - 0.5) == 0).sum() >= 4  # and of the even ones


def test_stored_push_coordinates_keep_every_address_to_two_addends():
    d = load_npz("grid_family_bits.npz")
    GB.check_two_addends(d)
    worst = max(GB.max_addends(d["atomic/grid_b%d" % b], GB.ATOMIC_SHAPE, o, b) for _, o, b in GB.atomic_cases())
    assert worst == 2                                    # and some address does take two: the cases are not trivial
    for name, arr in (("push", d["atomic/push"]), ("pushgrad", d["atomic/pushgrad"])):
        assert np.isfinite(arr).all() and (arr != 0).any(), name


def test_second_fixture_stays_small_and_holds_every_case():
    assert os.path.getsize(os.path.join(GOLDEN, "grid_nd_bits.npz")) < 1 << 20
    nd = load_npz("grid_nd_bits.npz")
    cases = GB.det2_cases()
    assert list(nd["cases2d"]) == [c[0] for c in cases] and len(cases) == len(GB.ORDERS2) * len(GB.CONFIGS) + 2
    assert len(set(nd["cases2d"])) == len(cases)
    assert nd["pull2d"].shape == (len(cases), 2, 2, 6, 5) and nd["pull2d"].dtype == np.float32
    assert nd["grad2d"].shape == (len(cases), 2, 2, 6, 5, 2) and nd["grad2d"].dtype == np.float32
    atomics = GB.atomic2_cases()
    assert list(nd["atomic2d/names"]) == [c[0] for c in atomics] and len(atomics) == 3 * len(GB.ORDERS2)
    assert nd["atomic2d/push"].shape == (len(atomics), 1, 2) + GB.ATOMIC_SHAPE2
    assert list(nd["lin3d/names"]) == [c[0] for c in GB.LIN3_CASES]
    assert nd["lin3d/pull"].shape == (2, 2, 2) + GB.GRID[1:] and nd["lin3d/grad"].shape == (2, 2, 2) + GB.GRID[1:] + (3,)
    assert tuple(nd["big/names"]) == GB.BIG2_CASES and nd["big/sha"].shape == (1, 32)


def test_2d_inputs_keep_the_ties_and_push_coordinates_keep_every_address_to_two_addends():
    d = load_npz("grid_family_bits.npz")
    vol, grid = GB.inputs2d(d)
    assert vol.shape == (2, 2, 5, 6) and grid.shape == (2, 6, 5, 2)
    g = grid.astype(np.float64)
    for a in range(2):
        assert g[..., a].min() < -1.5 and g[..., a].max() > vol.shape[2 + a] + 0.5
        assert (g[..., a] == np.round(g[..., a])).sum() >= 4
        assert (np.abs(g[..., a] - np.floor(g[..., a]) - 0.5) == 0).sum() >= 4
    GB.check_two_addends2(d)
    assert max(GB.max_addends(GB.atomic2_inputs(d, b)[1], GB.ATOMIC_SHAPE2, o, b) for _, o, b in GB.atomic2_cases()) == 2


def test_stored_2d_arrays_agree_with_the_float64_restatement():
    """pull2d / grad2d / atomic2d/push against tests/grid2d_refs.py at the bar of the family (test_gpu_grid2d.py):
    max|stored - ref| <= 2e-5 * max(1, max|ref|).  pull and push are held at every coordinate, the planted ties included:
    kernel and restatement take the same floor.  The gradient is held where GR.near_jumps finds no jump: on a tie it is
    one-sided in the kernels (iso1's slope at order 1) and sign(0) = 0 in the restatement, two values of a function that
    jumps there, which is why the fixtures held against the reference keep their margin from such points."""
    d, nd = load_npz("grid_family_bits.npz"), load_npz("grid_nd_bits.npz")
    vol, grid = GB.inputs2d(d)

    def close(got, ref, what):
        err = float(np.abs(got.astype(np.float64) - ref).max())
        assert err <= 2e-5 * max(1.0, float(np.abs(ref).max())), (what, err)

    for i, (name, o, b, ext, Bi, Bg) in enumerate(GB.det2_cases()):
        close(nd["pull2d"][i], GR.pull(vol[:Bi], grid[:Bg], list(o), list(b), ext), name + " pull")
        smooth = ~GR.near_jumps(grid[:Bg], vol.shape[2:]).any(-1)[:, None, :, :, None]
        close(nd["grad2d"][i] * smooth, GR.grad(vol[:Bi], grid[:Bg], list(o), list(b), ext) * smooth, name + " grad")
        assert smooth.mean() >= 0.5                      # the planted ties are up to 12 of the 30 pixels of a batch
    for i, (name, o, b) in enumerate(GB.atomic2_cases()):
        src, g = GB.atomic2_inputs(d, b)
        close(nd["atomic2d/push"][i], GR.push(src, g, GB.ATOMIC_SHAPE2, list(o), b, 1), name + " push")
