"""CPU checks of tests/golden/grid_family_bits.npz (the stored bits of the interpol grid kernels,
tests/test_gpu_grid_bits.py): its size, that every case of tests/grid_bits_cases.py is there, and that the coordinates of
the atomic cases keep every address to two addends."""
import os

import numpy as np

from conftest import GOLDEN, load_npz
import grid_bits_cases as GB


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
