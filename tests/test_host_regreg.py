"""The registration regularisers on the host: a NumPy restatement of SmoothnessLoss('l2') / HessianLoss('l2')
(Trainer/models/losses.py:72-130) and of their gradients, pinned against tests/golden/regreg.npz (made by running the
reference: tests/golden/make_golden_regreg.py), and the loss-name builder.  CPU only."""
from types import SimpleNamespace as NS

import numpy as np

from conftest import load_npz


def fdiff(u, axis):
    """Forward difference along `axis`, zero on the axis' last index (losses.py gradient())."""
    d = np.zeros_like(u)
    n = u.shape[axis]
    lo = [slice(None)] * u.ndim
    hi = [slice(None)] * u.ndim
    lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
    d[tuple(lo)] = u[tuple(hi)] - u[tuple(lo)]
    return d


def fdiff_t(g, axis):
    """Adjoint of fdiff: (D^T g)[i] = g[i-1] [i >= 1] - g[i] [i < n-1]."""
    n = g.shape[axis]
    out = np.zeros_like(g)
    a = [slice(None)] * g.ndim
    b = [slice(None)] * g.ndim
    a[axis], b[axis] = slice(1, n), slice(0, n - 1)
    out[tuple(a)] += g[tuple(b)]
    out[tuple(b)] -= g[tuple(b)]
    return out


X, Y, Z = 4, 3, 2                                        # (b, c, D, H, W): x = W, y = H, z = D


def smooth(u):
    ds = [fdiff(u, a) for a in (X, Y, Z)]
    n = u.size
    val = sum((d * d).sum() for d in ds) / n
    grad = sum(fdiff_t(d, a) for d, a in zip(ds, (X, Y, Z))) * (2.0 / n)
    return val, grad


def hessian_terms(u):
    dx, dy, dz = (fdiff(u, a) for a in (X, Y, Z))
    H = {"xx": fdiff(dx, X), "yy": fdiff(dy, Y), "zz": fdiff(dz, Z),
         "xy": fdiff(dy, X), "xz": fdiff(dz, X), "yz": fdiff(dz, Y)}
    return H


def det_of(H):
    xx, yy, zz, xy, xz, yz = (H[k] for k in ("xx", "yy", "zz", "xy", "xz", "yz"))
    return xx * (yy * zz - yz ** 2) - xy * (xy * zz - xz * yz) + xz * (xy * yz - xz * yy)


def hessian(u):
    H = hessian_terms(u)
    det = det_of(H)
    xx, yy, zz, xy, xz, yz = (H[k] for k in ("xx", "yy", "zz", "xy", "xz", "yz"))
    d2 = 2.0 * det
    G = {"xx": d2 * (yy * zz - yz * yz), "yy": d2 * (xx * zz - xz * xz), "zz": d2 * (xx * yy - xy * xy),
         "xy": 2.0 * d2 * (xz * yz - xy * zz), "xz": 2.0 * d2 * (xy * yz - xz * yy), "yz": 2.0 * d2 * (xy * xz - xx * yz)}
    ax = {"x": X, "y": Y, "z": Z}
    grad = np.zeros_like(u)
    for k, g in G.items():
        grad += fdiff_t(fdiff_t(g, ax[k[0]]), ax[k[1]])       # (D_a D_b)^T = D_b^T D_a^T
    return float((det * det).sum()), grad


def _cases():
    d = load_npz("regreg.npz")
    return d, sorted({k.split("/")[1] for k in d if k.startswith("unit/")})


def test_restatement_reproduces_reference():
    d, names = _cases()
    assert names == ["rand", "slab"]
    for name in names:
        u = d["unit/%s/u" % name].astype(np.float64)
        assert u.shape[:2] == (1, 3)
        for lname, fn in (("smooth", smooth), ("hessian", hessian)):
            val, grad = fn(u)
            ref = float(d["unit/%s/%s" % (name, lname)])
            rg = d["unit/%s/%s_grad" % (name, lname)].astype(np.float64)
            assert abs(val - ref) <= 1e-12 * abs(ref), (name, lname, val, ref)
            err = np.abs(grad - rg).max() / np.abs(rg).max()
            assert err <= 1e-6, (name, lname, err)            # the fixture's gradients are stored in fp32


def test_slab_case_has_flat_boundary():
    d, _ = _cases()
    u = d["unit/slab/u"]
    assert np.all(u[..., -2:] == u[..., -1:]) and np.all(u[..., :2, :] == u[..., :1, :]) and np.all(u[:, :, -2:] == u[:, :, -1:])
    # the Hessian vanishes inside the flat slabs: the gradient there comes only from the adjoints' edge terms
    _, g = hessian(u.astype(np.float64))
    assert np.abs(g[:, :, -1]).max() < np.abs(g).max()


def test_duplicated_derivatives_equal_single_form():
    """losses.py:132-135 forms ddxy, ddxz, ddyz twice (D_y D_x u, then D_x D_y u, ...) and keeps the second; with the
    zeroed last index the two forms are equal, so one kernel evaluation of each mixed derivative is the reference's."""
    d, names = _cases()
    for name in names:
        u = d["unit/%s/u" % name].astype(np.float64)
        dx, dy, dz = (fdiff(u, a) for a in (X, Y, Z))
        first = {"xy": fdiff(dx, Y), "xz": fdiff(dx, Z), "yz": fdiff(dy, Z)}       # gradient(dx), gradient(dy)
        second = {"xy": fdiff(dy, X), "xz": fdiff(dz, X), "yz": fdiff(dz, Y)}      # gradient(dy), gradient(dz): kept
        for k in first:
            assert np.array_equal(first[k], second[k]), (name, k)
        H = hessian_terms(u)
        ref = float(d["unit/%s/hessian" % name])
        assert abs(float((det_of(H) ** 2).sum()) - ref) <= 1e-12 * abs(ref)


def _train_args(**switches):
    losses = dict(image_grad=True, registration_grad=True, registration_smooth=False, registration_hessian=False,
                  implicit_pathol=False)
    losses.update(switches)
    w = NS(seg_ce=1.0, seg_dice=1.1, pathol_ce=1.2, pathol_dice=1.3, image=1.4, image_grad=1.5, bias_field_log=1.6,
           distance=1.7, registration=1.8, registration_grad=1.9, registration_smooth=2.0, registration_hessian=2.1,
           surface=2.2, age=2.3, contrastive=2.4, implicit_pathol_ce=2.5, implicit_pathol_dice=2.6)
    return NS(losses=NS(**losses), weights=w)


def test_loss_name_builder_emits_switches():
    from brainfm_amd import train as TR
    tasks = ["T1", "segmentation", "registration", "distance"]
    names, wd = TR.criterion_losses(_train_args(), tasks)
    assert names == ["T1", "T1_grad", "seg_ce", "seg_dice", "registration", "registration_grad", "distance"]
    names, wd = TR.criterion_losses(_train_args(registration_smooth=True, registration_hessian=True), tasks)
    assert names == ["T1", "T1_grad", "seg_ce", "seg_dice", "registration", "registration_grad", "registration_smooth",
                     "registration_hessian", "distance"]
    assert wd["loss_registration_smooth"] == 2.0 and wd["loss_registration_hessian"] == 2.1
    assert list(wd) == ["loss_" + n for n in names]
    names, _ = TR.criterion_losses(_train_args(registration_grad=False, registration_hessian=True), ["registration"])
    assert names == ["registration", "registration_hessian"]
    # the switches belong to the registration task: without it they add nothing
    names, _ = TR.criterion_losses(_train_args(registration_smooth=True, registration_hessian=True), ["T1"])
    assert names == ["T1", "T1_grad"]
    # a train_args.losses without the keys (the inference-side Namespace) leaves them off
    ta = NS(losses=NS(uncertainty=None, implicit_pathol=False), weights=_train_args().weights)
    assert TR.criterion_losses(ta, ["registration"])[0] == ["registration"]
    assert set(names) <= TR.SUPPORTED
    assert {"registration_smooth", "registration_hessian"} <= TR.SUPPORTED


def test_builder_matches_fixture_names():
    d = load_npz("regreg.npz")
    from brainfm_amd import train as TR
    names, wd = TR.criterion_losses(_train_args(registration_smooth=True, registration_hessian=True), ["registration"])
    assert names == [str(s) for s in d["loss_names"]]
