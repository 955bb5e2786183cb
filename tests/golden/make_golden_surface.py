"""Golden vectors for the generator's surface task, made by RUNNING the reference on the CPU:

  (a) BaseGen.random_nonlinear_transform with 'surface' in the tasks (Generator/datasets.py:202-226), 20x24x28, n = 8
  (b) the same in photo mode, 16x22x18, n = 3
  (c) one BrainIDGen.__getitem__ with task.surface on (datasets.py:686-757), 28^3, tasks trimmed to T1
  (d) read_and_deform_surface (Generator/utils.py:479-531) called positionally on four synthetic meshes with case (a)'s
      Fneg (stored once, as A/Fneg) and an A, c2 of random_affine_transform, flip off and on
  and the reference's inspect.signature of read_and_deform_surface and BaseGen.random_nonlinear_transform (JSON).

Run in the build container only (needs /root/reference):   python tests/golden/make_golden_surface.py
Writes tests/golden/svf_surface.npz (a, b, d, signatures) and tests/golden/svf_surface_item.npz (c): data only, each
under 1 MiB.  Every torch draw is recorded in call order (make_golden_gen.Recorder); NumPy's and `random`'s streams are
reproduced by their seeds.
"""
import inspect
import json
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_gen as MG  # noqa: E402  (sets up the reference import and the in-memory nibabel stand-in)

import torch  # noqa: E402
from scipy.io import savemat  # noqa: E402

TASKS_T1 = dict(T1=True, T2=False, FLAIR=False, CT=False, segmentation=False, distance=False, bias_field=False,
                registration=False, super_resolution=False, age=False, surface=True, pathology=False, contrastive=False)


def base_gen(size, overrides):
    g = MG.gen_args(size, 0., overrides)
    for k, v in TASKS_T1.items():
        setattr(g.task, k, v)
    ds, D = MG.build("BaseGen", g, "/mem/none.")
    return g, ds


def nonlinear_case(tag, out, size, n, photo_mode, spac, seed):
    ov = {"generator.n_steps_svf_integration": n, "generator.nonlin_scale_min": 0.15, "generator.nonlin_scale_max": 0.25,
          "generator.nonlin_std_max": 4}
    g, ds = base_gen(size, ov)
    np.random.seed(seed)
    torch.manual_seed(seed)
    with MG.Recorder() as rec, torch.no_grad():
        F, Fneg = ds.random_nonlinear_transform(photo_mode, spac)
    out[tag + "/seed"] = np.array(seed)
    out[tag + "/size"] = np.array(size)
    out[tag + "/n"] = np.array(n)
    out[tag + "/photo_mode"] = np.array(bool(photo_mode))
    out[tag + "/spac"] = np.array(spac)
    out[tag + "/cfg_json"] = np.array(json.dumps(MG.ns_to_dict(g), sort_keys=True))
    out[tag + "/ndraws"] = np.array(len(rec.log))
    for i, (kind, arr) in enumerate(rec.log):
        out[tag + "/draw%03d_%s" % (i, kind)] = arr
    out[tag + "/F"] = MG.tonp(F).astype(np.float32)
    out[tag + "/Fneg"] = MG.tonp(Fneg).astype(np.float32)
    print(tag, "size", size, "n", n, "draws", len(rec.log), "|F| max", float(np.abs(MG.tonp(F)).max()), flush=True)
    return ds, F, Fneg


def mesh(rs, nv, size, out_frac=0.04):
    """nv vertices on a jittered ellipsoid inside the field, out_frac of them pushed outside it; ~nv faces."""
    c = (np.array(size) - 1) / 2.
    d = rs.randn(nv, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    V = c + d * (0.3 * np.array(size)) * (1 + 0.1 * rs.rand(nv, 1))
    k = rs.rand(nv) < out_frac
    V[k] = c + d[k] * (0.9 * np.array(size))
    F = np.stack([np.arange(nv), (np.arange(nv) + 1) % nv, (np.arange(nv) + 7) % nv], 1)
    return V.astype(np.float32), F.astype(np.int32)


def surface_case(out, ds_a, Fneg_a, shp):
    import Generator.utils as U
    np.random.seed(5)
    torch.manual_seed(5)
    _, A, c2 = ds_a.random_affine_transform(shp)
    rs = np.random.RandomState(77)
    size = list(ds_a.size)
    mat = {}
    for k, nv in (("lw", 2100), ("rw", 2600), ("lp", 3100), ("rp", 3600)):
        mat["V" + k], mat["F" + k] = mesh(rs, nv, size)
    out["D/A"] = MG.tonp(A).astype(np.float32)
    out["D/c2"] = MG.tonp(c2).astype(np.float32)
    out["D/size"] = np.array(size)
    for k, v in mat.items():
        out["D/mesh/" + k] = v
    with tempfile.TemporaryDirectory() as td:
        fn = os.path.join(td, "case.nii.gz")
        savemat(os.path.join(td, "case.mat"), mat)
        for flip in (False, True):
            dd = {"Fneg": Fneg_a, "A": A, "c2": c2}
            with torch.no_grad():
                r = U.read_and_deform_surface(None, "surface", fn, {"flip": flip}, dd, "cpu", None, size)
            for k, v in r.items():
                out["D/flip%d/%s" % (flip, k)] = MG.tonp(v)
    outside = 0
    for k in ("lw", "rw", "lp", "rp"):
        V = out["D/mesh/V" + k].astype(np.float64) - out["D/c2"]
        P = V @ np.linalg.inv(out["D/A"].astype(np.float64)).T + out["D/c2"]
        outside += int(np.sum(~((P > 0).all(1) & (P <= np.array(size) - 1).all(1))))
    print("D vertices", sum(len(mat["V" + k]) for k in ("lw", "rw", "lp", "rp")), "outside the field", outside, flush=True)


def item_case(out):
    tag = "C"
    shp, size, seed = (32, 30, 34), (28, 28, 28), 41
    case = MG.make_case(shp, seed)
    prefix = "/mem/%s." % tag
    MG.register(prefix, case)
    g = MG.gen_args(size, 0., {"generator.pathology_prob": 0., "mix_synth_prob": 0., "generator.flip_prob": 10.,
                               "generator.photo_prob": 0.})
    for k, v in TASKS_T1.items():
        setattr(g.task, k, v)
    g0 = MG.copy.deepcopy(g)
    ds, D = MG.build("BrainIDGen", g, prefix)
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    with MG.Recorder() as rec, torch.no_grad():
        n, dname, mode, target, samples = ds[0]
    out[tag + "/seed"] = np.array(seed)
    out[tag + "/mode"] = np.array(mode)
    out[tag + "/shape"] = np.array(shp)
    out[tag + "/size"] = np.array(size)
    out[tag + "/cfg_json"] = np.array(json.dumps(MG.ns_to_dict(g0), sort_keys=True))
    for k in ("Gen", "T1"):
        out[tag + "/case/" + k] = case[k]
    out[tag + "/ndraws"] = np.array(len(rec.log))
    for i, (kind, arr) in enumerate(rec.log):
        out[tag + "/draw%03d_%s" % (i, kind)] = arr
    for k, v in target.items():
        if k != "name":
            out[tag + "/target/" + k] = MG.tonp(v)
    for i, smp in enumerate(samples):
        for k, v in smp.items():
            out[tag + "/sample%d/%s" % (i, k)] = MG.tonp(v)
    print(tag, "mode", mode, "draws", len(rec.log), "target", sorted(k for k in target if k != "name"),
          "samples", len(samples), flush=True)


def signatures(out):
    import Generator.datasets as D
    import Generator.utils as U
    sig = {"read_and_deform_surface": str(inspect.signature(U.read_and_deform_surface)),
           "BaseGen.random_nonlinear_transform": str(inspect.signature(D.BaseGen.random_nonlinear_transform))}
    out["signatures_json"] = np.array(json.dumps(sig, sort_keys=True))


if __name__ == "__main__":
    torch.set_num_threads(4)
    out = {}
    ds_a, F_a, Fneg_a = nonlinear_case("A", out, [20, 24, 28], 8, False, 1.0, 3)
    nonlinear_case("B", out, [16, 22, 18], 3, True, 2.5, 9)
    surface_case(out, ds_a, Fneg_a, (26, 30, 34))
    signatures(out)
    p = os.path.join(HERE, "svf_surface.npz")
    np.savez_compressed(p, **out)
    print("svf_surface.npz", os.path.getsize(p), "bytes,", len(out), "arrays")
    out = {}
    item_case(out)
    p = os.path.join(HERE, "svf_surface_item.npz")
    np.savez_compressed(p, **out)
    print("svf_surface_item.npz", os.path.getsize(p), "bytes,", len(out), "arrays")
