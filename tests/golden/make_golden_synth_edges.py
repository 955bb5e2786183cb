"""Golden results of the reference's OWN functions on the edge inputs of tests/synth_kernel_refs.py (build container only):

    python tests/golden/make_golden_synth_edges.py        -> tests/golden/synth_edges.npz

fast_3D_interp_torch (linear, both defaults, and nearest), myzoom_torch, gaussian_blur_3d (Generator/utils.py) and
get_deformed_atlas (utils/test_utils.py) are run on the CPU.  The inputs are functions of seeds in synth_kernel_refs, so the
file holds results only; tests/test_host_synth_kernel_refs.py holds the references of the kernel tests to it.  Left out:
the 2.1 M-point random set, and the blur cases above 10 000 voxels (synth_kernel_refs.CONV1D_GOLDEN lists the ones kept)."""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_import  # noqa: E402

R = ref_import.setup()
import torch  # noqa: E402

torch.set_num_threads(4)
import Generator.utils as GU  # noqa: E402
import synth_kernel_refs as K  # noqa: E402


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def main():
    d = {}
    for vi, (shape, spiked) in enumerate(K.INTERP_VOLUMES):
        X = T(K.interp_volume(shape, spiked))
        for pname, pts in (("lattice", K.lattice_points(shape)), ("hand", K.hand_points(shape))):
            for dv in K.INTERP_DEFAULTS:
                out = GU.fast_3D_interp_torch(X, T(pts[0]), T(pts[1]), T(pts[2]), "linear", dv)
                d["lin/%d/%s/%g" % (vi, pname, dv)] = out.numpy()
    # nearest mode indexes Y.shape[3]: the reference takes 3-D coordinate grids only there
    pts = [T(p).reshape(-1, 1, 1) for p in K.nearest_points()]
    for kind in ("int32", "bits"):
        for C in (1, 3):
            X = K.nearest_volume(kind, C)
            Xt = T(X) if kind == "int32" else T(X.view(np.int32))          # bit patterns travel as int32: indexing copies them
            out = GU.fast_3D_interp_torch(Xt, *pts, "nearest").numpy()
            d["near/%s/%d" % (kind, C)] = out.reshape((-1,) + out.shape[3:]) if C > 1 else out.reshape(-1)
    for name, _, _, _ in K.ZOOM_CASES:
        X, factor, _ = K.zoom_case(name)
        d["zoom/" + name] = GU.myzoom_torch(T(X), factor).numpy()
    for name in K.CONV1D_GOLDEN:
        x, k, axis, sigma, _ = K.conv1d_case(name, "gauss")
        d["blur/" + name] = GU.gaussian_blur_3d(T(x), K.blur_stds(axis, sigma), "cpu").numpy().reshape(x.shape)
    # get_deformed_atlas without importing its module (it reads an atlas file through nibabel at import)
    src = open(R + "/utils/test_utils.py").read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "get_deformed_atlas"]
    for name in K.ATLAS_CASES:
        mask, rx, ry, rz, atlas, A = K.atlas_case(name)
        ns = {"torch": torch, "A": T(A), "MNI": T(atlas), "fast_3D_interp_torch": GU.fast_3D_interp_torch}
        exec(compile(ast.Module(body=fn, type_ignores=[]), "x", "exec"), ns)
        d["atlas/" + name] = ns["get_deformed_atlas"](T(mask), T(rx), T(ry), T(rz)).numpy()
        d["atlas_tile/" + name] = ns["get_deformed_atlas"](T((mask != 0).astype(np.float32)), T(rx), T(ry), T(rz)).numpy()
    out = os.path.join(HERE, "synth_edges.npz")
    np.savez_compressed(out, **d)
    print(out, len(d), "arrays", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
