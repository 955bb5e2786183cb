"""Golden results of the reference's OWN tail on the small inputs of tests/tail_refs.py (build container only):

    python tests/golden/make_golden_tail.py        -> tests/golden/tail_edges.npz

Per head set of tail_refs.GOLDEN_SETS, on tail_refs.golden_case (40 voxels, 64 features): F.normalize, the TaskHead final
convs (Trainer/models/head.py), SegProcessor / DistProcessor / PatholProcessor (joiner.py) and get_postprocessor
(Trainer/models/__init__.py:272-354: fake_cortical, high_res, exp, CT * 1000, the label through
label_list_segmentation), for the full and the left-hemisphere head sets among them, all on the CPU in fp32.  The maps are
stored in the slot order of tail_refs.head_spec.  `nonfinite/*` are torch.softmax / torch.argmax on rows holding NaN and
infinities.  The inputs are functions of seeds in tail_refs, so the file holds results only;
tests/test_host_tail_refs.py holds the references of the kernel tests to it."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_import  # noqa: E402

R = ref_import.setup()
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

torch.set_num_threads(4)
import tail_refs as T  # noqa: E402


@torch.no_grad()
def run_set(name):
    from Trainer.models import get_postprocessor
    from Trainer.models.head import TaskHead
    from Trainer.models.joiner import SegProcessor, DistProcessor, PatholProcessor
    spec, x, W, b, inp = T.golden_case(name)
    tasks = T.GOLDEN_TASKS[name]
    oc = dict(tasks)
    left = oc["distance"] == 2
    gen_args = types.SimpleNamespace(generator=types.SimpleNamespace(left_hemis_only=left), max_surf_distance=spec["max_dist"],
                                     label_list_segmentation=[int(v) for v in spec["lut"]])
    head = TaskHead(None, [64], oc, True).eval()
    row = 0
    for t, n in tasks:
        conv = getattr(head, "final_conv_%s" % t)
        conv.weight.copy_(torch.from_numpy(W[row:row + n]).reshape(n, 64, 1, 1, 1))
        conv.bias.copy_(torch.from_numpy(b[row:row + n]))
        row += n
    n = x.shape[0]
    feat = F.normalize(torch.from_numpy(x).t().reshape(1, 64, n, 1, 1), dim=1)
    samples = [{"input": torch.from_numpy(inp).reshape(1, 1, n, 1, 1)}]
    outs = [head([feat])]
    raw = torch.cat([outs[0][t] for t, _ in tasks], 1).reshape(-1, n).t().numpy().copy()
    procs = [SegProcessor(), DistProcessor(gen_args)] + ([PatholProcessor()] if "pathology" in oc else [])
    for p in procs:
        outs = p(outs, samples)
    seg = outs[0]["segmentation"].reshape(-1, n).t().numpy().copy()
    task_names = {{"bias_field_log": "bias_field", "high_res_residual": "super_resolution"}.get(t, t) for t in oc}
    outs, _, _ = get_postprocessor(gen_args, None, outs, samples, None, None, task_names)
    o = {k: v.reshape(-1, n).numpy() for k, v in outs[0].items()}
    maps = np.full((spec["n_maps"], n), np.nan, np.float32)
    slot = 0
    for t, c in tasks:
        if t == "segmentation":
            continue
        key = {"bias_field_log": ["bias_field"], "distance": ["lp", "lw", "rp", "rw"][:c],
               "registration": ["regx", "regy", "regz"]}.get(t, [t])
        rows = np.concatenate([o[k] for k in key], 0)
        assert rows.shape[0] == c, (t, rows.shape)
        maps[slot:slot + c] = rows
        slot += c
    maps[spec["slot_high_res"]:spec["slot_high_res"] + spec["n_sr"]] = o["high_res"]
    maps[spec["slot_fake"]] = o["fake_cortical"][0]
    assert not np.isnan(maps).any()
    return {"fn": feat.reshape(64, n).t().numpy().copy(), "raw": raw, "maps": maps, "seg": seg,
            "label": o["label"][0].astype(np.int64)}


def main():
    d = {}
    for name in T.GOLDEN_SETS:
        for k, v in run_set(name).items():
            d["%s/%s" % (name, k)] = v
    z = torch.from_numpy(T.nonfinite_rows())
    p = torch.softmax(z, 1)
    d["nonfinite/softmax"] = p.numpy()
    d["nonfinite/argmax"] = torch.argmax(p, 1).numpy()
    out = os.path.join(HERE, "tail_edges.npz")
    np.savez_compressed(out, **d)
    print(out, len(d), "arrays", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
