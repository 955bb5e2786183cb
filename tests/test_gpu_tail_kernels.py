"""The fused network tail (bfm_tail_heads, bfm_tail_heads_rows, bfm_tail_raw_rows of brainfm_amd/csrc/tail_heads.hip) and the
per-voxel kernels beside it (bfm_ew_unary, bfm_ew_binary, bfm_softmax_cl, bfm_argmax_lut_cl, bfm_fake_cortical of
csrc/elementwise.hip, bfm_head_bias_lrelu of csrc/head_layers.hip) on their own, through the C ABI, route by route, against
the float64 references and derived bounds of tests/tail_refs.py (the derivations stand in its docstring;
tests/test_host_tail_refs.py pins them to the reference implementation and shows that each named mistake fails them).

Two stages, so that each tolerance is tight.  Stage A: the raw logits (bfm_tail_heads(..., raw_out) and bfm_tail_raw_rows,
which must agree bit for bit) and feat_norm against (a) the float64 emulation of the arithmetic as coded, under fp32
accumulation alone, and (b) the true float64 result under the derived per-logit bound.  Stage B: a second call on the same
operands gives maps, seg_prob and label, compared with float64 functions of the kernel's OWN logits -- bit for bit where the
definition is one fp32 operation (PLAIN, CT, DIST, high_res), in ulps for expf (exp, sigmoid), under derived bounds for
fake_cortical and the softmax, and the label rules of the issue.  Every tail case makes four calls: raw [nvox][n_out] +
feat_norm, raw rows (pitch > nvox), bfm_tail_heads_rows with seg_prob (row_stride > nvox), and bfm_tail_heads with the
pointer table and without seg_prob (the argmax shortcut); the two map forms and the two labels must agree exactly.  The
route is asked of the library (bfm_tail_route) and asserted.

Conventions (those of tests/test_gpu_synth_kernels.py): outputs start as 0xFFFFFFFF between a front guard and a sentinel
tail that must come back untouched; inputs sit between NaN guard bands.  Each case prints one line: kernel, route, worst
ratio to its bound (the bar is 1) or worst ulp distance.

The launcher branches of elementwise.hip have no query; EW_ROUTE restates the condition (contiguous, 16-byte aligned,
n >= 1024: float4 body + scalar tail launch when n & 3; else the strided scalar kernel) and every case names its branch.

Cases the issue's list words differently: the left-hemisphere set of process_args has 29 outputs (`left29`); `left27`
is a 27-output set for the count tail_launch's comment names; both take route 3.  nvox = 131 072 + 197 reaches slot 1 of
the groups of four only (chunk c sits in slot (c // 2048) % 4), so 3 * 131 072 + 71 is there for slots 2 and 3.  A set of
more than 64 non-segmentation outputs gives its rows beyond the 60th no map (the kernel takes at most 64 maps).

Measured on MI355X (also in HISTORY.md), worst over the module; ratios are to the bound (the bar is 1), 83 cases, no kernel
defect, module wall time 5.8 s (slowest case 1.0 s, nvox = 524 359):
    tail route                      0 fp32     1 split    2 split<56,3>   3 split<18,1>
    raw vs emulation (a)            0.390      0.911      0.037           0.039
    raw vs float64 (b)              0.390      0.904      0.031           0.035
    feat_norm, of 20 roundings      0.164      0.185      0.166           0.166
    exp, ulp                        0.674      0.706      0.679           0.659
    sigmoid, ulp                    1.39       1.61       -               -
    fake_cortical                   0.187      0.220      0.261           0.223
    softmax                         1.0        0.417      0.284           0.407
  The 0.39 / 0.91 of (a) and (b) are the rows of norm 1e-20, whose logits are the bias plus nothing: there the bound is the
  last rounding alone (EPS |e|, between one and two half-ulps); random rows stay below 0.18 (split) and 0.06 (fp32).
  Softmax 1.0: probabilities just under 2^-126 that the kernel flushes (the bound's floor); 0.549 over the probabilities
  above 2^-100 (softmax_n).  Tiny head_wmax: raw == bias.
  bit for bit, 0 differing elements: fragment layout (all four routes), PLAIN / CT / DIST / high_res maps, raw rows against
  raw [nvox][n_out], pointer-table against row maps, labels with against without seg_prob, gated against ungated calls.
    bfm_ew_unary EXP 0.842 ulp, SIGMOID 2.01 ulp, GAMMA 1.1e-7 of max |result| (stated: 2e-6); bfm_ew_binary MUL_EXP 1.51 ulp;
    every other op, bfm_argmax_lut_cl and bfm_head_bias_lrelu: 0 differing elements on every branch
    bfm_softmax_cl 0.66 (C = 2), 0.59, 0.37;  bfm_fake_cortical 0.176 / 0.170 with tanhf taken at 4.02 ulp
The limits of the expf-class comparisons are twice the measured worst (ULP_LIMIT, EW_ULP_LIMIT), never above 8 ulp.
Needs an MI355X: run with `-m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import tail_refs as T

pytestmark = pytest.mark.gpu

# limits of the expf-class comparisons, in ulps of the float64 value: min(2 x the measured worst, 8)
# (measured worst on MI355X: tail exp 0.706, tail sigmoid 1.61, EW_EXP 0.842, EW_SIGMOID 2.01, EW_MUL_EXP 1.51)
ULP_LIMIT = {"ulp_exp": 1.42, "ulp_sigmoid": 3.22}                     # the tail's exp(bias_field_log) and sigmoid(pathology)
EW_ULP_LIMIT = {"EXP": 1.69, "SIGMOID": 4.02, "MUL_EXP": 3.02}
TANHF_ULPS = 4.02                # taken for tanhf inside bfm_fake_cortical's bound: the largest of the measured limits
assert max(list(ULP_LIMIT.values()) + list(EW_ULP_LIMIT.values()) + [TANHF_ULPS]) <= T.ULP_CAP

GUARD = 64
TAIL = 4096
NAN_BITS = 0x7FC00000
UNWRITTEN = -1
SENT = -7777
E_ARG, E_SHAPE = -1, -2
F32, F64 = np.float32, np.float64
WORST = {}


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _lib():
    from brainfm_amd import _lib as L
    return L, L.load()


def _in(a, offset=0):
    """A device copy of a 4-byte array between NaN guard bands, `offset` words off the 16-byte alignment."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    n = a.size
    flat = torch.full((GUARD + offset + n + GUARD,), NAN_BITS, dtype=torch.int32, device=_dev())
    v = flat[GUARD + offset:GUARD + offset + n]
    v.copy_(torch.from_numpy(a.reshape(-1).view(np.int32)))
    assert v.data_ptr() % 16 == 4 * (offset % 4)
    return v


class _Out:
    """n unwritten 4-byte words, `offset` words off alignment, a guard in front and a sentinel tail behind."""

    def __init__(self, n, offset=0, init=None):
        self.n, self.lo = n, GUARD + offset
        self.flat = torch.full((self.lo + n + TAIL,), SENT, dtype=torch.int32, device=_dev())
        self.view = self.flat[self.lo:self.lo + n]
        if init is None:
            self.view.fill_(UNWRITTEN)
        else:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1).view(np.int32)))

    def ptr(self):
        return self.view.data_ptr()

    def get(self, label, dtype=np.float32, shape=None):
        torch.cuda.synchronize()
        h = self.flat.cpu().numpy()
        assert (h[:self.lo] == SENT).all(), label + ": wrote in front of the output"
        assert (h[self.lo + self.n:] == SENT).all(), label + ": wrote behind the output"
        out = h[self.lo:self.lo + self.n].view(dtype)
        return out.reshape(shape) if shape is not None else out

    def untouched(self, label):
        assert (self.get(label, np.int32) == UNWRITTEN).all(), label + ": written"


def _report(kernel, route, **figs):
    txt = "  ".join("%s %.3g" % kv for kv in figs.items())
    print("\n%s [route %s]: %s" % (kernel, route, txt), end="")
    for k, v in figs.items():
        if k == "near":
            continue
        key = (kernel if kernel.startswith("ew_") else kernel.split()[0], route, k)
        WORST[key] = max(WORST.get(key, 0.0), v)


def _unwritten(a):
    return np.asarray(a).view(np.int32) == UNWRITTEN


# ------------------------------------------------------------------------------------------------------------ the tail
PAD = 37                 # row_stride = nvox + PAD: rows past nvox keep their sentinel


def _tail(x, W, b, spec, unit, wmax, inp=None, gate=False, want_route=None, feat_norm=True):
    """The four calls of the module docstring.  Returns raw (nvox, n_out), fn, maps (n_maps, nvox), seg, label, label_fast
    (unwritten words still 0xFFFFFFFF / -1) and the route."""
    L, lib = _lib()
    n, c = x.shape
    no, nm, ns = spec["n_out"], spec["n_maps"], spec["n_seg"]
    dx = _in(x)
    dW, db = _in(W if no else np.zeros(4, F32)), _in(b if no else np.zeros(4, F32))
    drole, dslot = _in(spec["roles"] if no else np.zeros(4, np.int32)), _in(spec["out_slot"] if no else np.zeros(4, np.int32))
    dlut = _in(spec["lut"]) if ns else None
    dinp = _in(inp) if inp is not None else None

    def desc(skip=0):
        return L.TailDesc(no, c, dW.data_ptr(), db.data_ptr(), drole.data_ptr(), dslot.data_ptr(), spec["seg_first"], ns,
                          dlut.data_ptr() if ns else None, spec["n_dist"], spec["dist_first"], spec["max_dist"], unit,
                          spec["slot_high_res"], spec["slot_fake"], nm, wmax, skip)

    d = desc()
    route = lib.bfm_tail_route(C.byref(d))
    assert route == T.tail_route(c, no, ns, unit, wmax)
    if want_route is not None:
        assert route == want_route, "this case means route %d, the launcher takes %d" % (want_route, route)
    S = L.stream_ptr()
    res = dict(route=route, raw=np.zeros((n, 0), F32), maps=None, seg=None, label=None, label_fast=None, fn=None)
    # 1: raw logits [nvox][n_out] + feat_norm (n_out = 0: feat_norm alone, what engine.normalize calls)
    ofn = _Out(n * c) if feat_norm else None
    oraw = _Out(n * no) if no else None
    rc = lib.bfm_tail_heads(L.ptr(dx), None, n, C.byref(d), ofn.ptr() if ofn else None, None, None, None,
                            oraw.ptr() if oraw else None, S)
    assert rc == 0, L.ERR.get(rc, rc)
    if ofn:
        res["fn"] = ofn.get("feat_norm", shape=(n, c))
    if not no:
        return res
    res["raw"] = oraw.get("raw_out", shape=(n, no))
    # 2: the same as [n_out] rows of pitch nvox + PAD
    orow = _Out(no * (n + PAD))
    rc = lib.bfm_tail_raw_rows(L.ptr(dx), n, C.byref(d), None, orow.ptr(), n + PAD, S)
    assert rc == 0, L.ERR.get(rc, rc)
    rows = orow.get("raw_rows", shape=(no, n + PAD))
    assert T.bits_equal(rows[:, :n].T, res["raw"]), "bfm_tail_raw_rows != bfm_tail_heads(raw_out) transposed"
    assert _unwritten(rows[:, n:]).all(), "raw rows: wrote past nvox"
    # 3: maps as rows of one buffer, with seg_prob and label; the gate as the per-call flag
    omap = _Out(nm * (n + PAD)) if nm else _Out(4)
    oseg = _Out(n * ns) if ns else None
    olab = _Out(2 * n) if ns else None
    rc = lib.bfm_tail_heads_rows(L.ptr(dx), L.ptr(dinp), n, C.byref(d), None, omap.ptr(), n + PAD, oseg.ptr() if ns else None,
                                 olab.ptr() if ns else None, 1 if gate else 0, S)
    assert rc == 0, L.ERR.get(rc, rc)
    m = omap.get("maps_rows", shape=(nm, n + PAD)) if nm else np.zeros((0, n + PAD), F32)
    assert _unwritten(m[:, n:]).all(), "maps rows: wrote past nvox"
    res["maps"] = m[:, :n]
    if ns:
        res["seg"] = oseg.get("seg_prob", shape=(n, ns))
        res["label"] = olab.get("label", np.int64)
    # 4: maps through the pointer table, no seg_prob (the argmax shortcut); the gate as the descriptor's field
    otab = [_Out(n) for _ in range(nm)]
    tab = torch.tensor([o.ptr() for o in otab] or [0], dtype=torch.int64, device=_dev())
    olab2 = _Out(2 * n) if ns else None
    d2 = desc(1 if gate else 0)
    rc = lib.bfm_tail_heads(L.ptr(dx), L.ptr(dinp), n, C.byref(d2), None, tab.data_ptr(), None, olab2.ptr() if ns else None, None, S)
    assert rc == 0, L.ERR.get(rc, rc)
    for i, o in enumerate(otab):
        assert _same_words(o.get("maps[%d]" % i), res["maps"][i]), "pointer-table map %d != row form" % i
    if ns:
        res["label_fast"] = olab2.get("label (no seg_prob)", np.int64)
    return res


def _same_words(a, b):
    """The same 4-byte words; a computed NaN equals a computed NaN, an unwritten word only an unwritten word."""
    a, b = np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32)
    nan = np.isnan(a.view(F32)) & np.isnan(b.view(F32)) & (a != UNWRITTEN) & (b != UNWRITTEN)
    return bool(((a == b) | nan).all())


def _check(name, x, W, b, spec, unit, wmax, inp=None, gate=False, want_route=None, random_case=False):
    r = _tail(x, W, b, spec, unit, wmax, inp, gate, want_route)
    a = T.check_stage_a(r["raw"], x, W, b, unit, wmax, r["fn"])
    keep = T.gate_keep(inp, len(x)) if gate else None
    if keep is not None:
        for k in ("maps", "seg"):
            if r[k] is not None and r[k].size:
                arr = r[k] if k == "seg" else r[k].T
                assert _unwritten(arr[keep]).all(), "gated chunk: %s written" % k
    s = T.check_stage_b(r["raw"], r["maps"], r["seg"], r["label"], r["label_fast"], spec, inp, keep, ULP_LIMIT, random_case)
    figs = dict(emul=a.get("emul", 0), true=a.get("true", 0), fn=a.get("fn", 0), ulp_exp=s["ulp_exp"],
                ulp_sigmoid=s["ulp_sigmoid"], fake=s["fake"], softmax=s["softmax"], softmax_n=s["softmax_n"])
    _report("tail " + name, r["route"], **figs)
    return r


def _set(name, nvox, seed, c=64, wscale=4.0, **kw):
    spec = T.head_spec(T.HEAD_SETS[name], **kw)
    x, W, b = T.operands(c, spec["n_out"], nvox, seed, wscale=wscale)
    return spec, x, W, b, float(np.abs(W).max()), T.image_input(nvox, seed)


def test_stage_a_grid():
    """c_feat x n_out x unit_feat x nvox, pairwise (tail_refs.stage_a_grid): every output a PLAIN map, so stage B is the
    bit-for-bit copy.  c_feat 8 and 24 take route 0 even with unit_feat = 1."""
    for c, n_out, unit, nvox, seed in T.stage_a_grid():
        x, W, b = T.operands(c, n_out, nvox, seed)
        spec = T.head_spec([(T.PLAIN, n_out)])
        want = 1 if (unit and c % 16 == 0) else 0
        _check("grid c%d o%d u%d n%d" % (c, n_out, unit, nvox), x, W, b, spec, unit, float(np.abs(W).max()), want_route=want)


@pytest.mark.parametrize("route,c,n_out,n_seg", [(0, 64, 96, 0), (0, 8, 33, 0), (1, 64, 96, 0), (1, 16, 33, 0), (2, 64, 69, 56),
                                                 (3, 64, 29, 18)])
def test_fragment_layout_exact(route, c, n_out, n_seg):
    """Exact products, distinct per (voxel, channel, output): any lane, half, k-step or column-block mix-up changes a bit.
    Route 0: small-integer features and weights, unit_feat = 0.  Split routes: rows of exactly four entries of +-0.5
    (norm exactly 1, inv exactly 1, so a = +-2^13 exactly) against small-integer weights."""
    nvox = 131
    rs = np.random.RandomState(route * 7 + c)
    W = ((np.arange(n_out)[:, None] * 7 + np.arange(c)[None] * 3) % 23 - 11).astype(F32)
    b = (np.arange(n_out) % 5 - 2).astype(F32)
    if route == 0:
        x = ((np.arange(nvox)[:, None] * 5 + np.arange(c)[None] * 11) % 17 - 8).astype(F32)
        unit = 0
    else:
        x = np.zeros((nvox, c), F32)
        for v in range(nvox):
            x[v, rs.choice(c, 4, replace=False)] = rs.choice([-0.5, 0.5], 4)
        unit = 1
    groups = [(T.SEG, n_seg), (T.PLAIN, n_out - n_seg)] if n_seg else [(T.PLAIN, n_out)]
    spec = T.head_spec(groups)
    r = _tail(x, W, b, spec, unit, float(np.abs(W).max()), want_route=route)
    want = (x.astype(F64) @ W.astype(F64).T + b).astype(F32)
    bad = int((r["raw"] != want).sum())
    _report("tail fragment c%d o%d" % (c, n_out), route, differing=bad)
    assert bad == 0 and (np.abs(want) < 2 ** 24).all()
    if unit:
        assert T.bits_equal(r["fn"], x)


MAGNITUDES = [
    # name, c, n_out, unit, feature scale, weight scale, head_wmax (None: max |W|), route
    ("w 2^-20", 64, 33, 1, 1.0, 2.0 ** -20, None, 1), ("w 2^10", 64, 33, 1, 1.0, 2.0 ** 10, None, 1),
    ("w 1", 32, 65, 1, 1.0, 1.0, None, 1), ("w 2^10 fp32", 64, 33, 0, 1.0, 2.0 ** 10, None, 0),
    ("feat 1e-3", 64, 33, 0, 1e-3, 1.0, None, 0), ("feat 1e3", 48, 65, 0, 1e3, 1.0, None, 0),
    ("feat 1e3 unit", 64, 33, 1, 1e3, 1.0, None, 1), ("feat 1e-3 unit", 64, 33, 1, 1e-3, 1.0, None, 1),
    ("wmax generous", 64, 33, 1, 1.0, 1.0, 64.0, 1),
]


@pytest.mark.parametrize("case", MAGNITUDES, ids=[m[0] for m in MAGNITUDES])
def test_magnitudes(case):
    """With an all-zero row (F.normalize gives 0, the logits are the bias) and a row of norm 1e-20 (divided by 1e-12)."""
    name, c, n_out, unit, fs, ws, wmax, route = case
    x, W, b = T.operands(c, n_out, 130, 17, fscale=fs, wscale=ws)
    x[0] = 0
    x[67] *= F32(1e-20 / np.sqrt((x[67].astype(F64) ** 2).sum()))
    spec = T.head_spec([(T.PLAIN, n_out)])
    r = _check("magnitude " + name, x, W, b, spec, unit, float(np.abs(W).max()) if wmax is None else wmax, want_route=route)
    assert T.bits_equal(r["raw"][0], b) and (r["fn"][0] == 0).all()
    if unit:
        assert np.abs(r["fn"][67].astype(F64) - x[67].astype(F64) * 1e12).max() <= 3 * T.EPS * np.abs(x[67] * 1e12).max()


def test_tiny_head_wmax_clamps_the_exponent():
    """head_wmax = max |W| around 1e-30: wexp is clamped at 60, w 2^60 is below the fp16 subnormals, both weight halves are
    zero and the kernel returns the bias alone; the derived bound (about c_feat 2^-85 against logits of 1e-30) allows
    exactly that and the emulation says the same.  The fp32 chain on the same operands keeps the products."""
    x, W, b = T.operands(64, 33, 130, 23, wscale=1e-30, bscale=0.0)
    spec = T.head_spec([(T.PLAIN, 33)])
    wmax = float(np.abs(W).max())
    assert 1e-31 < wmax < 1e-29
    r = _check("tiny wmax split", x, W, b, spec, 1, wmax, want_route=1)
    assert (r["raw"] == 0).all()
    r0 = _check("tiny wmax fp32", x, W, b, spec, 0, wmax, want_route=0)
    assert (r0["raw"] != 0).mean() > 0.9


HEAD_CASES = [("full69", 1, 2), ("left29", 1, 3), ("left27", 1, 3), ("full69", 0, 0), ("left29", 0, 0), ("seg20_first7", 1, 1),
              ("seg70", 1, 1), ("seg96", 1, 1), ("seg96", 0, 0), ("uncert", 1, 1), ("uncert", 0, 0), ("sr2", 1, 1), ("dist2", 1, 1),
              ("dist4", 1, 1), ("noseg", 1, 1), ("noseg", 0, 0)]


@pytest.mark.parametrize("name,unit,route", HEAD_CASES, ids=["%s-u%d" % (n, u) for n, u, _ in HEAD_CASES])
def test_head_sets(name, unit, route):
    """257 voxels (four full chunks and one voxel: more than one wave, a partial chunk), logits of a few units so that
    the distance clamp, CT * 1000 and the exponentials see both sides of their thresholds.  n_out >= 62 takes the
    dynamic-LDS opt-in above 64 KB; n_seg 70 and 96 the > 64 path; `uncert` the LDS-table fallback beyond 16 outputs."""
    spec, x, W, b, wmax, inp = _set(name, 257, 31)
    r = _check("heads " + name, x, W, b, spec, unit, wmax, inp, want_route=route, random_case=True)
    if spec["n_dist"]:
        d = r["raw"][:, spec["dist_first"]:spec["dist_first"] + spec["n_dist"]]
        assert (np.abs(d) > spec["max_dist"]).any() and (np.abs(d) < spec["max_dist"]).any()


def test_no_heads_feat_norm_only():
    for c, nvox in ((64, 257), (8, 65), (48, 1)):
        x = T.operands(c, 1, nvox, 41)[0]
        x[0] = 0
        spec = T.head_spec([])
        r = _tail(x, np.zeros((0, c), F32), np.zeros(0, F32), spec, 1, 0.0, want_route=0)
        a = T.check_stage_a(r["raw"], x, np.zeros((0, c), F32), np.zeros(0, F32), 1, 0.0, r["fn"])
        _report("tail feat_norm only c%d n%d" % (c, nvox), 0, fn=a["fn"])
    # unit_feat = 0: feat_norm is the copy
    r = _tail(x, np.zeros((0, c), F32), np.zeros(0, F32), spec, 0, 0.0, want_route=0)
    assert T.bits_equal(r["fn"], x)


# ------------------------------------------------------------------------------------------------------------ planted logits
def _selection(spec, logits):
    """Route 0 with one 1 per weight row: the 64 features ARE the logits, exactly."""
    n_out = spec["n_out"]
    assert logits.shape[1] == n_out <= 64
    x = np.zeros((logits.shape[0], 64), F32)
    x[:, :n_out] = logits
    return x, np.eye(n_out, 64, dtype=F32), np.zeros(n_out, F32)


def _planted_expect(r, spec, pos, gap):
    z = r["raw"][:, spec["seg_first"]:spec["seg_first"] + spec["n_seg"]]
    if gap == 0.0:
        assert (z[:, pos] == z[:, pos + 1]).all(), "identical rows with equal biases gave different logits"
    return z


@pytest.mark.parametrize("name,route", [("full69", 2), ("left29", 3), ("seg20_first7", 1), ("seg70", 1), ("full69", 0)])
def test_planted_gaps_identical_rows(name, route):
    """Two identical weight rows whose biases differ by the gap, at the first, a middle and the last class pair; every
    gap around ARGMAX_GAP = 1e-5 on both sides.  Gap 0: the first index must win, also when the tie is not the first two
    classes.  The label without seg_prob (shortcut allowed) equals the label with it at every voxel."""
    spec = T.head_spec(T.HEAD_SETS[name])
    ns, sf = spec["n_seg"], spec["seg_first"]
    x = T.operands(64, spec["n_out"], 130, 11)[0]
    unit = 0 if route == 0 else 1
    for pos in (0, ns // 2, ns - 2):
        W, b = T.planted_rows(ns, sf, spec["n_out"], 64, 9, pos)
        wmax = float(np.abs(W).max())
        for gap in T.GAPS:
            bg = T.planted_bias(b, sf, pos, gap)
            xs = x if unit else x / np.sqrt((x.astype(F64) ** 2).sum(1, keepdims=True)).astype(F32)
            r = _tail(xs, W, bg, spec, unit, wmax, want_route=route, feat_norm=False)
            z = _planted_expect(r, spec, pos, gap)
            s = T.check_stage_b(r["raw"], r["maps"], r["seg"], r["label"], r["label_fast"], spec, None, None, ULP_LIMIT)
            g = (z[:, pos + 1].astype(F64) - z[:, pos]).min()
            top2 = np.sort(np.argsort(z, 1)[:, -2:], 1)
            assert (top2 == [pos, pos + 1]).all(), "the planted pair is not on top"
            want = spec["lut"][pos] if gap == 0.0 else spec["lut"][pos + 1]
            if gap == 0.0 or g > T.SOFTMAX_DELTA:
                assert (r["label"] == want).all() and (r["label_fast"] == want).all()
            _report("tail planted %s pos %d gap %s" % (name, pos, gap), r["route"], softmax=s["softmax"], near=s["near"])


@pytest.mark.parametrize("lane", [0, 63])
def test_planted_mixed_wave(lane):
    """One close voxel in lane 0 or lane 63 of an otherwise clear wave (the __any(!sure) vote), route 0 with the features
    as logits, and the same through the split route 2 with a third class that leads everywhere else."""
    spec = T.head_spec([(T.SEG, 56), (T.PLAIN, 8)])
    rs = np.random.RandomState(5)
    for gap in T.GAPS:
        z = (rs.randn(192, 64) * 0.1).astype(F32)
        z[:, 20] = 3.0                                      # clear everywhere ...
        v = 64 + lane
        z[v, 20] = -3.0                                     # ... but here: classes 7 and 41 within the gap
        z[v, 7] = 2.0
        z[v, 41] = np.nextafter(F32(2), F32(3)) if gap == "ulp" else F32(2.0 + gap)
        x, W, b = _selection(spec, z)
        r = _tail(x, W, b, spec, 0, 1.0, want_route=0, feat_norm=False)
        assert T.bits_equal(r["raw"], z)
        T.check_stage_b(r["raw"], r["maps"], r["seg"], r["label"], r["label_fast"], spec, None, None, ULP_LIMIT)
        want = np.full(192, spec["lut"][20])
        want[v] = spec["lut"][7 if gap == 0.0 else 41]
        assert np.array_equal(r["label"], want) and np.array_equal(r["label_fast"], want), gap
    # split route: identical rows 7 / 8, class 20 = 8 u_0 leads where u_0 > 0
    spec = T.head_spec(T.HEAD_SETS["full69"])
    sf = spec["seg_first"]
    W, b = T.planted_rows(56, sf, 69, 64, 9, 7)
    W[sf + 20] = 0
    W[sf + 20, 0] = 8.0
    b[sf + 20] = 0
    x = T.operands(64, 69, 192, 13)[0]
    x[:, 0] = 6.0
    x[64 + lane, 0] = -6.0
    for gap in T.GAPS:
        r = _tail(x, W, T.planted_bias(b, sf, 7, gap), spec, 1, float(np.abs(W).max()), want_route=2, feat_norm=False)
        s = T.check_stage_b(r["raw"], r["maps"], r["seg"], r["label"], r["label_fast"], spec, None, None, ULP_LIMIT)
        want = np.full(192, spec["lut"][20])
        want[64 + lane] = spec["lut"][7 if gap == 0.0 else 8]
        assert np.array_equal(r["label"], want) and np.array_equal(r["label_fast"], want), gap
    _report("tail planted mixed wave lane %d" % lane, "0+2", softmax=s["softmax"])


def test_non_finite_logits():
    """Route 0.  A NaN feature at single voxels makes every logit of the voxel NaN (NaN * 0); a +inf bias on one class
    makes the softmax row NaN; a -inf bias is an ordinary zero probability.  Labels and probabilities as torch.softmax +
    torch.argmax on the CPU give them (pinned in the host test): a NaN row gives class 0."""
    spec = T.head_spec(T.HEAD_SETS["left29"])
    sf, ns = spec["seg_first"], spec["n_seg"]
    x, W, b = T.operands(64, 29, 130, 19, wscale=4.0)
    wmax = float(np.abs(W).max())
    for kind in ("nan_feature", "pos_inf_bias", "neg_inf_bias"):
        xx, bb = x.copy(), b.copy()
        if kind == "nan_feature":
            xx[[0, 63, 64, 129], [3, 40, 0, 63]] = np.nan
        elif kind == "pos_inf_bias":
            bb[sf + 5] = np.inf
        else:
            bb[sf + 5] = -np.inf
        r = _check("nonfinite " + kind, xx, W, bb, spec, 0, wmax, T.image_input(130, 1), want_route=0)
        z = torch.from_numpy(r["raw"][:, sf:sf + ns].copy())
        p = torch.softmax(z, 1)
        assert np.array_equal(np.isnan(r["seg"]), torch.isnan(p).numpy())
        want = spec["lut"][torch.argmax(p, 1).numpy()]
        assert np.array_equal(r["label"], want) and np.array_equal(r["label_fast"], want), kind
        nanrows = torch.isnan(p).any(1).numpy()
        assert nanrows.sum() == {"nan_feature": 4, "pos_inf_bias": 130, "neg_inf_bias": 0}[kind]
        assert (r["label"][nanrows] == spec["lut"][0]).all()
        if kind == "neg_inf_bias":
            assert (r["seg"][:, 5] == 0).all()


def test_saturation():
    """Route 0 with the features as logits: distances at +-max_dist, one ulp inside and far outside; fast_tanh arguments
    beyond +-15 (max_dist = 10: 2 (v + 0.3) up to 20.6); softmax logits spread over +-80."""
    for name, md in (("dist4", 3.0), ("dist2", 10.0)):
        spec = T.head_spec(T.HEAD_SETS[name], max_dist=md)
        m = F32(md)
        vals = np.array([m, -m, np.nextafter(m, F32(0)), -np.nextafter(m, F32(0)), np.nextafter(m, F32(99)), 100.0, -100.0,
                         1e30, -1e30, 0.0, -0.3, 0.3, 7.2, -7.8, 7.6, -7.6], F32)
        rs = np.random.RandomState(3)
        z = rs.choice(vals, (130, spec["n_out"])).astype(F32)
        x, W, b = _selection(spec, z)
        r = _check("saturation %s max_dist %g" % (name, md), x, W, b, spec, 0, 1.0, want_route=0)
        assert T.bits_equal(r["raw"], z)
    spec = T.head_spec([(T.SEG, 56), (T.PLAIN, 2)])
    z = (np.random.RandomState(4).rand(130, 58) * 160 - 80).astype(F32)
    z[0, :56] = 80.0
    z[1, :56] = -80.0                                        # all-equal rows: 1 / 56 each
    x, W, b = _selection(spec, z)
    r = _check("saturation softmax +-80", x, W, b, spec, 0, 1.0, want_route=0)
    assert (r["label"][:2] == spec["lut"][0]).all()


# ------------------------------------------------------------------------------------------------------------ gate, big
def _same_where_written(r, ref, keep):
    live = ~keep
    assert T.bits_equal(r["maps"][:, live], ref["maps"][:, live]), "gated call differs from the ungated one where it writes"
    assert _unwritten(r["maps"][:, keep]).all(), "gated chunk: map written"
    if ref["seg"] is not None:
        assert T.bits_equal(r["seg"][live], ref["seg"][live]) and _unwritten(r["seg"][keep]).all()
        for k in ("label", "label_fast"):
            assert np.array_equal(r[k][live], ref[k][live]) and (r[k][keep] == -1).all(), k


@pytest.mark.parametrize("name,route", [("sr2", 1), ("left29", 3), ("full69", 2), ("sr2", 0)])
def test_zero_input_gate(name, route):
    """flags = 1 (rows form) and the descriptor field (pointer-table form), everything pre-filled: a chunk of 64 whose
    input is all zero keeps every sentinel; one non-zero at lane 0, at lane 63 or in the partial last chunk writes the
    chunk in full, equal to the ungated call bit for bit."""
    spec, x, W, b, wmax, _ = _set(name, 64 * 5 + 9, 4)
    inp = T.gate_input(len(x))
    unit = 0 if route == 0 else 1
    ref = _check("gate off " + name, x, W, b, spec, unit, wmax, inp, want_route=route)
    r = _check("gate on " + name, x, W, b, spec, unit, wmax, inp, gate=True, want_route=route)
    keep = T.gate_keep(inp, len(x))
    assert list(keep[::64]) == [True, False, False, True, False, False]
    _same_where_written(r, ref, keep)


@pytest.mark.parametrize("nvox", T.BIG_NVOX)
def test_groups_of_four_and_second_lap(nvox):
    """c_feat 16, nine outputs with SR and segmentation, at sizes that put chunks into slot 1, into slots 1..3 and into a
    second lap of the group loop (tail_refs.BIG_NVOX).  Ungated: every logit and map is checked, high_res exactly.  Gated
    with tail_refs.slot_pattern_input, in which neighbouring slots differ: equal to the ungated call where written."""
    spec = T.head_spec(T.HEAD_SETS["big"])
    x, W, b = T.operands(16, spec["n_out"], nvox, 21)
    wmax = float(np.abs(W).max())
    inp = T.slot_pattern_input(nvox)
    slot, lap, _ = T.chunk_slot(nvox)
    ref = _check("big n%d slots %s laps %d" % (nvox, sorted(set(slot)), lap.max() + 1), x, W, b, spec, 1, wmax, inp,
                 want_route=1, random_case=True)
    r = _tail(x, W, b, spec, 1, wmax, inp, gate=True, want_route=1, feat_norm=False)
    keep = T.gate_keep(inp, nvox)
    assert 0.3 < keep.mean() < 0.37
    _same_where_written(r, ref, keep)


def test_refusals_return_the_documented_code_and_write_nothing():
    L, lib = _lib()
    spec, x, W, b, wmax, inp = _set("sr2", 130, 2)
    n, no, nm, ns = 130, spec["n_out"], spec["n_maps"], spec["n_seg"]
    big = np.zeros(n * 80, F32)
    dx, dW, db = _in(big), _in(np.zeros(100 * 80, F32)), _in(np.zeros(100, F32))
    drole, dslot, dlut = _in(np.resize(spec["roles"], 100)), _in(np.resize(spec["out_slot"], 100)), _in(np.resize(spec["lut"], 100))
    dinp = _in(inp)
    outs = dict(fn=_Out(n * 80), maps=_Out(nm * n), seg=_Out(n * 100), lab=_Out(2 * n), raw=_Out(n * 100))
    tab = torch.tensor([outs["maps"].ptr() + 4 * n * i for i in range(nm)], dtype=torch.int64, device=_dev())
    S = L.stream_ptr()

    def desc(**kw):
        f = dict(n_out=no, c_feat=64, head_w=dW.data_ptr(), head_b=db.data_ptr(), roles=drole.data_ptr(),
                 out_slot=dslot.data_ptr(), seg_first=spec["seg_first"], n_seg=ns, seg_lut=dlut.data_ptr(), n_dist=0,
                 dist_first=0, max_dist=3.0, unit_feat=1, slot_high_res=spec["slot_high_res"], slot_fake_cortical=-1,
                 n_maps=nm, head_wmax=1.0, skip_zero_input=0)
        f.update(kw)
        return L.TailDesc(**f)

    def rows(d, feat=None, stride=n, flags=0, maps=True):
        return lib.bfm_tail_heads_rows(feat or dx.data_ptr(), dinp.data_ptr(), n, C.byref(d), outs["fn"].ptr(),
                                       outs["maps"].ptr() if maps else None, stride, outs["seg"].ptr(), outs["lab"].ptr(), flags, S)

    cases = [("c_feat 12", rows(desc(c_feat=12)), E_SHAPE), ("c_feat 72", rows(desc(c_feat=72)), E_SHAPE),
             ("n_out 97", rows(desc(n_out=97)), E_SHAPE),
             ("segmentation past n_out", rows(desc(seg_first=no - ns + 1)), E_SHAPE),
             ("n_dist 3", rows(desc(n_dist=3)), E_SHAPE),
             ("feat off by 4 bytes", rows(desc(), feat=dx.data_ptr() + 4), E_ARG),
             ("row_stride < nvox", rows(desc(), stride=n - 1), E_ARG),
             ("slot_high_res >= n_maps", rows(desc(slot_high_res=nm)), E_SHAPE),
             ("slot_fake_cortical >= n_maps", rows(desc(slot_fake_cortical=nm, n_dist=2)), E_SHAPE),
             ("n_maps 65", rows(desc(n_maps=65)), E_SHAPE), ("flags 2", rows(desc(), flags=2), E_ARG), ("no maps_rows", rows(desc(), maps=False), E_ARG),
             ("heads but nowhere to write them",
              lib.bfm_tail_heads(dx.data_ptr(), None, n, C.byref(desc()), outs["fn"].ptr(), None, None, None, None, S), E_SHAPE),
             ("nothing to write at all",
              lib.bfm_tail_heads(dx.data_ptr(), None, n, C.byref(desc()), None, None, None, None, None, S), E_ARG),
             ("n_seg without a LUT",
              lib.bfm_tail_heads(dx.data_ptr(), None, n, C.byref(desc(seg_lut=None)), None, tab.data_ptr(), None, None, None, S),
              E_SHAPE),
             ("nvox 0", lib.bfm_tail_heads(dx.data_ptr(), None, 0, C.byref(desc()), None, tab.data_ptr(), None, None, None, S),
              E_ARG),
             ("raw rows pitch < nvox", lib.bfm_tail_raw_rows(dx.data_ptr(), n, C.byref(desc()), None, outs["raw"].ptr(), n - 1, S),
              E_ARG),
             ("raw rows NULL", lib.bfm_tail_raw_rows(dx.data_ptr(), n, C.byref(desc()), None, None, n, S), E_ARG)]
    for name, rc, want in cases:
        assert rc == want, (name, L.ERR.get(rc, rc))
    for k, o in outs.items():
        o.untouched("refusal: " + k)
    print("tail refusals: %d calls refused with the documented code, nothing written" % len(cases))


# ------------------------------------------------------------------------------------------------------------ ew_unary / binary
EW_LAP_N = 4 * 1048576 + 4 * 300 + 3          # the float4 grid is capped at 4096 x 256: a second lap, and an n & 3 tail
# name, n, operand offset (words), in stride, out stride, expected branch
EW_CONFIGS = [("float4 n1024", 1024, 0, 1, 1, "float4"), ("float4 n1025", 1025, 0, 1, 1, "float4+tail"),
              ("float4 n1027", 1027, 0, 1, 1, "float4+tail"), ("scalar n1023", 1023, 0, 1, 1, "scalar"),
              ("base off 4 bytes", 1027, 1, 1, 1, "scalar"), ("stride 3 -> 1", 1030, 0, 3, 1, "scalar"),
              ("stride 1 -> 2", 1030, 0, 1, 2, "scalar"), ("n 1", 1, 0, 1, 1, "scalar")]


def EW_ROUTE(n, aligned, contiguous):
    if contiguous and aligned and n >= 1024:
        return "float4+tail" if n & 3 else "float4"
    return "scalar"


def _ew_compare(label, route, kind, got, ref, ulp_figs, limit=T.ULP_CAP):
    if kind == "bits":
        bad = 0 if T.bits_equal(got, ref) else int(((got.view(np.uint32) != ref.view(np.uint32)) & ~(np.isnan(got) & np.isnan(ref))).sum())
        assert bad == 0, (label, bad)
        return
    with np.errstate(all="ignore"):
        normal = np.isfinite(ref) & (np.abs(ref) >= 2.0 ** -126) & (np.abs(ref) <= 3.4028234e38)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), label + ": NaN pattern"
        over = np.isfinite(ref) & (np.abs(ref) > 3.4028236e38) | np.isinf(ref)
        assert (got[over] == np.sign(ref[over]) * np.inf).all(), label + ": overflow"
        tiny = np.isfinite(ref) & (np.abs(ref) < 2.0 ** -126)
        assert (np.abs(got[tiny]) <= 2.0 ** -126).all(), label + ": underflow"
    u = float(T.ulps32(got[normal], ref[normal]).max(initial=0.0))
    ulp_figs.append(u)
    assert u <= limit, (label, u, limit)


@pytest.mark.parametrize("op", range(len(T.EW_UNARY)), ids=T.EW_UNARY)
def test_ew_unary(op):
    L, lib = _lib()
    name = T.EW_UNARY[op]
    a, b = (F32(2.5), F32(1.1)) if name == "GAMMA" else (T.EW_A, T.EW_B)
    ulps, gam = [], 0.0
    configs = EW_CONFIGS + ([("second lap", EW_LAP_N, 0, 1, 1, "float4+tail")] if name in ("AFFINE", "EXP") else []) + \
        [("in place", 1027, 0, 1, 1, "float4+tail")]
    for cname, n, off, is_, os_, want in configs:
        if name == "GAMMA":
            x = (np.random.RandomState(n).rand(n) * a).astype(F32)        # x / a in [0, 1]
            if n >= 4:
                x[:4] = [0.0, a, -1.0, -0.5]                              # 0^b = 0, 1^b = 1, negative bases: NaN
        else:
            x = T.ew_operand(n, n)
        assert EW_ROUTE(n, off % 4 == 0, is_ == 1 and os_ == 1) == want
        src = np.full(n * is_, np.nan, F32)
        src[::is_] = x
        kind, ref = T.ew_unary_ref(op, x, a, b)
        if cname == "in place":
            out = _Out(n, init=src)
            rc = lib.bfm_ew_unary(op, out.ptr(), 1, out.ptr(), 1, n, a, b, L.stream_ptr())
        else:
            out = _Out(n * os_, off)
            dsrc = _in(src, off)
            rc = lib.bfm_ew_unary(op, L.ptr(dsrc), is_, out.ptr(), os_, n, a, b, L.stream_ptr())
        assert rc == 0
        got = out.get(name + " " + cname)
        if os_ > 1:
            gaps = np.ones(n * os_, bool)
            gaps[::os_] = False
            assert _unwritten(got[gaps]).all(), "wrote into the gaps of a strided output"
            got = got[::os_]
        if kind == "gamma":
            ok = ~np.isnan(ref)
            assert np.array_equal(np.isnan(got), ~ok)
            gam = max(gam, float(np.abs(got[ok] - ref[ok]).max(initial=0.0) / np.abs(ref[ok]).max()))
            assert gam <= 2e-6
        else:
            _ew_compare(name + " " + cname, want, kind, got, ref, ulps, EW_ULP_LIMIT.get(name))
    _report("ew_unary " + name, "float4|float4+tail|scalar", **({"ulp": max(ulps)} if ulps else {"gamma_of_max": gam} if gam else
                                                             {"differing": 0}))


@pytest.mark.parametrize("op", range(len(T.EW_BINARY)), ids=T.EW_BINARY)
def test_ew_binary(op):
    L, lib = _lib()
    name = T.EW_BINARY[op]
    ulps = []
    configs = [(c[0], c[1], c[2], c[3], 1, c[4], c[5]) for c in EW_CONFIGS] + \
        [("broadcast ys 0", 1027, 0, 1, 0, 1, "scalar"), ("in place", 1027, 0, 1, 1, 1, "float4+tail")] + \
        ([("second lap", EW_LAP_N, 0, 1, 1, 1, "float4+tail")] if name == "ADD" else [])
    for cname, n, off, xs, ys, os_, want in configs:
        p = T.ew_operand(n, n)
        q = T.ew_operand(n, n + 1)[::-1].copy() if ys else np.array([0.625], F32)
        assert EW_ROUTE(n, off % 4 == 0, xs == 1 and ys == 1 and os_ == 1) == want
        src = np.full(n * xs, np.nan, F32)
        src[::xs] = p
        kind, ref = T.ew_binary_ref(op, p, q if ys else np.full(n, q[0], F32))
        dq = _in(q, off if ys else 0)
        if cname == "in place":
            out = _Out(n, init=src)
            rc = lib.bfm_ew_binary(op, out.ptr(), 1, L.ptr(dq), 1, out.ptr(), 1, n, T.EW_A, L.stream_ptr())
        else:
            out = _Out(n * os_, off)
            dsrc = _in(src, off)
            rc = lib.bfm_ew_binary(op, L.ptr(dsrc), xs, L.ptr(dq), ys, out.ptr(), os_, n, T.EW_A, L.stream_ptr())
        assert rc == 0
        got = out.get(name + " " + cname)
        if os_ > 1:
            gaps = np.ones(n * os_, bool)
            gaps[::os_] = False
            assert _unwritten(got[gaps]).all(), "wrote into the gaps of a strided output"
            got = got[::os_]
        _ew_compare(name + " " + cname, want, kind, got, ref, ulps, EW_ULP_LIMIT.get(name))
    _report("ew_binary " + name, "float4|float4+tail|scalar", **({"ulp": max(ulps)} if ulps else {"differing": 0}))


def test_ew_refusals():
    L, lib = _lib()
    out = _Out(64)
    dx = _in(np.zeros(64, F32))
    S = L.stream_ptr()
    assert lib.bfm_ew_unary(0, L.ptr(dx), 0, out.ptr(), 1, 64, 0.0, 0.0, S) == E_ARG
    assert lib.bfm_ew_unary(0, L.ptr(dx), 1, out.ptr(), 0, 64, 0.0, 0.0, S) == E_ARG
    assert lib.bfm_ew_unary(0, None, 1, out.ptr(), 1, 64, 0.0, 0.0, S) == E_ARG
    assert lib.bfm_ew_unary(0, L.ptr(dx), 1, out.ptr(), 1, 0, 0.0, 0.0, S) == E_ARG
    assert lib.bfm_ew_binary(0, L.ptr(dx), 1, L.ptr(dx), -1, out.ptr(), 1, 64, 0.0, S) == E_ARG
    assert lib.bfm_ew_binary(0, L.ptr(dx), 1, None, 1, out.ptr(), 1, 64, 0.0, S) == E_ARG
    assert lib.bfm_softmax_cl(L.ptr(dx), 3, 4, out.ptr(), 4, 8, S) == E_ARG
    assert lib.bfm_argmax_lut_cl(L.ptr(dx), 3, 4, None, out.ptr(), 8, S) == E_ARG
    assert lib.bfm_fake_cortical(L.ptr(dx), 4, 3, out.ptr(), 8, S) == E_ARG
    assert lib.bfm_fake_cortical(L.ptr(dx), 1, 2, out.ptr(), 8, S) == E_ARG
    out.untouched("ew refusals")


# ------------------------------------------------------------------------------------------------------------ softmax / argmax / fake
@pytest.mark.parametrize("Cc", [1, 2, 18, 56])
def test_softmax_cl(Cc):
    """Row strides larger than C on both sides (a channel slice read in place), all-equal rows and -inf members, more than
    one block; against float64 under tail_refs.softmax_bound(arg_roundings=1)."""
    L, lib = _lib()
    n, xrs, yrs = 700, Cc + 5, Cc + 2
    rs = np.random.RandomState(Cc)
    z = (rs.randn(n, Cc) * 6).astype(F32)
    z[0] = 3.25
    z[1] = -80.0
    if Cc > 1:
        z[2, 0] = -np.inf
        z[3, 1:] = -np.inf
        z[4] = np.linspace(-80, 80, Cc)
    src = np.full((n, xrs), np.nan, F32)
    src[:, 3:3 + Cc] = z
    dsrc = _in(src)
    out = _Out(n * yrs)
    rc = lib.bfm_softmax_cl(dsrc.data_ptr() + 12, xrs, Cc, out.ptr() + 4, yrs, n - 1, L.stream_ptr())
    assert rc == 0
    got = out.get("softmax_cl", shape=(n, yrs)).reshape(-1)[1:1 + (n - 1) * yrs].reshape(n - 1, yrs)
    assert _unwritten(got[:, Cc:]).all(), "wrote between the rows"
    ratio = T._ratio(np.abs(got[:, :Cc].astype(F64) - T.softmax64(z[:n - 1])), T.softmax_bound(z[:n - 1], 1))
    _report("softmax_cl C%d" % Cc, "strided", softmax=ratio)
    assert ratio <= 1.0
    assert (got[0, :Cc] == got[0, 0]).all() and abs(got[0, 0] * Cc - 1) < 1e-6


def test_argmax_lut_cl():
    """First maximum wins; with and without a LUT; a strided slice; rows holding a NaN as the header documents (a NaN is
    never greater, so it wins only from column 0; all-NaN rows give 0)."""
    L, lib = _lib()
    n, Cc, prs = 600, 7, 11
    rs = np.random.RandomState(8)
    p = rs.randint(0, 4, (n, Cc)).astype(F32)               # many ties
    p[0] = 1.0
    p[1] = np.nan
    p[2] = [0.5, np.nan, 1.0, 0.0, 1.0, np.nan, 0.2]
    p[3] = [np.nan, 0.5, 1.0, 0.0, 1.0, 2.0, 0.2]
    p[4] = [-np.inf] * Cc
    p[5] = [0.0, -0.0, 0.0, -0.0, 0.0, 0.0, 0.0]
    p[6, Cc - 1] = np.inf
    src = np.full((n, prs), np.nan, F32)
    src[:, 2:2 + Cc] = p
    src[:, 2 + Cc] = 99.0                                   # a larger value just past the slice
    dsrc = _in(src)
    lut = np.array([40, 3, 17, 0, 250, 9, 11], np.int32)
    dlut = _in(lut)
    for use_lut in (False, True):
        out = _Out(2 * n)
        rc = lib.bfm_argmax_lut_cl(dsrc.data_ptr() + 8, prs, Cc, L.ptr(dlut) if use_lut else None, out.ptr(), n, L.stream_ptr())
        assert rc == 0
        got = out.get("argmax_lut_cl", np.int64)
        want = T.argmax_rule(p, lut if use_lut else None)
        assert np.array_equal(got, want)
        assert list(got[:6]) == ([40, 40, 17, 40, 40, 40] if use_lut else [0, 0, 2, 0, 0, 0])
    clean = ~np.isnan(p).any(1)
    assert np.array_equal(T.argmax_rule(p)[clean], torch.argmax(torch.from_numpy(p[clean]), 1).numpy())
    print("argmax_lut_cl [route strided]: 0 of %d rows differ, with and without LUT" % n)


@pytest.mark.parametrize("nd", [2, 4])
def test_fake_cortical(nd):
    L, lib = _lib()
    n, rs_ = 700, nd + 3
    rs = np.random.RandomState(nd)
    d = (rs.rand(n, nd) * 6 - 3).astype(F32)
    d[0] = 3.0
    d[1] = -3.0
    d[2] = 0.0
    d[3] = -0.3
    src = np.full((n, rs_), np.nan, F32)
    src[:, 1:1 + nd] = d
    out, dsrc = _Out(n), _in(src)
    rc = lib.bfm_fake_cortical(dsrc.data_ptr() + 4, rs_, nd, out.ptr(), n, L.stream_ptr())
    assert rc == 0
    got = out.get("fake_cortical")
    ratio = T._ratio(np.abs(got.astype(F64) - T.fake_cortical64(d)), T.fake_bound(d, tanh_ulps=TANHF_ULPS))
    _report("fake_cortical nd%d" % nd, "strided", fake=ratio)
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------ bias_lrelu
@pytest.mark.parametrize("Cc,nvox", [(4, 257), (12, 257), (20, 1031), (64, 130), (12, 350001)])
def test_head_bias_lrelu(Cc, nvox):
    """Bit for bit against numpy fp32 (one add, one select, one multiply); bound_out = max |y| of what was stored.
    C = 12, nvox = 350 001: 1 050 003 float4 columns against a grid of 4096 x 256, so a second lap whose column walk
    wraps (q = 3 does not divide the stride).  A mask with zeros: those voxels keep their bits and stay out of the bound."""
    L, lib = _lib()
    rs = np.random.RandomState(Cc)
    y = rs.randn(nvox, Cc).astype(F32)
    y[:, 0] *= 5
    bias = rs.randn(Cc).astype(F32)
    mask = (rs.rand(nvox) > 0.3).astype(F32) * F32(0.5)
    y[np.argmax(mask == 0)] = 1e6                           # the largest value sits at a masked-out voxel
    dbias, dmask = _in(bias), _in(mask)
    for use_mask, use_bound in ((False, True), (True, True), (True, False)):
        out = _Out(nvox * Cc, init=y)
        bound = _Out(4)
        rc = lib.bfm_head_bias_lrelu(out.ptr(), L.ptr(dbias), Cc, nvox, 0.2, L.ptr(dmask) if use_mask else None,
                                     bound.ptr() if use_bound else None, L.stream_ptr())
        assert rc == 0
        ref, bref = T.bias_lrelu_ref(y, bias, 0.2, mask if use_mask else None)
        got = out.get("head_bias_lrelu", shape=(nvox, Cc))
        assert T.bits_equal(got, ref), int((got.view(np.uint32) != ref.view(np.uint32)).sum())
        bw = bound.get("bound_out")
        if use_bound:
            assert bw[0] == bref and _unwritten(bw[1:]).all()
        else:
            assert _unwritten(bw).all()
    laps = -(-nvox * (Cc // 4) // (4096 * 256))
    print("head_bias_lrelu C%d n%d [route laps %d, column step %d]: 0 elements differ" % (Cc, nvox, laps, (4096 * 256) % (Cc // 4) if laps > 1 else 0))


def test_zz_summary():
    """The worst figure per kernel and route over the module (run last: the table of the docstring)."""
    for (kernel, route, fig), v in sorted(WORST.items(), key=str):
        print("worst %-12s route %-28s %-10s %.3g" % (kernel, route, fig, v))
