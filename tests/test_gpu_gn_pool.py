"""The GroupNorm statistics kernels (brainfm_amd/csrc/gn_stats.hip: bfm_gn_stats, _train, _batch, _rows, _rows_train,
_rows_sliced, _rows_batch) and the pooling half of csrc/pool_stitch.hip (bfm_maxpool2, _ex, _batch and their row counters)
on their own, through the C ABI, route by route, against the float64 / longdouble references and the derived bounds of
tests/gn_pool_refs.py (the derivations stand in its docstring; tests/test_host_gn_pool_refs.py pins them to torch and
shows that each named mistake fails them).  No flat tolerance: statistics are held to the derived bounds (the bar of every
ratio below is 1), `bound` and every "equal" is bit for bit.

Conventions: every output starts as NaN between a front guard and a sentinel tail that must come back untouched; inputs
sit between NaN guard bands; the workspace is exactly the advertised size plus a guard band that is checked afterwards.  The
route a case is meant to take is asked of the library (bfm_gn_stats_plan, bfm_gn_stats_rows_route) and asserted.

Where the issue's shapes were adjusted: 5x6x7 (210 voxels) splits into 14 blocks of 15 for every C here, so the short last
block is taken at 5x7x7 (16 blocks of 16, the last of 5: R.SHORT); 5x6x7 stays in the list of extents.

A group that holds an Inf or a NaN: its scale and shift are NaN (as nn.GroupNorm's output is), the other groups are untouched,
and its bound is 0 -- fmaxf drops the NaN (pinned in test_gn_nonfinite_stays_in_its_group; include/brainfm_hip.h says so).

Measured on MI355X (also in HISTORY.md): 139 cases, module 4.1 s to 6.7 s (slowest case 0.6 s), no kernel defect.
  worst ratio to the derived bound (bar 1; values near 0.9 are the last fp32 rounding, whose bound is exact)
                                   mean    rstd    scale   shift   bound (also bit for bit as coded)
    tensor pass, float4 rows       0.942   0.767   0.774   0.845   0.616
    tensor pass, scalar rows       0.828   0.801   0.634   0.749   0.379
    tensor pass, wide float4       0.638   0.742   0.858   0.763   0.470
    tensor pass, wide scalar       0.835   0.644   0.759   0.845   0.320
    tensor pass, non-finite        0.704   0.737   0.637   0.488   0.498
    virtual concat                 0.970   0.959   0.950   0.933   0.455
    batch                          -       -       0.806   0.729   0.452
    rows batch                     -       -       0.839   0.618   0.466
    rows sliced                    -       -       0.676   0.641   0.417
    rows direct                    0.917   0.947   0.822   0.731   0.393
    rows fold and rows one launch  0.879   0.982   0.877   0.827   0.713
    chain, rows as given           0.802   0.898   0.792   0.592   0.221
    pool rows against longdouble sums: S 0.157, Q 0.727
  offset field mean/std = 1e3 at 16^3 x 8: rstd error 2.38e-08 (G = 1, bound 1.87e-06), 3.51e-08 (G = 4, bound 5.16e-07)
  chain (rstd relative error: rows route / tensor route / torch fp32 group_norm on the CPU; the rows route's bound):
    randn    (mean/std 2.7)   3.03e-08 / 3.03e-08 / 8.56e-08;  3.06e-07
    offset30 (mean/std 51.7)  6.76e-07 / 3.59e-08 / 1.01e-07;  7.98e-05
    decoder  (mean/std 2.72)  5.41e-08 / 5.31e-08 / 6.41e-08;  3.10e-07
  bit-for-bit checks: 1165, differing elements: 0 (bound, scale / shift from mean_out / rstd_out, batch against single,
  sliced against a copy, tickets against none, three one-launch calls, pooled values, the pool's rows against the emulation).
Needs an MI355X: run with `-m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import gn_pool_refs as R

pytestmark = pytest.mark.gpu

F32, F64, LD = np.float32, np.float64, np.longdouble
GUARD = 256                      # words in front of every buffer (a multiple of 64: alignment is kept)
TAIL = 1024
NAN_BITS = 0x7FC00000
SENT = -7777
WS_GUARD = 4096
E_ARG, E_SHAPE, E_WS = -1, -2, -3
EPS = R.EPS
WORST = {}
DIFFS = {"checks": 0, "elements": 0}


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _lib():
    from brainfm_amd import _lib as L
    return L, L.load()


def _sync():
    """A HIP error ends the module: nothing more is launched on a device that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("HIP error, stopping: %s" % e, returncode=3)


def _in(a, offset=0):
    """A device copy of a 4-byte array between NaN guard bands, `offset` words off the 16-byte alignment."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    n = a.size
    flat = torch.full((GUARD + offset + n + GUARD,), NAN_BITS, dtype=torch.int32, device=_dev())
    v = flat[GUARD + offset:GUARD + offset + n]
    v.copy_(torch.from_numpy(a.reshape(-1).view(np.int32).copy()))
    assert v.data_ptr() % 16 == 4 * (offset % 4)
    return v


def _raw(b):
    """Device copy of bytes (a moment-row table), 256-byte aligned, NaN guard bands around it."""
    b = np.frombuffer(b, np.uint8)
    flat = torch.full((1024 + b.size + 1024,), 0xFF, dtype=torch.uint8, device=_dev())
    v = flat[1024:1024 + b.size]
    v.copy_(torch.from_numpy(b.copy()))
    assert v.data_ptr() % 256 == 0
    return v


class _Out:
    """n words of NaN, `offset` words off alignment, a guard in front and a sentinel tail behind."""

    def __init__(self, n, offset=0):
        self.n, self.lo = n, GUARD + offset
        self.flat = torch.full((self.lo + n + TAIL,), SENT, dtype=torch.int32, device=_dev())
        self.view = self.flat[self.lo:self.lo + n]
        self.view.fill_(NAN_BITS)

    def ptr(self):
        return self.view.data_ptr()

    def get(self, label, shape=None):
        _sync()
        h = self.flat.cpu().numpy()
        assert (h[:self.lo] == SENT).all(), label + ": wrote in front of the output"
        assert (h[self.lo + self.n:] == SENT).all(), label + ": wrote behind the output"
        out = h[self.lo:self.lo + self.n].view(F32)
        return out.reshape(shape) if shape is not None else out

    def untouched(self, label):
        assert (self.get(label).view(np.int32) == NAN_BITS).all(), label + ": written by a refused call"


class _Bytes:
    """n bytes of 0xFF (NaN in every float format) plus a guard band: row tables written by the pool, workspaces."""

    def __init__(self, n, fill=0xFF):
        self.n, self.fill = n, fill
        self.flat = torch.full((n + WS_GUARD,), fill, dtype=torch.uint8, device=_dev())
        self.flat[n:].fill_(0xA5)

    def ptr(self):
        return self.flat.data_ptr()

    def get(self, label):
        _sync()
        h = self.flat.cpu().numpy()
        assert (h[self.n:] == 0xA5).all(), label + ": wrote past its advertised size"
        return h[:self.n]

    def untouched(self, label):
        assert (self.get(label) == self.fill).all(), label + ": written by a refused call"


def _same(label, a, b):
    """Bit for bit; the count of differing elements goes into the module's report."""
    d = R.n_diff(a, b)
    DIFFS["checks"] += 1
    DIFFS["elements"] += d
    assert d == 0, "%s: %d of %d elements differ" % (label, d, np.asarray(a).size)


def _note(family, ratios):
    for k, v in ratios.items():
        WORST[(family, k)] = max(WORST.get((family, k), 0.0), v)
    worst = max(ratios.values()) if ratios else 0.0
    print("\n%s: %s" % (family, "  ".join("%s %.3g" % kv for kv in ratios.items())), end="")
    assert worst <= 1.0, (family, ratios)


def _plan(C_, nvox, aligned):
    _, lib = _lib()
    r, nb, vpb, rp = C.c_int(), C.c_int(), C.c_int64(), C.c_int()
    assert lib.bfm_gn_stats_plan(C_, nvox, 1 if aligned else 0, C.byref(r), C.byref(nb), C.byref(vpb), C.byref(rp)) == 0
    return r.value, nb.value, vpb.value, rp.value


class _Up:
    """bfm_upsample_t of lo -> hi with its six tables on the device."""

    def __init__(self, lo, hi):
        L, _ = _lib()
        self.maps = R.up_maps(lo, hi)
        self.reps = R.rep_counts(self.maps, lo)
        self.dev = [_in(m.astype(np.int32)) for m in self.maps] + [_in(r) for r in self.reps]
        self.desc = L.Upsample(lo[0], lo[1], lo[2], *[t.data_ptr() for t in self.dev])


def _gn(A, B, lo, gamma, beta, G, offA=0, offB=0, train=True, S=0, eps=EPS):
    """bfm_gn_stats_train / bfm_gn_stats (train=False) / bfm_gn_stats_batch (S >= 1: A and B carry a leading sample axis).
    Returns dict(scale, shift, bound, mean, rstd) and asserts the guards, the sentinels and the workspace band."""
    L, lib = _lib()
    batch = S >= 1
    s = max(S, 1)
    hi = A.shape[1:4] if batch else A.shape[:3]
    CA, CB = A.shape[-1], (B.shape[-1] if B is not None else 0)
    Ct = CA + CB
    dA, dB = _in(A, offA), (_in(B, offB) if B is not None else None)
    up = _Up(lo, hi) if B is not None else None
    upp = C.byref(up.desc) if up else None
    dg, db = _in(gamma), _in(beta)
    osc, osh, obd = _Out(s * Ct, 1), _Out(s * Ct, 3), _Out(s * G, 2)
    omn, ors = _Out(G, 1), _Out(G, 3)
    if batch:
        need = lib.bfm_gn_stats_batch_workspace(CA, CB, S, hi[0], hi[1], hi[2], upp)
    else:
        need = lib.bfm_gn_stats_workspace(CA, CB, hi[0], hi[1], hi[2], upp)
    ws = _Bytes(need)
    st = L.stream_ptr()
    pB = L.ptr(dB)
    if batch:
        rc = lib.bfm_gn_stats_batch(L.ptr(dA), CA, pB, CB, S, hi[0], hi[1], hi[2], upp, L.ptr(dg), L.ptr(db), G, eps,
                                    osc.ptr(), osh.ptr(), obd.ptr(), ws.ptr(), need, st)
    elif train:
        rc = lib.bfm_gn_stats_train(L.ptr(dA), CA, pB, CB, hi[0], hi[1], hi[2], upp, L.ptr(dg), L.ptr(db), G, eps,
                                    osc.ptr(), osh.ptr(), obd.ptr(), omn.ptr(), ors.ptr(), ws.ptr(), need, st)
    else:
        rc = lib.bfm_gn_stats(L.ptr(dA), CA, pB, CB, hi[0], hi[1], hi[2], upp, L.ptr(dg), L.ptr(db), G, eps,
                              osc.ptr(), osh.ptr(), obd.ptr(), ws.ptr(), need, st)
    assert rc == 0, L.ERR.get(rc, rc)
    ws.get("workspace")
    shp = (lambda n: (S, n)) if batch else (lambda n: (n,))
    res = dict(scale=osc.get("scale", shp(Ct)), shift=osh.get("shift", shp(Ct)), bound=obd.get("bound", shp(G)))
    if train and not batch:
        res["mean"], res["rstd"] = omn.get("mean_out"), ors.get("rstd_out")
    else:
        omn.untouched("mean_out")
        ors.untouched("rstd_out")
    return res


def _check_stats(family, res, truth, mn, mx, gamma, beta, G):
    """The derived bounds; bound bit for bit from the kernel's own scale and shift; mean / rstd the fp32 values that
    scale and shift imply."""
    _note(family, R.gn_ratios(truth, res["scale"], res["shift"], res.get("mean"), res.get("rstd"), bound=res["bound"]))
    assert not np.isnan(res["bound"]).any()
    _same(family + " bound", res["bound"], R.gn_bound_as_coded(res["scale"], res["shift"], mn, mx, G))
    if "mean" in res:
        sc, sh = R.affine_as_coded(res["mean"], res["rstd"], gamma, beta, G)
        _same(family + " scale from rstd_out", res["scale"], sc)
        _same(family + " shift from mean_out", res["shift"], sh)


# ---------------------------------------------------------------------------------------- A. tensor pass, one source
@pytest.mark.parametrize("case", R.GN_TENSOR_CASES, ids=lambda c: "C%d-%s-G%d-%s%s" % (c[0], "x".join(map(str, c[1])), c[2], c[4],
                                                                                      "-misaligned" if c[3] else ""))
def test_gn_stats_tensor_pass(case):
    Cc, dims, G, off, kind, want = case
    nvox = int(np.prod(dims))
    route, nb, vpb, rp = _plan(Cc, nvox, not off)
    assert route == want, "this case means route %d, the launcher takes %d" % (want, route)
    if (Cc, dims) in R.GN_UNROLLED:
        assert vpb > 3 * rp and vpb % (4 * rp) != 0              # the unrolled loop and its tail both run
    if dims == R.SHORT:
        assert nb > 1 and nvox % vpb != 0                        # a short last block
    cv = Cc // 4 if route in (R.ROUTE_ROWS_VEC4, R.ROUTE_WIDE_VEC4) else Cc
    if Cc in (12, 192) and not off:
        assert rp * cv < 256                                     # idle threads
    if Cc == 1024 and not off:
        assert rp == 1
    if Cc == 1028:
        assert cv == 257 and rp == 0                             # a second column lap with one live column
    if Cc == 1024 and off:
        assert cv == 4 * 256 and rp == 0                         # four column laps
    A, gamma, beta = R.tensor_inputs(case)
    truth = R.gn_truth(A, None, None, gamma, beta, G)
    mn, mx = R.extremes_as_coded(A)
    res = _gn(A, None, None, gamma, beta, G, offA=off)
    _check_stats("tensor pass route %d" % route, res, truth, mn, mx, gamma, beta, G)
    plain = _gn(A, None, None, gamma, beta, G, offA=off, train=False)
    for k in ("scale", "shift", "bound"):
        _same("bfm_gn_stats against _train " + k, plain[k], res[k])
    if kind == "const":
        assert (truth["var"] == 0).all()
        _same("rstd of a constant", res["rstd"], np.full(G, 1.0 / np.sqrt(F64(F32(EPS))), F64).astype(F32))
    if kind == "offset1e3":
        rel = float(np.max(np.abs(res["rstd"].astype(F64) - truth["rstd"]) / truth["rstd"]))
        print("  offset field mean/std = 1e3: rstd error %.3g (bound %.3g)" % (rel, float(np.max(truth["drstd"] / truth["rstd"]))),
              end="")
        WORST[("offset1e3 rstd rel", "G%d" % G)] = rel


@pytest.mark.parametrize("case", R.GN_NONFINITE_CASES, ids=str)
def test_gn_nonfinite_stays_in_its_group(case):
    Cc, dims, G, kind = case
    A, gamma, beta = R.tensor_inputs(case)
    g_bad = (Cc // 2) // (Cc // G)
    truth = R.gn_truth(A, None, None, gamma, beta, G)
    res = _gn(A, None, None, gamma, beta, G)
    cpg = Cc // G
    bad = np.zeros(Cc, bool)
    bad[g_bad * cpg:(g_bad + 1) * cpg] = True
    assert np.isnan(res["scale"][bad]).all() and np.isnan(res["shift"][bad]).all() and np.isnan(res["rstd"][g_bad])
    assert np.isfinite(res["scale"][~bad]).all() and np.isfinite(res["shift"][~bad]).all()
    assert np.isnan(truth["scale"][bad]).all() and np.isfinite(truth["scale"][~bad]).all()
    assert np.isfinite(res["mean"][g_bad]) == np.isfinite(truth["mean"][g_bad])
    _check_stats("tensor pass, non-finite", res, truth, *R.extremes_as_coded(A), gamma, beta, G)
    assert res["bound"][g_bad] == 0.0 and (np.delete(res["bound"], g_bad) > 0).all()      # pinned: fmaxf drops the NaN
    # the other groups are what they are without the planted value
    clean = A.copy()
    clean.reshape(-1, Cc)[clean.reshape(-1, Cc).shape[0] // 2, Cc // 2] = 1.0
    ref = _gn(clean, None, None, gamma, beta, G)
    for k in ("scale", "shift"):
        _same("other groups " + k, res[k][~bad], ref[k][~bad])
    _same("other groups bound", np.delete(res["bound"], g_bad), np.delete(ref["bound"], g_bad))


# ------------------------------------------------------------------------------- B. the virtual concatenation, tensor pass
@pytest.mark.parametrize("up, ch", [(u, c) for u in R.UPSAMPLES for c in R.GN_CAT_CHANNELS] +
                         [(R.GN_CAT_UNROLLED[:2], R.GN_CAT_UNROLLED[2:])], ids=str)
def test_gn_stats_virtual_concat(up, ch):
    lo, hi = up
    CA, CB, G = ch
    if (lo, hi, CA, CB, G) == R.GN_CAT_UNROLLED:
        r_, _, vpb, rp = _plan(CB, int(np.prod(lo)), True)
        assert r_ == R.ROUTE_ROWS_VEC4 and vpb > 3 * rp and vpb % (4 * rp) != 0      # four replication weights per pass
    A, B, gamma, beta = R.cat_inputs(lo, hi, CA, CB, G)
    upv = R.up_maps(lo, hi)
    ra = _plan(CA, int(np.prod(hi)), True)[0]
    rb = _plan(CB, int(np.prod(lo)), True)[0]
    if ch == (3, 5, 8):
        assert (ra, rb) == (R.ROUTE_ROWS_SCALAR, R.ROUTE_ROWS_SCALAR)
    if ch == (4, 2052, 8):
        assert (ra, rb) == (R.ROUTE_ROWS_VEC4, R.ROUTE_WIDE_VEC4)
    truth = R.gn_truth(A, B, upv, gamma, beta, G)
    res = _gn(A, B, lo, gamma, beta, G)
    _check_stats("virtual concat", res, truth, *R.extremes_as_coded(A, B), gamma, beta, G)


# ---------------------------------------------------------------------------------------------------- C. the batch form
@pytest.mark.parametrize("case", R.GN_BATCH_CASES, ids=str)
def test_gn_stats_batch_is_each_sample_alone(case):
    S, CA, CB, G = case
    lo, hi = R.UPSAMPLES[1]
    As, Bs = [], []
    for s in range(S):
        A, B, gamma, beta = R.cat_inputs(lo, hi, CA, max(CB, 4), G)
        A = (A + F32(0.25 * s)).astype(F32)
        if s == 1:
            A[...] = F32(0.75)                                   # one sample is constant
        As.append(A)
        Bs.append((B * F32(1 + s)).astype(F32))
    gamma, beta = R.affine(CA + CB, "batch", G)
    A = np.stack(As)
    B = np.stack(Bs) if CB else None
    res = _gn(A, B, lo, gamma, beta, G, S=S)
    for s in range(S):
        b = B[s] if CB else None
        truth = R.gn_truth(A[s], b, R.up_maps(lo, hi) if CB else None, gamma, beta, G)
        one = {k: v[s] for k, v in res.items()}
        _check_stats("batch", one, truth, *R.extremes_as_coded(A[s], b), gamma, beta, G)
        alone = _gn(A[s], b, lo, gamma, beta, G, train=False)
        for k in ("scale", "shift", "bound"):
            _same("sample %d of the batch against the one-sample call, %s" % (s, k), one[k], alone[k])


# ------------------------------------------------------------------------------------------------- D. the rows family
def _rows_call(form, tA, nA, CA, tB, nB, CB, wB, nvox, gamma, beta, G, ticket=None, slices=None, S=1, ws_bytes=None):
    """form: 'train' | 'plain' | 'sliced' (slices = (totalA, firstA, totalB, firstB)) | 'batch'.  tA / tB: device bytes."""
    L, lib = _lib()
    Ct = CA + CB
    dg, db = [v if v is None or isinstance(v, torch.Tensor) else _in(v) for v in (gamma, beta)]
    osc, osh, obd = _Out(max(S * Ct, 1), 1), _Out(max(S * Ct, 1), 3), _Out(max(S * G, 1), 2)      # never a null pointer of ours
    omn, ors = _Out(max(G, 1), 1), _Out(max(G, 1), 3)
    need = lib.bfm_gn_stats_rows_workspace(nA, CA, nB, CB) if ws_bytes is None else ws_bytes
    ws = _Bytes(need)
    st = L.stream_ptr()
    pa, pb, tk = L.ptr(tA), (L.ptr(tB) if CB else None), (L.ptr(ticket) if ticket is not None else None)
    if form == "train":
        rc = lib.bfm_gn_stats_rows_train(pa, nA, CA, pb, nB, CB, wB, nvox, L.ptr(dg), L.ptr(db), G, EPS, osc.ptr(), osh.ptr(),
                                         obd.ptr(), omn.ptr(), ors.ptr(), ws.ptr(), need, tk, st)
    elif form == "plain":
        rc = lib.bfm_gn_stats_rows(pa, nA, CA, pb, nB, CB, wB, nvox, L.ptr(dg), L.ptr(db), G, EPS, osc.ptr(), osh.ptr(), obd.ptr(),
                                   ws.ptr(), need, tk, st)
    elif form == "sliced":
        rc = lib.bfm_gn_stats_rows_sliced(pa, slices[0], slices[1], nA, CA, pb, slices[2], slices[3], nB, CB, wB, nvox, L.ptr(dg),
                                          L.ptr(db), G, EPS, osc.ptr(), osh.ptr(), obd.ptr(), ws.ptr(), need, tk, st)
    else:
        rc = lib.bfm_gn_stats_rows_batch(pa, nA, CA, pb, nB, CB, wB, nvox, S, L.ptr(dg), L.ptr(db), G, EPS, osc.ptr(), osh.ptr(),
                                         obd.ptr(), st)
    if rc != 0:
        return rc, (osc, osh, obd, omn, ors, ws)
    ws.get("rows workspace")
    shp = (lambda n: (S, n)) if form == "batch" else (lambda n: (n,))
    res = dict(scale=osc.get("scale", shp(Ct)), shift=osh.get("shift", shp(Ct)), bound=obd.get("bound", shp(G)))
    if form == "train":
        res["mean"], res["rstd"] = omn.get("mean_out"), ors.get("rstd_out")
    else:
        omn.untouched("mean_out")
        ors.untouched("rstd_out")
    return 0, res


@pytest.mark.parametrize("case", R.GN_ROWS_CASES, ids=str)
def test_gn_stats_rows_every_route(case):
    _, lib = _lib()
    nA, CA, nB, CB, G, wB, r0, r1 = case
    assert lib.bfm_gn_stats_rows_route(nA, CA, nB, CB, G, 0) == r0, "ticket-less route"
    assert lib.bfm_gn_stats_rows_route(nA, CA, nB, CB, G, 1) == r1, "route with tickets"
    tA, tB, gamma, beta, nvox = R.rows_inputs(case)
    truth = R.rows_truth(tA, tB, wB, nvox, gamma, beta, G)
    dA, dB = _raw(R.table_bytes(tA)), (_raw(R.table_bytes(tB)) if CB else None)
    fam = ("rows direct", "rows fold", "rows one launch")
    rc, ref = _rows_call("train", dA, nA, CA, dB, nB, CB, wB, nvox, gamma, beta, G)
    assert rc == 0
    _check_stats(fam[r0], ref, truth, truth["chan_min"], truth["chan_max"], gamma, beta, G)
    rc, plain = _rows_call("plain", dA, nA, CA, dB, nB, CB, wB, nvox, gamma, beta, G)
    assert rc == 0
    for k in ("scale", "shift", "bound"):
        _same("bfm_gn_stats_rows against _train " + k, plain[k], ref[k])
    ticket = torch.zeros(R.GN_TICKETS + 16, dtype=torch.int32, device=_dev())
    ticket[R.GN_TICKETS:] = SENT
    first = None
    for rep in range(3 if r1 == R.ROWS_ONE_LAUNCH else 1):
        rc, got = _rows_call("train", dA, nA, CA, dB, nB, CB, wB, nvox, gamma, beta, G, ticket=ticket[:R.GN_TICKETS])
        assert rc == 0
        tk = ticket.cpu().numpy()
        assert (tk[:R.GN_TICKETS] == 0).all() and (tk[R.GN_TICKETS:] == SENT).all(), "tickets after call %d" % rep
        if first is None:
            first = got
            _check_stats(fam[r1], got, truth, truth["chan_min"], truth["chan_max"], gamma, beta, G)
        for k in got:
            _same("one-launch call %d against the first, %s" % (rep, k), got[k], first[k])
    if r1 != R.ROWS_ONE_LAUNCH:                   # tickets given, yet direct or two launches: the ticket-less bits
        for k in first:
            _same("with tickets against without, %s" % k, first[k], ref[k])


@pytest.mark.parametrize("n, CA, CB, G", [(40, 64, 0, 8), (150, 64, 0, 8), (150, 8, 24, 4)])
def test_gn_stats_rows_sliced_is_the_plain_call_on_a_copy(n, CA, CB, G):
    g = np.random.default_rng(R._seed("sliced", n, CA, CB))
    vA = (g.standard_normal((3 * n, CA, R.ROWS_K)) * 2 + 0.3).astype(F32)
    vB = (g.standard_normal((3 * 7, max(CB, 1), R.ROWS_K)) * 1.3 - 0.5).astype(F32)
    fullA, fullB = R.make_table(vA), R.make_table(vB)
    gamma, beta = R.affine(CA + CB, "sliced", G)
    dg, db = _in(gamma), _in(beta)
    dA, dB = _raw(R.table_bytes(fullA)), (_raw(R.table_bytes(fullB)) if CB else None)
    nvox = R.ROWS_K * n
    for which in range(3):
        for tk in (None, torch.zeros(R.GN_TICKETS, dtype=torch.int32, device=_dev())):
            rc, got = _rows_call("sliced", dA, n, CA, dB, 7, CB, 3.7, nvox, dg, db, G, ticket=tk,
                                 slices=(3 * n, which * n, 21, which * 7))
            assert rc == 0
            cA = _raw(R.table_bytes(R.make_table(vA[which * n:(which + 1) * n])))
            cB = _raw(R.table_bytes(R.make_table(vB[which * 7:(which + 1) * 7]))) if CB else None
            rc, want = _rows_call("plain", cA, n, CA, cB, 7, CB, 3.7, nvox, dg, db, G, ticket=tk)
            assert rc == 0
            for k in want:
                _same("slice %d %s" % (which, k), got[k], want[k])
            if tk is not None:
                assert int(tk.abs().sum()) == 0
    tab = {k: v[n:2 * n] for k, v in fullA.items()}
    tb = {k: v[7:14] for k, v in fullB.items()} if CB else None
    truth = R.rows_truth(tab, tb, 3.7, nvox, gamma, beta, G)
    rc, got = _rows_call("sliced", dA, n, CA, dB, 7, CB, 3.7, nvox, dg, db, G, slices=(3 * n, n, 21, 7))
    _check_stats("rows sliced", got, truth, truth["chan_min"], truth["chan_max"], gamma, beta, G)


@pytest.mark.parametrize("n, CA, nB, CB, G", [(128, 64, 0, 0, 8), (5, 8, 128, 24, 4), (1, 3, 2, 5, 8)])
def test_gn_stats_rows_batch_is_three_plain_calls(n, CA, nB, CB, G):
    S = 3
    g = np.random.default_rng(R._seed("rbatch", n, CA, CB))
    vA = (g.standard_normal((S * n, CA, R.ROWS_K)) * 2 + 0.3).astype(F32)
    vB = (g.standard_normal((S * max(nB, 1), max(CB, 1), R.ROWS_K)) * 1.3 - 0.5).astype(F32)
    gamma, beta = R.affine(CA + CB, "rbatch", G)
    dg, db = _in(gamma), _in(beta)
    dA, dB = _raw(R.table_bytes(R.make_table(vA))), (_raw(R.table_bytes(R.make_table(vB))) if CB else None)
    nvox = R.ROWS_K * n
    rc, got = _rows_call("batch", dA, n, CA, dB, nB, CB, 8.0, nvox, dg, db, G, S=S)
    assert rc == 0
    for s in range(S):
        tA = R.make_table(vA[s * n:(s + 1) * n])
        tB = R.make_table(vB[s * nB:(s + 1) * nB]) if CB else None
        rc, want = _rows_call("plain", _raw(R.table_bytes(tA)), n, CA, _raw(R.table_bytes(tB)) if CB else None, nB, CB, 8.0, nvox,
                              dg, db, G)
        assert rc == 0
        for k in want:
            _same("rows batch sample %d %s" % (s, k), got[k][s], want[k])
        truth = R.rows_truth(tA, tB, 8.0, nvox, gamma, beta, G)
        _check_stats("rows batch", {k: v[s] for k, v in got.items()}, truth, truth["chan_min"], truth["chan_max"], gamma, beta, G)


# ----------------------------------------------------------------------------------------------------------- E. pooling
def _pool(x, off_in=0, off_out=0, rows=False, batch=False, form="ex"):
    """bfm_maxpool2 / _ex / _batch on x (D, H, W, C) or (S, D, H, W, C).  Returns (pooled, rows table or None, nrows)."""
    L, lib = _lib()
    S = x.shape[0] if batch else 1
    D, H, W, Cc = x.shape[-4:]
    d, h, w = D // 2, H // 2, W // 2
    dx = _in(x, off_in)
    out = _Out(S * d * h * w * Cc, off_out)
    nr = (lib.bfm_maxpool2_batch_rows if batch else lib.bfm_maxpool2_rows)(Cc, D, H, W) if rows else 0
    tab = _Bytes(lib.bfm_moment_rows_bytes(S * nr, Cc)) if rows else None
    st = L.stream_ptr()
    if batch:
        rc = lib.bfm_maxpool2_batch(L.ptr(dx), Cc, S, D, H, W, out.ptr(), tab.ptr() if rows else None, st)
    elif form == "plain":
        rc = lib.bfm_maxpool2(L.ptr(dx), Cc, D, H, W, out.ptr(), st)
    else:
        rc = lib.bfm_maxpool2_ex(L.ptr(dx), Cc, D, H, W, out.ptr(), tab.ptr() if rows else None, st)
    assert rc == 0, L.ERR.get(rc, rc)
    p = out.get("pooled", (S, d, h, w, Cc) if batch else (d, h, w, Cc))
    return p, (tab.get("moment rows") if rows else None), nr


def _pool_input(Cc, dims, key="pool"):
    """randn with +-Inf, a -0.0 / +0.0 window, a window of eight equal values; NaN in the dropped planes of odd extents."""
    x = R.field("randn", tuple(dims) + (Cc,), key)
    x[0, 0, 0, 0], x[1, 1, 1, 0] = np.inf, 5.0
    x[0, 0, 0, -1] = -np.inf
    if dims[1] >= 4:
        x[:2, 2:4, :2, 0] = [[[-0.0, 0.0], [-0.0, -0.0]], [[-0.0, -0.0], [0.0, -0.0]]]
        x[:2, 2:4, :2, -1] = F32(-1.25)
    for a in range(3):
        if dims[a] % 2:
            x[tuple(slice(None) if i != a else dims[a] - 1 for i in range(3))] = np.nan
    return x


def _pool_equal(label, got, want):
    assert not np.isnan(got).any() or np.isnan(want).any(), label + ": read a dropped plane"
    assert got.shape == want.shape
    zero = want == 0                                   # -0.0 against +0.0: torch keeps the first, fmaxf may keep either
    assert (got[zero] == 0).all(), label
    _same(label, np.where(zero, F32(0), got), np.where(zero, F32(0), want))


@pytest.mark.parametrize("dims", R.POOL_EXTENTS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("Cc", R.POOL_CHANNELS)
def test_maxpool2_is_max_pool3d(Cc, dims):
    x = _pool_input(Cc, dims)
    want = R.pool_truth(x)
    assert np.isfinite(want[np.isfinite(want)]).all() and not np.isnan(want).any()
    p, _, _ = _pool(x)
    _pool_equal("bfm_maxpool2_ex", p, want)
    p, _, _ = _pool(x, form="plain")
    _pool_equal("bfm_maxpool2", p, want)
    if Cc % 4 == 0:
        pb, _, _ = _pool(np.stack([x, x[::-1, ::-1].copy()]), batch=True)
        _pool_equal("bfm_maxpool2_batch sample 0", pb[0], want)
        _pool_equal("bfm_maxpool2_batch sample 1", pb[1], R.pool_truth(x[::-1, ::-1].copy()))


@pytest.mark.parametrize("off_in, off_out", [(1, 0), (0, 1), (3, 2)])
def test_maxpool2_misaligned_pointers_take_the_scalar_lanes(off_in, off_out):
    x = _pool_input(4, (5, 7, 9))
    p, _, _ = _pool(x, off_in, off_out)
    _pool_equal("misaligned", p, R.pool_truth(x))


def test_maxpool2_row_counters_follow_their_rule():
    _, lib = _lib()
    for Cc in R.POOL_NO_ROWS:
        assert lib.bfm_maxpool2_rows(Cc, 8, 8, 8) == 0 and lib.bfm_maxpool2_batch_rows(Cc, 8, 8, 8) == 0
    for Cc in R.POOL_ROWS_CHANNELS:
        for dims in R.POOL_ROWS_EXTENTS + [(20, 20, 20), (82, 82, 82)]:
            n = lib.bfm_maxpool2_rows(Cc, *dims)
            assert n == R.pool_rows(Cc, *dims) > 0
            assert lib.bfm_maxpool2_batch_rows(Cc, *dims) == min(n, 128)
    assert lib.bfm_maxpool2_batch_rows(256, 20, 20, 20) == 128 < lib.bfm_maxpool2_rows(256, 20, 20, 20)


def _check_rows(label, raw, pooled, Cc, nr):
    assert not (raw == 0xFF).reshape(-1, 4).all(1).any(), label + ": a word of the table was left unwritten"
    got = R.table_from_bytes(raw.tobytes(), nr, Cc)
    want = R.pool_rows_as_coded(pooled, Cc, nr)
    for k in ("sum", "sq"):
        d = int((got[k].view(np.int64) != want[k].view(np.int64)).sum())
        DIFFS["checks"] += 1
        DIFFS["elements"] += d
        assert d == 0, "%s %s: %d entries differ from the emulation" % (label, k, d)
    _same(label + " min", got["mn"], want["mn"])
    _same(label + " max", got["mx"], want["mx"])
    S, dS, Q, dQ, j = R.pool_row_bounds(pooled, Cc, nr)
    with np.errstate(all="ignore"):
        rs = np.abs(got["sum"].astype(LD).sum(0) - S) / dS
        rq = np.abs(got["sq"].astype(LD).sum(0) - Q) / dQ
    _note("pool rows", dict(S=float(np.nanmax(rs)), Q=float(np.nanmax(rq))))
    flat = np.asarray(pooled, F32).reshape(-1, Cc)
    _same(label + " total min", got["mn"].min(0), flat.min(0))
    _same(label + " total max", got["mx"].max(0), flat.max(0))
    return got, j


@pytest.mark.parametrize("dims", R.POOL_ROWS_EXTENTS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("Cc", R.POOL_ROWS_CHANNELS)
def test_maxpool2_rows_are_the_emulation_bit_for_bit(Cc, dims):
    x = R.field("offset30" if Cc == 16 else "randn", tuple(dims) + (Cc,), "prow")
    want = R.pool_truth(x)
    p, raw, nr = _pool(x, rows=True)
    _same("pooled", p, want)
    _check_rows("bfm_maxpool2_ex rows", raw, want, Cc, nr)
    x2 = np.stack([x, (x[::-1] * F32(0.5)).astype(F32)])
    pb, rawb, nrb = _pool(x2, rows=True, batch=True)
    per = nrb * Cc
    for s in range(2):
        w = R.pool_truth(x2[s])
        _same("batch pooled %d" % s, pb[s], w)
        planes = rawb.reshape(-1)
        one = np.concatenate([planes[o + s * per * k:o + (s + 1) * per * k]
                              for o, k in ((0, 8), (2 * per * 8, 8), (2 * per * 16, 4), (2 * per * 16 + 2 * per * 4, 4))])
        _check_rows("bfm_maxpool2_batch rows of sample %d" % s, one, w, Cc, nrb)
        alone_p, alone_raw, n1 = _pool(x2[s][None], rows=True, batch=True)
        assert n1 == nrb and (alone_raw == one).all(), "a sample's rows in a batch differ from its rows alone"


def test_maxpool2_second_grid_stride_lap_single_launch():
    Cc, dims = 64, (82, 82, 82)
    _, lib = _lib()
    assert lib.bfm_maxpool2_rows(Cc, *dims) == 4096 and 41 ** 3 * (Cc // 4) > 4096 * 256
    x = R.field("randn", dims + (Cc,), "lap2")
    want = R.pool_truth(x)
    p, raw, nr = _pool(x, rows=True)
    _same("pooled, two laps", p, want)
    _, j = _check_rows("two-lap rows", raw, want, Cc, nr)
    assert j == 2


def test_maxpool2_second_grid_stride_lap_batch():
    Cc, dims = 256, (20, 20, 20)
    x = np.stack([R.field("randn", dims + (Cc,), "lap2b", s) for s in range(2)])
    pb, raw, nr = _pool(x, rows=True, batch=True)
    assert nr == 128 and 10 ** 3 * (Cc // 4) > 128 * 256
    per = nr * Cc
    for s in range(2):
        w = R.pool_truth(x[s])
        _same("batch pooled, two laps", pb[s], w)
        one = np.concatenate([raw[o + s * per * k:o + (s + 1) * per * k]
                              for o, k in ((0, 8), (2 * per * 8, 8), (2 * per * 16, 4), (2 * per * 16 + 2 * per * 4, 4))])
        _, j = _check_rows("two-lap batch rows", one, w, Cc, nr)
        assert j == 2


# ------------------------------------------------------------------------------- F. the two routes the engine chooses between
@pytest.mark.parametrize("kind", ["randn", "offset30", "decoder"])
def test_chain_pool_rows_against_tensor_pass(kind):
    L, lib = _lib()
    Cc, dims, G = 64, (20, 20, 20), 8
    x = R.field("offset30" if kind == "offset30" else "randn", dims + (Cc,), "chain")
    p, raw, nr = _pool(x, rows=True)
    pooled = R.pool_truth(x)
    _same("pooled", p, pooled)
    hi = pooled.shape[:3]
    tabA = R.table_from_bytes(raw.tobytes(), nr, Cc)
    _, dS, _, dQ, j = R.pool_row_bounds(pooled, Cc, nr)
    B = tabB = None
    CB, nrB, lo, wB = 0, 0, None, 1.0
    if kind == "decoder":
        xb = R.field("randn", hi + (128,), "chainB")
        pB, rawB, nrB = _pool(xb, rows=True)
        B, CB, lo, wB = R.pool_truth(xb), 128, tuple(n // 2 for n in hi), 8.0
        _same("pooled B", pB, B)
        tabB = R.table_from_bytes(rawB.tobytes(), nrB, CB)
        _, dSb, _, dQb, _ = R.pool_row_bounds(B, CB, nrB)
        dS, dQ = np.concatenate([dS, dSb * wB]), np.concatenate([dQ, dQb * wB])
    gamma, beta = R.affine(Cc + CB, "chain", kind)
    nvox = int(np.prod(hi))
    truth = R.gn_truth(pooled, B, R.up_maps(lo, hi) if CB else None, gamma, beta, G)
    mn, mx = R.extremes_as_coded(pooled, B)
    # the tensor route
    tens = _gn(pooled, B, lo, gamma, beta, G)
    _check_stats("chain, tensor route", tens, truth, mn, mx, gamma, beta, G)
    # the rows route: its own bound = the bound for given rows + the producer's share
    rt = R.rows_truth(tabA, tabB, wB, nvox, gamma, beta, G)
    extra = R.pool_rows_extra(truth, dS, dQ, G)
    rc, rows = _rows_call("train", _raw(raw.tobytes()), nr, Cc, _raw(rawB.tobytes()) if CB else None, nrB, CB, wB, nvox, gamma, beta, G)
    assert rc == 0
    _check_stats("chain, rows as given", rows, rt, mn, mx, gamma, beta, G)
    _note("chain, rows route against the tensor's truth", R.gn_ratios(truth, rows["scale"], rows["shift"], rows["mean"], rows["rstd"],
                                                                         extra=extra))
    # figures: rstd error of the two routes and of torch's fp32 group_norm on the CPU on the same data
    rel = lambda r: float(np.max(np.abs(np.asarray(r, F64) - truth["rstd"]) / truth["rstd"]))
    xt = torch.from_numpy(R.materialise(pooled, B, R.up_maps(lo, hi) if CB else None)).permute(3, 0, 1, 2)[None].contiguous()
    y32 = torch.nn.functional.group_norm(xt, G, None, None, float(F32(EPS)))
    y64 = torch.nn.functional.group_norm(xt.double(), G, None, None, float(F32(EPS)))
    # torch returns no rstd: take it from the slope of its output against the float64 output, per group
    cpg = (Cc + CB) // G
    a32 = y32[0].double().reshape(G, -1)
    a64 = y64[0].reshape(G, -1)
    slope = ((a32 - a32.mean(1, keepdim=True)) * (a64 - a64.mean(1, keepdim=True))).sum(1) / ((a64 - a64.mean(1, keepdim=True)) ** 2).sum(1)
    torch_rel = float((slope - 1).abs().max())
    fig = dict(rows=rel(rows["rstd"]), tensor=rel(tens["rstd"]), torch_fp32=torch_rel,
               rows_bound=float(np.max((truth["drstd"] + extra["drstd"]) / truth["rstd"])), j=j)
    print("\nchain %s (mean/std = %.3g): rstd relative error rows %.3g  tensor %.3g  torch fp32 group_norm (CPU) %.3g;"
          " rows bound %.3g, j = %d" % (kind, float(np.max(np.abs(truth["mean"]) / np.sqrt(truth["var"]))), fig["rows"], fig["tensor"],
                                        fig["torch_fp32"], fig["rows_bound"], j), end="")
    for k, v in fig.items():
        WORST[("chain " + kind, k)] = v


# ---------------------------------------------------------------------------------------------------------- G. refusals
def test_gn_stats_refusals_write_nothing():
    L, lib = _lib()
    A = R.field("randn", (4, 6, 4, 8), "refA")
    B = R.field("randn", (2, 3, 2, 8), "refB")
    dA, dB = _in(A), _in(B)
    up = _Up((2, 3, 2), (4, 6, 4))
    gamma, beta = R.affine(16, "ref")
    dg, db = _in(gamma), _in(beta)
    need = lib.bfm_gn_stats_workspace(8, 8, 4, 6, 4, C.byref(up.desc))
    needb = lib.bfm_gn_stats_batch_workspace(8, 0, 2, 2, 6, 4, None)
    st = L.stream_ptr()

    def call(want, A_=dA, CA=8, B_=dB, CB=8, dims=(4, 6, 4), upd=up.desc, g_=dg, b_=db, G=4, nul=None, wsb=need, nows=False):
        outs = [_Out(16), _Out(16), _Out(4), _Out(4), _Out(4)]
        ws = _Bytes(need)
        ptrs = [o.ptr() for o in outs]
        if nul is not None:
            ptrs[nul] = None
        rc = lib.bfm_gn_stats_train(L.ptr(A_), CA, L.ptr(B_), CB, dims[0], dims[1], dims[2], C.byref(upd) if upd is not None else None,
                                    L.ptr(g_), L.ptr(b_), G, EPS, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4],
                                    None if nows else ws.ptr(), wsb, st)
        assert rc == want, (rc, want)
        for o in outs:
            o.untouched("gn_stats refusal")
        ws.untouched("gn_stats refusal workspace")

    call(E_ARG, A_=None)
    call(E_ARG, B_=None)
    call(E_ARG, upd=None)
    call(E_ARG, g_=None)
    call(E_ARG, b_=None)
    for i in range(3):
        call(E_ARG, nul=i)
    call(E_ARG, nows=True)
    call(E_ARG, CA=0)
    call(E_ARG, CB=-1)
    call(E_ARG, dims=(0, 6, 4))
    bad = L.Upsample(2, 3, 2, *([up.dev[0].data_ptr()] * 3 + [0, up.dev[4].data_ptr(), up.dev[5].data_ptr()]))
    call(E_ARG, upd=bad)
    bad = L.Upsample(0, 3, 2, *[t.data_ptr() for t in up.dev])
    call(E_ARG, upd=bad)
    call(E_SHAPE, G=3)
    call(E_SHAPE, G=0)
    call(E_WS, wsb=need - 1)
    for S in (0, -1, 65536):
        outs = [_Out(32), _Out(32), _Out(8)]
        ws = _Bytes(needb)
        rc = lib.bfm_gn_stats_batch(L.ptr(dA), 8, None, 0, S, 2, 6, 4, None, L.ptr(dg), L.ptr(db), 4, EPS, outs[0].ptr(), outs[1].ptr(),
                                    outs[2].ptr(), ws.ptr(), needb, st)
        assert rc == E_ARG
        for o in outs:
            o.untouched("gn_stats_batch refusal")
    outs = [_Out(32), _Out(32), _Out(8)]
    rc = lib.bfm_gn_stats_batch(L.ptr(dA), 8, None, 0, 2, 2, 6, 4, None, L.ptr(dg), L.ptr(db), 4, EPS, outs[0].ptr(), outs[1].ptr(),
                                outs[2].ptr(), _Bytes(needb).ptr(), needb - 1, st)
    assert rc == E_WS
    for o in outs:
        o.untouched("gn_stats_batch workspace refusal")


def test_gn_stats_rows_refusals_write_nothing():
    L, lib = _lib()
    nA, CA, nB, CB, G = 200, 8, 150, 8, 4
    g = np.random.default_rng(3)
    tA = R.make_table(g.standard_normal((nA, CA, 4)).astype(F32))
    tB = R.make_table(g.standard_normal((nB, CB, 4)).astype(F32))
    dA, dB = _raw(R.table_bytes(tA)), _raw(R.table_bytes(tB))
    gamma, beta = R.affine(16, "rref")
    dg, db = _in(gamma), _in(beta)
    need = lib.bfm_gn_stats_rows_workspace(nA, CA, nB, CB)
    exact = R.rows_fold_bytes(nA, CA) + R.rows_fold_bytes(nB, CB)
    assert need == exact + 256
    ticket = torch.zeros(R.GN_TICKETS + 4, dtype=torch.int32, device=_dev())

    def refuse(want, form="train", **kw):
        a = dict(tA=dA, nA=nA, CA=CA, tB=dB, nB=nB, CB=CB, wB=8.0, nvox=800, gamma=dg, beta=db, G=G, ticket=ticket[:R.GN_TICKETS])
        a.update(kw)
        rc, bufs = _rows_call(form, **a)
        assert rc == want, (rc, want, kw)
        for o in bufs:
            o.untouched("rows refusal")
        assert int(ticket.abs().sum()) == 0, "tickets touched by a refused call"

    refuse(E_ARG, tA=None)
    refuse(E_ARG, tB=None)
    refuse(E_ARG, nA=0)
    refuse(E_ARG, nB=0)
    refuse(E_ARG, CA=0)
    refuse(E_ARG, CB=-1)
    refuse(E_ARG, nvox=0)
    refuse(E_ARG, gamma=None, beta=db)
    refuse(E_ARG, wB=0.0)
    refuse(E_ARG, wB=-8.0)
    refuse(E_ARG, wB=float("nan"))
    refuse(E_ARG, tA=dA[4:])                                       # rows 4 bytes off the 8-byte alignment
    refuse(E_ARG, tB=dB[4:])
    refuse(E_ARG, ticket=ticket.view(torch.uint8)[2:2 + 4 * R.GN_TICKETS])          # a ticket off its 4-byte alignment
    refuse(E_SHAPE, G=3)
    refuse(E_SHAPE, G=0)
    refuse(E_WS, ws_bytes=exact - 1)
    refuse(E_ARG, form="sliced", slices=(nA, 1, nB, 0))                  # first + nrows > total
    refuse(E_ARG, form="sliced", slices=(nA, 0, nB - 1, 0))
    refuse(E_ARG, form="sliced", slices=(nA, -1, nB, 0))
    refuse(E_SHAPE, form="batch", nA=129, S=1)                          # more than 128 rows per sample
    refuse(E_SHAPE, form="batch", nA=100, nB=129, S=1)
    refuse(E_ARG, form="batch", nA=10, nB=10, S=0)
    refuse(E_ARG, form="batch", nA=10, nB=10, S=65536)
    refuse(E_ARG, form="batch", nA=10, nB=10, S=1, wB=float("nan"))
    refuse(E_SHAPE, form="batch", nA=10, nB=10, S=1, G=3)
    # a misaligned workspace: the fold would write doubles there
    outs = [_Out(16), _Out(16), _Out(4)]
    ws = _Bytes(need + 8)
    rc = lib.bfm_gn_stats_rows(L.ptr(dA), nA, CA, L.ptr(dB), nB, CB, 8.0, 800, L.ptr(dg), L.ptr(db), G, EPS, outs[0].ptr(), outs[1].ptr(),
                               outs[2].ptr(), ws.ptr() + 4, need, None, L.stream_ptr())
    assert rc == E_ARG
    for o in outs + [ws]:
        o.untouched("misaligned workspace")


def test_maxpool2_refusals_write_nothing():
    L, lib = _lib()
    st = L.stream_ptr()
    x = _in(R.field("randn", (4, 4, 4, 12), "pref"))
    x1 = _in(R.field("randn", (4, 4, 4, 8), "pref"), 1)

    def refuse(want, fn, *args):
        out = _Out(2 * 2 * 2 * 2 * 2048)
        tab = _Bytes(4096)
        a = [out.ptr() if v == "out" else (tab.ptr() if v == "tab" else (tab.ptr() + 4 if v == "tab4" else v)) for v in args]
        rc = fn(*a, st)
        assert rc == want, (rc, want, args)
        out.untouched("pool refusal")
        tab.untouched("pool refusal rows")

    ex, ba = lib.bfm_maxpool2_ex, lib.bfm_maxpool2_batch
    refuse(E_ARG, ex, None, 12, 4, 4, 4, "out", None)
    refuse(E_ARG, ex, L.ptr(x), 12, 4, 4, 4, None, None)
    refuse(E_ARG, ex, L.ptr(x), 0, 4, 4, 4, "out", None)
    for dims in ((1, 4, 4), (4, 1, 4), (4, 4, 1)):
        refuse(E_ARG, ex, L.ptr(x), 12, *dims, "out", None)
        refuse(E_ARG, ba, L.ptr(x), 12, 1, *dims, "out", None)
    for Cc in (12, 6):                                                  # rows where the counter says 0
        assert lib.bfm_maxpool2_rows(Cc, 4, 4, 4) == 0
        refuse(E_SHAPE, ex, L.ptr(x), Cc, 4, 4, 4, "out", "tab")
    refuse(E_SHAPE, ba, L.ptr(x), 12, 1, 4, 4, 4, "out", "tab")
    refuse(E_SHAPE, ex, L.ptr(x1), 8, 4, 4, 4, "out", "tab")              # misaligned input: scalar lanes cannot emit rows
    refuse(E_ARG, ex, L.ptr(x), 8, 4, 4, 4, "out", "tab4")                # rows off their 8-byte alignment
    refuse(E_ARG, ba, L.ptr(x), 8, 1, 4, 4, 4, "out", "tab4")
    refuse(E_ARG, ba, None, 8, 1, 4, 4, 4, "out", None)
    refuse(E_ARG, ba, L.ptr(x), 8, 0, 4, 4, 4, "out", None)
    refuse(E_ARG, ba, L.ptr(x), 8, 65536, 4, 4, 4, "out", None)
    refuse(E_SHAPE, ba, L.ptr(x), 6, 1, 4, 4, 4, "out", None)             # the batch form has float4 lanes only
    refuse(E_SHAPE, ba, L.ptr(x1), 8, 1, 4, 4, 4, "out", None)


def test_zz_report():
    """Prints the worst figure per family (run the module with -s)."""
    fam = {}
    for (f, k), v in sorted(WORST.items()):
        fam.setdefault(f, []).append("%s %.3g" % (k, v))
    print()
    for f, items in fam.items():
        print("  %-48s %s" % (f, "  ".join(items)))
    print("  bit-for-bit checks: %d, differing elements: %d" % (DIFFS["checks"], DIFFS["elements"]))
    assert DIFFS["elements"] == 0
