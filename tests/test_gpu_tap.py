"""Kernel-level tests of the tap-wise GEMM route of the smallest deep levels (conv3d_tap.hip): bfm_conv3x3x3_tap_batch
(per-tap products on the batch's densely packed rows) + bfm_tap_sum_batch (gather-sum, LeakyReLU, moment rows) against
float64, and every sample against its own S = 1 launch and the reversed batch, bit for bit.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

S, G, CA, CB, COUT, SLOPE = 3, 8, 64, 96, 128, 0.01


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    return torch.device("cuda:0")


def _lib():
    from brainfm_amd import _lib as L
    return L, L.load()


def _nearest(B, hi):
    x = B.permute(0, 4, 1, 2, 3)
    return F.interpolate(x, size=tuple(hi), mode="nearest").permute(0, 2, 3, 4, 1)


def _group_bound(Y, groups):
    s, c = Y.shape[0], Y.shape[-1]
    return Y.abs().reshape(s, -1, groups, c // groups).amax((1, 3)).float().contiguous()


def _pack_mfma(w):
    """conv_mfma's fragment pack of w (Cout, Cin, 3, 3, 3) on the device -> (buffer, wexp)."""
    L, lib = _lib()
    cout, cin = w.shape[:2]
    wp = torch.empty(lib.bfm_pack_conv_weights_mfma_bytes(cin, cout), dtype=torch.uint8, device=w.device)
    wexp = C.c_int(0)
    L.check(lib.bfm_pack_conv_weights_mfma(L.ptr(w), cin, cout, float(w.abs().max()), L.ptr(wp), C.byref(wexp),
                                           L.stream_ptr()), "pack_mfma")
    return wp, wexp.value


def _table(lo, hi, dev):
    from brainfm_amd.engine import tap_row_table
    return torch.from_numpy(tap_row_table(lo, hi)).to(dev)


def _tap(X, cx, ss, n_lo, sc, sh, bd, wp, wexp, cout, kc_first, kc_pack, passes, aff, tab, n_hi, out, act=0, accumulate=0,
         rows=None):
    """tap_batch + tap_sum of `ss` samples into `out`."""
    L, lib = _lib()
    st = L.stream_ptr()
    nb = lib.bfm_conv3x3x3_tap_batch_workspace(cx, cout, ss, n_lo)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=out.device)
    L.check(lib.bfm_conv3x3x3_tap_batch(L.ptr(X), cx, ss, n_lo, L.ptr(sc), L.ptr(sh), L.ptr(bd), G, L.ptr(wp), wexp, cout,
                                        kc_first, kc_pack, passes, L.ptr(ws), ws.numel(), aff, st), "tap_batch")
    L.check(lib.bfm_tap_sum_batch(L.ptr(ws), cx, cout, ss, n_lo, L.ptr(tab), n_hi, SLOPE, act, accumulate, L.ptr(out),
                                  L.ptr(rows) if rows is not None else None, st), "tap_sum_batch")
    torch.cuda.synchronize()


_TWO = {}


def _two_source_case(lo, hi):
    """Inputs of the two-source case and its float64 reference, made once per shape and left unchanged."""
    key = (lo, hi)
    if key not in _TWO:
        dev = _dev()
        g = torch.Generator().manual_seed(CB + 10 * lo[0] + hi[2])
        B = torch.randn((S,) + lo + (CB,), generator=g)
        B[1] = B[1] * 3 + 0.5                                      # samples of different statistics
        B[2] = 0                                                   # and an all-zero one
        A = torch.randn((S,) + hi + (CA,), generator=g)
        w = torch.randn(COUT, CA + CB, 3, 3, 3, generator=g) * 0.02
        scale = torch.rand(S, CA + CB, generator=g) + 0.5
        shift = torch.randn(S, CA + CB, generator=g) * 0.2
        Y = torch.cat((A * scale[:, None, None, None, :CA] + shift[:, None, None, None, :CA],
                       _nearest(B, hi) * scale[:, None, None, None, CA:] + shift[:, None, None, None, CA:]), -1)
        bound = _group_bound(Y, G).to(dev)
        want = F.conv3d(Y[..., CA:].double().permute(0, 4, 1, 2, 3), w[:, CA:].double(), padding=1).permute(0, 2, 3, 4, 1)
        w = w.to(dev).contiguous()
        wp, wexp = _pack_mfma(w)
        _TWO[key] = dict(B=B.to(dev), scale=scale.to(dev).contiguous(), shift=shift.to(dev).contiguous(), bound=bound,
                         want=want, wp=wp, wexp=wexp, tab=_table(lo, hi, dev))
    return _TWO[key]


def _two_launch(c, lo, hi, Bs, ss, sc, sh, bd, out, passes=3, accumulate=0):
    _tap(Bs, CB, ss, lo[0] * lo[1] * lo[2], sc, sh, bd, c["wp"], c["wexp"], COUT, CA // 16, (CA + CB) // 16, passes,
         CA + CB, c["tab"], hi[0] * hi[1] * hi[2], out, 0, accumulate)


@pytest.mark.parametrize("lo,hi", [((2, 2, 2), (5, 5, 5)), ((5, 5, 2), (10, 10, 5))])
def test_tap_two_sources_vs_float64_alone_and_reversed_bitwise(lo, hi):
    """The upsampled half of a decoder's first conv: cb = 96 (six K chunks), cout = 128 (two Cout tiles), S = 3 with one
    sample scaled x3 + 0.5 and one all zero, scale / shift the columns ca.. of a [S][ca + cb] table.  (5,5,2) -> (10,10,5)
    packs 3 x 50 = 150 rows: across 32-row blocks and past the 128-row group.  Within 2e-5 of max |y| per sample of the
    float64 conv3d of the upsampled, affine-applied tensor with w[:, ca:] (the bound of
    test_upfold_batch_vs_float64_and_each_sample_alone_bitwise); every sample the bits of its own S = 1 launch and of the
    launch with the batch reversed."""
    c = _two_source_case(lo, hi)
    dev = _dev()
    B, scale, shift, bound = c["B"], c["scale"], c["shift"], c["bound"]
    out = torch.full((S,) + hi + (COUT,), float("nan"), device=dev)
    _two_launch(c, lo, hi, B, S, scale[:, CA:], shift[:, CA:], bound, out)
    got = out.double().cpu()
    errs = [float((got[s_] - c["want"][s_]).abs().max() / c["want"][s_].abs().max()) for s_ in range(S)]
    print("tap two sources %s -> %s: float64 errors %s" % (lo, hi, ["%.2e" % e for e in errs]))
    assert max(errs) <= 2e-5, errs
    for s_ in range(S):
        one = torch.full(hi + (COUT,), float("nan"), device=dev)
        _two_launch(c, lo, hi, B[s_], 1, scale[s_, CA:], shift[s_, CA:], bound[s_], one)
        assert torch.equal(out[s_], one), s_
    rev = torch.full_like(out, float("nan"))
    rs, rh = scale.flip(0).contiguous(), shift.flip(0).contiguous()
    _two_launch(c, lo, hi, B.flip(0).contiguous(), S, rs[:, CA:], rh[:, CA:], bound.flip(0).contiguous(), rev)
    assert torch.equal(out, rev.flip(0))


def _gn64(X, gamma, beta, groups, eps=1e-5):
    X = X.double()
    n, c = X.shape
    cpg = c // groups
    xg = X.reshape(n, groups, cpg)
    mean = xg.mean((0, 2))
    var = ((xg - mean[None, :, None]) ** 2).mean((0, 2))
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.double() * rstd.repeat_interleave(cpg)
    shift = beta.double() - mean.repeat_interleave(cpg) * scale
    bound = (X * scale + shift).abs().reshape(n, groups, cpg).amax((0, 2))
    return scale, shift, bound


@pytest.mark.parametrize("dims", [(2, 2, 2), (5, 2, 2)])
def test_tap_one_source_vs_float64_rows_and_bitwise(dims):
    """A plain conv on a tiny volume (identity map): cin = 96, cout = 128, S = 3, LeakyReLU on, moment rows on, output
    NaN-prefilled so that an unwritten voxel shows.  Same float64 bound and bitwise checks as the two-source case;
    bfm_gn_stats_rows_batch on the emitted rows gives scale / shift / bound within 1e-5 of float64 statistics of the stored
    output (the bound of test_gn_stats_batch_vs_float64_and_each_sample_alone_bitwise)."""
    L, lib = _lib()
    dev = _dev()
    cin, nv, eps = CB, dims[0] * dims[1] * dims[2], 1e-5
    g = torch.Generator().manual_seed(cin + nv)
    X = torch.randn((S,) + dims + (cin,), generator=g)
    X[1] = X[1] * 3 + 0.5
    X[2] = 0
    w = torch.randn(COUT, cin, 3, 3, 3, generator=g) * 0.02
    scale = torch.rand(S, cin, generator=g) + 0.5
    shift = torch.randn(S, cin, generator=g) * 0.2
    Y = X * scale[:, None, None, None] + shift[:, None, None, None]
    bound = _group_bound(Y, G).to(dev)
    want = F.leaky_relu(F.conv3d(Y.double().permute(0, 4, 1, 2, 3), w.double(), padding=1), SLOPE).permute(0, 2, 3, 4, 1)
    X, scale, shift, w = X.to(dev), scale.to(dev).contiguous(), shift.to(dev).contiguous(), w.to(dev).contiguous()
    wp, wexp = _pack_mfma(w)
    tab = _table(dims, dims, dev)
    nrows = lib.bfm_tap_sum_rows(nv, COUT)
    assert 0 < nrows <= 128

    def launch(Xs, ss, sc, sh, bd, out, rows):
        _tap(Xs, cin, ss, nv, sc, sh, bd, wp, wexp, COUT, 0, cin // 16, 3, 0, tab, nv, out, 1, 0, rows)

    out = torch.full((S,) + dims + (COUT,), float("nan"), device=dev)
    rows = torch.zeros(lib.bfm_moment_rows_bytes(S * nrows, COUT), dtype=torch.uint8, device=dev)
    launch(X, S, scale, shift, bound, out, rows)
    assert bool(torch.isfinite(out).all()), "an output voxel was not written"
    got = out.double().cpu()
    errs = [float((got[s_] - want[s_]).abs().max() / want[s_].abs().max()) for s_ in range(S)]
    print("tap one source %s: float64 errors %s" % (dims, ["%.2e" % e for e in errs]))
    assert max(errs) <= 2e-5, errs
    for s_ in range(S):
        one = torch.full(dims + (COUT,), float("nan"), device=dev)
        r1 = torch.zeros(lib.bfm_moment_rows_bytes(nrows, COUT), dtype=torch.uint8, device=dev)
        launch(X[s_], 1, scale[s_], shift[s_], bound[s_], one, r1)
        assert torch.equal(out[s_], one), s_
    rev = torch.full_like(out, float("nan"))
    rr = torch.zeros_like(rows)
    launch(X.flip(0).contiguous(), S, scale.flip(0).contiguous(), shift.flip(0).contiguous(), bound.flip(0).contiguous(),
           rev, rr)
    assert torch.equal(out, rev.flip(0))
    # the consumer's GroupNorm statistics from the rows
    gamma = (torch.rand(COUT, generator=g) + 0.5).to(dev)
    beta = (torch.randn(COUT, generator=g) * 0.1).to(dev)
    s2 = torch.full((S, COUT), float("nan"), device=dev)
    h2, b2 = torch.full_like(s2, float("nan")), torch.full((S, G), float("nan"), device=dev)
    L.check(lib.bfm_gn_stats_rows_batch(L.ptr(rows), nrows, COUT, None, 0, 0, 8.0, nv, S, L.ptr(gamma), L.ptr(beta), G, eps,
                                        L.ptr(s2), L.ptr(h2), L.ptr(b2), L.stream_ptr()), "gn_stats_rows_batch")
    torch.cuda.synchronize()
    serr = []
    for s_ in range(S):
        ref = _gn64(out[s_].cpu().reshape(-1, COUT), gamma.cpu(), beta.cpu(), G, eps)
        for a, b in zip((s2[s_], h2[s_], b2[s_]), ref):
            serr.append(float((a.double().cpu() - b).abs().max() / b.abs().max()))
    print("tap one source %s: statistics from the rows vs float64 %s" % (dims, ["%.1e" % e for e in serr]))
    assert max(serr) <= 1e-5, serr


def test_tap_sum_accumulates_onto_a_prior_tensor_bitwise():
    """bfm_tap_sum_batch with accumulate = 1 onto a prior tensor == prior + the non-accumulating result, bit for bit."""
    lo, hi = (2, 2, 2), (5, 5, 5)
    c = _two_source_case(lo, hi)
    dev = _dev()
    plain = torch.full((S,) + hi + (COUT,), float("nan"), device=dev)
    _two_launch(c, lo, hi, c["B"], S, c["scale"][:, CA:], c["shift"][:, CA:], c["bound"], plain)
    prior = torch.randn(plain.shape, generator=torch.Generator().manual_seed(5)).to(dev)
    acc = prior.clone()
    _two_launch(c, lo, hi, c["B"], S, c["scale"][:, CA:], c["shift"][:, CA:], c["bound"], acc, accumulate=1)
    for s_ in range(S):
        assert torch.equal(acc[s_], prior[s_] + plain[s_]), s_


def test_tap_single_pass_error_at_most_twice_conv_mfma_single_pass():
    """passes = 1 (one fp16 product): the two-source case against float64; the bound is twice the error of
    bfm_conv3x3x3_mfma_batch with passes = 1 on the same inputs and the same pack, measured here (its skip half reads a
    zero tensor with a zero shift, LeakyReLU slope 1: the same linear map)."""
    from brainfm_amd.engine import nearest_index_map
    L, lib = _lib()
    lo, hi = (2, 2, 2), (5, 5, 5)
    c = _two_source_case(lo, hi)
    dev = _dev()
    out = torch.full((S,) + hi + (COUT,), float("nan"), device=dev)
    _two_launch(c, lo, hi, c["B"], S, c["scale"][:, CA:], c["shift"][:, CA:], c["bound"], out, passes=1)
    # the yardstick: conv_mfma on cat((0, up(B)))
    A0 = torch.zeros((S,) + hi + (CA,), device=dev)
    sh0 = c["shift"].clone()
    sh0[:, :CA] = 0
    maps = [nearest_index_map(lo[a], hi[a]) for a in range(3)]
    reps = [np.bincount(maps[a], minlength=lo[a]).astype(np.int32) for a in range(3)]
    keep = [torch.from_numpy(m).to(dev) for m in maps + reps]
    up = L.Upsample(lo[0], lo[1], lo[2], *[t.data_ptr() for t in keep])
    cfg = (C.c_int * 8)()
    L.check(lib.bfm_conv3x3x3_mfma_plan(CA + CB, COUT, hi[0], hi[1], hi[2], cfg), "plan")
    cfg[6] = 0
    ws = torch.empty(max(lib.bfm_conv3x3x3_mfma_batch_workspace(CA + CB, COUT, S, hi[0], hi[1], hi[2], cfg[5]), 256),
                     dtype=torch.uint8, device=dev)
    ref = torch.full_like(out, float("nan"))
    L.check(lib.bfm_conv3x3x3_mfma_batch(L.ptr(A0), CA, L.ptr(c["B"]), CB, S, hi[0], hi[1], hi[2], C.byref(up),
                                         L.ptr(c["scale"]), L.ptr(sh0), L.ptr(c["bound"]), G, L.ptr(c["wp"]), c["wexp"], COUT,
                                         1.0, 1, cfg, L.ptr(ref), L.ptr(ws), ws.numel(), None, 0, L.stream_ptr()),
            "conv_mfma_batch")
    torch.cuda.synchronize()
    want = c["want"]
    e_tap = max(float((out[s_].double().cpu() - want[s_]).abs().max() / want[s_].abs().max()) for s_ in range(S))
    e_ref = max(float((ref[s_].double().cpu() - want[s_]).abs().max() / want[s_].abs().max()) for s_ in range(S))
    print("passes = 1: tap error %.3e, conv_mfma error %.3e" % (e_tap, e_ref))
    assert e_tap <= 2 * e_ref, (e_tap, e_ref)
