"""Conformance of the HuBERT front-end kernels -- csrc/frontend.hip (triad_chgn_gelu_fwd / _bwd,
triad_c0gn_fwd, triad_conv0_dw) and csrc/posconv.hip (triad_posconv, triad_posconv_dw) -- against fp64
references of the same bf16 / fp32 operands, through the C ABI (`triad_amd._lib.call`), and of
frontend._Conv0GNGelu / _PosConv and the padded frame stack over them.

Operands come from a seeded CPU generator (tests/frontend_ref.py, which also holds the references,
the bounds and their derivation; tests/test_frontend_checks_cpu.py shows that each bound passes an
fp32 emulation of its kernel and fails the planted errors). Every output, workspace and partial
buffer is filled with NaN before the call, carries guard elements or rows past its end that must
survive, and is checked to be finite before it is compared; the padding frames T .. Tp - 1 of the
inputs and the unused waveform tail hold NaN, the padding frames of the outputs must come out as
exact zeros. The bounds are derived from the rounding steps of the code, per element, u = 2^-24
(nothing is fitted to what the kernels return; h = ceil(128 / rows) + rows, rows = 256 / (C / 8)):

    chgn / c0gn mean   (h + 1) u mean|x|                        exact-sum channels: 2 u |mean|
    chgn / c0gn rstd   rstd (0.5 ((h + 1) u E2 + 2 |m| dm + dm^2) / (var + eps) + 2 u)
                                                                exact-sum channels: rstd (3 u + 4 2^-53 E2 / (var + eps))
    chgn / c0gn y      1.13 (|gamma| rstd dm + |xhat gamma| (rel_rstd + 4 u) + u |z|) + gelu_err + 2^-8 |ref|
    chgn dgamma/dbeta  (h + B + 2) u sum|terms| + the function-error term
    chgn dx            rstd (u-level terms on dz gamma, cA, xhat cB) + 2^-8 |ref|
    c0gn y0out         == bf16(fp64 sum), or one bf16 gap off where that sum lies within 24 u sum|w||s| of
                       a rounding boundary (at most 2 % of a case's elements, asserted)
    conv0_dw           2 (n + 2) u sum|dy||s|,  n = ceil(1024 / rows) + rows + slab depth
    posconv y          2 (128 CG + 2) u (sum|x||w| + |bias|) + 2^-8 |ref|
    posconv_dw slab    2 (n + 2) u sum|dy||x|,  n = rows of one split;  sum: 2 (n + 2 + splits) u sum|dy||x|

Bit-identities read from the code: a repeated call returns the same bits (no atomics, fixed orders);
triad_chgn_gelu_fwd over triad_c0gn_fwd's y0out reproduces its mean, rstd and out; the autograd
functions return what the same entry points return when called directly; in the padded frame stack
a sample's output frames and its contribution to every weight gradient do not depend on the other
samples of the batch. All of them held on MI355X.

Largest err / bound per group on MI355X (38 cases, 1 242 bound comparisons, 14 s; also in DESIGN.md
section 2). bf16 outputs, where the one rounding fills its 2^-8 term: chgn y 0.995, dx 0.995, c0gn y
0.995, posconv y 0.791 (CG 48) / 0.735 (CG 64). fp32 outputs: chgn mean 0.400, rstd 0.330, dgamma
0.068, dbeta 0.077 (the ASSUMED erff / __expf limits of frontend_ref.py are not tight), c0gn mean
0.008, rstd 0.233, conv0_dw 0.0026, posconv_dw slab 0.100 / sum 0.070. conv0_dw stays far inside a
worst-case bound of 67 - 263 roundings; a dropped one-row slab still exceeds it 540 x
(tests/test_frontend_checks_cpu.py). At most 2 elements of a case's y0out took the flip allowance.
"""
import ctypes
import functools

import pytest
import torch

from tests import frontend_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
EPS = 1e-5
GUARD = 64        # NaN elements past the end of a flat fp32 output
GROWS = 2         # guard rows past row B * Tp - 1 of a frame buffer
PATTERN = 0x7FC1  # their bf16 bit pattern (a NaN)
WORST = {}        # group -> largest err / bound of this run (printed per check; pytest -s shows them)


def _lib():
    from triad_amd import _lib
    return _lib


def _at(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _nan(n, dt=F32):
    return torch.full((n,), NAN, dtype=dt, device=dev)


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _check(got, ref, bound, group, what):
    got = got.cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (unwritten or poisoned elements)"
    r = R.ratio(got, ref, bound)
    WORST[group] = max(WORST.get(group, 0.0), r)
    print(f"{group} {what}: err/bound {r:.4f}")
    assert r <= 1.0, f"{group} {what}: err/bound {r}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nfront-end kernels, largest err/bound per group:",
          ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))


def _frames_out(B, Tp, C):
    """A NaN-filled bf16 frame buffer [B * Tp + GROWS][C] whose guard rows hold PATTERN."""
    buf = torch.full((B * Tp + GROWS, C), NAN, dtype=BF, device=dev)
    buf[B * Tp:].view(torch.int16).fill_(PATTERN)
    return buf


def _frames_ok(buf, B, T, Tp, what):
    """Guard rows untouched, padding frames exactly zero; returns the [B][Tp][C] view."""
    assert bool((buf[B * Tp:].view(torch.int16) == PATTERN).all()), what + ": wrote past row B * Tp - 1"
    v = buf[:B * Tp].view(B, Tp, -1)
    assert bool((v[:, T:].view(torch.int16) == 0).all()), what + ": padding frames are not +0"
    return v


def _ws(nbytes):
    return torch.full((int(nbytes) + 64,), 0xFF, dtype=torch.uint8, device=dev)   # all-ones bytes: NaN as float / double


def _ws_ok(ws, what):
    assert bool((ws[-64:] == 0xFF).all()), what + ": wrote past the workspace"


# ---- triad_chgn_gelu_fwd / triad_chgn_gelu_bwd ------------------------------------------------------

def _chgn_fwd(xd, B, T, Tp, C, gd, bd, what):
    L = _lib()
    y = _frames_out(B, Tp, C)
    mean, rstd = _nan(B * C + GUARD), _nan(B * C + GUARD)
    ws = _ws(L.call("triad_chgn_workspace_bytes", B, T, C))
    L.call("triad_chgn_gelu_fwd", _at(xd), B, T, Tp, C, _at(gd), _at(bd), EPS, _at(mean), _at(rstd), _at(ws), _at(y),
           L.stream_ptr())
    assert _all_nan(mean[B * C:]) and _all_nan(rstd[B * C:]), what + ": wrote past mean / rstd"
    _ws_ok(ws, what)
    return _frames_ok(y, B, T, Tp, what), mean[:B * C].view(B, C), rstd[:B * C].view(B, C)


def _chgn_bwd(xd, dyd, B, T, Tp, C, gd, bd, mean, rstd, what):
    L = _lib()
    dx = _frames_out(B, Tp, C)
    dg, db = _nan(C + GUARD), _nan(C + GUARD)
    ws = _ws(L.call("triad_chgn_workspace_bytes", B, T, C))
    L.call("triad_chgn_gelu_bwd", _at(xd), _at(dyd), B, T, Tp, C, _at(gd), _at(bd), _at(mean), _at(rstd), _at(ws),
           _at(dx), _at(dg), _at(db), L.stream_ptr())
    assert _all_nan(dg[C:]) and _all_nan(db[C:]), what + ": wrote past dgamma / dbeta"
    _ws_ok(ws, what)
    return _frames_ok(dx, B, T, Tp, what), dg[:C], db[:C]


def _chgn_forward_checks(x, T, gamma, beta, y, mean, rstd, group, what):
    want = R.chgn_fwd_ref(x, T, gamma, beta, R.f32(EPS))
    _check(mean, *want["mean"], group + ".mean", what)
    _check(rstd, *want["rstd"], group + ".rstd", what)
    _check(y[:, :T], *want["y"], group + ".y", what)
    return want


@pytest.mark.parametrize("C", [8, 64, 512, 2048])
def test_chgn_gelu_forward_and_backward(C):
    """rows = 256, 32, 4, 1 x T in {1, 5, 127, 128, 129, 300} (below, at and past one chunk; three
    chunks) x B in {1, 3} x Tp - T in {0, 1, 3}, NaN in the padding frames of x and dy: mean, rstd, y,
    then dx, dgamma, dbeta (started as NaN) from the kernel's own statistics. At C = 64 channels 8 .. 10
    are the mean-100 / sigma-0.1, the mean-0 / sigma-1e-3 and the constant channel."""
    for T in (1, 5, 127, 128, 129, 300):
        for B in (1, 3):
            for dT in (0, 1, 3):
                Tp = T + dT
                what = f"C {C} T {T} B {B} Tp {Tp}"
                x, dy, gamma, beta = R.chgn_case(B, T, Tp, C)
                xd, dyd, gd, bd = x.to(dev), dy.to(dev), gamma.to(dev), beta.to(dev)
                y, mean, rstd = _chgn_fwd(xd, B, T, Tp, C, gd, bd, what)
                want = _chgn_forward_checks(x, T, gamma, beta, y, mean, rstd, "chgn", what)
                if C == 64:
                    k100, kc = R.SPECIAL["mean100"], R.SPECIAL["const"]
                    assert bool(want["exact"][:, [k100, kc]].all()), what + ": the special channels' sums are not exact"
                    assert bool((mean[:, kc] == R.CONST).all()), what + ": constant channel's mean"
                    gb = R.gelu64(torch.tensor(R.CONST_BETA, dtype=R.F64)).to(F32).to(BF)
                    assert bool((y[:, :T, kc].cpu() == gb).all()), what + ": constant channel's y != bf16(gelu(beta))"
                mean, rstd = mean.contiguous(), rstd.contiguous()
                dx, dg, db = _chgn_bwd(xd, dyd, B, T, Tp, C, gd, bd, mean, rstd, what)
                wantb = R.chgn_bwd_ref(x, dy, T, gamma, beta, mean.cpu(), rstd.cpu())
                _check(dx[:, :T], *wantb["dx"], "chgn.dx", what)
                _check(dg, *wantb["dgamma"], "chgn.dgamma", what)
                _check(db, *wantb["dbeta"], "chgn.dbeta", what)


def test_chgn_gelu_repeat_is_bit_identical():
    B, T, Tp, C = 3, 300, 301, 512
    x, dy, gamma, beta = R.chgn_case(B, T, Tp, C)
    xd, dyd, gd, bd = x.to(dev), dy.to(dev), gamma.to(dev), beta.to(dev)
    runs = []
    for i in range(2):
        y, mean, rstd = _chgn_fwd(xd, B, T, Tp, C, gd, bd, f"run {i}")
        mean, rstd = mean.contiguous(), rstd.contiguous()
        runs.append((y, mean, rstd) + _chgn_bwd(xd, dyd, B, T, Tp, C, gd, bd, mean, rstd, f"run {i}"))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "a repeat changed the result"


# ---- triad_c0gn_fwd -------------------------------------------------------------------------------

def _c0gn(waved, w0d, B, T, Tp, C, gd, bd, what):
    L = _lib()
    out, y0 = _frames_out(B, Tp, C), _frames_out(B, Tp, C)
    mean, rstd = _nan(B * C + GUARD), _nan(B * C + GUARD)
    ws = _ws(L.call("triad_chgn_workspace_bytes", B, T, C))
    L.call("triad_c0gn_fwd", _at(waved), waved.shape[1], _at(w0d), B, T, Tp, C, _at(gd), _at(bd), EPS, _at(mean),
           _at(rstd), _at(ws), _at(out), _at(y0), L.stream_ptr())
    assert _all_nan(mean[B * C:]) and _all_nan(rstd[B * C:]), what + ": wrote past mean / rstd"
    _ws_ok(ws, what)
    return (_frames_ok(out, B, T, Tp, what), _frames_ok(y0, B, T, Tp, what), mean[:B * C].view(B, C),
            rstd[:B * C].view(B, C))


def _y0_check(y0, wave, w0, T, what):
    """y0out against the fp64 conv with the flip allowance, and the cap on the allowance's reach."""
    ref, gap = R.conv0_ref(wave, w0, T)
    share = float((gap > 0).double().mean())
    assert share <= 0.02, f"{what}: {share:.4f} of the elements lie near a rounding boundary"
    got = y0[:, :T].cpu()
    assert bool(torch.isfinite(got).all()), what + ": y0out not finite"
    err = (got.double() - ref).abs()
    assert bool((err <= gap).all()), f"{what}: y0out differs from bf16(fp64 conv) beyond the flip allowance"
    flips = int((err > 0).sum())
    WORST["c0gn.y0 flips"] = max(WORST.get("c0gn.y0 flips", 0), flips)
    print(f"c0gn.y0 {what}: near-boundary share {share:.4f}, {flips} flipped")


@pytest.mark.parametrize("C", [64, 512])
def test_c0gn_forward(C):
    """B = 2, T in {1, 128, 129, 300} x Tp in {T, T + 1}, NaN in the waveform past sample 5 (T - 1) + 9:
    y0out against the fp64 conv, mean / rstd / out against the fp64 GroupNorm + GELU of the kernel's own
    y0out, and triad_chgn_gelu_fwd over that y0out reproduces mean, rstd and out bit for bit."""
    B = 2
    for T in (1, 128, 129, 300):
        for Tp in (T, T + 1):
            what = f"C {C} T {T} Tp {Tp}"
            wave, w0, gamma, beta, _ = R.conv0_case(B, T, Tp, C)
            waved, w0d, gd, bd = wave.to(dev), w0.to(dev), gamma.to(dev), beta.to(dev)
            out, y0, mean, rstd = _c0gn(waved, w0d, B, T, Tp, C, gd, bd, what)
            _y0_check(y0, wave, w0, T, what)
            _chgn_forward_checks(y0.cpu(), T, gamma, beta, out, mean, rstd, "c0gn", what)
            y2, mean2, rstd2 = _chgn_fwd(y0.contiguous(), B, T, Tp, C, gd, bd, what)
            assert torch.equal(mean2, mean) and torch.equal(rstd2, rstd), what + ": chgn over y0out: other statistics"
            assert torch.equal(y2.view(torch.int16), out.view(torch.int16)), what + ": chgn over y0out: other output"


# ---- triad_conv0_dw -------------------------------------------------------------------------------

def _conv0_dw(waved, dyd, B, T, Tp, C, what):
    L = _lib()
    nbytes = L.call("triad_conv0_dw_workspace_bytes", B, T, C)
    ws = _ws(nbytes)
    dw = _nan(C * 10 + GUARD)
    L.call("triad_conv0_dw", _at(waved), waved.shape[1], _at(dyd), B, T, Tp, C, _at(ws), _at(dw), L.stream_ptr())
    assert _all_nan(dw[C * 10:]), what + ": wrote past dw0"
    _ws_ok(ws, what)
    assert bool(torch.isfinite(ws[:nbytes].view(F32)).all()), what + ": slab elements left unwritten"
    return dw[:C * 10].view(C, 10)


@pytest.mark.parametrize("C", [64, 512])
def test_conv0_dw(C):
    """B = 2, T on either side of the 1024-row block (1023, 1024, 1025: the third with a one-row second
    block), 1 and 2100 (three blocks), Tp in {T, T + 1}; NaN in dy0's padding frames and in the unused
    waveform tail."""
    B = 2
    for T in (1, 1023, 1024, 1025, 2100):
        for Tp in (T, T + 1):
            what = f"C {C} T {T} Tp {Tp}"
            wave, _, _, _, dy0 = R.conv0_case(B, T, Tp, C)
            dw = _conv0_dw(wave.to(dev), dy0.to(dev), B, T, Tp, C, what)
            _check(dw, *R.conv0_dw_ref(wave, dy0, T), "conv0_dw", what)


# ---- triad_posconv --------------------------------------------------------------------------------

def _posconv(xd, wtd, biasd, B, T, C, G, pad, what):
    L = _lib()
    y = _nan(B * T * C + GUARD, BF)
    L.call("triad_posconv", _at(xd), _at(wtd), _at(biasd), _at(y), B, T, C, G, pad, L.stream_ptr())
    assert _all_nan(y[B * T * C:]), what + ": wrote past y"
    return y[:B * T * C].view(B, T, C)


def _posconv_cases(C, G, Ts, pads):
    B = 3
    for T in Ts:
        x, _, W, bias = R.posconv_case(B, T, C, G)
        wt = R.posconv_wt(W, G)
        xd, wtd, biasd = x.to(dev), wt.to(dev), bias.to(dev)
        for pad in pads:
            refs = R.posconv_refs(x, wt, bias, pad)
            for has_bias in (False, True):
                what = f"C {C} G {G} T {T} pad {pad} bias {has_bias}"
                y = _posconv(xd, wtd, biasd if has_bias else None, B, T, C, G, pad, what)
                _check(y, *refs[has_bias], f"posconv.{C // G}", what)


@pytest.mark.parametrize("pad", [64, 63, 0, 127])
@pytest.mark.parametrize("C,G", [(96, 2), (128, 2)])
def test_posconv_small(C, G, pad):
    """CG = 48 and 64, B = 3, T around the 16-row tile (1, 15, 16, 17) and the 208-row time block (207,
    208, 209; 417 = three blocks, the third with one row), with the bias and with bias == NULL."""
    _posconv_cases(C, G, (1, 15, 16, 17, 207, 208, 209, 417), (pad,))


@pytest.mark.parametrize("C,G", [(768, 16), (1024, 16)])
def test_posconv_wide(C, G):
    """HuBERT-base and -large widths (16 groups: the group offsets and row strides of production), one
    and two time blocks, every pad, with the bias and with bias == NULL."""
    _posconv_cases(C, G, (199, 209), (64, 63, 0, 127))


@pytest.mark.parametrize("C,G", [(96, 2), (128, 2)])
def test_posconv_zero_fill_isolates_the_samples(C, G):
    """Samples 0 and 2 entirely NaN: sample 1, whose windows reach up to 127 rows past either end, must
    come out finite and within its bound (rows outside [0, T) are zeros, not the neighbours' rows)."""
    B = 3
    for T in (15, 209, 417):
        x, _, W, bias = R.posconv_case(B, T, C, G)
        wt = R.posconv_wt(W, G)
        xn = x.clone()
        xn[0] = NAN
        xn[2] = NAN
        for pad in (64, 63, 0, 127):
            what = f"C {C} G {G} T {T} pad {pad} NaN neighbours"
            y = _posconv(xn.to(dev), wt.to(dev), None, B, T, C, G, pad, what)
            ref, bound = R.posconv_ref(x[1:2], wt, None, pad)
            _check(y[1:2], ref, bound, f"posconv.{C // G}", what)
            assert _all_nan(y[0]) and _all_nan(y[2]), what


# ---- triad_posconv_dw -----------------------------------------------------------------------------

def _posconv_dw(C, G, T, B, splits, pad):
    L = _lib()
    what = f"C {C} G {G} T {T} B {B} splits {splits} pad {pad}"
    CG = C // G
    x, dy, _, _ = R.posconv_case(B, T, C, G)
    n = splits * G * R.KT * CG * CG
    assert L.call("triad_posconv_dw_part_bytes", C, G, splits) == 4 * n
    part = _nan(n + GUARD)
    xd, dyd = x.to(dev), dy.to(dev)
    L.call("triad_posconv_dw", _at(xd), _at(dyd), B, T, C, G, pad, splits, _at(part), L.stream_ptr())
    assert _all_nan(part[n:]), what + ": wrote past the slabs"
    slabs = part[:n].view(splits, G, R.KT, CG, CG)
    sref, sbound, ref, bound = R.posconv_dw_ref(x, dy, G, pad, splits)
    used = R.dw_used_splits(B, splits)
    assert bool(torch.isfinite(slabs).all()), what + ": slab elements left unwritten"
    _check(slabs[:used], sref, sbound, "posconv_dw.slab", what)
    assert not bool(slabs[used:].view(torch.int32).any()), what + ": a split without samples did not write +0"
    total = _nan(n // splits + GUARD)
    L.call("triad_sum_slabs", _at(part), splits, n // splits, None, 0, _at(total), L.stream_ptr())
    assert _all_nan(total[n // splits:]), what + ": the slab sum wrote past its end"
    _check(total[:n // splits].view(G, R.KT, CG, CG), ref, bound, "posconv_dw.sum", what)


@pytest.mark.parametrize("B,splits", [(1, 1), (5, 2), (3, 16)])
@pytest.mark.parametrize("pad", [64, 0])
def test_posconv_dw_small(B, splits, pad):
    """C = 96 in 2 groups, T around the 32-row k-step (1, 31, 32, 33) and the 224-row block step (223,
    224, 225: the third with a last k-step of one row; 300); 13 of 16 splits without a sample must write
    zero slabs over the NaN. Each split's slab, then their sum through triad_sum_slabs."""
    for T in (1, 31, 32, 33, 223, 224, 225, 300):
        _posconv_dw(96, 2, T, B, splits, pad)


@pytest.mark.parametrize("T,B,splits,pad", [(33, 1, 1, 64), (33, 5, 2, 0), (33, 3, 16, 64), (225, 5, 2, 64),
                                            (225, 3, 16, 0)])
def test_posconv_dw_wide(T, B, splits, pad):
    """HuBERT-base's 768 channels in 16 groups (the group offset and the row stride of production) at one
    and two block steps; the other lengths repeat test_posconv_dw_small's paths per group."""
    _posconv_dw(768, 16, T, B, splits, pad)


# ---- frontend._PosConv / frontend._Conv0GNGelu ----------------------------------------------------

@pytest.mark.parametrize("C,G", [(96, 2), (128, 2)])
def test_posconv_module_vs_fp64(C, G):
    """_PosConv forward + backward (B = 3, T = 209, padding 64) against the fp64 Conv1d of the bf16
    operands: y, dx (the input-gradient form with the flipped weights as _PosConv.backward builds them),
    and at 48 channels per group dW (triad_posconv_dw + triad_sum_slabs, min(B, 16) splits) and db."""
    import torch.nn.functional as F
    from triad_amd.frontend import _PosConv
    B, T = 3, 209
    x, dy, W, bias = R.posconv_case(B, T, C, G)
    hip_dw = C // G == 48
    xd = x.to(dev).requires_grad_(True)
    Wd = W.float().to(dev).requires_grad_(hip_dw)      # an fp32 leaf: dW comes back as fp32
    bd = bias.to(dev).requires_grad_(hip_dw)
    y = _PosConv.apply(xd, Wd, bd, G, 64)
    grads = torch.autograd.grad((y.float() * dy.to(dev).float()).sum(), (xd, Wd, bd) if hip_dw else (xd,))
    xr, Wr, br = x.double().requires_grad_(True), W.double().requires_grad_(True), bias.double().requires_grad_(True)
    yr = F.conv1d(xr.transpose(1, 2), Wr, br, padding=64, groups=G)[:, :, :-1].transpose(1, 2)
    rx, rW, rb = torch.autograd.grad((yr * dy.double()).sum(), (xr, Wr, br))
    ref, bound = R.posconv_ref(x, R.posconv_wt(W, G), bias, 64)
    assert float((ref - yr.detach()).abs().max()) < 1e-12
    _check(y.detach(), ref, bound, "PosConv.y", f"C {C}")
    dref, dbound = R.posconv_ref(dy, R.posconv_wt_bwd(W, G), None, 63)
    assert float((dref - rx).abs().max()) < 1e-12
    _check(grads[0], dref, dbound, "PosConv.dx", f"C {C}")
    if hip_dw:
        _, _, wref, wbound = R.posconv_dw_ref(x, dy, G, 64, min(B, 16))
        assert float((R.posconv_dw_to_weight(wref) - rW).abs().max()) < 1e-10
        _check(grads[1].float(), rW, R.posconv_dw_to_weight(wbound), "PosConv.dW", f"C {C}")
        # db: an fp32 column sum of B T bf16 values in any order
        _check(grads[2], rb, 2.0 * (B * T + 2) * R.U * dy.double().abs().sum((0, 1)), "PosConv.db", f"C {C}")


@pytest.mark.parametrize("C,T", [(64, 129), (512, 128)])
def test_conv0_module_vs_fp64_chain(C, T):
    """_Conv0GNGelu forward + backward (B = 2; Tp = T rounded up to even): the module returns bit for bit
    what the entry points return when called directly, and that chain -- y0out (bf16), mean / rstd, out,
    then dy0 (bf16), dgamma, dbeta from the kernel's y0out and statistics, then dW0 from the kernel's
    dy0 -- stays within the fp64 references' bounds at every stage."""
    from triad_amd.frontend import _Conv0GNGelu
    B, Tp = 2, T + (T & 1)
    what = f"C {C} T {T} Tp {Tp}"
    wave, w0, gamma, beta, dy = R.conv0_case(B, T, Tp, C, fill=0.25)
    L_in = 5 * (T - 1) + 10 + (3 if Tp > T else 0)        # the module pads the waveform to 5 (Tp - 1) + 10 itself
    waved = wave[:, :L_in].to(dev)
    wd = w0.to(dev).float().view(C, 1, 10).requires_grad_(True)
    gd, bd = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    out = _Conv0GNGelu.apply(waved.float(), wd, gd, bd, EPS, Tp)
    gy = torch.zeros(B * Tp + 2, C, dtype=BF, device=dev)
    gy[:B * Tp] = dy.to(dev).view(B * Tp, C)
    dW, dg, db = torch.autograd.grad((out.float() * gy.float()).sum(), (wd, gd, bd))
    # the same entry points, directly
    xw = torch.zeros(B, 5 * (Tp - 1) + 10, dtype=BF)
    xw[:, :L_in] = wave[:, :L_in]
    xwd, w0d, g0, b0 = xw.to(dev), w0.to(dev), gamma.to(dev), beta.to(dev)
    out2, y0, mean, rstd = _c0gn(xwd, w0d, B, T, Tp, C, g0, b0, what)
    assert torch.equal(out[:B * Tp].view(torch.int16), out2.reshape(B * Tp, C).view(torch.int16)), what + ": out"
    assert not bool(out[B * Tp:].view(torch.int16).any()), what + ": the two spare frames are not zero"
    _y0_check(y0, xw, w0, T, what)
    _chgn_forward_checks(y0.cpu(), T, gamma, beta, out2, mean, rstd, "Conv0GNGelu", what)
    mean, rstd, y0 = mean.contiguous(), rstd.contiguous(), y0.contiguous()
    dy0, dg2, db2 = _chgn_bwd(y0, dy.to(dev), B, T, Tp, C, g0, b0, mean, rstd, what)
    dW2 = _conv0_dw(xwd, dy0.contiguous(), B, T, Tp, C, what)
    assert torch.equal(dg, dg2) and torch.equal(db, db2) and torch.equal(dW.view(C, 10), dW2), what + ": gradients"
    wantb = R.chgn_bwd_ref(y0.cpu(), dy, T, gamma, beta, mean.cpu(), rstd.cpu())
    _check(dy0[:, :T], *wantb["dx"], "Conv0GNGelu.dy0", what)
    _check(dg, *wantb["dgamma"], "Conv0GNGelu.dgamma", what)
    _check(db, *wantb["dbeta"], "Conv0GNGelu.dbeta", what)
    _check(dW.view(C, 10), *R.conv0_dw_ref(xw, dy0.cpu(), T), "Conv0GNGelu.dW0", what)


# ---- batch isolation of the padded frame stack ------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _encoder():
    import transformers
    from triad_amd import frontend
    torch.manual_seed(0)
    m = transformers.HubertModel(transformers.HubertConfig())
    frontend.install_hubert_frontend(m)
    return m.feature_extractor.to(dev).train()


@pytest.mark.parametrize("B,L", [(4, 645), (2, 16000)])
def test_frame_stack_isolates_the_samples(B, L):
    """HuBERT's feature encoder over padded frame buffers under bf16 autocast. L = 645: T0 = 128 and the
    seven layers' Tp are 128, 64, .., 2 (layer 1 on the HIP overlapping-row GEMM at M = 256, the later
    ones on the torch route); L = 16000: 3199 frames in 3200. With the other samples replaced by other
    waveforms, sample 1's valid output frames are bit-identical, and with the output gradient nonzero on
    sample 1 only, so are every conv weight's gradient and conv0's gamma / beta gradients: a row's
    GEMM result depends on its own operands only and zero dy rows contribute exact zeros, unless a
    straddling padding row carries data or gradient into a neighbour."""
    from triad_amd import frontend
    fe = _encoder()
    g = torch.Generator().manual_seed(L)
    a = torch.randn(B, L, generator=g) * 0.5
    b = torch.randn(B, L, generator=g) * 0.5
    b[1] = a[1]
    assert frontend._frame_stack_plan(fe, a.to(BF).to(dev)) is not None
    results = []
    for wave in (a, b):
        fe.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF):
            out = fe(wave.to(dev))            # (B, C, T) view of channels-last storage
        gy = torch.zeros_like(out, dtype=F32)
        gy[1] = torch.randn(out.shape[1:], generator=torch.Generator().manual_seed(7)).to(dev)
        (out.float() * gy).sum().backward()
        grads = {n: p.grad.clone() for n, p in fe.named_parameters()}
        assert all(bool(torch.isfinite(v).all()) for v in grads.values()) and bool(torch.isfinite(out).all())
        results.append((out[1].detach().clone(), grads))
    (o1, g1), (o2, g2) = results
    assert bool((a[0] != b[0]).any()) and len(g1) == 7 + 2
    assert torch.equal(o1, o2), "sample 1's output frames depend on the other samples"
    for n in g1:
        assert bool(g1[n].any()), n
        assert torch.equal(g1[n], g2[n]), f"{n}: sample 1's gradient contribution depends on the other samples"
