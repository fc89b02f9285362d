"""The checks of tests/test_frontend_conformance_gpu.py bite: for each kernel of csrc/frontend.hip and
csrc/posconv.hip a plain-torch fp32 emulation with the kernel's rounding points and summation
grouping (tests/frontend_ref.py) passes the fp64 reference's per-element bound, and the same
emulation with one planted error fails it. No device.

Every planted error the issue lists is seen by a bound, two of them only where stated:
* a CHUNK of 1024 instead of 128 is invisible to the general statistics bound (a worst-case h u
  bound; the emulation's error is far inside it at either depth) and invisible up to T of about 400
  even on the mean-100 channel (sum x^2 ~ 10 000 T < 2^24 * 0.25 is still exact). It is seen on the
  mean-100 channel beyond that, where a 1024-deep fp32 sum of x^2 leaves the 0.25 grid: the case
  here uses T = 640.
* tanh-GELU differs from erf-GELU by a few 1e-4 at most, inside 2^-8 |ref| wherever |gelu| is not
  small; it is seen in the negative tail (z in -4 .. -2: |gelu| < 0.05, difference up to 4e-4).
"""
import pytest
import torch
import torch.nn.functional as F

from tests import frontend_ref as R

EPS = R.f32(1e-5)
JUNK = 3.0   # finite content of the padding frames, so that a read of them shows as an error and not as NaN


def _sel(pair, idx):
    return pair[0][idx], pair[1][idx]


# ---- GroupNorm + GELU forward ---------------------------------------------------------------------

@pytest.mark.parametrize("C", [8, 64, 512, 2048])
def test_chgn_forward_bounds(C):
    B, T, Tp = 2, 300, 303
    x, _, gamma, beta = R.chgn_case(B, T, Tp, C, fill=JUNK)
    want = R.chgn_fwd_ref(x, T, gamma, beta, EPS)
    y, mean, rstd = R.emul_chgn_fwd(x, T, gamma, beta, EPS)
    assert R.passes(mean, *want["mean"]) and R.passes(rstd, *want["rstd"]) and R.passes(y[:, :T], *want["y"])
    assert not bool(y[:, T:].any())
    # statistics over the Tp frames of the buffer
    y1, mean1, rstd1 = R.emul_chgn_fwd(x, T, gamma, beta, EPS, stats_over_tp=True)
    assert not R.passes(mean1, *want["mean"]) and not R.passes(rstd1, *want["rstd"])
    assert not R.passes(y1[:, :T], *want["y"])
    # tanh-GELU: seen in the negative tail
    y2, _, _ = R.emul_chgn_fwd(x, T, gamma, beta, EPS, tanh=True)
    assert not R.passes(y2[:, :T], *want["y"])


def test_chgn_forward_special_channels():
    B, T, Tp, C = 2, 300, 303, 64
    x, _, gamma, beta = R.chgn_case(B, T, Tp, C, fill=JUNK)
    want = R.chgn_fwd_ref(x, T, gamma, beta, EPS)
    k100, kc = R.SPECIAL["mean100"], R.SPECIAL["const"]
    assert bool(want["exact"][:, k100].all()) and bool(want["exact"][:, kc].all())
    assert not bool(want["exact"][:, :8].any())          # N(0.3, 1.5) channels take the general bound
    y, mean, rstd = R.emul_chgn_fwd(x, T, gamma, beta, EPS)
    assert bool((mean[:, kc] == R.CONST).all())
    assert R.passes(rstd[:, kc], *_sel(want["rstd"], (slice(None), kc)))
    gb = R.gelu64(torch.tensor(R.CONST_BETA, dtype=R.F64))
    assert float(R.bf16_flip(gb, 2.0 ** -16 * gb)[1]) == 0.0     # far from a rounding boundary
    assert bool((y[:, :T, kc].double() == gb.to(R.F32).to(R.BF).double()).all())
    # the finalize in fp32: fails on the mean-100 channel, in rstd and in y
    y1, _, rstd1 = R.emul_chgn_fwd(x, T, gamma, beta, EPS, finalize_f32=True)
    assert not R.passes(rstd1[:, k100], *_sel(want["rstd"], (slice(None), k100)))
    assert not R.passes(y1[:, :T, k100], *_sel(want["y"], (slice(None), slice(None), k100)))


def test_chgn_forward_chunk_depth_is_seen_on_the_mean_100_channel():
    B, T, C = 1, 640, 64
    x, _, gamma, beta = R.chgn_case(B, T, T, C)
    want = R.chgn_fwd_ref(x, T, gamma, beta, EPS)
    k = R.SPECIAL["mean100"]
    assert bool(want["exact"][:, k].all())
    _, mean, rstd = R.emul_chgn_fwd(x, T, gamma, beta, EPS)
    assert R.passes(mean, *want["mean"]) and R.passes(rstd, *want["rstd"])
    _, _, rstd1 = R.emul_chgn_fwd(x, T, gamma, beta, EPS, chunk=1024)
    assert not R.passes(rstd1[:, k], *_sel(want["rstd"], (slice(None), k)))
    others = [c for c in range(C) if c != k]
    assert R.passes(rstd1[:, others], *_sel(want["rstd"], (slice(None), others)))   # invisible elsewhere


# ---- GroupNorm + GELU backward --------------------------------------------------------------------

@pytest.mark.parametrize("C", [8, 64, 512])
def test_chgn_backward_bounds(C):
    B, T, Tp = 2, 300, 303
    x, dy, gamma, beta = R.chgn_case(B, T, Tp, C, fill=JUNK)
    _, mean, rstd = R.emul_chgn_fwd(x, T, gamma, beta, EPS)
    want = R.chgn_bwd_ref(x, dy, T, gamma, beta, mean, rstd)

    def ok(out):
        return [R.passes(out[0][:, :T], *want["dx"]), R.passes(out[1], *want["dgamma"]), R.passes(out[2], *want["dbeta"])]

    good = R.emul_chgn_bwd(x, dy, T, gamma, beta, mean, rstd)
    assert ok(good) == [True, True, True]
    assert not bool(good[0][:, T:].any())
    if C == 64:
        kc = R.SPECIAL["const"]
        assert float(want["dx"][0][:, :, kc].abs().max()) < 1e-9       # the constant channel's dx is 0 ..
        assert R.passes(good[0][:, :T, kc], *_sel(want["dx"], (slice(None), slice(None), kc)))   # .. up to its bound
    assert ok(R.emul_chgn_bwd(x, dy, T, gamma, beta, mean, rstd, no_cA=True)) == [False, True, True]
    assert ok(R.emul_chgn_bwd(x, dy, T, gamma, beta, mean, rstd, no_cB=True)) == [False, True, True]
    assert ok(R.emul_chgn_bwd(x, dy, T, gamma, beta, mean, rstd, swap_params=True)) == [True, False, False]
    assert ok(R.emul_chgn_bwd(x, dy, T, gamma, beta, mean, rstd, drop_chunk=1)) == [False, False, False]
    assert ok(R.emul_chgn_bwd(x, dy, T, gamma, beta, mean, rstd, drop_row=T - 1)) == [False, False, False]


# ---- conv0 ----------------------------------------------------------------------------------------

def test_conv0_flip_allowance_and_planted_taps():
    B, T, C = 2, 300, 64
    wave, w0, _, _, _ = R.conv0_case(B, T, T + 1, C, fill=0.0)
    ref, gap = R.conv0_ref(wave, w0, T)
    assert float((gap > 0).double().mean()) <= 0.02
    assert R.passes(R.emul_conv0(wave, w0, T), ref, gap)
    assert not R.passes(R.emul_conv0(wave, w0, T, reverse_taps=True), ref, gap)
    assert not R.passes(R.emul_conv0(wave, w0, T, stride=4), ref, gap)


@pytest.mark.parametrize("C,T", [(64, 1025), (512, 2100)])
def test_conv0_dw_bound(C, T):
    B = 2
    wave, _, _, _, dy0 = R.conv0_case(B, T, T + 1, C, fill=0.0)
    ref, bound = R.conv0_dw_ref(wave, dy0, T)
    assert R.passes(R.emul_conv0_dw(wave, dy0, T), ref, bound)
    assert not R.passes(R.emul_conv0_dw(wave, dy0, T, late_window=True), ref, bound)
    nblk = -(-T // 1024)
    for slab in (0, nblk - 1, B * nblk - 1):      # the last slab of T = 1025 holds one row
        assert not R.passes(R.emul_conv0_dw(wave, dy0, T, drop_slab=slab), ref, bound), slab


# ---- positional conv ------------------------------------------------------------------------------

def _conv1d_grads(x, dy, W, bias, G):
    """fp64 autograd of HuBERT's positional conv (padding 64, last output dropped)."""
    xr = x.double().requires_grad_(True)
    Wr = W.double().requires_grad_(True)
    y = F.conv1d(xr.transpose(1, 2), Wr, bias.double(), padding=64, groups=G)[:, :, :-1].transpose(1, 2)
    dx, dW = torch.autograd.grad((y * dy.double()).sum(), (xr, Wr))
    return y.detach(), dx, dW


@pytest.mark.parametrize("C,G", [(96, 2), (128, 2)])
def test_posconv_bounds(C, G):
    B, T = 3, 209
    x, dy, W, bias = R.posconv_case(B, T, C, G)
    wt = R.posconv_wt(W, G)
    ref, bound = R.posconv_ref(x, wt, bias, 64)
    y64, dx64, _ = _conv1d_grads(x, dy, W, bias, G)
    assert float((ref - y64).abs().max()) < 1e-12            # the reference is the module's conv
    assert R.passes(R.emul_posconv(x, wt, bias, 64), ref, bound)
    for plant in ("neighbours", "keep_last", "late_block", "bias_twice"):
        assert not R.passes(R.emul_posconv(x, wt, bias, 64, **{plant: True}), ref, bound), plant
    # the input-gradient form: flipped, transposed weights and pad 63
    wtb = R.posconv_wt_bwd(W, G)
    dref, dbound = R.posconv_ref(dy, wtb, None, 63)
    assert float((dref - dx64).abs().max()) < 1e-12
    assert R.passes(R.emul_posconv(dy, wtb, None, 63), dref, dbound)
    assert not R.passes(R.emul_posconv(dy, wtb, None, 64), dref, dbound)
    assert not R.passes(R.emul_posconv(dy, R.posconv_wt_bwd(W, G, flip=False), None, 63), dref, dbound)


@pytest.mark.parametrize("B,splits", [(3, 2), (3, 16)])
def test_posconv_dw_bounds(B, splits):
    C, G, T = 96, 2, 300
    x, dy, W, bias = R.posconv_case(B, T, C, G)
    sref, sbound, ref, bound = R.posconv_dw_ref(x, dy, G, 64, splits)
    _, _, dW = _conv1d_grads(x, dy, W, bias, G)
    assert float((R.posconv_dw_to_weight(ref) - dW).abs().max()) < 1e-10
    slabs, total = R.emul_posconv_dw(x, dy, G, 64, splits)
    used = R.dw_used_splits(B, splits)
    assert used == (2 if splits == 2 else B)
    assert R.passes(slabs[:used], sref, sbound) and R.passes(total, ref, bound)
    assert not bool(slabs[used:].any())                               # splits past the samples: zero slabs
    for row in ((0, 0), (B - 1, T - 1), (1, 224)):
        assert not R.passes(R.emul_posconv_dw(x, dy, G, 64, splits, drop_row=row)[1], ref, bound), row
    assert not R.passes(R.emul_posconv_dw(x, dy, G, 64, splits, shift_step=True)[1], ref, bound)
    bad, badsum = R.emul_posconv_dw(x, dy, G, 64, splits, drop_slab=1)
    assert not R.passes(bad[:used], sref, sbound) and not R.passes(badsum, ref, bound)
