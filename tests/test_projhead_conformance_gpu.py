"""Conformance of the projection-head kernels through the C ABI (`triad_amd._lib.call`): the row-panel
GEMMs of csrc/rowgemm.hip -- triad_projhead_fwd, triad_projhead_ln_fwd, triad_rowgemm_bias,
triad_projhead_ln_bwd, triad_wpack / triad_wpack2 -- and the passes of csrc/projhead.hip --
triad_ln_fwd, triad_ln_bwd3, triad_sum_slabs, triad_colsum_dma -- and of the wrapper
ops.projection_head over both forms.

Operands come from a seeded CPU generator (tests/projhead_ref.py, which also holds the fp64
references, the bounds with their derivation and the shape lists; tests/test_projhead_checks_cpu.py
shows that each bound passes an emulation of its kernel and that each planted error fails one). Every
output buffer is NaN-filled; row outputs carry 4 NaN guard rows past the padded row count 128 P and
part a NaN guard tail, unchanged afterwards; inputs documented as [M] rows (h, dy, the backward's y1 /
mean / rstd) are followed by NaN rows, which the kernels must never read; results must be finite
before they are compared; pad rows M .. 128 P - 1 must be exact zeros. Each stage is referenced from
the operands that stage read: mean / rstd / ln from the kernel's own y1, y from its own ln, dy1 and
the partials from its own dln.

The epilogue's internal dln = bf16(dy W2) is obtained as triad_rowgemm_bias(dy, W2p_bwd, zero bias):
as read from rowgemm.hip, EPI 0 and EPI 2 share the k loop (same instantiation-independent code before
the epilogue branch) and EPI 0 adds an exact 0.0 before the same rounding, so it is the epilogue's dln
bit for bit. triad_projhead_ln_bwd runs with the pad rows of y1 / mean / rstd NaN: it reads none of them.

Identities asserted exactly: fused forward == ln_fwd + rowgemm_bias; every strided layout == the
contiguous one; repeats; triad_wpack2 == two triad_wpack == the index formula; triad_bfrag_pack16(W2,
dk = 1) == the formula on W2^T; the wrapper's fall-back inputs == the in-place "rows" form.

Largest err / bound per group on MI355X (88 cases, 3 s in all; also in DESIGN.md section 2). bf16
outputs, where the one rounding fills its 2^-8 term: fwd y1 0.987, ln 0.996, y 0.930; bwd dln 0.909,
dy1 0.996; ln_fwd ln 0.996; ln_bwd3 dy1 0.996; sum_slabs bf16 0.994 (reduce) / 0.996 (stream);
colsum_dma bf16 0.988; wrapper y1 0.778, ln 0.995, y 0.875. fp32 outputs: fwd mean 0.004, rstd 0.099;
bwd part dgamma 0.542 (the one-row panel, where only the roundings of xh count), dbeta 0.003, db1 0.005,
totals 0.542 / 0.002 / 0.003; ln_fwd mean 0.104, rstd 0.147; ln_bwd3 part dgamma 0.586, dbeta 0.328,
db1 0.315 (blocks of two rows: one add), totals 0.586 / 0.002 / 0.002; sum_slabs fp32 0.151 (reduce) /
0.492 (stream); colsum_dma fp32 0.311; wrapper mean 0.005, rstd 0.124. The any-order partial bounds
of a 128-row panel are loose against the kernel's 12-deep order (0.003 .. 0.02), as they are against
the CPU emulation of the same cases (0.003 / 0.005 / 0.02); a pad row counted into dbeta or dgamma
summed from g still exceeds them by factors above 10^5 (CPU file). Wrapper gradients against fp64
autograd: 2.4e-3 .. 3.8e-3 relative L2 (bar 1e-2). Every identity held. The backward test fails on the
kernel as it was before the pad rows were selected at the loads: NaN pad rows of dy1 at M = 1, 127,
129, 300, the first assertion it reaches (as read from the code, 0 * NaN poisons the last panel's
dgamma and db1 partials the same way); M = 128 has no pad row and passes. No other kernel defect was
found.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn as nn

from tests import projhead_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
D = R.D
EPS = R.f32(R.EPS)
GUARD = 64     # NaN elements past the end of a flat output
GROWS = 4      # NaN rows past the last row of a row buffer
WORST = {}     # group -> largest err / bound of this run


def _lib():
    from triad_amd import _lib
    return _lib


def _at(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _nan(shape, dt):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), NAN, dtype=dt, device=dev)


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _with_nan_rows(t, rows):
    """t's rows in a device buffer of `rows` + GROWS rows, NaN past t's own."""
    out = _nan((rows + GROWS,) + tuple(t.shape[1:]), t.dtype)
    out[:t.shape[0]] = t.to(dev)
    return out


def _check(got, ref, bound, group, what):
    got = got.cpu()
    assert bool(torch.isfinite(got).all()), f"{group} {what}: non-finite output (unwritten or poisoned elements)"
    r = R.ratio(got, ref, bound)
    WORST[group] = max(WORST.get(group, 0.0), r)
    print(f"{group} {what}: err/bound {r:.4f}")
    assert r <= 1.0, f"{group} {what}: err/bound {r}"


def _rows_out(M, outs, what):
    """Guard rows still NaN, pad rows exact zeros; the tensors cut to the padded row count."""
    Mp = R.panels(M) * 128
    res = []
    for t in outs:
        assert _all_nan(t[Mp:]), what + ": wrote past the padded rows"
        assert bool(torch.isfinite(t[:M]).all()), what + ": valid rows not finite"
        assert not bool(t[M:Mp].float().abs().sum()) and not bool(torch.isnan(t[M:Mp]).any()), what + ": pad rows not zero"
        res.append(t[:Mp])
    return res


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nprojection-head kernels, largest err/bound per group:",
          ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))


# ---- forward: triad_projhead_fwd, triad_projhead_ln_fwd + triad_rowgemm_bias ----------------------------

@functools.lru_cache(maxsize=4)
def _weights(M, H):
    """The case on the CPU, its weights on the device, packed by triad_wpack2."""
    L = _lib()
    c = R.head_case(M, H)
    d = {k: c[k].to(dev) for k in ("W1", "b1", "W2", "b2", "gamma", "beta")}
    d["W1p"], d["W2p"] = _nan(H * D + GUARD, BF), _nan(D * D + GUARD, BF)
    L.call("triad_wpack2", _at(d["W1"]), H, _at(d["W1p"]), _at(d["W2"]), D, _at(d["W2p"]), L.stream_ptr())
    assert _all_nan(d["W1p"][H * D:]) and _all_nan(d["W2p"][D * D:])
    return c, d


def _forward(d, hbuf, off, M, H, lda, n_per, bstride, fused):
    """(y1, ln, mean, rstd, y) cut to 128 P rows, from NaN-filled buffers with guard rows."""
    L = _lib()
    Mp = R.panels(M) * 128
    assert L.call("triad_rowpanel_count", M) == R.panels(M)
    y1, ln, y = (_nan((Mp + GROWS, D), BF) for _ in range(3))
    mean, rstd = _nan(Mp + GROWS, F32), _nan(Mp + GROWS, F32)
    st = L.stream_ptr()
    if fused:
        L.call("triad_projhead_fwd", _at(hbuf, off), M, H, lda, n_per, bstride, _at(d["W1p"]), _at(d["b1"]),
               _at(d["gamma"]), _at(d["beta"]), R.EPS, _at(d["W2p"]), _at(d["b2"]), _at(y1), _at(ln), _at(mean),
               _at(rstd), _at(y), st)
    else:
        L.call("triad_projhead_ln_fwd", _at(hbuf, off), M, H, lda, n_per, bstride, _at(d["W1p"]), _at(d["b1"]),
               _at(d["gamma"]), _at(d["beta"]), R.EPS, _at(y1), _at(ln), _at(mean), _at(rstd), st)
        L.call("triad_rowgemm_bias", _at(ln), M, D, D, _at(d["W2p"]), _at(d["b2"]), _at(y), st)
    return _rows_out(M, (y1, ln, mean, rstd, y), f"forward M {M} H {H} fused {fused}")


def _check_forward(c, outs, M, what):
    y1, ln, mean, rstd, y = (t[:M].cpu() for t in outs)
    _check(y1, *R.gemm_bias_ref(c["h"], c["W1"], c["b1"]), "fwd.y1", what)
    want = R.ln_fwd_ref(y1, c["gamma"], c["beta"], EPS, R.H_PANEL)
    _check(mean, *want["mean"], "fwd.mean", what)
    _check(rstd, *want["rstd"], "fwd.rstd", what)
    _check(ln, *want["ln"], "fwd.ln", what)
    _check(y, *R.gemm_bias_ref(ln, c["W2"], c["b2"]), "fwd.y", what)


def _same(a, b):
    return all(torch.equal(x, z) for x, z in zip(a, b))


@pytest.mark.parametrize("M,H", R.FWD_CASES)
def test_forward(M, H):
    """H = 32 .. 224 at M = 129: nkt = 1, 2, 3 (no whole ring group, the TAIL stages alone), 4 (one group,
    no tail), 5, 6, 7 (a group and each tail); 768 / 1024 the model's own; M around one panel and 300
    (three panels, a ragged last one). h is followed by NaN rows. Every stage per element; the fused
    kernel == its two halves; a repeat is bit-identical."""
    c, d = _weights(M, H)
    hbuf = _with_nan_rows(c["h"], M)
    fused = _forward(d, hbuf, 0, M, H, H, M, 0, True)
    _check_forward(c, fused, M, f"M {M} H {H}")
    assert _same(fused, _forward(d, hbuf, 0, M, H, H, M, 0, False)), "fused forward != ln_fwd + rowgemm_bias"
    assert _same(fused, _forward(d, hbuf, 0, M, H, H, M, 0, True)), "repeat differs"


@pytest.mark.parametrize("H", R.ADDR_HS)
def test_forward_row_addressing(H):
    """M = 150 rows as contiguous, lda = H + 8, two-level (3 samples of n_per = 50 behind 5 prefix rows,
    bstride = 55 lda) and n_per = 1; prefix, gap and trailing elements NaN. Each against the
    references, fused == halves, and every layout == the contiguous one bit for bit."""
    M = R.ADDR_M
    c, d = _weights(M, H)
    base = None
    for form in R.ADDR_FORMS:
        buf, off, lda, n_per, bstride = R.strided_rows(c["h"], form)
        hbuf = torch.cat([buf, torch.full((GROWS * lda,), NAN, dtype=BF)]).to(dev)
        fused = _forward(d, hbuf, off, M, H, lda, n_per, bstride, True)
        _check_forward(c, fused, M, f"M {M} H {H} {form}")
        assert _same(fused, _forward(d, hbuf, off, M, H, lda, n_per, bstride, False)), form
        if base is None:
            base = fused
        assert _same(fused, base), f"{form}: differs from the contiguous layout"


# ---- backward: triad_projhead_ln_bwd ------------------------------------------------------------------

def _pack_w2_bwd(W2d):
    L = _lib()
    Bp = _nan(D * D + GUARD, BF)
    L.call("triad_bfrag_pack16", _at(W2d), D // 32, 1, _at(Bp), L.stream_ptr())
    assert _all_nan(Bp[D * D:])
    return Bp


@pytest.mark.parametrize("M", R.BWD_MS)
def test_backward(M):
    """y1 / mean / rstd built on the host (the fp64 statistics rounded to fp32), their pad rows and the
    rows after dy NaN. dln (the bias-free row GEMM, see the module docstring) against the fp64 GEMM;
    dy1, every panel's three partials and the totals from that dln; pad rows of dy1 zero; a repeat is
    bit-identical."""
    L = _lib()
    c = R.bwd_case(M)
    P = R.panels(M)
    Mp = P * 128
    st = L.stream_ptr()
    W2p = _pack_w2_bwd(c["W2"].to(dev))
    assert torch.equal(W2p[:D * D].cpu(), R.wpack_ref(c["W2"].t().contiguous())), "bfrag_pack16(dk = 1) != formula"
    dy = _with_nan_rows(c["dy"], M)
    y1 = _with_nan_rows(c["y1"], Mp)
    mean, rstd = _with_nan_rows(c["mean"], Mp), _with_nan_rows(c["rstd"], Mp)
    gamma = c["gamma"].to(dev)
    what = f"M {M}"
    dln = _nan((Mp + GROWS, D), BF)
    zero = torch.zeros(D, dtype=BF, device=dev)
    L.call("triad_rowgemm_bias", _at(dy), M, D, D, _at(W2p), _at(zero), _at(dln), st)
    dln = _rows_out(M, (dln,), "dln " + what)[0][:M].cpu()
    _check(dln, *R.gemm_bias_ref(c["dy"], c["W2"].t().contiguous()), "bwd.dln", what)
    runs = []
    for _ in range(2):
        dy1, part = _nan((Mp + GROWS, D), BF), _nan(P * 3 * D + GUARD, F32)
        L.call("triad_projhead_ln_bwd", _at(dy), M, _at(W2p), _at(y1), _at(mean), _at(rstd), _at(gamma), _at(dy1),
               _at(part), st)
        assert _all_nan(part[P * 3 * D:]), what + ": wrote past part[panels][3][512]"
        runs.append((_rows_out(M, (dy1,), "dy1 " + what)[0], part[:P * 3 * D].view(P, 3, D)))
    (dy1, part), again = runs
    assert bool(torch.isfinite(part).all()), what + ": partials not finite (poisoned by a pad row?)"
    assert _same((dy1, part), again), what + ": repeat differs"
    dy1c, part = dy1[:M].cpu(), part.cpu()
    want = R.ln_bwd_ref(dln, c["y1"], c["mean"], c["rstd"], c["gamma"], R.H_PANEL, R.row_groups_panel(M), dy1c)
    _check(dy1c, *want["dy1"], "bwd.dy1", what)
    for i, k in enumerate(("dgamma", "dbeta", "db1")):
        _check(part[:, i], *want[k], "bwd.part." + k, what)
        _check(part[:, i].double().sum(0), *want["total." + k], "bwd.total." + k, what)


# ---- the passes form's row kernels -----------------------------------------------------------------------

@pytest.mark.parametrize("M", R.LN_FWD_MS)
def test_ln_fwd(M):
    """One wave, a partial block, a full block, one past it, 130, and 16,389 rows: past the 4,096-block
    grid, a second grid-stride trip with a partial tail. y1 is followed by NaN rows."""
    L = _lib()
    c = R.ln_case(M)
    y1 = _with_nan_rows(c["y1"], M)
    ln, mean, rstd = _nan((M + GROWS, D), BF), _nan(M + GROWS, F32), _nan(M + GROWS, F32)
    gamma, beta = c["gamma"].to(dev), c["beta"].to(dev)
    L.call("triad_ln_fwd", _at(y1), M, _at(gamma), _at(beta), R.EPS, _at(ln), _at(mean), _at(rstd), L.stream_ptr())
    for t in (ln, mean, rstd):
        assert _all_nan(t[M:]), f"ln_fwd M {M}: wrote past row M - 1"
    want = R.ln_fwd_ref(c["y1"], c["gamma"], c["beta"], EPS, R.H_WAVE)
    _check(mean[:M], *want["mean"], "ln_fwd.mean", f"M {M}")
    _check(rstd[:M], *want["rstd"], "ln_fwd.rstd", f"M {M}")
    _check(ln[:M], *want["ln"], "ln_fwd.ln", f"M {M}")


@pytest.mark.parametrize("M", R.LN_BWD3_MS)
def test_ln_bwd3(M):
    """nblocks = 1, 2, the wrapper's min(1024, ceil(M / 4)) and ceil(M / 4) + 3 (idle blocks: exact-zero
    partials); M = 4101 at 1024 blocks is a second trip with a partial tail."""
    L = _lib()
    c = R.ln_case(M)
    mean, rstd = R.stats_f32(c["y1"], EPS)
    dv = {k: _with_nan_rows(v, M) for k, v in dict(dln=c["dln"], y1=c["y1"], mean=mean, rstd=rstd).items()}
    gamma = c["gamma"].to(dev)
    for nb in R.ln_bwd3_blocks(M):
        what = f"M {M} nblocks {nb}"
        dy1, part = _nan((M + GROWS, D), BF), _nan(nb * 3 * D + GUARD, F32)
        L.call("triad_ln_bwd3", _at(dv["dln"]), _at(dv["y1"]), _at(dv["mean"]), _at(dv["rstd"]), _at(gamma), M,
               _at(dy1), _at(part), nb, L.stream_ptr())
        assert _all_nan(dy1[M:]) and _all_nan(part[nb * 3 * D:]), what + ": wrote past an output"
        dy1c, pc = dy1[:M].cpu(), part[:nb * 3 * D].view(nb, 3, D).cpu()
        want = R.ln_bwd_ref(c["dln"], c["y1"], mean, rstd, c["gamma"], R.H_WAVE, R.row_groups_bwd3(M, nb), dy1c)
        _check(dy1c, *want["dy1"], "ln_bwd3.dy1", what)
        for i, k in enumerate(("dgamma", "dbeta", "db1")):
            _check(pc[:, i], *want[k], "ln_bwd3.part." + k, what)
            _check(pc[:, i].double().sum(0), *want["total." + k], "ln_bwd3.total." + k, what)
        idle = [b for b in range(nb) if 4 * b >= M]
        assert not bool(pc[idle].abs().sum()), what + ": a block without rows wrote non-zero partials"


@pytest.mark.parametrize("S,n", R.SLAB_CASES)
def test_sum_slabs(S, n):
    """Both kernels (colsum_reduce for S >= 16 and n <= 16384, else the 4-chain stream with its S % 4
    remainder), alpha NULL and a device scalar, fp32 and bf16 out."""
    L = _lib()
    slabs, alpha = R.slab_case(S, n)
    sd, ad = slabs.to(dev), alpha.to(dev)
    for a, ap in ((1.0, None), (float(alpha), ad)):
        for ob in (0, 1):
            out = _nan(n + GUARD, BF if ob else F32)
            L.call("triad_sum_slabs", _at(sd), S, n, _at(ap), ob, _at(out), L.stream_ptr())
            assert _all_nan(out[n:]), f"sum_slabs S {S} n {n}: wrote past out[n]"
            _check(out[:n], *R.sum_slabs_ref(slabs, a, ob), f"sum_slabs.{R.slab_path(S, n)}.{'bf16' if ob else 'f32'}",
                   f"S {S} n {n} alpha {a:.2f}")


@pytest.mark.parametrize("cols", R.COLSUM_COLS)
def test_colsum_dma(cols):
    """rows around the 16-row chunk and the 64 rows of a split, 200 (3 splits of 67 rows: 5 chunks, past
    the 4-slot ring); cols with a masked last tile; ld = cols and cols + 264 with NaN in columns
    [cols, ld) and in the rows past `rows`; alpha = 0.37; both output types."""
    L = _lib()
    alpha = R.f32(0.37)
    for rows in R.COLSUM_ROWS:
        X = R.colsum_case(rows, cols)
        S = L.call("triad_colsum_dma_splits", rows, cols)
        assert S == R.colsum_dma_splits(rows, cols)
        for ld in (cols, cols + 264):
            Xd = _nan((rows + 2, ld), BF)
            Xd[:rows, :cols] = X.to(dev)
            for ob in (0, 1):
                what = f"rows {rows} cols {cols} ld {ld}"
                part, out = _nan(S * cols + GUARD, F32), _nan(cols + GUARD, BF if ob else F32)
                L.call("triad_colsum_dma", _at(Xd), rows, cols, ld, _at(part), 0.37, ob, _at(out), L.stream_ptr())
                assert _all_nan(part[S * cols:]) and _all_nan(out[cols:]), what + ": wrote past an output"
                assert bool(torch.isfinite(part[:S * cols]).all()), what + ": partials not finite"
                _check(out[:cols], *R.colsum_ref(X, alpha, ob), "colsum_dma." + ("bf16" if ob else "f32"), what)


def test_wpack():
    L = _lib()
    st = L.stream_ptr()
    packed = {}
    for K in sorted({k for ks in R.WPACK2_KS for k in ks} | set(R.WPACK_KS)):
        W = R.weight_case(K)
        Wd, Bp = W.to(dev), _nan(K * D + GUARD, BF)
        L.call("triad_wpack", _at(Wd), K, _at(Bp), st)
        assert _all_nan(Bp[K * D:]), K
        assert torch.equal(Bp[:K * D].cpu(), R.wpack_ref(W)), f"wpack K {K} != the index formula"
        packed[K] = Bp[:K * D].clone()
    for K1, K2 in R.WPACK2_KS:
        B1, B2 = _nan(K1 * D + GUARD, BF), _nan(K2 * D + GUARD, BF)
        W1d, W2d = R.weight_case(K1).to(dev), R.weight_case(K2).to(dev)
        L.call("triad_wpack2", _at(W1d), K1, _at(B1), _at(W2d), K2, _at(B2), st)
        assert _all_nan(B1[K1 * D:]) and _all_nan(B2[K2 * D:]), (K1, K2)
        assert torch.equal(B1[:K1 * D], packed[K1]) and torch.equal(B2[:K2 * D], packed[K2]), (K1, K2)


# ---- the wrapper ---------------------------------------------------------------------------------------

def _head(B, N, H):
    g = R._gen(16, B, N, H)
    p1, ln, p2 = nn.Linear(H, D), nn.LayerNorm(D), nn.Linear(D, D)
    with torch.no_grad():
        for p in list(p1.parameters()) + list(p2.parameters()):
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * p.shape[-1] ** -0.5 if p.dim() == 2 else
                    torch.randn(p.shape, generator=g) * 0.1)
        ln.weight.copy_(torch.rand(D, generator=g) + 0.5)
        ln.bias.copy_(torch.randn(D, generator=g) * 0.2)
    h = torch.randn(B, N, H, generator=g).to(BF)
    gy = (torch.randn(B, N, D, generator=g) * 0.01).to(BF)
    return [m.to(dev) for m in (p1, ln, p2)], h, gy


def _run_head(mods, h, gy, form):
    from triad_amd import ops
    for m in mods:
        for p in m.parameters():
            p.grad = None
    hd = h.to(dev).requires_grad_(True)
    y = ops.projection_head(hd, *mods, form=form)
    saved = y.grad_fn.saved_tensors
    y.backward(gy.to(dev).view(y.shape))
    return y.detach(), [hd.grad] + [p.grad.clone() for m in mods for p in m.parameters()], saved


@pytest.mark.parametrize("form", ["rows", "passes"])
@pytest.mark.parametrize("B,N,H", [(2, 65, 768), (1, 1, 1024)])
def test_wrapper(B, N, H, form):
    """y through the per-stage references chained from the tensors the wrapper saved for its backward
    (y1 from h, mean / rstd / ln from that y1, y from that ln); the seven gradients against fp64
    autograd of the unrounded head at the 1e-2 relative-L2 bar of tests/test_projhead_gpu.py."""
    mods, h, gy = _head(B, N, H)
    M = B * N
    y, grads, saved = _run_head(mods, h, gy, form)
    assert y.dtype == BF and y.shape == (B, N, D)
    _, w1b, w2b, g32, y1, ln, mean, rstd = (t.cpu() for t in saved)
    b1b, b2b = mods[0].bias.detach().to(BF).cpu(), mods[2].bias.detach().to(BF).cpu()
    what = f"{form} {B} x {N} x {H}"
    depth = R.H_PANEL if form == "rows" else R.H_WAVE
    _check(y1[:M], *R.gemm_bias_ref(h.reshape(M, H), w1b, b1b), "wrapper.y1", what)
    want = R.ln_fwd_ref(y1[:M], g32, mods[1].bias.detach().float().cpu(), R.f32(mods[1].eps), depth)
    _check(mean[:M], *want["mean"], "wrapper.mean", what)
    _check(rstd[:M], *want["rstd"], "wrapper.rstd", what)
    _check(ln[:M], *want["ln"], "wrapper.ln", what)
    _check(y.reshape(M, D), *R.gemm_bias_ref(ln[:M], w2b, b2b), "wrapper.y", what)
    wd = [p.detach().double().requires_grad_(True) for m in mods for p in m.parameters()]
    hc = h.to(dev).double().requires_grad_(True)
    yr = nn.functional.linear(hc, wd[0], wd[1])
    yr = nn.functional.layer_norm(yr, (D,), wd[2], wd[3], mods[1].eps)
    yr = nn.functional.linear(yr, wd[4], wd[5])
    yr.backward(gy.to(dev).double())
    for name, got, ref in zip(["dh", "dW1", "db1", "dgamma", "dbeta", "dW2", "db2"], grads, [hc.grad] + [x.grad for x in wd]):
        assert bool(torch.isfinite(got).all()), (what, name)
        e = float((got.double() - ref).norm() / ref.norm().clamp_min(1e-30))
        print(f"wrapper {what} {name}: relative L2 {e:.2e}")
        assert e < 1e-2, (what, name, e)


def test_rows_view_fallbacks():
    """An fp32 input, a 4-D input and a bf16 view whose row stride is no multiple of 8 take _rows_view's
    packing copy: outputs and all seven gradients equal, bit for bit, the "rows" form on a contiguous
    bf16 copy (which is read in place)."""
    from triad_amd import ops
    B, N, H = 2, 65, 768
    mods, h, gy = _head(B, N, H)
    hb = h.to(dev)
    assert ops._rows_view(hb)[0] is hb, "the contiguous bf16 input must be read in place"
    base_y, base_g, _ = _run_head(mods, h, gy, "rows")
    wide = torch.zeros(B, N, H + 4, dtype=BF)
    wide[..., :H] = h
    inputs = {"fp32": h.float(), "4-D": h.view(B, 5, 13, H), "odd row stride": None}
    for name, x in inputs.items():
        if x is None:
            for m in mods:
                for p in m.parameters():
                    p.grad = None
            wd = wide.to(dev).requires_grad_(True)
            view = wd[..., :H]
            assert view.stride(-2) % 8 != 0
            hv = ops._rows_view(view)
            assert hv[0].data_ptr() != view.data_ptr() and hv[3] == H, "the view must take the copy"
            y = ops.projection_head(view, *mods, form="rows")
            y.backward(gy.to(dev))
            g = [wd.grad[..., :H]] + [p.grad.clone() for m in mods for p in m.parameters()]
            assert not bool(wd.grad[..., H:].abs().sum())
            y = y.detach()
        else:
            y, g, _ = _run_head(mods, x, gy, "rows")
        assert torch.equal(y.reshape(B, N, D), base_y), name
        for a, b in zip(g, base_g):
            assert torch.equal(a.reshape(b.shape).to(b.dtype), b), name
