"""fp64 references, derived per-element bounds, seeded cases and fp32 emulations for the HuBERT
front-end kernels of csrc/frontend.hip (triad_chgn_gelu_fwd / _bwd, triad_c0gn_fwd, triad_conv0_dw)
and csrc/posconv.hip (triad_posconv, triad_posconv_dw). No device needed:
tests/test_frontend_conformance_gpu.py applies the references and bounds to what the kernels return,
tests/test_frontend_checks_cpu.py applies them to the emulations below, intact (must pass) and with
one planted error (must fail).

Every reference is computed in fp64 from the operands the kernel reads (bf16 / fp32 values, exact in
fp64). Bounds are first-order, u = 2^-24, follow the rounding steps of the code, and none is fitted
to what a kernel returns. An fp32 sum whose order is known errs by at most h u sum|terms|, h the
number of roundings on the longest path; one store to bf16 adds 2^-8 |ref|; a factor 2 covers an MFMA
accumulator that does not round like IEEE at every step.

GroupNorm statistics (chgn_sums_kernel<0> / c0gn_kernel<0> + chgn_stats_kernel). A 256-thread block
covers rows = 256 / (C / 8) time rows per sweep of a 128-row chunk: a thread adds at most
ceil(128 / rows) terms in turn, one thread then adds the `rows` partials in turn:
h = ceil(128 / rows) + rows. The chunk partials are combined, divided and square-rooted in double.
With A = mean|x|, E2 = mean x^2 over the T valid frames of a (sample, channel):
    mean:  dm = (h + 1) u A                                              (+ 1: the fp32 store)
    rstd:  relative 0.5 ((h + 1) u E2 + 2 |m| dm + dm^2) / (var + eps) + 2 u
           (the one-pass q / T - m^2 errs against E[x^2] and m^2, not against the variance; the sums
           of x^2 are fmaf chains of exact products; + 2 u: the store and the double arithmetic)
That bound is useless on a mean-100 / sigma-0.1 channel (E2 / var ~ 10^6), by design. The exactness
route covers such channels: if in every 128-row chunk every x is a multiple of a grid g1 (the ulp of
the chunk's smallest nonzero |x|) with sum|x| < 2^24 g1, and every x^2 a multiple of g1^2 with
sum x^2 < 2^24 g1^2, every fp32 partial sum of the chunk is exact in any order, and what is left is
the double finalize (its cancellation q / T - m^2: 8 2^-53 E2 / (var + eps) relative on var) and the
two fp32 stores:
    mean:  2 u |m|          rstd:  relative 3 u + 4 2^-53 E2 / (var + eps)
bf16 values of one or two adjacent binades at <= 128 rows qualify. chgn_fwd_ref checks the
precondition in fp64 and returns the mask; the tests assert it on the special channels, so a kernel
that loses the exactness (a deeper chunk, an fp32 finalize) fails them.

y = bf16(gelu(z)), z = xhat gamma + beta:
    dz = |gamma| rstd dm + |xhat gamma| (rel_rstd + 4 u) + u |z|
    y:   1.13 dz + gelu_err(z) + 2^-8 |ref|            (sup |gelu'| = 1.13)
The first term is the cancellation term: x - mean errs by dm against |x| and |mean|, not against the
difference.

GELU function error. ASSUMED (HIP's published maximum errors as recalled, not verifiable in this
repository, each doubled; never tuned to a kernel's output): erff 4 ulp, __expf 1 ulp.
    gelu_err(z)  = 0.5 |z| (E_erf + u |1 + erf|) + 2 u |gelu|,
    E_erf        = 2 ERFF_ULP 2 u |erf(t)| + 2 u |t| erf'(t),  t = z / sqrt 2   (argument scaling)
    gelu'_err(z) = 0.5 E_erf + |z phi(z)| ((2 2 EXPF_ULP + 3 |a|) u + 3 u) + 2 u |gelu'|,  a = -z^2 / 2
                   (2 |a| u: the two products forming a; |a| u: __expf's own argument scaling)
These terms matter only for the fp32 outputs dgamma / dbeta.

Backward, from the kernel's own fp32 mean / rstd (exact inputs). xhat carries 2 u, z = fma: dz_arg =
2 u |xhat gamma| + u |z|; E_gp = 0.8 dz_arg + gelu'_err (sup |gelu''| = 0.8); dz = dy gelu'(z) errs by
e = |dy| E_gp + u |dz|. Sums S1 = sum dz, S2 = sum dz xhat per (sample, channel) have the forward's
depth h, then double:
    dbeta:   (h + B + 2) u sum|dz|      + sum e
    dgamma:  (h + B + 2) u sum|dz xhat| + sum (e |xhat| + 2 u |dz xhat|)     (the function-error term)
    dx = rstd (dz gamma - cA - xhat cB), cA = gamma S1 / T, cB = gamma S2 / T:
         rstd (e |gamma| + u |dz gamma| + e_cA + |xhat| e_cB + 3 u |xhat cB| + 3 u Tsum) + 2^-8 |ref|,
         e_cA = |gamma| (sum e + h u sum|dz|) / T + u |cA|,
         e_cB = |gamma| (sum (e |xhat| + 2 u |dz xhat|) + h u sum|dz xhat|) / T + u |cB|,
         Tsum = |dz gamma| + |cA| + |xhat cB|   (the cancellation is among these three).

conv0 (y0out): the fp64 sum of the 10 products rounded to bf16. The kernel's fp32 fmaf chain can round
differently only where the fp64 value lies within 2 * 12 u sum|w||s| of a bf16 rounding boundary, and
there by one gap (vit_rows_ref.bf16_flip). The statistics and `out` are referenced from the kernel's
own y0out, so a flip does not cascade; the tests cap the share of near-boundary elements at 2 %.

conv0_dw (fp32): 2 (n + 2) u sum|dy||s|, n = ceil(1024 / rows) + rows + slab depth: a thread's fmaf
chain over its rows of the 1024-row block, the `rows`-deep LDS sum, then triad_sum_slabs over
S = B nblk slabs (S < 16: four chains of ceil(S / 4) and two adds; else ceil(S / 64) + 2 + 16).

posconv y (bf16): 2 (128 CG + 2) u (sum|x||w| + |bias|) + 2^-8 |ref|.
posconv_dw (fp32): a split's slab 2 (n + 2) u sum|dy||x| over its own rows, n = rows of one split
(samples per split x T); the sum over the slabs 2 (n + 2 + splits) u sum|dy||x|.
"""
import math

import torch

from tests.vit_rows_ref import BF, F32, F64, R8, U, _gen, bf16_flip, f32, passes, ratio  # noqa: F401

CHUNK = 128
C0_ROWS = 1024
PC_ROWS = 208
DW_TP = 224
KT = 128
ERFF_ULP = 4.0    # ASSUMED
EXPF_ULP = 1.0    # ASSUMED
GP_SUP, GPP_SUP = 1.13, 0.8
SQRT1_2 = math.sqrt(0.5)
INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)


def rows_of(C):
    return 256 // (C // 8)


def depth(C, chunk=CHUNK):
    r = rows_of(C)
    return -(-chunk // r) + r


# ---- GELU in fp64 and its evaluation-error terms --------------------------------------------------

def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z * SQRT1_2))


def gelu_grad64(z):
    return 0.5 * (1.0 + torch.erf(z * SQRT1_2)) + z * INV_SQRT_2PI * torch.exp(-0.5 * z * z)


def _erf_err(z):
    t = z * SQRT1_2
    return 2 * ERFF_ULP * 2 * U * torch.erf(t).abs() + 2 * U * t.abs() * (2 / math.sqrt(math.pi)) * torch.exp(-t * t)


def gelu_err(z):
    return 0.5 * z.abs() * (_erf_err(z) + U * (1.0 + torch.erf(z * SQRT1_2)).abs()) + 2 * U * gelu64(z).abs()


def gelu_grad_err(z):
    a = 0.5 * z * z
    zphi = (z * INV_SQRT_2PI * torch.exp(-a)).abs()
    return 0.5 * _erf_err(z) + zphi * ((2 * 2 * EXPF_ULP + 3 * a) * U + 3 * U) + 2 * U * gelu_grad64(z).abs()


# ---- GroupNorm + GELU forward ---------------------------------------------------------------------

def _exact_chunks(xv):
    """xv [B][T][C] fp64 -> [B][C] bool: in every 128-row chunk the fp32 sums of x and of x^2 are
    exact in any order (module docstring)."""
    B, T, C = xv.shape
    ok = torch.ones(B, C, dtype=torch.bool)
    for t0 in range(0, T, CHUNK):
        c = xv[:, t0:t0 + CHUNK]
        a = c.abs()
        _, e = torch.frexp(torch.where(a > 0, a, torch.full_like(a, float("inf"))).amin(1))   # |x|min = m 2^e
        g1 = torch.ldexp(torch.ones_like(a[:, 0]), e - 8)   # ulp of a bf16 value with that exponent
        allzero = ~(a > 0).any(1)
        g1 = torch.where(allzero, torch.ones_like(g1), g1)
        lim = 2.0 ** 24
        ok &= allzero | ((a.sum(1) < lim * g1) & ((c * c).sum(1) < lim * g1 * g1))
    return ok


def chgn_fwd_ref(x, T, gamma, beta, eps):
    """x [B][Tp][C] bf16 (frames T.. ignored), gamma, beta [C] fp32, eps the fp32 value ->
    {"mean", "rstd": (ref [B][C], bound), "y": (ref [B][T][C], bound), "exact": [B][C] bool}."""
    xv = x[:, :T].double()
    C = xv.shape[2]
    h = depth(C)
    m = xv.mean(1)
    var = ((xv - m[:, None]) ** 2).mean(1)
    E2 = (xv * xv).mean(1)
    A = xv.abs().mean(1)
    rstd = (var + eps) ** -0.5
    exact = _exact_chunks(xv)
    dm = torch.where(exact, 2 * U * m.abs(), (h + 1) * U * A)
    rel_gen = 0.5 * ((h + 1) * U * E2 + 2 * m.abs() * dm + dm * dm) / (var + eps) + 2 * U
    rel_ex = 3 * U + 4 * 2.0 ** -53 * E2 / (var + eps)
    rel_r = torch.where(exact, rel_ex, rel_gen)
    g, b = gamma.double(), beta.double()
    xg = (xv - m[:, None]) * rstd[:, None] * g
    z = xg + b
    ref = gelu64(z)
    dz = g.abs() * (rstd * dm)[:, None] + xg.abs() * (rel_r[:, None] + 4 * U) + U * z.abs()
    bound = GP_SUP * dz + gelu_err(z) + R8 * ref.abs()
    return {"mean": (m, dm), "rstd": (rstd, rstd * rel_r), "y": (ref, bound), "exact": exact}


def _seq_sum(v, rows):
    """v [n][...] fp32 -> the block's sum in the kernels' order: row group r adds rows r, r + rows, ..
    in turn, then the `rows` partials are added in turn."""
    n = v.shape[0]
    k = -(-n // rows)
    pad = torch.zeros((k * rows - n,) + v.shape[1:], dtype=v.dtype)
    v = torch.cat([v, pad]).view((k, rows) + v.shape[1:])
    s = torch.zeros_like(v[0])
    for i in range(k):
        s = s + v[i]
    acc = torch.zeros_like(s[0])
    for r in range(rows):
        acc = acc + s[r]
    return acc


def _chunk_sums(a, b, T, C, chunk, drop_chunk=None, drop_row=None):
    """Per-chunk fp32 sums of a and b ([B][T][C] fp32) in the kernels' order -> two [nchunk][B][C]."""
    rows = rows_of(C)
    sa, sb = [], []
    for k, t0 in enumerate(range(0, T, chunk)):
        t1 = min(T, t0 + chunk)
        if drop_row is not None and t0 <= drop_row < t1:
            a, b = a.clone(), b.clone()
            a[:, drop_row] = 0
            b[:, drop_row] = 0
        pa = _seq_sum(a[:, t0:t1].transpose(0, 1), rows)
        pb = _seq_sum(b[:, t0:t1].transpose(0, 1), rows)
        if k == drop_chunk:
            pa, pb = torch.zeros_like(pa), torch.zeros_like(pb)
        sa.append(pa)
        sb.append(pb)
    return torch.stack(sa), torch.stack(sb)


def _gelu32(z, tanh=False):
    if tanh:
        return torch.nn.functional.gelu(z, approximate="tanh")
    return 0.5 * z * (1.0 + torch.erf(z * f32(SQRT1_2)))


def _gelu_grad32(z):
    return 0.5 * (1.0 + torch.erf(z * f32(SQRT1_2))) + z * f32(INV_SQRT_2PI) * torch.exp(-0.5 * z * z)


def emul_chgn_fwd(x, T, gamma, beta, eps, stats_over_tp=False, finalize_f32=False, chunk=CHUNK, tanh=False):
    """(y [B][Tp][C] bf16 with zero padding frames, mean, rstd) with the kernel's fp32 chunk sums and
    double finalize. Planted errors: the statistics over all Tp frames, the finalize in fp32, another
    chunk depth, tanh-GELU."""
    B, Tp, C = x.shape
    n = Tp if stats_over_tp else T
    xf = x.float()
    s, q = _chunk_sums(xf[:, :n], xf[:, :n] * xf[:, :n], n, C, chunk)   # x^2 of a bf16 value: exact in fp32
    if finalize_f32:
        sm, qm = torch.zeros_like(s[0]), torch.zeros_like(q[0])
        for k in range(s.shape[0]):
            sm, qm = sm + s[k], qm + q[k]
        m = sm / n
        var = (qm / n - m * m).clamp_min(0)
        mean, rstd = m, 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
    else:
        m = s.double().sum(0) / n
        var = (q.double().sum(0) / n - m * m).clamp_min(0)
        mean, rstd = m.float(), (1.0 / torch.sqrt(var + eps)).float()
    z = (xf[:, :T] - mean[:, None]) * rstd[:, None] * gamma + beta
    y = torch.zeros(B, Tp, C, dtype=BF)
    y[:, :T] = _gelu32(z, tanh).to(BF)
    return y, mean, rstd


# ---- GroupNorm + GELU backward --------------------------------------------------------------------

def chgn_bwd_ref(x, dy, T, gamma, beta, mean, rstd):
    """x, dy [B][Tp][C] bf16, gamma, beta [C], mean, rstd [B][C] fp32 (the forward kernel's outputs,
    exact inputs) -> {"dx": (ref [B][T][C], bound), "dgamma", "dbeta": (ref [C], bound)}."""
    xv, dv = x[:, :T].double(), dy[:, :T].double()
    B, _, C = xv.shape
    h = depth(C)
    g, be = gamma.double(), beta.double()
    rs = rstd.double()[:, None]
    xh = (xv - mean.double()[:, None]) * rs
    z = xh * g + be
    E_gp = GPP_SUP * (2 * U * (xh * g).abs() + U * z.abs()) + gelu_grad_err(z)
    dz = dv * gelu_grad64(z)
    e = dv.abs() * E_gp + U * dz.abs()
    dzx = dz * xh
    ex = e * xh.abs() + 2 * U * dzx.abs()
    S1, S2 = dz.sum(1), dzx.sum(1)
    A1, A2 = dz.abs().sum(1), dzx.abs().sum(1)
    E1, E2 = e.sum(1), ex.sum(1)
    dbeta = (S1.sum(0), (h + B + 2) * U * A1.sum(0) + E1.sum(0))
    dgamma = (S2.sum(0), (h + B + 2) * U * A2.sum(0) + E2.sum(0))
    cA, cB = (g * S1 / T)[:, None], (g * S2 / T)[:, None]
    e_cA = (g.abs() * (E1 + h * U * A1) / T)[:, None] + U * cA.abs()
    e_cB = (g.abs() * (E2 + h * U * A2) / T)[:, None] + U * cB.abs()
    ref = rs * (dz * g - cA - xh * cB)
    Tsum = (dz * g).abs() + cA.abs() + (xh * cB).abs()
    bound = rs * (e * g.abs() + U * (dz * g).abs() + e_cA + xh.abs() * e_cB + 3 * U * (xh * cB).abs() + 3 * U * Tsum) \
        + R8 * ref.abs()
    return {"dx": (ref, bound), "dgamma": dgamma, "dbeta": dbeta}


def emul_chgn_bwd(x, dy, T, gamma, beta, mean, rstd, no_cA=False, no_cB=False, swap_params=False, drop_chunk=None,
                  drop_row=None):
    """(dx [B][Tp][C] bf16 with zero padding frames, dgamma, dbeta) with the kernel's chunk sums.
    Planted errors: cA / cB omitted, dgamma and dbeta exchanged, chunk `drop_chunk`'s partial or row
    `drop_row` left out of the sums."""
    B, Tp, C = x.shape
    xf, df = x[:, :T].float(), dy[:, :T].float()
    xh = (xf - mean[:, None]) * rstd[:, None]
    dz = df * _gelu_grad32(xh * gamma + beta)
    s, q = _chunk_sums(dz, (dz.double() * xh.double()).float(), T, C, CHUNK, drop_chunk, drop_row)
    S1, S2 = s.double().sum(0), q.double().sum(0)
    gm = gamma.double()
    cA = torch.zeros(B, C) if no_cA else (gm * S1 / T).float()
    cB = torch.zeros(B, C) if no_cB else (gm * S2 / T).float()
    dx = torch.zeros(B, Tp, C, dtype=BF)
    dx[:, :T] = (rstd[:, None] * (dz * gamma - cA[:, None] - xh * cB[:, None])).to(BF)
    dgamma, dbeta = S2.sum(0).float(), S1.sum(0).float()
    return (dx, dbeta, dgamma) if swap_params else (dx, dgamma, dbeta)


# ---- conv0 ----------------------------------------------------------------------------------------

def _windows(wave, T, stride=5):
    """wave [B][L] -> [B][T][10]: samples stride t .. stride t + 9."""
    return wave.unfold(1, 10, stride)[:, :T]


def conv0_ref(wave, w0, T):
    """wave [B][Lp], w0 [C][10] bf16 -> (bf16(y0) as fp64 [B][T][C], gap [B][T][C]): the kernel's y0out
    may differ from the first by at most gap (0 except near a bf16 rounding boundary)."""
    win = _windows(wave.double(), T)
    y = win @ w0.double().t()
    mag = win.abs() @ w0.double().abs().t()
    return bf16_flip(y, 2.0 * 12 * U * mag)


def emul_conv0(wave, w0, T, reverse_taps=False, stride=5):
    """y0 [B][T][C] bf16 by the kernel's fp32 fmaf chain (bf16 products are exact in fp32)."""
    win = _windows(wave.float(), T, stride)
    wf = w0.float().flip(1) if reverse_taps else w0.float()
    a = torch.zeros(win.shape[0], T, w0.shape[0])
    for j in range(10):
        a = a + win[:, :, j:j + 1] * wf[:, j]
    return a.to(BF)


def slab_depth(S, n):
    """Roundings on the longest path of triad_sum_slabs over S slabs of n elements."""
    return -(-S // 64) + 18 if S >= 16 and n <= 16384 else -(-S // 4) + 2


def conv0_dw_ref(wave, dy0, T):
    """wave [B][Lp], dy0 [B][Tp][C] bf16 -> (ref [C][10], bound)."""
    B, _, C = dy0.shape
    win = _windows(wave.double(), T)
    d = dy0[:, :T].double()
    ref = torch.einsum("btc,btj->cj", d, win)
    mag = torch.einsum("btc,btj->cj", d.abs(), win.abs())
    rows = rows_of(C)
    n = -(-C0_ROWS // rows) + rows + slab_depth(B * -(-T // C0_ROWS), C * 10)
    return ref, 2.0 * (n + 2) * U * mag


def emul_conv0_dw(wave, dy0, T, late_window=False, drop_slab=None):
    """dw0 [C][10] fp32: per 1024-row block a thread's fmaf chain over its rows, the rows-deep sum,
    the slabs added in fp32. Planted: block 1's waveform window taken from t0 - 1; one slab dropped."""
    B, _, C = dy0.shape
    rows = rows_of(C)
    wf = wave.float()
    slabs = []
    for b in range(B):
        for blk, t0 in enumerate(range(0, T, C0_ROWS)):
            t1 = min(T, t0 + C0_ROWS)
            first = t0 - 1 if late_window and blk == 1 else t0
            win = wf[b, 5 * first:].unfold(0, 10, 5)[:t1 - t0]
            terms = dy0[b, t0:t1].float()[:, :, None] * win[:, None, :]       # exact products
            s = _seq_sum(terms, rows)
            slabs.append(torch.zeros_like(s) if len(slabs) == drop_slab else s)
    out = torch.zeros_like(slabs[0])
    for s in slabs:
        out = out + s
    return out


# ---- positional conv ------------------------------------------------------------------------------

def posconv_wt(W, G):
    """Conv1d weight W [C][CG][128] -> the forward operand wt[g][n][j * CG + c] = W[g CG + n][c][j]."""
    C, CG, K = W.shape
    return W.view(G, CG, CG, K).permute(0, 1, 3, 2).reshape(G, CG, K * CG).contiguous()


def posconv_wt_bwd(W, G, flip=True):
    """The input-gradient operand as _PosConv.backward builds it: wt[g][c][j * CG + n] =
    W[g CG + n][c][127 - j] (flip = False: the planted error, taps not reversed)."""
    C, CG, K = W.shape
    Wg = W.view(G, CG, CG, K)
    if flip:
        Wg = Wg.flip(-1)
    return Wg.permute(0, 2, 3, 1).reshape(G, CG, K * CG).contiguous()


def _pc_windows(x, pad, neighbours=False, late_block=False):
    """x [B][T][C] -> [B][T][128][C]: rows t + j - pad, zero outside [0, T). Planted errors:
    neighbours = rows outside [0, T) read from the neighbouring samples (zero only outside the whole
    tensor); late_block = the windows of t >= 208 start one row late."""
    B, T, C = x.shape
    if neighbours:
        flat = torch.cat([torch.zeros(pad, C, dtype=x.dtype), x.reshape(B * T, C), torch.zeros(KT, C, dtype=x.dtype)])
        xp = torch.stack([flat[b * T:b * T + T + KT] for b in range(B)])
    else:
        xp = torch.zeros(B, T + KT, C, dtype=x.dtype)
        xp[:, pad:pad + T] = x
    win = xp.unfold(1, KT, 1).permute(0, 1, 3, 2)        # [B][T + 1][128][C]
    if late_block and T > PC_ROWS:
        return torch.cat([win[:, :PC_ROWS], win[:, PC_ROWS + 1:T + 1]], 1)
    return win[:, :T]


def _pc_product(x, wt, pad, **kw):
    B, T, C = x.shape
    G, CG, _ = wt.shape
    win = _pc_windows(x, pad, **kw)
    out = torch.empty(B, T, C, dtype=x.dtype)
    for g in range(G):
        a = win[:, :, :, g * CG:(g + 1) * CG].reshape(B * T, KT * CG)
        out[:, :, g * CG:(g + 1) * CG] = (a @ wt[g].t()).view(B, T, CG)
    return out


def posconv_refs(x, wt, bias, pad):
    """x [B][T][C] bf16, wt [G][CG][128 CG] bf16, bias [C] fp32 -> ((ref, bound) without the bias,
    (ref, bound) with it), the products computed once."""
    CG = wt.shape[1]
    ref = _pc_product(x.double(), wt.double(), pad)
    mag = _pc_product(x.double().abs(), wt.double().abs(), pad)
    k = 2.0 * (KT * CG + 2) * U
    refb = ref + bias.double()
    return (ref, k * mag + R8 * ref.abs()), (refb, k * (mag + bias.double().abs()) + R8 * refb.abs())


def posconv_ref(x, wt, bias, pad):
    """x [B][T][C] bf16, wt [G][CG][128 CG] bf16, bias [C] fp32 or None -> (ref [B][T][C], bound)."""
    zero = torch.zeros(x.shape[2])
    return posconv_refs(x, wt, zero if bias is None else bias, pad)[bias is not None]


def emul_posconv(x, wt, bias, pad, neighbours=False, keep_last=False, late_block=False, bias_twice=False):
    """y [B][T][C] bf16 from an fp32 product. Planted errors: _pc_windows', keep_last = outputs
    1 .. T of the padding-64 conv's T + 1 instead of 0 .. T - 1 (the same product at pad - 1), the bias
    added twice."""
    y = _pc_product(x.float(), wt.float(), pad - 1 if keep_last else pad, neighbours=neighbours, late_block=late_block)
    if bias is not None:
        y = y + bias * (2 if bias_twice else 1)
    return y.to(BF)


def dw_used_splits(B, splits):
    """Splits of triad_posconv_dw that hold a sample: ceil(B / splits) samples each, in order."""
    return -(-B // -(-B // splits))


def posconv_dw_ref(x, dy, G, pad, splits):
    """x, dy [B][T][C] bf16 -> (slab refs [used][G][128][CG][CG], slab bounds, sum ref, sum bound):
    part[s][g][j][n][c] = sum over split s's samples and t of dy[b][t][g CG + n] x[b][t + j - pad][g CG + c],
    for the used = dw_used_splits(B, splits) splits that hold a sample (the others' slabs are zero)."""
    B, T, C = x.shape
    CG = C // G
    spb = -(-B // splits)
    n = spb * T
    ref = torch.zeros(dw_used_splits(B, splits), G, KT, CG, CG, dtype=F64)
    mag = torch.zeros_like(ref)
    win = _pc_windows(x.double(), pad)
    d = dy.double()
    for b in range(B):
        for g in range(G):
            a = win[b, :, :, g * CG:(g + 1) * CG].reshape(T, KT * CG)
            dg = d[b, :, g * CG:(g + 1) * CG]
            ref[b // spb, g] += (dg.t() @ a).view(CG, KT, CG).transpose(0, 1)
            mag[b // spb, g] += (dg.abs().t() @ a.abs()).view(CG, KT, CG).transpose(0, 1)
    return ref, 2.0 * (n + 2) * U * mag, ref.sum(0), 2.0 * (n + 2 + splits) * U * mag.sum(0)


def emul_posconv_dw(x, dy, G, pad, splits, drop_row=None, shift_step=False, drop_slab=None):
    """(slabs [splits][G][128][CG][CG] fp32, their fp32 sum). Planted errors: drop_row = (b, t) left
    out; shift_step = the x window of the second 224-row step (t >= 224) one row late; one slab zero."""
    B, T, C = x.shape
    CG = C // G
    spb = -(-B // splits)
    slabs = torch.zeros(splits, G, KT, CG, CG)
    xf, d = x.float(), dy.float().clone()
    if drop_row is not None:
        d[drop_row[0], drop_row[1]] = 0
    win = _pc_windows(xf, pad)
    if shift_step and T > DW_TP:
        late = _pc_windows(torch.cat([xf[:, 1:], torch.zeros_like(xf[:, :1])], 1), pad)
        win = torch.cat([win[:, :DW_TP], late[:, DW_TP:]], 1)
    for b in range(B):
        for g in range(G):
            a = win[b, :, :, g * CG:(g + 1) * CG].reshape(T, KT * CG)
            slabs[b // spb, g] += (d[b, :, g * CG:(g + 1) * CG].t() @ a).view(CG, KT, CG).transpose(0, 1)
    if drop_slab is not None:
        slabs[drop_slab] = 0
    total = torch.zeros_like(slabs[0])
    for s in range(splits):
        total = total + slabs[s]
    return slabs, total


def posconv_dw_to_weight(total):
    """[G][128][CG][CG] (g, j, n, c) -> Conv1d's dW [C][CG][128]."""
    G, K, CG, _ = total.shape
    return total.permute(0, 2, 3, 1).reshape(G * CG, CG, K)


# ---- seeded cases (CPU), shared by the GPU and the CPU tests ------------------------------------------

SPECIAL = {"mean100": 8, "tiny": 9, "const": 10}   # channels of a chgn case with C = 64
CONST = 2.5       # every partial sum of <= 2^15 of them, and of their squares, is exact in fp32
CONST_BETA = 0.5  # gelu(0.5) lies far from a bf16 rounding boundary
CONST_DY = 0.75   # dy of the constant channel: constant over t, so its dx is 0 (dz - mean(dz) = 0)


def chgn_case(B, T, Tp, C, fill=float("nan")):
    """x, dy [B][Tp][C] bf16 (frames T .. Tp - 1 hold `fill`), gamma, beta [C] fp32. At C = 64 channel 8
    is a mean-100 / sigma-0.1 channel (its values as bf16 yields them: 99.5, 100, 100.5), channel 9 a
    mean-0 / sigma-1e-3 channel, channel 10 a constant channel with a constant dy."""
    g = _gen(11, B, T, C)
    x = torch.randn(B, Tp, C, generator=g) * 1.5 + 0.3
    dy = torch.randn(B, Tp, C, generator=g)
    gamma = 1.0 + 0.5 * torch.randn(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    if C == 64:
        x[:, :, SPECIAL["mean100"]] = 100.0 + 0.1 * torch.randn(B, Tp, generator=g)
        x[:, :, SPECIAL["tiny"]] = 1e-3 * torch.randn(B, Tp, generator=g)
        x[:, :, SPECIAL["const"]] = CONST
        dy[:, :, SPECIAL["const"]] = CONST_DY
        beta[SPECIAL["const"]] = CONST_BETA
    x[:, T:] = fill
    dy[:, T:] = fill
    return x.to(BF), dy.to(BF), gamma, beta


def conv0_case(B, T, Tp, C, fill=float("nan"), seed=0):
    """wave [B][Lp] bf16 N(0, 1) with Lp = 5 (Tp - 1) + 10 and `fill` past sample 5 (T - 1) + 9,
    w0 [C][10] bf16 0.3 N(0, 1), gamma, beta, dy [B][Tp][C] bf16 (`fill` in frames T ..)."""
    g = _gen(12, B, T, C, seed)
    Lp = 5 * (Tp - 1) + 10
    wave = torch.randn(B, Lp, generator=g)
    wave[:, 5 * (T - 1) + 10:] = fill
    w0 = 0.3 * torch.randn(C, 10, generator=g)
    gamma = 1.0 + 0.5 * torch.randn(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    dy = torch.randn(B, Tp, C, generator=g)
    dy[:, T:] = fill
    return wave.to(BF), w0.to(BF), gamma, beta, dy.to(BF)


def posconv_case(B, T, C, G):
    """x, dy [B][T][C] bf16, Conv1d weight W [C][C / G][128] bf16 (std (128 CG)^-1/2), bias [C] fp32."""
    g = _gen(13, B, T, C, G)
    CG = C // G
    x = torch.randn(B, T, C, generator=g).to(BF)
    dy = torch.randn(B, T, C, generator=g).to(BF)
    W = (torch.randn(C, CG, KT, generator=g) * (KT * CG) ** -0.5).to(BF)
    bias = 0.5 * torch.randn(C, generator=g)
    return x, dy, W, bias
