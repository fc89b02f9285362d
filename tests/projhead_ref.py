"""fp64 references, derived per-element bounds and plain-torch emulations for the projection-head
kernels: csrc/rowgemm.hip (triad_projhead_fwd / _ln_fwd / _ln_bwd, triad_rowgemm_bias, triad_wpack /
triad_wpack2) and csrc/projhead.hip (triad_ln_fwd, triad_ln_bwd3, triad_sum_slabs, triad_colsum_dma).
No device needed: tests/test_projhead_conformance_gpu.py applies the references and bounds to what
the kernels return, tests/test_projhead_checks_cpu.py applies them to the emulations below, intact
(must pass) and with one planted error (must fail). Both files take their shapes from the lists here.

Every stage is referenced in fp64 from the operands that stage reads (bf16 / fp32 values, exact in
fp64): mean / rstd / ln from the kernel's own y1, y from its own ln, dy1 and the partials from its own
dln. A bf16 rounding flip upstream therefore never loosens a bound downstream. Bounds are first-order,
u = 2^-24; a sum whose order is known errs by at most h u sum|terms|, h the roundings on the longest
path to the result, a sum in any order by (n - 1) u sum|terms|; a factor 2 covers an MFMA accumulator
that does not round like IEEE at every step; a store to bf16 adds 2^-8 |ref| (the terms of
tests/test_gemm_conformance_gpu.py).

* GEMMs with bias (y1, y, dln; K-deep MFMA sum, the bias added in fp32, one bf16 store):
      2 (K + 2) u (|X| . |W| + |b|) + 2^-8 |ref|
* LayerNorm forward (mean, rstd, ln): the forward bounds of tests/vit_rows_ref.py (addln_fwd_ref,
  derived there) at D = 512 with the depth h of the row sum the code has, read from the source:
    - row-panel epilogue (rowgemm.hip, EPI 1 / 3): a lane adds its 16 values of the row (4 column
      blocks x 4) in turn, two lane swaps (__shfl_xor 16, 32), then thread r adds the 8 waves'
      partials in turn: h = 16 + 2 + 8 = 26;
    - ln_fwd_kernel (projhead.hip): a lane adds its 8 values in turn, wave_sum adds 6 butterfly
      levels: h = 8 + 6 = 14.
  Both kernels multiply by 1 / 512 (exact) where addln divides; the + 1 of that bound stays (slack).
  ln is stored as bf16: + 2^-8 |ref|.
* LayerNorm backward (dy1) from exact y1 / mean / rstd inputs: the backward bound of vit_rows_ref
  (addln_bwd_ref, derived there) with the same two depths (the row sums of g and g xh take the same
  path as the forward's: 26 in the epilogue, 14 in ln_bwd3_kernel), + 2^-8 |ref| for the bf16 store.
* Column partials over the n rows a panel / block owns, in any order:
      dgamma  (n - 1 + 4) u sum|dln xh|   (4: xh = (y1 - mean) rstd rounds twice, the product once,
                                           one spare for a contracted fma)
      dbeta   (n - 1) u sum|dln|          (bf16 terms are exact in fp32)
      db1     the sum of the kernel's OWN bf16 dy1 values of those rows, (n - 1) u sum|dy1|
              (127 u for a panel: n <= 128)
  Masked rows add exact zeros. Totals: the partials summed in fp64 against the summed bounds.
* triad_sum_slabs over S slabs (depth read from projhead.hip):
    - sum_slabs_kernel: chain s0 takes S // 4 adds and the S % 4 remainder slabs, the combine
      (s0 + s1) + (s2 + s3) is two deep, alpha one more: h = S // 4 + S % 4 + 3;
    - colsum_reduce_kernel (S >= 16 and n <= 16384): slab lane sl's chain a0 takes ceil(S / 64) adds
      of the 4-chain loop and up to 3 of its remainder loop, the combine 2, the 16 slab lanes are
      added in turn, alpha: h = ceil(S / 64) + 3 + 2 + 16 + 1.
  bound = h u |alpha| sum|slab| (+ 2^-8 |ref| for bf16 out).
* triad_colsum_dma: any order over the rows and the S = triad_colsum_dma_splits partials, alpha:
      (rows + S + 1) u |alpha| sum|x| (+ 2^-8 |ref| for bf16 out).
* triad_wpack / triad_wpack2: a permutation (wpack_ref, the index formula of the comment above
  wpack_t_kernel); the check is equality.
"""
import torch

from tests.vit_rows_ref import BF, F32, F64, R8, U, f32, passes, ratio  # noqa: F401  (re-exported)

D = 512
EPS = 1e-5
H_PANEL = 16 + 2 + 8     # row-sum depth of the row-panel epilogues
H_WAVE = 8 + 6           # row-sum depth of ln_fwd_kernel / ln_bwd3_kernel

# ---- the shapes both test files run ---------------------------------------------------------------
FWD_HS = (32, 64, 96, 128, 160, 192, 224, 768, 1024)      # at M = 129: nkt 1..7, 24, 32
FWD_MS = (1, 127, 128, 129, 300)                          # at H = 768
FWD_CASES = tuple((129, H) for H in FWD_HS) + tuple((M, 768) for M in FWD_MS if M != 129) + ((300, 1024),)
ADDR_HS = (96, 768)
ADDR_FORMS = ("contig", "lda", "two_level", "n_per1")
BWD_MS = (1, 127, 128, 129, 300)
LN_FWD_MS = (1, 3, 4, 5, 130, 16389)
LN_BWD3_MS = (1, 5, 130, 4101)
SLAB_CASES = tuple((S, n) for S in (1, 3, 4, 5, 15, 16, 17, 1024) for n in (1, 63, 64, 65, 1536)) + (
    (15, 16384), (16, 16384), (17, 16385), (16, 16385), (5, 16385), (3, 16384))
COLSUM_ROWS = (1, 15, 16, 17, 63, 64, 65, 200)
COLSUM_COLS = (8, 248, 256, 264, 520)
WPACK_KS = (32, 512, 768)
WPACK2_KS = ((768, 512), (32, 512), (1024, 32))


def ln_bwd3_blocks(M):
    q = -(-M // 4)
    return sorted({1, 2, min(1024, q), q + 3})


def panels(M):
    return -(-M // 128)


def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1000003 + int(k)
    return torch.Generator().manual_seed(seed % (2 ** 31))


# ---- seeded operands ------------------------------------------------------------------------------

def head_case(M, H):
    """h [M][H], W1 [512][H], b1, W2 [512][512], b2 bf16; gamma, beta fp32; dy [M][512] bf16."""
    g = _gen(11, M, H)
    return dict(
        h=torch.randn(M, H, generator=g).to(BF),
        W1=(torch.randn(D, H, generator=g) / H ** 0.5).to(BF),
        b1=(torch.randn(D, generator=g) * 0.3).to(BF),
        W2=(torch.randn(D, D, generator=g) / D ** 0.5).to(BF),
        b2=(torch.randn(D, generator=g) * 0.3).to(BF),
        gamma=1.0 + 0.5 * torch.randn(D, generator=g),
        beta=0.3 * torch.randn(D, generator=g),
        dy=(torch.randn(M, D, generator=g) * 0.05).to(BF))


def ln_case(M):
    """y1 [M][512] bf16 (row means and scales vary), dln bf16, gamma, beta fp32."""
    g = _gen(12, M)
    y1 = torch.randn(M, D, generator=g) * (0.2 + 2.0 * torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)
    return dict(y1=y1.to(BF), dln=(torch.randn(M, D, generator=g) * 0.05).to(BF),
                gamma=1.0 + 0.5 * torch.randn(D, generator=g), beta=0.3 * torch.randn(D, generator=g))


def stats_f32(y1, eps):
    """The fp64 row statistics of y1 rounded to fp32: the backward's operands, independent of any
    forward kernel."""
    v = y1.double()
    m = v.mean(1)
    var = ((v - m[:, None]) ** 2).mean(1)
    return m.to(F32), ((var + eps) ** -0.5).to(F32)


def bwd_case(M):
    """Operands of triad_projhead_ln_bwd built on the host, independent of the forward kernel: dy, W2,
    y1 bf16, the fp64 statistics of y1 rounded to fp32, gamma."""
    c, l = head_case(M, 32), ln_case(M)
    mean, rstd = stats_f32(l["y1"], f32(EPS))
    return dict(dy=c["dy"], W2=c["W2"], y1=l["y1"], mean=mean, rstd=rstd, gamma=c["gamma"])


def slab_case(S, n):
    g = _gen(13, S, n)
    return torch.randn(S, n, generator=g), torch.tensor([0.37], dtype=F32)


def colsum_case(rows, cols):
    return torch.randn(rows, cols, generator=_gen(14, rows, cols)).to(BF)


def weight_case(K):
    return torch.randn(D, K, generator=_gen(15, K)).to(BF)


def strided_rows(h, form, fill=float("nan")):
    """h [M][H] laid out as triad_projhead_fwd's two-level addressing reads it: (flat buffer, offset of
    row 0 in elements, lda, n_per, bstride). Every element that is not a row's is `fill`.
      contig     rows back to back
      lda        row stride H + 8
      two_level  samples of n_per = 50 rows behind 5 prefix rows each, row stride H + 8, sample stride
                 55 lda: with M = 150 both 128-row panels straddle sample boundaries
      n_per1     one row per sample, sample stride 3 (H + 8)"""
    M, H = h.shape
    if form == "contig":
        return h.reshape(-1).clone(), 0, H, M, 0
    lda = H + 8
    if form == "lda":
        buf = torch.full((M, lda), fill, dtype=h.dtype)
        buf[:, :H] = h
        return buf.reshape(-1), 0, lda, M, 0
    if form == "two_level":
        n_per, pre = 50, 5
        B = -(-M // n_per)
        buf = torch.full((B, pre + n_per, lda), fill, dtype=h.dtype)
        for b in range(B):
            rows = h[b * n_per:(b + 1) * n_per]
            buf[b, pre:pre + rows.shape[0], :H] = rows
        return buf.reshape(-1), pre * lda, lda, n_per, (pre + n_per) * lda
    if form == "n_per1":
        buf = torch.full((M, 3, lda), fill, dtype=h.dtype)
        buf[:, 0, :H] = h
        return buf.reshape(-1), 0, lda, 1, 3 * lda
    raise ValueError(form)


def gather_rows(buf, off, lda, n_per, bstride, M, H):
    """The rows the kernel's address formula reads: row r at off + (r / n_per) bstride + (r % n_per) lda."""
    r = torch.arange(M)
    start = off + (r // n_per) * bstride + (r % n_per) * lda
    return buf[start[:, None] + torch.arange(H)[None, :]]


ADDR_M = 150


# ---- references and bounds --------------------------------------------------------------------------

def gemm_bias_ref(X, W, b=None):
    """X [M][K], W [N][K], b [N] (or None) bf16 -> (ref of X W^T + b, bound)."""
    K = X.shape[1]
    ref = X.double() @ W.double().t()
    mag = X.double().abs() @ W.double().abs().t()
    if b is not None:
        ref = ref + b.double()
        mag = mag + b.double().abs()
    return ref, 2.0 * (K + 2) * U * mag + R8 * ref.abs()


def ln_fwd_ref(y1, gamma, beta, eps, h):
    """y1 [M][512] bf16, gamma, beta fp32, eps the fp32 value, h the row-sum depth -> {mean, rstd, ln:
    (ref, bound)}: tests/vit_rows_ref.py addln_fwd_ref's bounds with the depth as an argument, ln bf16."""
    v = y1.double()
    m = v.mean(1)
    var = ((v - m[:, None]) ** 2).mean(1)
    rstd = (var + eps) ** -0.5
    dm = (h + 1) * U * v.abs().mean(1)
    rel_r = 0.5 * (dm * rstd) ** 2 + (0.5 * (h + 6) + 4) * U
    xhat = (v - m[:, None]) * rstd[:, None]
    wd = gamma.double()
    ref = xhat * wd + beta.double()
    bound = (wd.abs() * (rstd * dm)[:, None] + (xhat * wd).abs() * (rel_r[:, None] + 4 * U) + U * ref.abs()
             + R8 * ref.abs())
    return {"mean": (m, dm), "rstd": (rstd, rstd * rel_r), "ln": (ref, bound)}


def row_groups_panel(M):
    """Row -> the panel whose partial it is summed into."""
    return torch.arange(M) // 128, panels(M)


def row_groups_bwd3(M, nblocks):
    """Row -> the block of ln_bwd3_kernel that owns it (row r: block (r / 4) mod nblocks)."""
    return (torch.arange(M) // 4) % nblocks, nblocks


def ln_bwd_ref(dln, y1, mean, rstd, gamma, h, groups, dy1_got=None):
    """dln, y1 [M][512] bf16, mean, rstd fp32 [M] (exact inputs), gamma fp32, h the row-sum depth,
    groups = (row -> group, group count) -> {dy1, dgamma, dbeta: (ref, bound), total: ...}; with
    dy1_got (the kernel's own bf16 dy1 [M][512]) also db1, the group sums of those values."""
    grp, G = groups
    r = rstd.double()[:, None]
    xh = (y1.double() - mean.double()[:, None]) * r
    dl = dln.double()
    wd = gamma.double() * dl
    c1 = wd.mean(1, keepdim=True)
    c2 = (wd * xh).mean(1, keepdim=True)
    ref = r * (wd - c1 - xh * c2)
    W1 = wd.abs().mean(1, keepdim=True)
    W2 = (wd * xh).abs().mean(1, keepdim=True)
    T = wd.abs() + c1.abs() + (xh * c2).abs()
    bound = r * (U * wd.abs() + (h + 2) * U * W1 + xh.abs() * (h + 5) * U * W2 + 3 * U * (xh * c2).abs()
                 + 3 * U * T) + U * ref.abs() + R8 * ref.abs()

    def per_group(v):
        return torch.zeros(G, D, dtype=F64).index_add_(0, grp, v)
    n = torch.zeros(G, dtype=F64).index_add_(0, grp, torch.ones(len(grp), dtype=F64))[:, None]
    nm1 = (n - 1).clamp_min(0)
    out = {"dy1": (ref, bound),
           "dgamma": (per_group(dl * xh), (nm1 + 4) * U * per_group((dl * xh).abs())),
           "dbeta": (per_group(dl), nm1 * U * per_group(dl.abs()))}
    if dy1_got is not None:
        d1 = dy1_got.double()
        out["db1"] = (per_group(d1), nm1 * U * per_group(d1.abs()))
    for k in list(out):
        if k != "dy1":
            out["total." + k] = (out[k][0].sum(0), out[k][1].sum(0))
    return out


def slab_path(S, n):
    return "reduce" if S >= 16 and n <= 16384 else "stream"


def slab_depth(S, n):
    if slab_path(S, n) == "reduce":
        return -(-S // 64) + 3 + 2 + 16 + 1
    return S // 4 + S % 4 + 3


def sum_slabs_ref(slabs, alpha, out_bf16):
    """slabs [S][n] fp32, alpha the fp32 value (1.0 for NULL) -> (ref, bound)."""
    S, n = slabs.shape
    ref = alpha * slabs.double().sum(0)
    bound = slab_depth(S, n) * U * abs(alpha) * slabs.double().abs().sum(0)
    return ref, bound + (R8 * ref.abs() if out_bf16 else 0.0)


def colsum_dma_splits(rows, cols):
    """triad_colsum_dma_splits (projhead.hip: one round of >= 512 workgroups, >= 4 chunks of 16 rows
    per split)."""
    tiles = -(-cols // 256)
    return max(1, min(-(-512 // tiles), rows // 64))


def colsum_ref(X, alpha, out_bf16):
    """X [rows][cols] bf16, alpha the fp32 value -> (ref, bound)."""
    rows, cols = X.shape
    ref = alpha * X.double().sum(0)
    bound = (rows + colsum_dma_splits(rows, cols) + 1) * U * abs(alpha) * X.double().abs().sum(0)
    return ref, bound + (R8 * ref.abs() if out_bf16 else 0.0)


def wpack_ref(W, swap_lanes=None):
    """W [512][K] -> the packed fragments, K * 512 elements: fragment (kt, w, cb, l) at
    ((kt * 8 + w) * 4 + cb) * 512 + l * 8 holds W[64 w + 16 cb + (l & 15)][32 kt + 8 (l >> 4) + i],
    i = 0..7. swap_lanes = (a, b): those two lanes of fragment (0, 0, 0) exchanged (planted)."""
    K = W.shape[1]
    # W[n][k]: n = (w, cb, l16), k = (kt, q, i)  ->  [kt][w][cb][q][l16][i], lane l = 16 q + l16
    P = W.reshape(8, 4, 16, K // 32, 4, 8).permute(3, 0, 1, 4, 2, 5).reshape(K // 32, 8, 4, 64, 8).clone()
    if swap_lanes is not None:
        a, b = swap_lanes
        P[0, 0, 0, [a, b]] = P[0, 0, 0, [b, a]]
    return P.reshape(-1)


# ---- emulations (fp32, the kernels' operation order) ---------------------------------------------------

def emul_rowgemm(X, W, b, drop_last_ktile=False, bias_after=False, swap_cols=None, copy_last_row_to=None):
    """bf16(X W^T + b) with the bias added in fp32 before the one rounding, [panels * 128][N] with zero
    pad rows. Planted: the last 32-deep k tile dropped; the bias added after the rounding; swap_cols =
    (row, c): columns c + 1, c + 2 of that row's 4-column group exchanged; copy_last_row_to = Mp: row
    M - 1 written into the pad rows."""
    M, K = X.shape
    Xf = X.float().clone()
    if drop_last_ktile:
        Xf[:, K - 32:] = 0
    acc = Xf @ W.float().t()
    bf = torch.zeros(W.shape[0]) if b is None else b.float()
    y = (acc.to(BF).float() + bf).to(BF) if bias_after else (acc + bf).to(BF)
    if swap_cols is not None:
        r, c = swap_cols
        y[r, [c + 1, c + 2]] = y[r, [c + 2, c + 1]]
    out = torch.zeros(panels(M) * 128, W.shape[0], dtype=BF)
    out[:M] = y
    if copy_last_row_to is not None:
        out[M:] = y[M - 1]
    return out


def _panel_row_sum(v):
    """Row sums of v [M][512] fp32 in the row-panel epilogue's order: wave w, lane group q hold columns
    64 w + 16 cb + 4 q + i; a lane adds its 16 values over (cb, i) in turn, lanes meet by xor 16, 32
    (q ^ 1, q ^ 2), thread r adds the 8 waves' sums in turn."""
    M = v.shape[0]
    per = v.reshape(M, 8, 4, 4, 4).permute(0, 1, 3, 2, 4).reshape(M, 8, 4, 16)   # [M][w][q][(cb, i)]
    s = torch.zeros(M, 8, 4)
    for k in range(16):
        s = s + per[..., k]
    q = torch.arange(4)
    s = s + s[:, :, q ^ 1]
    s = s + s[:, :, q ^ 2]
    t = torch.zeros(M)
    for w in range(8):
        t = t + s[:, w, 0]
    return t


def _wave8_row_sum(v):
    """Row sums in ln_fwd_kernel / ln_bwd3_kernel's order: lane l adds columns 8 l .. 8 l + 7 in turn,
    then wave_sum's xor butterfly (32 .. 1)."""
    M = v.shape[0]
    per = v.reshape(M, 64, 8)
    s = torch.zeros(M, 64)
    for k in range(8):
        s = s + per[..., k]
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, 0]


def _row_sum(form):
    return _panel_row_sum if form == "panel" else _wave8_row_sum


def emul_ln_fwd(y1, gamma, beta, eps, form, unbiased=False, stat_shift=0):
    """(ln bf16, mean, rstd fp32) over y1 [M][512] bf16; form "panel" (the row-panel epilogue) or "wave"
    (ln_fwd_kernel). Planted: the variance over 511; the statistics of row r + stat_shift used for row
    r's ln."""
    rs_ = _row_sum(form)
    x = y1.float()
    mean = rs_(x) * (1.0 / D)
    d = x - mean[:, None]
    var = rs_(d * d) / (D - 1) if unbiased else rs_(d * d) * (1.0 / D)
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=F32))
    mu, rs = mean, rstd
    if stat_shift:
        idx = (torch.arange(x.shape[0]) + stat_shift) % x.shape[0]
        mu, rs = mean[idx], rstd[idx]
    ln = ((x - mu[:, None]) * rs[:, None] * gamma + beta).to(BF)
    return ln, mean, rstd


def _rows_of_bwd(dln, y1, mean, rstd, gamma, form):
    rs_ = _row_sum(form)
    xh = (y1.float() - mean[:, None]) * rstd[:, None]
    dv = dln.float()
    g = dv * gamma
    m1 = (rs_(g) * (1.0 / D))[:, None]
    m2 = (rs_(g * xh) * (1.0 / D))[:, None]
    dy1 = (rstd[:, None] * (g - m1 - xh * m2)).to(BF)
    return xh, dv, g, dy1


def emul_panel_ln_bwd(dln, y1, mean, rstd, gamma, pad_row_in_dbeta=False, dgamma_from_g=False,
                      copy_last_row_to_pad=False):
    """(dy1 [panels * 128][512] bf16 with zero pad rows, part [panels][3][512] fp32) as
    rowpanel_kernel<2> forms them from its dln: a lane's partial takes its 8 row blocks in turn (row
    16 rb + l16 of the panel), then the 16 lanes meet by an xor butterfly (1, 2, 4, 8). Pad rows
    contribute exact zeros. Planted: the pad rows' dbeta terms taken from row M - 1; dgamma summed from
    g = dln gamma; row M - 1's dy1 written into the pad rows."""
    M = dln.shape[0]
    P = panels(M)
    xh, dv, g, dy1 = _rows_of_bwd(dln, y1, mean, rstd, gamma, "panel")

    def padded(v, fill_last=False):
        out = torch.zeros(P * 128, D)
        out[:M] = v
        if fill_last:
            out[M:] = v[M - 1]
        return out

    def colsum(t):
        t = t.reshape(P, 8, 16, D)
        s = torch.zeros(P, 16, D)
        for rb in range(8):
            s = s + t[:, rb]
        l = torch.arange(16)
        for o in (1, 2, 4, 8):
            s = s + s[:, l ^ o]
        return s[:, 0]
    part = torch.stack([colsum(padded((g if dgamma_from_g else dv) * xh)), colsum(padded(dv, pad_row_in_dbeta)),
                        colsum(padded(dy1.float()))], 1)
    out = torch.zeros(P * 128, D, dtype=BF)
    out[:M] = dy1
    if copy_last_row_to_pad:
        out[M:] = dy1[M - 1]
    return out, part


def emul_ln_bwd3(dln, y1, mean, rstd, gamma, nblocks):
    """(dy1 [M][512] bf16, part [nblocks][3][512]) as ln_bwd3_kernel: wave w of block b takes rows
    4 b + w + 4 nblocks k in turn, the block adds its 4 waves in turn; a block without rows writes zeros."""
    M = dln.shape[0]
    xh, dv, g, dy1 = _rows_of_bwd(dln, y1, mean, rstd, gamma, "wave")
    W = 4 * nblocks
    trips = -(-M // W)

    def colsum(t):
        tp = torch.zeros(trips * W, D)
        tp[:M] = t
        tp = tp.reshape(trips, W, D)
        acc = torch.zeros(W, D)
        for k in range(trips):
            acc = acc + tp[k]
        a = acc.reshape(nblocks, 4, D)
        return ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]
    return dy1, torch.stack([colsum(dv * xh), colsum(dv), colsum(dy1.float())], 1)


def emul_sum_slabs(slabs, alpha, out_bf16, skip_remainder=False):
    """triad_sum_slabs in fp32 on the path the entry point takes for (S, n); alpha a Python float holding
    the fp32 value (1.0 for NULL). Planted: the S % 4 remainder slabs of the streaming path skipped."""
    S, n = slabs.shape
    a = torch.tensor(alpha, dtype=F32)
    z = torch.zeros(n)
    if slab_path(S, n) == "reduce":
        red = []
        for sl in range(16):
            c = [z, z, z, z]
            i = sl
            while i + 48 < S:
                c = [c[j] + slabs[i + 16 * j] for j in range(4)]
                i += 64
            while i < S:
                c[0] = c[0] + slabs[i]
                i += 16
            red.append((c[0] + c[1]) + (c[2] + c[3]))
        t = z
        for sl in range(16):
            t = t + red[sl]
    else:
        c = [z, z, z, z]
        i = 0
        while i + 3 < S:
            c = [c[j] + slabs[i + j] for j in range(4)]
            i += 4
        if not skip_remainder:
            while i < S:
                c[0] = c[0] + slabs[i]
                i += 1
        t = (c[0] + c[1]) + (c[2] + c[3])
    t = t * a
    return t.to(BF) if out_bf16 else t


def _dma_pass(X, per):
    """One pass of colsum_dma_kernel over X [rows][cols] fp32: per split of `per` rows, a thread adds
    every other row (parity of the row within the split; chunks of 16 keep it) in turn, then the two
    parities meet."""
    rows = X.shape[0]
    out = []
    for r0 in range(0, rows, per):
        blk = X[r0:r0 + per]
        a = [torch.zeros(X.shape[1]), torch.zeros(X.shape[1])]
        for i in range(blk.shape[0]):
            a[i & 1] = a[i & 1] + blk[i]
        out.append(a[0] + a[1])
    return torch.stack(out)


def emul_colsum_dma(X, alpha, out_bf16, sum_masked=False):
    """triad_colsum_dma over X [rows][cols] bf16 (the valid columns): the first pass into the splits'
    fp32 partials, the second over them, alpha once. Planted: the masked lanes of the last 256-column
    tile -- they re-read the tile's last valid 16 bytes -- added into those 8 columns."""
    rows, cols = X.shape
    S = colsum_dma_splits(rows, cols)
    Xf = X.float()
    if sum_masked and cols % 256:
        Xf = Xf.clone()
        Xf[:, cols - 8:] = Xf[:, cols - 8:] * (1 + (256 - cols % 256) // 8)
    part = _dma_pass(Xf, -(-rows // S))
    t = torch.tensor(alpha, dtype=F32) * _dma_pass(part, part.shape[0])[0]
    return t.to(BF) if out_bf16 else t
