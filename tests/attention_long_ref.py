"""What the streaming attention kernels of csrc/attention_long.hip (triad_attn_long_fwd,
triad_attn_long_bwd, triad_attn_long_dropmask; 321 <= N <= 2048) add to tests/attention_ref.py: the
forward's bound with the online-softmax terms, the `rising` input family, the keep-word layout, and
plain-torch fp32 / bf16 emulations of the three kernels in their chunked order, clean and with one
planted error. No device needed. References, the other bounds, the five input families, `ratio` and
`passes` are attention_ref's, imported as they are.

The kernels stream the other side of each product in chunks of KC = 64 rows (two 32-row MFMA
tiles); nch = ceil(N / 64). Notation of attention_ref.py: u = 2^-24, r = 2^-8, EXP = 4 u.

* Forward (online rescaling). Per chunk c the kernel takes the running max m_c = max(m_{c-1}, chunk
  max) of the fp32 scores, mo_c = fl(m_c c2), and forms
      p^_k = exp2(fma(acc_k, c2, -mo_c))                      k in chunk c
      alpha_c = exp2(fl(mo_{c-1} - mo_c))                     (exactly 1 where the max stood)
      l = fma(l, alpha_c, sum_chunk p^),  O = fl(O alpha_c) + P^ V (MFMA)
  The same fp32 number mo_c enters p^_k with one sign and alpha_{c+1} with the other, so in the
  product p^_k alpha_{c+1} ... alpha_last every intermediate mo cancels and the key is weighted by
  exp2(acc_k c2 - mo_last), whatever the rounding of each m c2: the factor 2^(-m c2 d) common to the
  row is the final one and cancels in out as before. The fma's rounding acts on |arg| = (m_c - s_k) c2
  <= (m - s_k) c2, inside the 3 u a_k of eps_k. What is new, per key and per LATER chunk j:
      EXP                     alpha_j's v_exp_f32
      u |mo_{j-1} - mo_j|     the rounding of the difference (ln 2 < 1 dropped)
      u                       the product with alpha_j (fl(O alpha) for out, the fma for l)
  Summed over the later chunks the differences telescope to (m - m_c(k)) c2, taken from the fp64
  scores (their own error times u is second order). A chunk whose max stood contributes nothing
  (alpha = 1, products exact), but which chunks rise is decided by the fp32 scores, so the bound
  counts every later chunk:
      extra_k = (nch - 1 - c(k)) (EXP + u) + u (m - m_c(k)) log2e          <= 31 * 5 u + small
      eps_k(long) = eps_k + extra_k
  in both places eps_k stands in attention_ref's pre_out and lse bounds (sum_k P w |v| eps and
  sum_k P eps). l takes 32 adds per chunk on a lane, one fma per chunk and the half-wave exchange;
  keys >= N of the last chunk have p^ = 0 exactly (score -inf) and add nothing, so the
  (16 nkt + 4) u and (16 nkt + 1) u of the short form become (16 nkt + nch + 4) u and
  (16 nkt + nch + 1) u with nkt = ceil(N / 32). The second MFMA still sums 32 nkt non-zero key slots in
  order (the rescales between them are the u above): mfma2(N) as it is. log l <= log 2048.
  In numbers: extra <= 31 * 5 u ~ 1e-5 against r = 3.9e-3, so the out bound grows by well under 3 %
  (asserted in tests/test_attention_long_checks_cpu.py); the lse bound, whose sum_k P eps is itself
  ~1e-5, can about double for the keys of the first chunks.
* Backward. Per 32 x 32 tile the dq and dk / dv kernels do the arithmetic of the short kernels: p^
  from the fp32 lse, delta, dS, bf16 operands, fp32 MFMA sums over the key (query) tiles in order,
  zero rows past N adding exact zeros. attention_ref.bwd_ref's bounds hold unchanged, with
  nkt = ceil(N / 32) up to 64.

Keep words: wpr(N) = 2 nch words per row in both layouts (rows padded to whole chunks), against the
short form's ceil(N / 32); the two differ when ceil(N / 32) is odd (N = 321, 1374, not 499).
"""
import functools
import math

import torch

from tests import attention_ref as R

KC = 64
U, R8, EXP, LOG, FLUSH, ACC64 = R.U, R.R8, R.EXP, R.LOG, R.FLUSH, R.ACC64
BF, F32, F64 = R.BF, R.F32, R.F64
FAMILIES = R.FAMILIES + ("rising",)


def nch(N):
    return (N + KC - 1) // KC


def wpr(N):
    """Keep words per row of triad_attn_long_dropmask."""
    return 2 * nch(N)


# ---- input families ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=8)
def case(family, B, H, N, seed):
    """attention_ref.case plus
    rising   gauss with a ramp along one direction w (+-1 per dim, per head): k_j += 0.5 (j / 64) w,
             q += 0.5 w, so a query's logits gain about 2 per 64-key chunk (q . w ~ 32 +- 12, times
             scale 1/8 times 0.5): the running max of nearly every query rises in every chunk and
             the weight sits on the last chunks. Do not modify."""
    if family != "rising":
        return R.case(family, B, H, N, seed)
    g = R._gen(6, B, H, N, seed)
    q, k = (torch.randn(B, N, H, R.HD, generator=g) * 1.5 for _ in range(2))
    v, do = torch.randn(B, N, H, R.HD, generator=g) * 1.5, torch.randn(B, N, H, R.HD, generator=g)
    w = torch.randint(0, 2, (1, 1, H, R.HD), generator=g).float() * 2 - 1
    k = k + 0.5 * (torch.arange(N).float() / KC).view(1, N, 1, 1) * w
    q = q + 0.5 * w
    return dict(q=q.to(BF), k=k.to(BF), v=v.to(BF), do=do.to(BF))


def rises(q, k, scale):
    """Mean number of chunks (of nch - 1) in which a query's running max rises (fp64 scores)."""
    S = (R._bh(q) @ R._bh(k).transpose(-1, -2)) * scale
    N = S.shape[-1]
    pad = torch.full((*S.shape[:-1], nch(N) * KC - N), -math.inf, dtype=F64)
    cm = torch.cat([S, pad], -1).view(*S.shape[:-1], nch(N), KC).amax(-1).cummax(-1).values
    return float((cm[..., 1:] > cm[..., :-1]).double().sum(-1).mean())


# ---- the forward's reference and bound -------------------------------------------------------------

def fwd_ref(q, k, v, scale, keep=None, p=0.0):
    """attention_ref.fwd_ref with eps_k(long) and the l terms of the streaming forward (module
    docstring). -> {"out": (ref, bound), "lse": (ref, bound)}."""
    Q, K, V = R._bh(q), R._bh(k), R._bh(v)
    N = Q.shape[2]
    nc, nkt = nch(N), R.nkt(N)
    S = (Q @ K.transpose(-1, -2)) * scale
    m = S.amax(-1, keepdim=True)
    E = (S - m).exp()
    L = E.sum(-1, keepdim=True)
    P = E / L
    lse = m + L.log()
    W = P * R._weights(keep, p, P)
    out = W @ V
    eps = scale * ACC64 * (Q.abs() @ K.abs().transpose(-1, -2)) + 3 * U * (S - m).abs() + EXP
    # the online-softmax terms: every later chunk, and the telescoped rise of the running max
    cidx = torch.arange(N) // KC
    pad = torch.full((*S.shape[:-1], nc * KC - N), -math.inf, dtype=F64)
    run = torch.cat([S, pad], -1).view(*S.shape[:-1], nc, KC).amax(-1).cummax(-1).values   # (B, H, N, nch)
    rise = (m - run[..., cidx]) * math.log2(math.e)
    eps = eps + (nc - 1 - cidx).double() * (EXP + U) + U * rise
    Wv = W @ V.abs()
    avg = (P * eps).sum(-1, keepdim=True)
    pre = ((W * (eps + R8)) @ V.abs() + R.mfma2(N) * Wv + out.abs() * (avg + (16 * nkt + nc + 4) * U)
           + FLUSH * V.abs().sum(-2, keepdim=True))
    b_out = pre + R8 * (out.abs() + pre)
    b_lse = 2 * U * m.abs() + avg + (16 * nkt + nc + 1) * U + LOG * L.log().abs() + U * lse.abs()
    return {"out": (R._bn(out), R._bn(b_out)), "lse": (lse.squeeze(-1), b_lse.squeeze(-1))}


bwd_ref = R.bwd_ref   # unchanged (module docstring)


# ---- the keep words ----------------------------------------------------------------------------------

def keep_short_words(keep):
    """The mask a kernel sees that indexes the long form's keep words with the short form's
    ceil(N / 32) words per row: word (row, kt) read at flat index row * nkt + kt of an array laid out
    with wpr words per row. keep (B, H, N, N) bool [b, h, q, key] -> the same shape."""
    B, H, N, _ = keep.shape
    w, nkt = wpr(N), R.nkt(N)
    bits = torch.zeros(B * H * N, w * 32, dtype=torch.bool)
    bits[:, :N] = keep.reshape(B * H * N, N)
    words = bits.view(B * H * N * w, 32)
    idx = (torch.arange(B * H * N)[:, None] * nkt + torch.arange(nkt)[None, :]).reshape(-1)
    return words[idx].view(B * H * N, nkt * 32)[:, :N].reshape(B, H, N, N)


# ---- emulations ----------------------------------------------------------------------------------------

def emul_fwd(q, k, v, scale, keep=None, p=0.0, skip_rescale=None, l_not_rescaled=False, drop_last_chunk=False,
             count_pad_keys=False, v_lag=False, short_words=False):
    """-> (out bf16 (B, N, H, 64), lse fp32 (B, H, N)) in the forward kernel's order: chunks of 64
    keys, running m / mo / l / O in fp32, bf16 probabilities into the second product.
    Planted errors: skip_rescale = c (chunk c's alpha taken as 1 for O and l), l_not_rescaled (O
    rescaled, l not), drop_last_chunk, count_pad_keys (the zero rows past N of the last chunk counted
    in l: score 0 instead of -inf), v_lag (chunk c of K with chunk c - 1 of V), short_words (keep
    words indexed with ceil(N / 32) per row)."""
    Q, K, V = R._f(q), R._f(k), R._f(v)
    N = Q.shape[2]
    if keep is not None and short_words:
        keep = keep_short_words(keep)
    s = torch.tensor(scale, dtype=F32)
    c2 = s * R.LOG2E_F
    acc = Q @ K.transpose(-1, -2)
    m = torch.full((*Q.shape[:3], 1), -math.inf, dtype=F32)
    mo = m.clone()
    l = torch.zeros_like(m)
    O = torch.zeros_like(Q)
    nc = nch(N)
    for c in range(nc - 1 if drop_last_chunk else nc):
        lo, hi = c * KC, min(N, (c + 1) * KC)
        a = acc[..., lo:hi]
        mn = torch.maximum(m, a.amax(-1, keepdim=True))
        if count_pad_keys and hi - lo < KC:
            mn = torch.maximum(mn, torch.zeros_like(mn))
        mon = mn * c2
        alpha = torch.exp2(mo - mon)
        pr = torch.exp2(R._fma(a, c2, -mon))
        ls = pr.sum(-1, keepdim=True)
        if count_pad_keys and hi - lo < KC:
            ls = ls + (KC - (hi - lo)) * torch.exp2(-mon)
        one = torch.ones_like(alpha)
        a_o = one if skip_rescale == c else alpha
        a_l = one if (skip_rescale == c or (l_not_rescaled and c > 0)) else alpha
        l = R._fma(l, a_l, ls)
        if keep is not None:
            pr = pr * keep[..., lo:hi]
        Vc = V[:, :, lo - KC:lo - KC + (hi - lo)] if (v_lag and c > 0) else V[:, :, lo:hi]
        O = O * a_o + pr.to(BF).float() @ Vc
        m, mo = mn, mon
    ds = torch.tensor(R.drop_scale(p) if keep is not None else 1.0, dtype=F32)
    out = O * (ds / l)
    return R._store(out), (m * s + l.log()).squeeze(-1)


def emul_bwd(q, k, v, o, lse, do, scale, keep=None, p=0.0, stat_chunk0=False, short_words=False,
             dv_no_drop_scale=False, dq_no_scale=False):
    """-> (dq, dk, dv bf16 (B, N, H, 64), delta fp32 (B, H, N)) in the two backward kernels' order:
    dq summed over key chunks, dk / dv over query chunks, bf16 dS and P operands.
    Planted errors: stat_chunk0 (the dk / dv kernel reads lse and delta of query chunk 0 for every
    chunk), short_words (both kernels index the keep words with ceil(N / 32) per row),
    dv_no_drop_scale, dq_no_scale."""
    Q, K, V, O, DO = R._f(q), R._f(k), R._f(v), R._f(o), R._f(do)
    N = Q.shape[2]
    if keep is not None and short_words:
        keep = keep_short_words(keep)
    s = torch.tensor(scale, dtype=F32)
    c2 = s * R.LOG2E_F
    acc = Q @ K.transpose(-1, -2)
    lse2 = (lse.float() * R.LOG2E_F)[..., None]
    delta = (DO * O).sum(-1, keepdim=True)
    dp = DO @ V.transpose(-1, -2)
    ds = torch.tensor(R.drop_scale(p) if keep is not None else 1.0, dtype=F32)
    M = torch.ones_like(acc) if keep is None else keep.float()
    # dq kernel: key chunks
    pr = torch.exp2(R._fma(acc, c2, -lse2))
    dS = (pr * (dp * (M * ds) - delta)).to(BF).float()
    dq = torch.zeros_like(Q)
    for c in range(nch(N)):
        lo, hi = c * KC, min(N, (c + 1) * KC)
        dq = dq + dS[..., lo:hi] @ K[:, :, lo:hi]
    if not dq_no_scale:
        dq = dq * s
    # dk / dv kernel: query chunks with their staged lse log2e and delta
    if stat_chunk0:
        idx = torch.arange(N) % KC
        lse_k, delta_k = lse2[:, :, idx], delta[:, :, idx]
    else:
        lse_k, delta_k = lse2, delta
    pr = torch.exp2(R._fma(acc, c2, -lse_k))
    pd = (pr * M if dv_no_drop_scale else pr * (M * ds)).to(BF).float()
    dS = (pr * (dp * (M * ds) - delta_k)).to(BF).float()
    dk, dv = torch.zeros_like(K), torch.zeros_like(V)
    for c in range(nch(N)):
        lo, hi = c * KC, min(N, (c + 1) * KC)
        dk = dk + dS[:, :, lo:hi].transpose(-1, -2) @ Q[:, :, lo:hi]
        dv = dv + pd[:, :, lo:hi].transpose(-1, -2) @ DO[:, :, lo:hi]
    return R._store(dq), R._store(dk * s), R._store(dv), delta.squeeze(-1)
