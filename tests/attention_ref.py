"""fp64 references, derived per-element bounds, seeded input families and fp32 / bf16 emulations for
the attention kernels of csrc/attention.hip (triad_attn_fwd, triad_attn_bwd and their _dropout
forms). No device needed: tests/test_attention_conformance_gpu.py applies the references and bounds
to what the kernels return, tests/test_attention_checks_cpu.py applies them to the emulations below,
intact (must pass) and with one planted error (must fail).

Tensors are (B, N, H, 64) bf16 as the ABI takes them; lse, delta are (B, H, N); a keep mask is
(B, H, N, N) bool indexed [b, h, query, key]. Every reference is the fp64 result on the operands
the kernel reads (bf16 values and, for the backward, the fp32 lse and the bf16 o it is handed: exact
inputs). The normaliser keeps dropped keys, as the kernel does: with w = keep / (1 - p),

    S = scale Q K^T,  P = softmax(S),  lse = logsumexp(S),  out = (P w) V
    delta = rowsum(dO o),  p = exp(S - lse),  dP = dO V^T,  dS = p (w dP - delta)
    dq = scale dS K,  dk = scale dS^T Q,  dv = (p w)^T dO

Bounds are first-order in u = 2^-24 and r = 2^-8 (the largest relative error of one rounding to
bf16), per element, and follow the rounding steps of the code; nothing is fitted to what the kernels
return. All sums below run over keys k (queries for dk, dv) with the magnitudes of the reference.

* A score is an fp32 MFMA sum of 64 exact bf16 products: |d acc| <= 2 (64 + 2) u (|q| . |k|); the
  factor 2 covers an accumulator that does not round like IEEE at every step (as in
  tests/vit_rows_ref.py). In natural-log units eS = scale * that. dP = dO . v likewise (eP).
* exp2 is the raw v_exp_f32, the forward's log is logf. The guides do not state their accuracy:
  ASSUMED 1 ulp each and given a factor 2, EXP = LOG = 4 u (relative). Far below r either way.
  Results below 2^-126 flush to zero (at the exp, at a product and at the bf16 cast): an absolute
  FLUSH = 2^-124 per probability.
* Forward. arg = fma(acc, c2, -fl(m c2)), c2 = fl(scale * log2e) (two roundings). The fma forms
  (acc - m) c2 exactly, so with a = |S - max S| the probability p^_k = exp2(arg) has the relative
  error
      eps_k = eS_k + 3 u a_k + EXP           (2 u for c2, u for the fma's result)
  besides the factor 2^(-m c2 d), |d| <= u, that fl(m c2) puts on every key of the row alike: it
  cancels in out and enters lse as u |m scale|. p^ is rounded to bf16 (r) for the second MFMA, an
  fp32 sum over the 32 nkt key slots; l sums the unrounded p^ in fp32, 16 nkt adds on a lane and one
  exchange; inv = w / l and the product with it round (3 u); one bf16 store:
      pre_out = sum_k P_k w_k |v_k| (eps_k + r) + 2 (32 nkt + 2) u sum_k P_k w_k |v_k|
                + |out| (sum_k P_k eps_k + (16 nkt + 4) u) + FLUSH sum_k |v_k|
      out:  pre_out + r (|out| + pre_out)
      lse:  2 u |m scale| + sum_k P_k eps_k + (16 nkt + 1) u + LOG |log l| + u |lse|
  (fl(m scale) and fl(m c2) give the 2 u |m scale|; log l <= log 320, so a relative error of l is an
  absolute one of lse.)
* Backward. p^ = exp2(fma(acc, c2, -fl(lse log2e))) is recomputed from the fp32 lse. Nothing
  cancels here: c2's roundings act on |S| and the two of lse log2e on |lse|, so
      eta_k = eS_k + 2 u |S_k| + 2 u |lse| + u |S_k - lse| + EXP
  grows with |lse| (the `offset` family has |lse| up to a few hundred: 2 u |lse| ~ 4e-5, still far
  below r). delta is a chain of 32 fmas per half-wave and one add over exact bf16 pairs (64 terms):
      e_delta = (64 + 1) u sum_d |dO_d o_d|
  dS = p^ (fl(dp w) - delta): with T = w |dP| + |delta|,
      e_dS = |dS| (eta + u + r) + p (w eP + e_delta + 2 u T) + FLUSH (1 + T)
  (the subtraction cancels, so its operands' errors count against T, not against the difference;
  r is the bf16 rounding of dS before the second MFMA). Then, with X = K for dq and Q for dk,
      pre = scale (sum e_dS |X| + 2 (32 nkt + 2) u sum |dS| |X|) + u |ref|      (the final * scale)
      dq, dk:  pre + r (|ref| + pre)
      dv:      pre = sum_q (p w (eta + u + r) + FLUSH w) |dO| + 2 (32 nkt + 2) u sum_q p w |dO|,
               pre + r (|ref| + pre)
* Chained (the forward's own out and lse go into the backward, compared with the backward of the
  fp64 out and lse): the forward's bounds become input errors. eta grows by bound(lse) and e_delta
  by sum_d |dO_d| bound(out_d); the rest is unchanged (`lse_err`, `o_err` of bwd_ref).

Input families (each a function of (B, H, N, seed), from a seeded CPU generator): see `case`.
"""
import functools
import math

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
R8 = 2.0 ** -8
EXP = 4 * U       # v_exp_f32: 1 ulp assumed, times 2
LOG = 4 * U       # logf: 1 ulp assumed, times 2
FLUSH = 2.0 ** -124
ACC64 = 2.0 * (64 + 2) * U
HD = 64
SCALE = 0.125
LOG2E_F = torch.tensor(1.4426950408889634, dtype=F32)
FAMILIES = ("gauss", "peaked", "offset", "ties", "selector")


def f32(v):
    """The fp32 value a C float argument takes, as a Python float."""
    return float(torch.tensor(v, dtype=F32))


def drop_scale(p):
    """1.f / (1.f - p) as the entry points form it."""
    one = torch.tensor(1.0, dtype=F32)
    return float(one / (one - torch.tensor(p, dtype=F32)))


def nkt(N):
    return (N + 31) // 32


def mfma2(N):
    """Relative error of the second MFMA's fp32 sum over the 32 nkt key (query) slots."""
    return 2.0 * (32 * nkt(N) + 2) * U


def ratio(got, ref, bound):
    """Largest err / bound over the elements (NaN if anything is not finite)."""
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    return float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())


def passes(got, ref, bound):
    r = ratio(got, ref, bound)
    return r == r and r <= 1.0


def _bh(t):
    """(B, N, H, 64) -> (B, H, N, 64) fp64."""
    return t.double().permute(0, 2, 1, 3)


def _bn(t):
    """(B, H, N, 64) -> (B, N, H, 64)."""
    return t.permute(0, 2, 1, 3)


def _weights(keep, p, like):
    ds = drop_scale(p) if keep is not None else 1.0
    return (torch.ones_like(like) if keep is None else keep.to(like.dtype)) * ds


# ---- fp64 references with their bounds ----------------------------------------------------------

def fwd_ref(q, k, v, scale, keep=None, p=0.0):
    """-> {"out": (ref (B, N, H, 64), bound), "lse": (ref (B, H, N), bound)}; scale the fp32 value."""
    Q, K, V = _bh(q), _bh(k), _bh(v)
    N = Q.shape[2]
    S = (Q @ K.transpose(-1, -2)) * scale
    m = S.amax(-1, keepdim=True)
    E = (S - m).exp()
    L = E.sum(-1, keepdim=True)
    P = E / L
    lse = m + L.log()
    W = P * _weights(keep, p, P)
    out = W @ V
    eps = scale * ACC64 * (Q.abs() @ K.abs().transpose(-1, -2)) + 3 * U * (S - m).abs() + EXP
    Wv = W @ V.abs()
    avg = (P * eps).sum(-1, keepdim=True)
    pre = ((W * (eps + R8)) @ V.abs() + mfma2(N) * Wv + out.abs() * (avg + (16 * nkt(N) + 4) * U)
           + FLUSH * V.abs().sum(-2, keepdim=True))
    b_out = pre + R8 * (out.abs() + pre)
    b_lse = 2 * U * m.abs() + avg + (16 * nkt(N) + 1) * U + LOG * L.log().abs() + U * lse.abs()
    return {"out": (_bn(out), _bn(b_out)), "lse": (lse.squeeze(-1), b_lse.squeeze(-1))}


def bwd_ref(q, k, v, o, lse, do, scale, keep=None, p=0.0, lse_err=None, o_err=None):
    """o (B, N, H, 64) and lse (B, H, N) are the backward's inputs (any dtype; taken as exact unless
    lse_err (B, H, N) / o_err (B, N, H, 64) give their error). -> {name: (ref, bound)} for dq, dk,
    dv (B, N, H, 64) and delta (B, H, N)."""
    Q, K, V, O, DO = _bh(q), _bh(k), _bh(v), _bh(o), _bh(do)
    N = Q.shape[2]
    lse = lse.double()[..., None]
    S = (Q @ K.transpose(-1, -2)) * scale
    P = (S - lse).exp()
    delta = (DO * O).sum(-1, keepdim=True)
    e_delta = (64 + 1) * U * (DO.abs() * O.abs()).sum(-1, keepdim=True)
    if o_err is not None:
        e_delta = e_delta + (DO.abs() * _bh(o_err)).sum(-1, keepdim=True)
    dP = DO @ V.transpose(-1, -2)
    eP = ACC64 * (DO.abs() @ V.abs().transpose(-1, -2))
    M = _weights(keep, p, P)
    dS = P * (dP * M - delta)
    Pd = P * M
    eta = (scale * ACC64 * (Q.abs() @ K.abs().transpose(-1, -2)) + 2 * U * S.abs() + 2 * U * lse.abs()
           + U * (S - lse).abs() + EXP)
    if lse_err is not None:
        eta = eta + lse_err.double()[..., None]
    T = (dP * M).abs() + delta.abs()
    e_dS = dS.abs() * (eta + U + R8) + P * (M * eP + e_delta + 2 * U * T) + FLUSH * (1 + T)
    res = {"delta": (delta.squeeze(-1), e_delta.squeeze(-1))}
    for name, ref, e, a, X in (("dq", dS @ K, e_dS, dS.abs(), K),
                               ("dk", dS.transpose(-1, -2) @ Q, e_dS.transpose(-1, -2), dS.abs().transpose(-1, -2), Q)):
        ref = scale * ref
        pre = scale * (e @ X.abs() + mfma2(N) * (a @ X.abs())) + U * ref.abs()
        res[name] = (_bn(ref), _bn(pre + R8 * (ref.abs() + pre)))
    dv = Pd.transpose(-1, -2) @ DO
    pre = ((Pd * (eta + U + R8) + FLUSH * M).transpose(-1, -2) @ DO.abs()
           + mfma2(N) * (Pd.transpose(-1, -2) @ DO.abs()))
    res["dv"] = (_bn(dv), _bn(pre + R8 * (dv.abs() + pre)))
    return res


# ---- fp32 / bf16 emulations of the three kernels (plain torch), with the planted errors -----------

def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64, the sum rounds once more to fp32."""
    return (a.double() * b.double() + c.double()).float()


def _f(t):
    return t.float().permute(0, 2, 1, 3)


def _store(t):
    return t.to(BF).permute(0, 2, 1, 3).contiguous()


def misread_rows(t, s_true, s_wrong):
    """t (B, N, H, 64) as a kernel reads it that applies the row stride s_wrong to a buffer laid out
    with row stride s_true (zeros in the padding)."""
    B, N, H, D = t.shape
    flat = torch.zeros(B, N * max(s_true, s_wrong) + H * D, dtype=t.dtype)
    cols = torch.arange(H * D)
    flat[:, (torch.arange(N) * s_true)[:, None] + cols] = t.reshape(B, N, H * D)
    return flat[:, (torch.arange(N) * s_wrong)[:, None] + cols].reshape(B, N, H, D)


def emul_fwd(q, k, v, scale, keep=None, p=0.0, drop_last_key=False, count_pad_key=False, swap_keys=None,
             v_stride=None, head_shift=0, lse_no_log=False):
    """-> (out bf16 (B, N, H, 64), lse fp32 (B, H, N)) with the forward kernel's rounding points.
    Planted errors: drop_last_key (key N - 1 masked like a padded one), count_pad_key (the zero row
    N of the staged K counted in l), swap_keys = (i, j) (V rows i, j exchanged in the PV product, a
    wrong k-index permutation), v_stride = (true, wrong) row strides, head_shift (q of another
    head), lse_no_log."""
    if v_stride is not None:
        v = misread_rows(v, *v_stride)
    Q, K, V = _f(q), _f(k), _f(v)
    if head_shift:
        Q = Q.roll(head_shift, 1)
    s = torch.tensor(scale, dtype=F32)
    c2 = s * LOG2E_F
    acc = Q @ K.transpose(-1, -2)
    if drop_last_key:
        acc[..., -1] = -math.inf
    m = acc.amax(-1, keepdim=True)
    mo = m * c2
    pr = torch.exp2(_fma(acc, c2, -mo))
    l = pr.sum(-1, keepdim=True)
    if count_pad_key:
        l = l + torch.exp2(-mo)
    if keep is not None:
        pr = pr * keep
    if swap_keys is not None:
        i, j = swap_keys
        V = V.clone()
        V[:, :, [i, j]] = V[:, :, [j, i]]
    ds = torch.tensor(drop_scale(p) if keep is not None else 1.0, dtype=F32)
    out = (pr.to(BF).float() @ V) * (ds / l)
    lse = m * s if lse_no_log else m * s + l.log()
    return _store(out), lse.squeeze(-1)


def emul_bwd(q, k, v, o, lse, do, scale, keep=None, p=0.0, delta_half=False, mask_transposed_dkv=False,
             dv_no_drop_scale=False, dq_no_scale=False):
    """-> (dq, dk, dv bf16 (B, N, H, 64), delta fp32 (B, H, N)) with the two backward kernels'
    rounding points. Planted errors: delta_half (delta from dims 0..31), mask_transposed_dkv (the
    dk / dv kernel reads the keep bit of (key, q)), dv_no_drop_scale, dq_no_scale."""
    Q, K, V, O, DO = _f(q), _f(k), _f(v), _f(o), _f(do)
    s = torch.tensor(scale, dtype=F32)
    c2 = s * LOG2E_F
    acc = Q @ K.transpose(-1, -2)
    pr = torch.exp2(_fma(acc, c2, -(lse.float() * LOG2E_F)[..., None]))
    prod = DO * O
    delta = (prod[..., :32] if delta_half else prod).sum(-1, keepdim=True)
    dp = DO @ V.transpose(-1, -2)
    ds = torch.tensor(drop_scale(p) if keep is not None else 1.0, dtype=F32)
    Mq = torch.ones_like(pr) if keep is None else keep.float()
    Mk = Mq.transpose(-1, -2) if mask_transposed_dkv else Mq
    dS = pr * (dp * (Mq * ds) - delta)
    dq = dS.to(BF).float() @ K
    if not dq_no_scale:
        dq = dq * s
    dS2 = pr * (dp * (Mk * ds) - delta)
    dk = (dS2.to(BF).float().transpose(-1, -2) @ Q) * s
    pd = pr * Mk if dv_no_drop_scale else pr * (Mk * ds)
    dv = pd.to(BF).float().transpose(-1, -2) @ DO
    return _store(dq), _store(dk), _store(dv), delta.squeeze(-1)


# ---- seeded input families -------------------------------------------------------------------------

def _gen(*key):
    seed = 0
    for x in key:
        seed = seed * 1000003 + int(x)
    return torch.Generator().manual_seed(seed % (2 ** 31))


SEL_VALUES = torch.tensor([1.0, -1.0, 1.5, -1.5])
SEL_LEAD = 33.0   # the selected logit leads every other by at least this


def _selector(B, H, N, seed):
    """K[k] = 3 code[k] (code random +-1 in 64 dims), Q[q] = K[perm[q]], V and dO in {+-1, +-1.5}.
    One code book per case, its columns sign-flipped per (b, h) (the pairwise distances are the
    book's); perm per (b, h). The seed is advanced until every pair of codes differs in >= 15 of
    the 64 places: then the selected logit 72 leads every other by >= 9 * 2 * 15 / 8 = 33.75."""
    for attempt in range(200):
        g = _gen(5, B, H, N, seed, attempt)
        code = torch.randint(0, 2, (N, HD), generator=g).float() * 2 - 1
        ham = (HD - code @ code.t()) / 2 + torch.eye(N) * HD
        if N == 1 or float(ham.min()) >= 15:
            break
    else:
        raise AssertionError(f"selector: no code book with distance >= 15 at N {N}")
    flip = torch.randint(0, 2, (B, 1, H, HD), generator=g).float() * 2 - 1
    k = 3 * code[None, :, None, :] * flip                                  # (B, N, H, 64)
    perm = torch.stack([torch.randperm(N, generator=g) for _ in range(B * H)]).view(B, H, N)
    q = torch.gather(k, 1, perm.permute(0, 2, 1)[..., None].expand(B, N, H, HD))
    v = SEL_VALUES[torch.randint(0, 4, (B, N, H, HD), generator=g)]
    do = SEL_VALUES[torch.randint(0, 4, (B, N, H, HD), generator=g)]
    return dict(q=q.to(BF), k=k.to(BF), v=v.to(BF), do=do.to(BF), perm=perm)


@functools.lru_cache(maxsize=8)
def case(family, B, H, N, seed):
    """-> dict of q, k, v, do (B, N, H, 64) bf16 (and perm (B, H, N) for `selector`). Do not modify.
    gauss    N(0, 1) * 1.5 (logits of std ~2.3 at scale 1/8)
    peaked   q, k ~ N(0, 1) * 3.5: logits of std ~12, a few keys carry each row
    offset   gauss with one vector w (+-128 per dim) added to every key row: the softmax is that of
             the rows without w, but |q . w| scale is 100 .. 300 with both signs across queries, so
             the row max and lse are large
    ties     every key row equal: p = 1 / N exactly, out the column mean of V, the reference dq 0
    selector see _selector; the answer is known exactly: out[q] = V[perm[q]], dv[perm[q]] = dO[q]"""
    if family == "selector":
        c = _selector(B, H, N, seed)
        _assert_selector(c)
        return c
    g = _gen(FAMILIES.index(family), B, H, N, seed)
    std = 3.5 if family == "peaked" else 1.5
    q, k = (torch.randn(B, N, H, HD, generator=g) * std for _ in range(2))
    v, do = torch.randn(B, N, H, HD, generator=g) * 1.5, torch.randn(B, N, H, HD, generator=g)
    if family == "offset":
        k = k + 128.0 * (torch.randint(0, 2, (1, 1, H, HD), generator=g).float() * 2 - 1)
    if family == "ties":
        k = k[:, :1].expand(B, N, H, HD).contiguous()
    return dict(q=q.to(BF), k=k.to(BF), v=v.to(BF), do=do.to(BF))


def _assert_selector(c):
    """The two conditions the exact checks rest on: the selected logit leads every other by >=
    SEL_LEAD, and the fp64 out rounds to V[perm[q]] in bf16 for every element."""
    Q, K = _bh(c["q"]), _bh(c["k"])
    N = Q.shape[2]
    S = (Q @ K.transpose(-1, -2)) * SCALE
    sel = torch.gather(S, -1, c["perm"][..., None])
    others = S.scatter(-1, c["perm"][..., None], -math.inf)
    assert N == 1 or float((sel.squeeze(-1) - others.amax(-1)).min()) >= SEL_LEAD, "selector: lead below 33"
    out = fwd_ref(c["q"], c["k"], c["v"], SCALE)["out"][0]
    assert torch.equal(out.to(F32).to(BF), selected_rows(c["v"], c["perm"])), "selector: fp64 out != V[perm]"


def selected_rows(t, perm):
    """t (B, N, H, 64), perm (B, H, N) -> t[b, perm[b, h, q], h, :] at [b, q, h, :]."""
    B, N, H, D = t.shape
    return torch.gather(t, 1, perm.permute(0, 2, 1)[..., None].expand(B, N, H, D))


def cpu_keep(B, H, N, p, seed):
    """A seeded Bernoulli keep mask (B, H, N, N) for the CPU checks (the GPU tests use the mask the
    kernel drew)."""
    return torch.rand(B, H, N, N, generator=_gen(9, B, H, N, seed)) >= p
