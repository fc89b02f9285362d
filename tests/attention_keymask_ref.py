"""Key-padding masks in the attention kernels of csrc/attention.hip (triad_attn_fwd_keymask,
triad_attn_bwd_keymask, triad_attn_keymask_pack): mask families, the host restatement of the packing,
fp64 references with bounds, and an fp32 / bf16 emulation of the three masked kernels with planted
errors. No device needed; tests/test_attention_keymask_conformance_gpu.py applies the references to
what the kernels return, tests/test_attention_keymask_checks_cpu.py to the emulation.

A key mask is (B, N) bool, True = the key takes part, one row per sample for all heads. Nothing new
is derived or fitted here: masked attention on (N, mask) IS unmasked attention on the sample's
compacted key set, so the reference of sample b is tests/attention_ref.py's fwd_ref / bwd_ref on
(q[b], k[b, set], v[b, set], keep[b, :, :, set]). They take N from the queries, so nkt(N) and mfma2(N)
stay those of the full tile count the kernel sums over (a cleared key is a slot that adds an exact
zero). dk / dv are scattered back with reference 0 and bound 0 at cleared keys; a sample with no key
set has out = dq = dk = dv = 0 with bound 0 and lse = -inf (`ratio` wants -inf there exactly).
"""
import math

import numpy as np
import torch

from tests import attention_ref as R

BF, F32 = R.BF, R.F32
MASK_FAMILIES = ("full", "prefix", "scattered", "single", "empty")


# ---- masks ----------------------------------------------------------------------------------------------

def prefix_lengths(N):
    """N, 1, ceil(N / 2) and every 32 j, 32 j + 1 below N (a word boundary and one past it)."""
    ls = [N, 1, (N + 1) // 2]
    for j in range(1, (N + 31) // 32):
        ls += [x for x in (32 * j, 32 * j + 1) if x < N]
    out = []
    for x in ls:
        if x not in out:
            out.append(x)
    return out


def prefix_mask(lengths, N):
    return torch.arange(N)[None, :] < torch.tensor(lengths)[:, None]


def masks(family, B, N, seed=0):
    """-> list of (B, N) bool masks of the family (one, except `prefix`: as many as it takes to give
    every length of prefix_lengths(N) to some sample). Content differs per sample where it can."""
    g = R._gen(11, B, N, seed)
    if family == "full":
        return [torch.ones(B, N, dtype=torch.bool)]
    if family == "prefix":
        ls = prefix_lengths(N)
        while len(ls) % B:
            ls.append(ls[len(ls) % len(prefix_lengths(N))])
        return [prefix_mask(ls[i:i + B], N) for i in range(0, len(ls), B)]
    scattered = torch.rand(B, N, generator=g) < 0.5
    scattered[torch.arange(B), torch.randint(0, N, (B,), generator=g)] = True    # at least one per sample
    if family == "scattered":
        return [scattered]
    if family == "single":
        m = torch.zeros(B, N, dtype=torch.bool)
        m[:, N - 1] = True
        return [m]
    if family == "empty":
        m = scattered.clone()
        m[1] = False
        if B > 2:
            m[2] = torch.arange(N) < (N + 1) // 2
        return [m]
    raise KeyError(family)


def pack_words(mask, past_n=0):
    """Host restatement of triad_attn_keymask_pack: (B, N) bool / uint8 (non-zero = keep) -> (B,
    ceil(N / 32)) uint32 numpy, bit j of word kt = key 32 kt + j; the bits past N in the last word
    are `past_n` (the pack writes 0; the tests of the attention entry points set them to 1)."""
    m = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask) != 0
    B, N = m.shape
    wpr = (N + 31) // 32
    pad = np.full((B, wpr * 32), bool(past_n))
    pad[:, :N] = m
    return (pad.reshape(B, wpr, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def words_tensor(words):
    """uint32 numpy words -> int32 torch tensor (the dtype the device buffers have)."""
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32).copy())


# ---- fp64 references by compaction ------------------------------------------------------------------------

def ratio(got, ref, bound):
    """R.ratio, except that where the reference is -inf (lse of a sample with no key) got must be -inf."""
    inf = torch.isinf(ref)
    if bool(inf.any()):
        if not torch.equal(got[inf].double(), ref[inf].double()):
            return float("nan")
        if bool(inf.all()):
            return 0.0
    return R.ratio(got[~inf], ref[~inf], bound[~inf])


def _cat(parts):
    return {n: tuple(torch.cat([p[n][i] for p in parts], 0) for i in range(2)) for n in parts[0]}


def fwd_ref(q, k, v, scale, mask, keep=None, p=0.0):
    """As R.fwd_ref with a (B, N) key mask."""
    parts = []
    for b in range(q.shape[0]):
        idx = mask[b].nonzero().squeeze(-1)
        s = slice(b, b + 1)
        if idx.numel() == 0:
            z = torch.zeros(q[s].shape, dtype=torch.float64)
            ninf = torch.full((1, q.shape[2], q.shape[1]), -math.inf, dtype=torch.float64)
            parts.append({"out": (z, z.clone()), "lse": (ninf, torch.zeros_like(ninf))})
            continue
        parts.append(R.fwd_ref(q[s], k[s][:, idx], v[s][:, idx], scale, None if keep is None else keep[s][..., idx], p))
    return _cat(parts)


def bwd_ref(q, k, v, o, lse, do, scale, mask, keep=None, p=0.0, lse_err=None, o_err=None):
    """As R.bwd_ref with a (B, N) key mask; dk, dv are 0 with bound 0 at cleared keys."""
    parts = []
    B, N, H, D = q.shape
    for b in range(B):
        idx = mask[b].nonzero().squeeze(-1)
        s = slice(b, b + 1)
        if idx.numel() == 0:
            z = torch.zeros(1, N, H, D, dtype=torch.float64)
            DO, O = R._bh(do[s]), R._bh(o[s])
            e = (64 + 1) * R.U * (DO.abs() * O.abs()).sum(-1)
            if o_err is not None:
                e = e + (DO.abs() * R._bh(o_err[s])).sum(-1)
            parts.append({"delta": ((DO * O).sum(-1), e), "dq": (z, z.clone()), "dk": (z.clone(), z.clone()),
                          "dv": (z.clone(), z.clone())})
            continue
        r = R.bwd_ref(q[s], k[s][:, idx], v[s][:, idx], o[s], lse[s], do[s], scale,
                      None if keep is None else keep[s][..., idx], p,
                      None if lse_err is None else lse_err[s], None if o_err is None else o_err[s])
        for n in ("dk", "dv"):
            full = [torch.zeros(1, N, H, D, dtype=torch.float64) for _ in range(2)]
            for f, t in zip(full, r[n]):
                f[:, idx] = t
            r[n] = tuple(full)
        parts.append(r)
    return _cat(parts)


# ---- fp32 / bf16 emulation of the three masked kernels, from the packed words -------------------------------

PLANTS = ("mask ignored", "word row taken by bh instead of b", "bit order reversed within a word",
          "bits past N honoured", "a cleared key counted in l", "dkv kernel reads the query's bit",
          "dk / dv of a cleared key not zeroed", "empty sample produces NaN")


def _bits(words, B, H, N, plant=None, width=None):
    """(B, H, W) bool: the bit the kernels read for key j of (sample b, head h); W = 32 nkt when
    `width` asks for the padded slots. words: (B, wpr) uint32 numpy."""
    wpr = words.shape[1]
    W = wpr * 32 if width is None else width
    j = np.arange(W)
    sh = (31 - (j & 31)) if plant == "bit order reversed within a word" else (j & 31)
    out = np.zeros((B, H, W), dtype=bool)
    for b in range(B):
        for h in range(H):
            row = (b * H + h) % B if plant == "word row taken by bh instead of b" else b
            out[b, h] = (words[row, j >> 5].astype(np.uint64) >> sh.astype(np.uint64)) & np.uint64(1)
    if plant == "mask ignored":
        out[:] = True
    return torch.from_numpy(out)


def _pad_keys(t, W):
    """(B, H, N, 64) -> (B, H, W, 64) with the zero rows the kernels stage past N."""
    B, H, N, D = t.shape
    return torch.cat([t, torch.zeros(B, H, W - N, D, dtype=t.dtype)], 2)


def _valid(words, B, H, N, plant):
    """(B, H, 32 nkt) bool: the key slots that take part as the (planted) kernel sees them."""
    W = R.nkt(N) * 32
    bits = _bits(words, B, H, N, plant, W)
    if plant != "bits past N honoured":
        bits = bits & (torch.arange(W) < N)
    return bits


def emul_fwd(q, k, v, scale, words, keep=None, p=0.0, plant=None):
    """-> (out bf16 (B, N, H, 64), lse fp32 (B, H, N)) with the forward kernel's rounding points and
    guards; words (B, wpr) uint32 numpy as the kernel is handed them."""
    B, N, H, _ = q.shape
    W = R.nkt(N) * 32
    Q, K, V = R._f(q), _pad_keys(R._f(k), W), _pad_keys(R._f(v), W)
    valid = _valid(words, B, H, N, plant)[:, :, None, :]
    s = torch.tensor(scale, dtype=F32)
    c2 = s * R.LOG2E_F
    raw = Q @ K.transpose(-1, -2)
    acc = torch.where(valid, raw, torch.tensor(-math.inf))
    m = acc.amax(-1, keepdim=True)
    mo = m * c2
    if plant != "empty sample produces NaN":
        mo = torch.where(m == -math.inf, torch.zeros_like(mo), mo)
    pr = torch.exp2(R._fma(acc, c2, -mo))
    if plant == "a cleared key counted in l":
        l = (torch.exp2(R._fma(raw, c2, -mo)) * (torch.arange(W) < N)).sum(-1, keepdim=True)
    else:
        l = pr.sum(-1, keepdim=True)
    if keep is not None:
        pr = pr * torch.cat([keep, torch.zeros(B, H, N, W - N, dtype=torch.bool)], -1)
    ds = torch.tensor(R.drop_scale(p) if keep is not None else 1.0, dtype=F32)
    o = pr.to(BF).float() @ V
    if plant == "empty sample produces NaN":
        out = o * (ds / l)
    else:
        out = torch.where(l == 0, torch.zeros_like(o), o * (ds / l))
    return R._store(out), (m * s + l.log()).squeeze(-1)


def emul_bwd(q, k, v, o, lse, do, scale, words, keep=None, p=0.0, plant=None):
    """-> (dq, dk, dv bf16 (B, N, H, 64), delta fp32 (B, H, N)) with the two backward kernels' rounding
    points and selects."""
    B, N, H, _ = q.shape
    W = R.nkt(N) * 32
    Q, K, V, O, DO = R._f(q), _pad_keys(R._f(k), W), _pad_keys(R._f(v), W), R._f(o), R._f(do)
    valid_q = _valid(words, B, H, N, plant)[:, :, None, :]                 # dq kernel: the key's bit
    if plant == "dkv kernel reads the query's bit":
        qbits = _valid(words, B, H, N, None)[:, :, :N]
        valid_k = qbits[:, :, :, None].expand(B, H, N, W) & (torch.arange(W) < N)
    elif plant == "dk / dv of a cleared key not zeroed":
        valid_k = (torch.arange(W) < N).expand(B, H, 1, W)
    else:
        valid_k = valid_q
    s = torch.tensor(scale, dtype=F32)
    c2 = s * R.LOG2E_F
    acc = Q @ K.transpose(-1, -2)
    e = torch.exp2(R._fma(acc, c2, -(lse.float() * R.LOG2E_F)[..., None]))
    delta = (DO * O).sum(-1, keepdim=True)
    dp = DO @ V.transpose(-1, -2)
    ds = torch.tensor(R.drop_scale(p) if keep is not None else 1.0, dtype=F32)
    M = torch.ones_like(e) if keep is None else torch.cat([keep.float(), torch.zeros(B, H, N, W - N)], -1)
    zero = torch.zeros_like(e)
    if plant == "empty sample produces NaN":     # multiplied by a 0 / 1 mask instead of selected: inf * 0
        pq, pk = e * valid_q, e * valid_k
    else:
        pq, pk = torch.where(valid_q, e, zero), torch.where(valid_k, e, zero)
    dq = (pq * (dp * (M * ds) - delta)).to(BF).float() @ K * s
    dk = ((pk * (dp * (M * ds) - delta)).to(BF).float().transpose(-1, -2) @ Q) * s
    dv = (pk * (M * ds)).to(BF).float().transpose(-1, -2) @ DO
    if plant != "dk / dv of a cleared key not zeroed":    # the store's own select, by the key's bit
        rows = valid_q[:, :, 0]
        dk = torch.where(rows[..., None], dk, torch.zeros_like(dk))
        dv = torch.where(rows[..., None], dv, torch.zeros_like(dv))
    return R._store(dq), R._store(dk[:, :, :N]), R._store(dv[:, :, :N]), delta.squeeze(-1)
