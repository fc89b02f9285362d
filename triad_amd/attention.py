"""Backbone self-attention on the HIP kernels of csrc/attention.hip and csrc/attention_long.hip.

The reference's encoders (SajayR/TRIAD model.py:29-30,79-80,218-227: DINOv2, HuBERT,
DistilBERT) run softmax(Q K^T * scale) V over short sequences -- 261 visual tokens, 199 audio
frames, 32 text tokens -- with head dim 64. PyTorch-ROCm's flash-attention kernels are tuned for
long sequences; here each (sample, head) sequence sits in LDS and a wave keeps a whole 32-row
tile of scores in registers (exact softmax, no online rescaling). Used for attention with N <= 320
and head dim 64 in bf16, with or without dropout on the attention probabilities (keep bits from the
common.h counter hash, stored as bit words for the backward), and with or without a key-padding
mask: `key_mask` (B, N), non-zero = the key takes part, one row per sample for all its heads
(padded caption batches of DistilBERT). It is packed on the device into B x ceil(N / 32) bit words
(triad_attn_keymask_pack; `pack_key_mask`, or pass the words), the softmax runs over the set keys
only, every position stays a query, cleared keys get dk = dv = +0, and a sample with no key set
gives out = 0. K / V rows of cleared keys must be finite.

Longer sequences, 321 .. 2048 tokens (configuration c5: 1374 visual tokens of DINOv2-L/14 at
518 px, 499 audio frames of HuBERT-large on 10 s), take the streaming kernels of
csrc/attention_long.hip: K / V (or Q / dO) pass through LDS in chunks of 64 rows and the forward
keeps an online softmax per query; same tensors, same dropout bits, words padded to whole chunks.
Both families have one C signature per step, so one _fwd / _bwd / _dropmask serves them: _is_long(N)
picks the entry points (_ENTRY) and the words per mask row. Which token counts are routed to the
streaming kernels is LONG_ROUTE. The streaming kernels take no mask: key_mask with N > 320 raises
TriadError, callers gate on it. Anything else -- per-query or additive masks (hf_attention_forward
falls back on ANY mask: the 4-D mask transformers builds cannot be shown to be a key mask without
reading it back), causal attention, head dim != 64, fp32, N > 2048 -- goes to
F.scaled_dot_product_attention.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from ._lib import TriadError, call, ptr, stream_ptr

HEAD_DIM = 64
MAX_TOKENS = 320
MAX_TOKENS_LONG = 2048
MAX_SEQUENCES = 65535   # B * H: one grid row per (sample, head)
# token counts the wrappers send to the streaming kernels (inclusive). The entry points accept all of
# 321 .. 2048; narrow this only where a measurement shows PyTorch's kernels ahead
LONG_ROUTE = (321, 2048)
# (dropmask, forward, backward) entry points by _is_long(N)
_ENTRY = {False: ("triad_attn_dropmask", "triad_attn_fwd_dropout", "triad_attn_bwd_dropout"),
          True: ("triad_attn_long_dropmask", "triad_attn_long_fwd", "triad_attn_long_bwd")}


def _gate(x, n, lo, hi, head_dim, scale, sequences):
    if scale is not None and not (math.isfinite(scale) and scale > 0.0):
        return False
    return (x.is_cuda and x.dtype == torch.bfloat16 and head_dim == HEAD_DIM and lo <= n <= hi
            and 0 < sequences <= MAX_SEQUENCES)


def supported(x: torch.Tensor, n: int, head_dim: int, scale=None, sequences: int = 1) -> bool:
    """What the entry points accept (they return TRIAD_EINVAL otherwise): bf16 on the device, head
    dim 64, 1 .. 320 tokens, at most 65535 (sample, head) sequences, a finite scale > 0 (None = the
    default 1 / sqrt(head dim)). The kernels take the row max of the unscaled scores."""
    return _gate(x, n, 1, MAX_TOKENS, head_dim, scale, sequences)


def supported_long(x: torch.Tensor, n: int, head_dim: int, scale=None, sequences: int = 1) -> bool:
    """What the wrappers send to the streaming kernels (triad_attn_long_*): as `supported`, with
    LONG_ROUTE[0] <= n <= LONG_ROUTE[1] tokens (inside the entry points' 321 .. 2048)."""
    return _gate(x, n, max(LONG_ROUTE[0], MAX_TOKENS + 1), min(LONG_ROUTE[1], MAX_TOKENS_LONG), head_dim, scale,
                 sequences)


def takes(x: torch.Tensor, B: int, H: int, n: int, head_dim: int, scale=None) -> bool:
    """Do the HIP kernels (either family) take B * H sequences of n tokens of x's kind?"""
    return supported(x, n, head_dim, scale, B * H) or supported_long(x, n, head_dim, scale, B * H)


def _rows(t):
    """(B, N, H, 64) view with the head dim contiguous and heads adjacent -> (sB, sN)."""
    return t.stride(0), t.stride(1)


def _as_bnhd(t):
    """t as the kernels read it: head dim contiguous, heads adjacent, and -- for their 16-byte
    accesses -- a 16-byte aligned base with sB and sN multiples of 8 elements. Anything else is
    copied."""
    if (t.stride(3) != 1 or t.stride(2) != HEAD_DIM or t.stride(0) % 8 or t.stride(1) % 8
            or t.data_ptr() % 16):
        t = t.clone(memory_format=torch.contiguous_format)   # (.contiguous() keeps an offset view as it is)
    return t


def _is_long(N):
    """Which family _Attention / _AttentionQKV run: the streaming kernels past MAX_TOKENS."""
    return N > MAX_TOKENS


def _words_per_row(N):
    """Keep words per mask row: ceil(N / 32), or 2 ceil(N / 64) for the streaming kernels (rows padded
    to whole 64-row chunks)."""
    return 2 * ((N + 63) // 64) if _is_long(N) else (N + 31) // 32


def _dropmask(B, H, N, p, device, seed=None):
    """Keep bits of the attention-probability dropout in both layouts (triad_attn[_long]_dropmask);
    seed None = one draw from _SEEDS."""
    wq = torch.empty(B * H * N * _words_per_row(N), dtype=torch.int32, device=device)
    wk = torch.empty_like(wq)
    call(_ENTRY[_is_long(N)][0], B, H, N, float(p), _SEEDS() if seed is None else seed, ptr(wq), ptr(wk),
         stream_ptr(device))
    return wq, wk


def pack_key_mask(key_mask):
    """(B, N) device mask (any dtype, non-zero = the key takes part) -> (B, ceil(N / 32)) int32 bit words
    (triad_attn_keymask_pack; bit j of word kt = key 32 kt + j, bits past N zero). No host sync."""
    if key_mask.dim() != 2 or not key_mask.is_cuda:
        raise TriadError(f"key_mask: expected a (B, N) device tensor, got {tuple(key_mask.shape)} on {key_mask.device}")
    B, N = key_mask.shape
    if not 1 <= N <= MAX_TOKENS:
        raise TriadError(f"key_mask over {N} tokens: the masked kernels take 1 .. {MAX_TOKENS}")
    m = key_mask if key_mask.dtype in (torch.bool, torch.uint8) else key_mask.ne(0)
    m = m.contiguous()
    words = torch.empty(B, (N + 31) // 32, dtype=torch.int32, device=m.device)
    call("triad_attn_keymask_pack", ptr(m), B, N, ptr(words), stream_ptr(m.device))
    return words


def _key_words(key_mask, B, N):
    """key_mask of attention_bnhd / attention_qkv -> packed words (B, ceil(N / 32)) int32, or None. Words are
    recognised by dtype int32 and shape (B, ceil(N / 32)); anything else is a (B, N) mask to pack."""
    if key_mask is None:
        return None
    if N > MAX_TOKENS:
        raise TriadError(f"key_mask with {N} tokens: the streaming kernels (N > {MAX_TOKENS}) take no mask")
    if key_mask.dtype == torch.int32 and tuple(key_mask.shape) == (B, (N + 31) // 32) and (N + 31) // 32 != N:
        return key_mask.contiguous()
    if tuple(key_mask.shape) != (B, N):
        raise TriadError(f"key_mask {tuple(key_mask.shape)}: expected ({B}, {N}) or packed ({B}, {(N + 31) // 32}) int32")
    return pack_key_mask(key_mask)


def _fwd(q, k, v, scale, drop=None, km=None):
    B, N, H, D = q.shape
    out = torch.empty(B, N, H, D, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(B * H, N, dtype=torch.float32, device=q.device)
    wq, p = (drop[0], drop[2]) if drop is not None else (None, 0.0)
    if km is not None:   # whole-sequence kernels only (_key_words refuses N > MAX_TOKENS)
        call("triad_attn_fwd_keymask", ptr(q), *_rows(q), ptr(k), *_rows(k), ptr(v), *_rows(v), B, H, N, D,
             float(scale), ptr(wq), float(p), ptr(km), ptr(out), *_rows(out), ptr(lse), stream_ptr(q.device))
        return out, lse
    call(_ENTRY[_is_long(N)][1], ptr(q), *_rows(q), ptr(k), *_rows(k), ptr(v), *_rows(v), B, H, N, D, float(scale),
         ptr(wq), float(p), ptr(out), *_rows(out), ptr(lse), stream_ptr(q.device))
    return out, lse


def _bwd(q, k, v, out, lse, dout, scale, drop=None, km=None):
    """-> (B, N, 3, H, 64) buffer holding dq, dk, dv (a fused qkv projection's gradient layout)."""
    B, N, H, D = q.shape
    do = _as_bnhd(dout.to(torch.bfloat16))
    g = torch.empty(B, N, 3, H, D, dtype=torch.bfloat16, device=q.device)
    dq, dk, dv = g[:, :, 0], g[:, :, 1], g[:, :, 2]
    delta = torch.empty(B * H, N, dtype=torch.float32, device=q.device)
    wq, wk, p = drop if drop is not None else (None, None, 0.0)
    if km is not None:
        call("triad_attn_bwd_keymask", ptr(q), *_rows(q), ptr(k), *_rows(k), ptr(v), *_rows(v), ptr(out), *_rows(out),
             ptr(do), *_rows(do), ptr(lse), B, H, N, D, float(scale), ptr(wq), ptr(wk), float(p), ptr(km), ptr(dq),
             *_rows(dq), ptr(dk), *_rows(dk), ptr(dv), *_rows(dv), ptr(delta), stream_ptr(q.device))
        return g
    call(_ENTRY[_is_long(N)][2], ptr(q), *_rows(q), ptr(k), *_rows(k), ptr(v), *_rows(v), ptr(out), *_rows(out),
         ptr(do), *_rows(do), ptr(lse), B, H, N, D, float(scale), ptr(wq), ptr(wk), float(p), ptr(dq), *_rows(dq),
         ptr(dk), *_rows(dk), ptr(dv), *_rows(dv), ptr(delta), stream_ptr(q.device))
    return g


def _SEEDS():
    """Per-call 32-bit dropout seed drawn from torch's default CPU generator (no device sync):
    torch.manual_seed reproduces the masks, as it does for torch's own dropout kernels."""
    return int(torch.randint(0, 2 ** 32 - 1, (1,)))


class _Attention(torch.autograd.Function):
    """q, k, v: (B, N, H, 64) bf16 views (head dim contiguous, heads adjacent) -> O (B, N, H, 64);
    N <= 320 on the whole-sequence kernels, longer on the streaming ones; dropout p > 0 drops
    attention probabilities (keep bits drawn per call, kept for the backward); km: packed key-mask
    words (B, ceil(N / 32)) int32 or None (N <= 320 only), kept for the backward."""

    @staticmethod
    def forward(ctx, q, k, v, scale, p=0.0, km=None):
        q, k, v = _as_bnhd(q), _as_bnhd(k), _as_bnhd(v)
        drop = None
        if p > 0.0:
            B, N, H, _ = q.shape
            drop = (*_dropmask(B, H, N, p, q.device), float(p))
        out, lse = _fwd(q, k, v, scale, drop) if km is None else _fwd(q, k, v, scale, drop, km)
        ctx.save_for_backward(q, k, v, out, lse, *(drop[:2] if drop else ()), *(() if km is None else (km,)))
        ctx.scale = float(scale)
        ctx.p = float(p)
        ctx.masked = km is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        saved = ctx.saved_tensors
        q, k, v, out, lse = saved[:5]
        drop = (saved[5], saved[6], ctx.p) if ctx.p > 0.0 else None
        g = _bwd(q, k, v, out, lse, dout, ctx.scale, drop, saved[-1] if ctx.masked else None)
        return g[:, :, 0], g[:, :, 1], g[:, :, 2], None, None, None


class _AttentionQKV(torch.autograd.Function):
    """qkv: (B, N, 3*H*64) bf16 output of a fused projection (q | k | v, heads inside each) ->
    O (B, N, H*64); dropout p > 0 on the probabilities as in _Attention; the backward returns
    d qkv as one tensor (the fused projection's gradient, no per-view scatter)."""

    @staticmethod
    def forward(ctx, qkv, heads, scale, p=0.0, km=None):
        B, N, C3 = qkv.shape
        x = qkv.contiguous()
        if x.data_ptr() % 16:   # a contiguous view at an odd storage offset: the kernels need 16 bytes
            x = x.clone()
        x = x.view(B, N, 3, heads, HEAD_DIM)
        q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
        drop = (*_dropmask(B, heads, N, p, qkv.device), float(p)) if p > 0.0 else None
        out, lse = _fwd(q, k, v, scale, drop) if km is None else _fwd(q, k, v, scale, drop, km)
        ctx.save_for_backward(x, out, lse, *(drop[:2] if drop else ()), *(() if km is None else (km,)))
        ctx.scale = float(scale)
        ctx.p = float(p)
        ctx.masked = km is not None
        return out.view(B, N, heads * HEAD_DIM)

    @staticmethod
    def backward(ctx, dout):
        saved = ctx.saved_tensors
        x, out, lse = saved[:3]
        drop = (saved[3], saved[4], ctx.p) if ctx.p > 0.0 else None
        B, N = x.shape[0], x.shape[1]
        g = _bwd(x[:, :, 0], x[:, :, 1], x[:, :, 2], out, lse, dout.view(out.shape), ctx.scale, drop,
                 saved[-1] if ctx.masked else None)
        return g.view(B, N, -1), None, None, None, None


def attention_qkv(qkv, heads, scale=None, dropout=0.0, key_mask=None):
    """Fused-projection attention: qkv (B, N, 3*heads*64) bf16 -> (B, N, heads*64). key_mask: (B, N)
    device mask (non-zero = the key takes part) or its packed words (pack_key_mask); N <= 320, else
    TriadError."""
    if scale is None:
        scale = 1.0 / math.sqrt(HEAD_DIM)
    return _AttentionQKV.apply(qkv, heads, scale, float(dropout), _key_words(key_mask, qkv.shape[0], qkv.shape[1]))


def attention_bnhd(q, k, v, scale=None, dropout=0.0, key_mask=None):
    """dropout(softmax(q k^T * scale)) v over (B, N, H, 64) bf16 views -> (B, N, H, 64); key_mask as in
    attention_qkv."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    return _Attention.apply(q, k, v, scale, float(dropout), _key_words(key_mask, q.shape[0], q.shape[1]))


def dropout_keep_dense(B, H, N, p, seed, device):
    """(B, H, N, N) keep mask (bool) of the attention dropout for a given seed, unpacked from both
    stored layouts (tests: the two must agree)."""
    wq, wk = _dropmask(B, H, N, p, device, seed)
    bits = torch.arange(32, device=device, dtype=torch.int32)

    def unpack(w):
        m = ((w.view(B, H, N, -1, 1) >> bits) & 1).bool().view(B, H, N, -1)
        return m[..., :N]
    return unpack(wq), unpack(wk).transpose(-1, -2)


def sdpa(q, k, v, scale=None):
    """F.scaled_dot_product_attention(q, k, v) (no mask / dropout) for (B, H, N, d) inputs: the
    HIP kernels when supported (<= 320 tokens, or LONG_ROUTE on the streaming kernels), else PyTorch."""
    B, H, N, d = q.shape
    if not takes(q, B, H, N, d, scale) or k.shape != q.shape or v.shape != q.shape:
        return F.scaled_dot_product_attention(q, k, v, scale=scale)
    o = attention_bnhd(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), scale)
    return o.transpose(1, 2)


def hf_attention_forward(module, query, key, value, attention_mask, dropout=0.0, scaling=None, is_causal=None,
                         **kwargs):
    """transformers attention-interface function ("triad"): the HIP kernels for unmasked attention
    over <= 320 tokens, or LONG_ROUTE tokens on the streaming kernels (attention dropout included),
    else the stock sdpa implementation.
    Returns (B, N, H, d) as the interface requires."""
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    B, H, N, d = query.shape
    p = float(dropout) if module.training else 0.0
    if (attention_mask is not None or kwargs.get("output_attentions") or not 0.0 <= p < 1.0
            or key.shape != query.shape or value.shape != query.shape
            or not takes(query, B, H, N, d, scaling) or getattr(module, "is_causal", False)):
        return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling,
                                      is_causal=is_causal, **kwargs)
    o = attention_bnhd(query.transpose(1, 2), key.transpose(1, 2), value.transpose(1, 2), scaling, dropout=p)
    return o, None
