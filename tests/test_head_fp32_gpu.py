"""GPU parity of the fp32-accurate contrastive head (`precision="fp32"`, csrc/pairsim_split.hip)
against the fp64 CPU oracle on fp32 features that are NOT bf16-representable.

Bars: losses, statistics and clip at test_head_gpu's forward bars (1e-4 relative), d/dtemp 1e-3
relative, feature gradients relative L2 < 1e-3 (the project's fp32 bar) and
elementwise within 3e-3 * max|g| (test_head_gpu._check_grad's 3:1 ratio at that bar). Rows whose
top-two gap in the oracle is <= 2^-12 of |max| (about ten times the worst gap error of the
three-term product) may be skipped; at most 2 % of the query rows and of the key rows.

Every test prints its figures before it asserts; the measured values are in DESIGN.md §2.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import ref_cpu

pytestmark = pytest.mark.gpu

dev = "cuda"
TEMP, THR, W = 1.5, 0.02, 0.01
TIE_REL = 2.0 ** -12

# name: (kind, B, Nq, Nk, padded keys)
CASES = {
    "av_6_40_70": ("av", 6, 40, 70, True),     # 240 rows < one 256-row workgroup; Nk % 32 != 0; zero keys
    "av_2_33_32": ("av", 2, 33, 32, False),    # smallest batch; Nk exactly one tile
    "tv_5_12_70": ("tv", 5, 12, 70, True),     # masked mean; sparsity active
    "av_8_20_40": ("av", 8, 20, 40, True),     # run in >= 2 key-sample chunks
}


def _ops():
    from triad_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _inputs(name):
    kind, B, Nq, Nk, pad = CASES[name]
    g = torch.Generator().manual_seed(700 + B)
    q = torch.randn(B, Nq, 512, generator=g) * 0.58
    k = torch.randn(B, Nk, 512, generator=g) * 0.58
    if pad:
        lens = torch.randint(Nk // 2, Nk + 1, (B,), generator=g)
        lens[0] = Nk
        for j in range(B):
            k[j, lens[j]:] = 0
    mask = None
    if kind == "tv":
        ml = torch.randint(1, Nq + 1, (B,), generator=g)
        ml[0] = Nq
        mask = torch.zeros(B, Nq, dtype=torch.long)
        for i in range(B):
            mask[i, :ml[i]] = 1
    return kind, q, k, mask


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """fp64 oracle of a case, computed once and shared (never modified): head_loss_chunked's dict
    plus the near-tie row masks at 2^-12."""
    kind, q, k, mask = _inputs(name)
    ref = ref_cpu.head_loss_chunked(kind, q.double(), k.double(), TEMP, q_mask=mask, threshold=THR, weight=W)
    tq, tk, _ = ref_cpu.near_ties(q.double(), k.double(), TEMP, rel=TIE_REL)
    ref["tie_q"], ref["tie_k"] = tq, tk
    return ref


def _scalar_close(a, b, rtol=1e-4, atol=1e-5):   # test_head_gpu._scalar_close
    if math.isnan(b):
        return math.isnan(a)
    return abs(a - b) <= atol + rtol * abs(b)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _check_grad32(got, ref, skip, what):
    """The fp32 bar on a (B, N, 512) feature gradient, compared in fp32 as it came back."""
    assert got.dtype == torch.float32, (what, got.dtype)
    got = got.detach().cpu().numpy()
    ref = np.asarray(ref)
    sk = skip.cpu().numpy().reshape(-1)
    assert sk.mean() <= 0.02, f"{what}: {sk.sum()} of {sk.size} rows near-tied"
    got = got.reshape(-1, got.shape[-1])[~sk]
    ref = ref.reshape(-1, ref.shape[-1])[~sk]
    rel, worst = _rel(got, ref), float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"{what}: skipped {sk.sum()} of {sk.size} rows, relative L2 {rel:.3e}, worst element / max|g| {worst:.3e}")
    assert rel < 1e-3, (what, rel)
    assert worst <= 3e-3, (what, worst)


def _check_forward(losses, stats, clip, ref):
    lv = [float(x.detach()) for x in losses]
    for got, key in zip(lv, ("total", "ce", "reg", "aux")):
        print(f"{key}: {got!r} oracle {ref[key]!r}")
        assert _scalar_close(got, ref[key]), (key, got, ref[key])
    sv = stats.cpu().double().numpy()
    want = list(ref["stats"].values()) + [ref["l_nonneg"], ref["l_cal"], ref["diag"]]
    assert len(sv) == len(want) == 9
    for got, w in zip(sv, want):
        assert _scalar_close(float(got), float(w), 1e-4, 1e-4), (float(got), float(w))
    np.testing.assert_allclose(clip.cpu().numpy(), ref["clip"].numpy(), rtol=1e-4, atol=1e-4)


def _run(name, objective=None, **kw):
    """Forward + backward of one case on the device; returns (q, k, t leaves, losses, stats, clip)."""
    ops = _ops()
    kind, q, k, mask = _inputs(name)
    qg = q.to(dev).requires_grad_(True)
    kg = k.to(dev).requires_grad_(True)
    tg = torch.tensor(TEMP, device=dev, requires_grad=True)
    if kind == "tv":
        kw = dict(q_mask=mask.to(dev), threshold=THR, sparsity_weight=W, **kw)
    losses, stats, clip = ops.contrastive_head(ops.AV if kind == "av" else ops.TV, qg, kg, tg, precision="fp32",
                                               **kw)
    (losses[0] if objective is None else objective(losses)).backward()
    return qg, kg, tg, losses, stats, clip


@pytest.mark.parametrize("name", ["av_6_40_70", "av_2_33_32", "tv_5_12_70"])
def test_fp32_head_vs_oracle(name):
    ref = _oracle(name)
    qg, kg, tg, losses, stats, clip = _run(name)
    _check_forward(losses, stats, clip, ref)
    _check_grad32(qg.grad, ref["dq"].numpy(), ref["tie_q"], name + " dq")
    _check_grad32(kg.grad, ref["dk"].numpy(), ref["tie_k"], name + " dk")
    print(f"dtemp: {float(tg.grad)!r} oracle {ref['dtemp']!r}")
    assert tg.grad.dtype == torch.float32
    assert _scalar_close(float(tg.grad), ref["dtemp"], 1e-3, 1e-5), (float(tg.grad), ref["dtemp"])


def test_fp32_head_in_chunks_vs_oracle():
    """ds_budget one byte under the whole-batch working set: the chunk helper reports >= 2 chunks,
    stays inside the budget in its own accounting, and the chunked backward meets the same bars."""
    ops = _ops()
    name = "av_8_20_40"
    _, B, Nq, Nk, _ = CASES[name]
    geo = ops.Geometry(B, Nq, B, Nk)
    budget = ops.split_working_bytes(geo, B) - 1
    assert ops.split_num_chunks(geo, budget) >= 2
    assert ops.split_working_bytes(geo, ops.split_chunk_samples(geo, budget)) <= budget
    ref = _oracle(name)
    qg, kg, tg, losses, stats, clip = _run(name, ds_budget=budget)
    _check_forward(losses, stats, clip, ref)
    _check_grad32(qg.grad, ref["dq"].numpy(), ref["tie_q"], name + " dq")
    _check_grad32(kg.grad, ref["dk"].numpy(), ref["tie_k"], name + " dk")
    assert _scalar_close(float(tg.grad), ref["dtemp"], 1e-3, 1e-5), (float(tg.grad), ref["dtemp"])
    # the same call in one chunk: the chunking only changes the summation order of dq
    q1, k1, t1, *_ = _run(name)
    assert _rel(qg.grad.cpu(), q1.grad.cpu()) < 1e-5 and _rel(kg.grad.cpu(), k1.grad.cpu()) < 1e-5


def test_fp32_head_mixed_objective_vs_oracle():
    """0.5 total + 1.5 ce - 0.7 reg + 3 aux, as test_av_head_vs_oracle_random's mix."""
    name = "av_6_40_70"
    _, q, k, _ = _inputs(name)
    qr, kr = q.double().requires_grad_(True), k.double().requires_grad_(True)
    tr = torch.tensor(TEMP, dtype=torch.float64, requires_grad=True)
    total, ce, reg, sm, _ = ref_cpu.av_loss(qr, kr, tr)

    def mix(l):
        return 0.5 * l[0] + 1.5 * l[1] - 0.7 * l[2] + 3.0 * l[3]

    mix((total, ce, reg, sm)).backward()
    ref = _oracle(name)
    qg, kg, tg, losses, stats, clip = _run(name, objective=mix)
    for got, want in zip(losses, (total, ce, reg, sm)):
        assert _scalar_close(float(got), float(want)), (float(got), float(want))
    _check_grad32(qg.grad, qr.grad.numpy(), ref["tie_q"], "mix dq")
    _check_grad32(kg.grad, kr.grad.numpy(), ref["tie_k"], "mix dk")
    assert _scalar_close(float(tg.grad), float(tr.grad), 1e-3, 1e-5), (float(tg.grad), float(tr.grad))


def test_fp32_head_is_bit_reproducible():
    a = _run("av_6_40_70")
    b = _run("av_6_40_70")
    for x, y in zip(a[3], b[3]):
        assert torch.equal(x, y)
    assert torch.equal(a[4], b[4]) and torch.equal(a[5], b[5])
    for x, y in zip(a[:3], b[:3]):
        assert x.grad.dtype == torch.float32 and torch.equal(x.grad, y.grad)


def test_fp32_head_returns_the_inputs_dtypes():
    """fp32 in -> fp32 gradients; any float dtype is accepted and read as fp32 (bf16 in -> the
    fp32 result of those values, returned as bf16)."""
    ops = _ops()
    _, q, k, _ = _inputs("av_2_33_32")
    qb = q.to(dev, torch.bfloat16).requires_grad_(True)
    kf = k.to(dev).requires_grad_(True)
    t = torch.tensor(TEMP, device=dev, requires_grad=True)
    losses, _, _ = ops.contrastive_head(ops.AV, qb, kf, t, precision="fp32")
    losses[0].backward()
    assert qb.grad.dtype == torch.bfloat16 and kf.grad.dtype == torch.float32 and t.grad.dtype == torch.float32


def test_default_precision_is_the_bf16_path_unchanged():
    ops = _ops()
    _, q, k, _ = _inputs("av_6_40_70")
    res = []
    for kw in ({}, dict(precision="bf16")):
        qg = q.to(dev, torch.bfloat16).requires_grad_(True)
        kg = k.to(dev, torch.bfloat16).requires_grad_(True)
        tg = torch.tensor(TEMP, device=dev, requires_grad=True)
        losses, stats, clip = ops.contrastive_head(ops.AV, qg, kg, tg, **kw)
        losses[0].backward()
        res.append((*losses, stats, clip, qg.grad, kg.grad, tg.grad))
    for x, y in zip(*res):
        assert x.dtype == y.dtype and torch.equal(x, y)
    assert res[0][6].dtype == torch.bfloat16


def test_fp32_pair_equals_the_two_single_heads():
    ops = _ops()
    _, qa, ka, _ = _inputs("av_6_40_70")
    _, qt, kt, mask = _inputs("tv_5_12_70")
    a = _run("av_6_40_70")
    b = _run("tv_5_12_70")
    leaves = [x.to(dev).requires_grad_(True) for x in (qa, ka, qt, kt)]
    t = torch.tensor(TEMP, device=dev, requires_grad=True)
    (la, sa, ca), (lt, st, ct) = ops.contrastive_heads_av_tv(*leaves, t, mask.to(dev), threshold=THR,
                                                             sparsity_weight=W, precision="fp32")
    (la[0] + lt[0]).backward()
    for x, y in zip((*la, sa, ca, *lt, st, ct), (*a[3], a[4], a[5], *b[3], b[4], b[5])):
        assert torch.equal(x, y)
    for x, y in zip(leaves, (a[0], a[1], b[0], b[1])):
        assert torch.equal(x.grad, y.grad)
    assert torch.equal(t.grad, a[2].grad + b[2].grad)


def test_precision_refusals():
    ops = _ops()
    from triad_amd._lib import TriadError
    _, q, k, _ = _inputs("av_2_33_32")
    qg, kg = q.to(dev), k.to(dev)
    t = torch.tensor(TEMP, device=dev)
    with pytest.raises(ValueError):
        ops.contrastive_head(ops.AV, qg, kg, t, precision="fp64")
    with pytest.raises(ValueError):
        ops.contrastive_heads_av_tv(qg, kg, qg, kg, t, None, precision="fp64")
    with pytest.raises(TriadError, match="global negatives"):
        ops.contrastive_head(ops.AV, qg, kg, t, group=object(), precision="fp32")
    with pytest.raises(TriadError, match="global negatives"):
        ops.contrastive_heads_av_tv(qg, kg, qg, kg, t, torch.ones(q.shape[:2], device=dev), group=object(),
                                    precision="fp32")


# ---- model level: use_amp=False routes the loss heads to precision="fp32" -------------------
def _light_model(temp, thr=THR, w=W):
    """test_dropin_gpu.light_model with use_amp = False."""
    from triad_amd.model import MultiModalModel
    m = MultiModalModel.__new__(MultiModalModel)
    nn.Module.__init__(m)
    m.temperature = nn.Parameter(torch.tensor(float(temp), device=dev))
    m.patch_sparsity_threshold = thr
    m.patch_sparsity_weight = w
    m.use_amp = False
    m.amp_dtype = torch.bfloat16
    m.negatives_group = None
    return m


class _Stub(nn.Module):
    """Embedder stand-in: returns its fp32 features as they are (and a mask for text)."""

    def __init__(self, feats, mask=None):
        super().__init__()
        self.feats = feats
        self.mask = mask

    def forward(self, _x):
        return self.feats if self.mask is None else (self.feats, self.mask)


def _leaf(x):
    return x.to(dev).requires_grad_(True)


def test_model_forward_audio_visual_fp32():
    name = "av_6_40_70"
    ref = _oracle(name)
    _, q, k, _ = _inputs(name)
    m = _light_model(TEMP)
    A, V = _leaf(q), _leaf(k)
    m.audio_embedder, m.visual_embedder = _Stub(A), _Stub(V)
    total, ce, reg, sm, stats = m.forward_audio_visual(None, None)
    total.backward()
    for got, key in ((total, "total"), (ce, "ce"), (reg, "reg"), (sm, "aux")):
        assert _scalar_close(float(got), ref[key]), (key, float(got), ref[key])
    for got, want in zip(stats.values(), ref["stats"].values()):
        assert _scalar_close(float(got), float(want), 1e-4, 1e-4)
    _check_grad32(A.grad, ref["dq"].numpy(), ref["tie_q"], "model AV dA")
    _check_grad32(V.grad, ref["dk"].numpy(), ref["tie_k"], "model AV dV")
    assert _scalar_close(float(m.temperature.grad), ref["dtemp"], 1e-3, 1e-5)


def test_model_forward_text_visual_fp32():
    name = "tv_5_12_70"
    ref = _oracle(name)
    _, q, k, mask = _inputs(name)
    m = _light_model(TEMP)
    T, V = _leaf(q), _leaf(k)
    m.text_embedder, m.visual_embedder = _Stub(T, mask.to(dev)), _Stub(V)
    total, stats = m.forward_text_visual(None, None)
    total.backward()
    assert _scalar_close(float(total), ref["total"]), (float(total), ref["total"])
    for got, want in zip(stats.values(), ref["stats"].values()):
        assert _scalar_close(float(got), float(want), 1e-4, 1e-4)
    _check_grad32(T.grad, ref["dq"].numpy(), ref["tie_q"], "model TV dT")
    _check_grad32(V.grad, ref["dk"].numpy(), ref["tie_k"], "model TV dV")
    assert _scalar_close(float(m.temperature.grad), ref["dtemp"], 1e-3, 1e-5)


def test_model_triad_heads_fp32():
    ra, rt = _oracle("av_6_40_70"), _oracle("tv_5_12_70")
    _, qa, ka, _ = _inputs("av_6_40_70")
    _, qt, kt, mask = _inputs("tv_5_12_70")
    m = _light_model(TEMP)
    A, Va, T, Vt = _leaf(qa), _leaf(ka), _leaf(qt), _leaf(kt)
    av, tv = m._triad_heads(A, Va, T, Vt, mask.to(dev))
    (av[0] + tv[0]).backward()
    for got, key in zip(av[:4], ("total", "ce", "reg", "aux")):
        assert _scalar_close(float(got), ra[key]), (key, float(got), ra[key])
    assert _scalar_close(float(tv[0]), rt["total"]), (float(tv[0]), rt["total"])
    _check_grad32(A.grad, ra["dq"].numpy(), ra["tie_q"], "triad dA")
    _check_grad32(Va.grad, ra["dk"].numpy(), ra["tie_k"], "triad dV(av)")
    _check_grad32(T.grad, rt["dq"].numpy(), rt["tie_q"], "triad dT")
    _check_grad32(Vt.grad, rt["dk"].numpy(), rt["tie_k"], "triad dV(tv)")
    want = ra["dtemp"] + rt["dtemp"]
    assert _scalar_close(float(m.temperature.grad), want, 1e-3, 1e-5), (float(m.temperature.grad), want)
