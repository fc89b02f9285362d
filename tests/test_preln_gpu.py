"""The pre-LN (stable layer norm, HuBERT-large) path on the device: triad_preln_fwd / _bwd through the C
ABI against the fp64 references and derived bounds of tests/preln_ref.py (tests/test_preln_checks_cpu.py
shows that each bound passes an emulation of its kernel and that each planted error fails one), one fused
stable-LN layer against a plain-torch restatement on the recorded dropout masks, and the fused
HubertEncoderStableLayerNorm against the stock transformers loop, with and without LayerDrop, plus the
entry points a 10 s clip takes.

Operands come from a seeded CPU generator. Every output buffer is filled with NaN before the call and
carries NaN rows past row M - 1 that must be unchanged afterwards; outputs the call does not use (res_out
without y, dy without y) must stay NaN. Bounds (u = 2^-24, h = D / 64 + 5; derivations in preln_ref):
    res_out  bit-equal to torch's bf16 add on the numpy mask
    mean     (h + 1) u mean|z|          rstd  rstd (0.5 (dm rstd)^2 + (0.5 (h + 6) + 4) u)
    n        |w| rstd dm + |xhat w| (rel_rstd + 4 u) + u |ref|      [bf16: + 2^-8 |ref|]
    dres     postln_ref's LN' bound + u |g| (both gradients given) + 2^-8 |g|
    part     postln_ref's per-block bound; total: summed
Identities: bf16(n_f32) == n_bf16 across two calls; dy == keep ? bf16(float(dres) scale) : 0 of the
kernel's own dres; repeats are bit-identical.

Largest err / bound per group on MI355X: fwd mean 0.033, rstd 0.149, n_f32 0.551, n_bf16 0.996 (the one
bf16 rounding fills its 2^-8 term); bwd dres 0.996 (likewise), part dgamma 0.586, part dbeta 0.593, total
0.457. The fused layer against the fp32 restatement: output 2.3e-3, parameter gradients 1e-7 .. 6.4e-3
relative L2; the 2- and 6-layer encoders against the stock loop: every gradient below 8.1e-3, the largest
on the first conv layer's weight (bars 1e-2 / 3e-2).
"""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import postln_ref as R
from tests import preln_ref as P

pytestmark = pytest.mark.gpu

dev = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
EPS = P.EPS
GROWS = 4      # NaN rows past row M - 1 of a row-kernel output
GUARD = 64
WORST = {}


def _lib():
    from triad_amd import _lib
    return _lib


def _at(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _rows(M, D, dt):
    return torch.full((M + GROWS, D), NAN, dtype=dt, device=dev)


def _nan(n, dt):
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
    print("\npre-LN kernels, largest err/bound per group:", ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))


@pytest.fixture(autouse=True)
def _route_on(monkeypatch):
    """The encoder tests exercise the fused path whatever postln.STABLE_ROUTE's default is."""
    from triad_amd import postln
    monkeypatch.setattr(postln, "STABLE_ROUTE", True)


@functools.lru_cache(maxsize=4)
def _case(M, D):
    c = P.preln_case(M, D)
    return c, {k: v.to(dev) for k, v in c.items()}


# ---- triad_preln_fwd ----------------------------------------------------------------------------------------

def _fwd(d, M, D, p, seed, with_y=True, out_f32=False):
    L = _lib()
    res_out = _rows(M, D, BF)
    n = _rows(M, D, F32 if out_f32 else BF)
    mean, rstd = _nan(M + GROWS, F32), _nan(M + GROWS, F32)
    L.call("triad_preln_fwd", _at(d["res"]), _at(d["y"]) if with_y else None, _at(d["w"]), _at(d["b"]), EPS, M, D, p,
           seed, _at(res_out), _at(n), int(out_f32), _at(mean), _at(rstd), L.stream_ptr())
    for t in (res_out, n, mean, rstd):
        assert _all_nan(t[M:]), f"preln_fwd M {M} D {D}: wrote past row M - 1"
    return res_out[:M], n[:M], mean[:M], rstd[:M]


@pytest.mark.parametrize("D", P.FWD_DS)
def test_preln_forward(D):
    """Every D instance x M = 1, 3, 4, 5, 130 x p = 0, 0.1, 0.5 with a seed >= 2^31, and the y = NULL
    form: res_out bit-equal to torch's bf16 add on the numpy mask (NaN-filled and untouched without y),
    mean, rstd and both forms of n against fp64, bf16(n_f32) == n_bf16 from two calls."""
    eps = R.f32(EPS)
    for M in P.FWD_MS:
        c, d = _case(M, D)
        for p, with_y in [(p, True) for p in P.FWD_PS] + [(0.0, False)]:
            what = f"M {M} D {D} p {p} y {with_y}"
            seed = P.SEED_HI if with_y else 0
            y = c["y"] if with_y else None
            want = P.preln_fwd_ref(c["res"], y, c["w"], c["b"], eps, p, seed)
            res_out, nb, mean, rstd = _fwd(d, M, D, p, seed, with_y)
            res_out32, n32, mean32, rstd32 = _fwd(d, M, D, p, seed, with_y, out_f32=True)
            if with_y:
                keep = R.keep_mask(c["res"].shape, p, seed).to(dev)
                yd = (d["y"].float() * torch.tensor(R.drop_scale(p), dtype=F32, device=dev)).to(BF)
                torch_z = d["res"] + torch.where(keep, yd, torch.zeros_like(yd))
                assert torch.equal(res_out, torch_z), what + ": res_out != torch's bf16 add on the mask"
                assert torch.equal(res_out32, torch_z), what
                assert torch.equal(res_out.cpu(), want["z"]), what
            else:
                assert _all_nan(res_out) and _all_nan(res_out32), what + ": res_out written without y"
            _check(mean, *want["mean"], "fwd.mean", what)
            _check(rstd, *want["rstd"], "fwd.rstd", what)
            _check(nb, *want["nb"], "fwd.n_bf16", what)
            _check(n32, *want["n32"], "fwd.n_f32", what)
            assert torch.equal(n32.to(BF), nb), what + ": bf16(n_f32) != n_bf16"
            assert torch.equal(mean, mean32) and torch.equal(rstd, rstd32), what


# ---- triad_preln_bwd ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def _operands(M, D, p, seed):
    """(z, keep, scale, mean, rstd) on the CPU and (z, mean, rstd) on the device: z exact, the
    statistics the fp64 ones rounded to fp32, independent of the forward kernel."""
    c, _ = _case(M, D)
    z, keep, scale = P.stream(c["res"], c["y"], p, seed)
    mean, rstd = P.ref_stats(z, c["w"], c["b"], R.f32(EPS))
    return (z, keep, scale, mean, rstd), (z.to(dev), mean.to(dev), rstd.to(dev))


def _bwd(d, zd, md, rd, M, D, p, seed, mode, has_y=True):
    L = _lib()
    G = L.call("triad_preln_bwd_blocks", M)
    assert G == R.bwd_blocks(M)
    dres, dy = _rows(M, D, BF), _rows(M, D, BF)
    part = _nan(G * 2 * D + GUARD, F32)
    dz = d["dz"] if "dz" in mode else None
    dn = d["dn32"] if "dn32" in mode else d["dn"] if "dn" in mode else None
    L.call("triad_preln_bwd", _at(dz), _at(dn), int("dn32" in mode), _at(zd), _at(md), _at(rd), _at(d["w"]), M, D, p,
           seed, _at(dres), _at(dy) if has_y else None, _at(part), L.stream_ptr())
    what = f"preln_bwd M {M} D {D} {mode}"
    assert _all_nan(dres[M:]) and _all_nan(dy[M:]), what + ": wrote past row M - 1"
    assert _all_nan(part[G * 2 * D:]), what + ": wrote past part[blocks][2][D]"
    if not has_y:
        assert _all_nan(dy), what + ": dy written though not given"
    return dres[:M], (dy[:M] if has_y else None), part[:G * 2 * D].view(G, 2, D)


def _bwd_case(M, D, mode, p=0.1):
    c, d = _case(M, D)
    (z, keep, scale, mean, rstd), (zd, md, rd) = _operands(M, D, p, P.SEED_HI)
    dres, dy, part = _bwd(d, zd, md, rd, M, D, p, P.SEED_HI, mode)
    dz, dn = P.pick(c, mode)
    want = P.preln_bwd_ref(dz, dn, z, mean, rstd, c["w"])
    what = f"M {M} D {D} p {p} {'+'.join(mode)}"
    _check(dres, *want["dres"], "bwd.dres", what)
    ref, bound = want["part"]
    _check(part[:, 0], ref[:, 0], bound[:, 0], "bwd.part.dgamma", what)
    _check(part[:, 1], ref[:, 1], bound[:, 1], "bwd.part.dbeta", what)
    _check(part.double().sum(0), *want["total"], "bwd.total", what)
    assert bool(torch.isfinite(dy.float()).all()), what + ": dy not finite"
    assert torch.equal(dy.cpu(), R.dy_of(dres.cpu(), keep, scale)), what + ": dy != bf16(dres keep scale)"
    return dres, dy, part


@pytest.mark.parametrize("D", P.FWD_DS)
def test_preln_backward(D):
    """The forward's D x M grid at p = 0.1 with dz only, dn only and both (and the fp32 dn at M = 130):
    dres, every block's dgamma / dbeta partials, their totals, the dy identity; without dn the partials
    are exact zeros; the form without dy leaves a NaN-filled dy untouched and gives the same dres."""
    for M in P.FWD_MS:
        for mode in P.BWD_MODES:
            got = _bwd_case(M, D, mode)
            if mode == ("dz",):
                assert not bool(got[2].any()), "partials without dn must be zero"
        if M == 130:
            _bwd_case(M, D, ("dz", "dn32"))
            c, d = _case(M, D)
            _, (zd, md, rd) = _operands(M, D, 0.1, P.SEED_HI)
            with_dy = _bwd(d, zd, md, rd, M, D, 0.1, P.SEED_HI, ("dz", "dn"))
            no_dy = _bwd(d, zd, md, rd, M, D, 0.1, P.SEED_HI, ("dz", "dn"), has_y=False)
            assert torch.equal(with_dy[0], no_dy[0]) and torch.equal(with_dy[2], no_dy[2])


@pytest.mark.parametrize("M,D", P.BWD_BIG)
def test_preln_backward_past_one_trip(M, D):
    """Rows from 4096 on are a block's second (and third) trip of the grid-stride loop, the last trip
    partial; D = 1024 is the NB = 4 instance."""
    assert R.bwd_trips(M) == (3 if M == 8197 else 2)
    for mode in P.BWD_MODES:
        _bwd_case(M, D, mode)


def test_preln_repeats_are_bit_identical():
    M, D, p = 4101, 256, 0.1
    _, d = _case(M, D)
    _, (zd, md, rd) = _operands(M, D, p, P.SEED_HI)
    f = [_fwd(d, M, D, p, P.SEED_HI) for _ in range(3)]
    b = [_bwd(d, zd, md, rd, M, D, p, P.SEED_HI, ("dz", "dn")) for _ in range(3)]
    for runs in (f, b):
        for r in runs[1:]:
            assert all(torch.equal(x, y) for x, y in zip(r, runs[0])), "a repeat changed the result"


# ---- one fused stable-LN layer -------------------------------------------------------------------------------

P_HIDDEN, P_ACT = 0.1, 0.1
SEED_ARGS = {"triad_preln_fwd": (7, 8), "triad_preln_bwd": (9, 10), "triad_geludrop_fwd": (2, 3),
             "triad_geludrop_bwd": (3, 4)}     # positions of (p, seed)
QUERIES = ("triad_preln_bwd_blocks", "triad_dropaddln_bwd_blocks", "triad_gelu_table_bytes", "triad_gelu_table")


def _count_calls(monkeypatch, record=None):
    """Count the entry-point calls of postln.py and attention.py by name (size queries and the table
    build left out)."""
    from triad_amd import attention, postln
    seen = {}

    def wrap(real):
        def counting(name, *a, **k):
            if name not in QUERIES:
                seen[name] = seen.get(name, 0) + 1
                if record is not None:
                    record.append((name, a))
            return real(name, *a, **k)
        return counting
    monkeypatch.setattr(postln, "call", wrap(postln.call))
    monkeypatch.setattr(attention, "call", wrap(attention.call))
    return seen


def _stable_over(layers, **kw):
    """The small stable-LN config. 4 positional-conv groups: 64 channels per group, HuBERT-large's
    (1024 / 16), which triad_posconv has an instance for (the default 16 groups would give 16)."""
    over = dict(num_conv_pos_embedding_groups=4,hidden_size=256, num_hidden_layers=layers, num_attention_heads=4, intermediate_size=512,
                do_stable_layer_norm=True, feat_extract_norm="layer", hidden_dropout=0.0, activation_dropout=0.0,
                attention_dropout=0.0, layerdrop=0.0, feat_proj_dropout=0.0, final_dropout=0.0, mask_time_prob=0.0,
                mask_feature_prob=0.0)
    over.update(kw)
    return over


def _stable_hubert(layers, **kw):
    from transformers.models.hubert.modeling_hubert import HubertEncoderStableLayerNorm
    from triad_amd import model as Mdl
    torch.manual_seed(0)
    hub = Mdl.hubert_execution_tweaks(Mdl._hf_model("HubertModel", "none/none", _stable_over(layers, **kw))).to(dev)
    assert type(hub.encoder) is HubertEncoderStableLayerNorm and hasattr(hub.encoder, "_triad_stock_forward")
    return hub


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _layer_restatement(layer, final_norm, res, gy, masks):
    """LN -> attention -> add -> LN -> MLP -> add -> encoder LN in plain fp32 torch on the CPU with the
    given (mask, scale) per dropout."""
    ref, fin = copy.deepcopy(layer).cpu().float(), copy.deepcopy(final_norm).cpu().float()
    at, ff = ref.attention, ref.feed_forward
    B, N, E = res.shape
    H = at.num_heads

    def heads(t):
        return t.view(B, N, H, E // H).transpose(1, 2)

    def ln(m, t):
        return F.layer_norm(t, (E,), m.weight, m.bias, m.eps)
    n0 = ln(ref.layer_norm, res)
    q, k, v = (heads(F.linear(n0, m.weight, m.bias)) for m in (at.q_proj, at.k_proj, at.v_proj))
    a = torch.softmax(q @ k.transpose(-1, -2) * at.scaling, -1) @ v
    a = F.linear(a.transpose(1, 2).reshape(B, N, E), at.out_proj.weight, at.out_proj.bias)
    (m1, s1), (m2, s2), (m3, s3) = masks
    r1 = res + a * m1 * s1
    g = F.gelu(F.linear(ln(ref.final_layer_norm, r1), ff.intermediate_dense.weight, ff.intermediate_dense.bias)) * m2 * s2
    r2 = r1 + F.linear(g, ff.output_dense.weight, ff.output_dense.bias) * m3 * s3
    out = ln(fin, r2)
    (out * gy).sum().backward()
    grads = {"layer." + n: q.grad.clone() for n, q in ref.named_parameters() if q.grad is not None}
    grads.update({"final." + n: q.grad.clone() for n, q in fin.named_parameters()})
    return out.detach(), grads


def test_fused_stable_layer_dropout_seeds(monkeypatch):
    """One fused stable-LN layer (hidden 256, 4 heads of 64, intermediate 512, 2 x 24 tokens) at p = 0.1 on
    all three sites, followed by the encoder norm in its fp32 form: the three seeds of the pass are
    pairwise distinct, forward and backward use the same seed and the module's p, and the fp32 output and
    every parameter gradient match a plain fp32 torch restatement on the numpy masks of the recorded seeds
    (1e-2 / 3e-2 relative L2, k_proj.bias is noise)."""
    from triad_amd import postln
    record = []
    _count_calls(monkeypatch, record)
    hub = _stable_hubert(1, hidden_dropout=P_HIDDEN, activation_dropout=P_ACT).train()
    layer, final_norm = hub.encoder.layers[0], hub.encoder.layer_norm
    B, N, E, I = 2, 24, 256, 512
    g = torch.Generator().manual_seed(11)
    res = torch.randn(B, N, E, generator=g).to(BF)
    gy = torch.randn(B, N, E, generator=g)
    seeds = postln._Seeds()
    r = res.to(dev).requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        r0, nb = postln.drop_add_norm(r, None, layer.layer_norm, 0.0, 0)
        r2, out = postln.fused_stable_layer(layer, r0, nb, final_norm, seeds, True)
    assert out.dtype == F32 and r2.dtype == BF and nb.dtype == BF
    (out * gy.to(dev)).sum().backward()
    calls = [(n, float(a[SEED_ARGS[n][0]]), int(a[SEED_ARGS[n][1]])) for n, a in record if n in SEED_ARGS]
    assert [c[0] for c in calls] == ["triad_preln_fwd", "triad_preln_fwd", "triad_geludrop_fwd", "triad_preln_fwd",
                                     "triad_preln_bwd", "triad_geludrop_bwd", "triad_preln_bwd", "triad_preln_bwd"]
    fwd, bwd = calls[1:4], calls[4:7][::-1]
    assert [c[2] for c in fwd] == [c[2] for c in bwd], "backward seeds differ from the forward's"
    want_p = [P_HIDDEN, P_ACT, P_HIDDEN]
    for (_, p, _), (_, pb, _), wp in zip(fwd, bwd, want_p):
        assert abs(p - wp) < 1e-7 and abs(pb - wp) < 1e-7
    assert len({c[2] for c in fwd}) == 3, "two dropouts of one pass share a seed"
    assert calls[0][1] == 0.0 and calls[7][1] == 0.0
    shapes = [(B, N, E), (B, N, I), (B, N, E)]
    masks = [(R.keep_mask(s, p, sd).float(), R.drop_scale(p)) for (_, p, sd), s in zip(fwd, shapes)]
    ref_out, ref_grads = _layer_restatement(layer, final_norm, res.float(), gy, masks)
    grads = {"layer." + n: q.grad for n, q in layer.named_parameters() if q.grad is not None}
    grads.update({"final." + n: q.grad for n, q in final_norm.named_parameters()})
    e = _rel(out, ref_out)
    print(f"fused stable layer output rel L2 {e:.2e}")
    assert e < 1e-2, e
    assert set(grads) == set(ref_grads)
    for n in ref_grads:
        if n.endswith("k_proj.bias"):   # exactly 0 in exact arithmetic (softmax shift invariance): noise
            continue
        e = _rel(grads[n], ref_grads[n])
        print(f"fused stable layer grad {n} rel L2 {e:.2e}")
        assert e < 3e-2, (n, e)


# ---- the encoder against the stock loop ----------------------------------------------------------------------

def _run_encoder(hub, x, fwd, seed=None, autocast=True):
    """Forward + backward of hub with the encoder's forward set to fwd -> (output, {parameter: gradient},
    indices of the layers whose attention ran)."""
    from triad_amd import postln
    enc = hub.encoder
    ran = []
    attn_index = {id(layer.attention): i for i, layer in enumerate(enc.layers)}
    hooks = [layer.attention.register_forward_hook(lambda m, a, o: ran.append(attn_index[id(m)])) for layer in enc.layers]
    real = postln.self_attention

    def counted(attn, x, key_mask=None):
        ran.append(("fused", attn_index[id(attn)]))
        return real(attn, x, key_mask)
    postln.self_attention = counted
    keep_fwd = enc.forward
    try:
        hub.zero_grad(set_to_none=True)
        enc.forward = fwd
        if seed is not None:
            torch.manual_seed(seed)
        with torch.autocast("cuda", dtype=BF, enabled=autocast):
            out = hub(x).last_hidden_state
        gy = torch.linspace(-1, 1, out.numel(), device=dev).view_as(out)
        (out.float() * gy).sum().backward()
    finally:
        enc.forward = keep_fwd
        postln.self_attention = real
        for h in hooks:
            h.remove()
    grads = {n: q.grad.float().clone() for n, q in hub.named_parameters() if q.grad is not None}
    return out.detach(), grads, ran


def _compare_with_stock(hub, x, seed=None):
    """The bars of test_fused_hubert_encoder_matches_stock_without_dropout. A miss is reported with both
    runs' distance to the stock encoder with autocast off."""
    enc = hub.encoder
    o_f, g_f, ran_f = _run_encoder(hub, x, enc.forward, seed)
    o_s, g_s, ran_s = _run_encoder(hub, x, enc._triad_stock_forward, seed)
    assert o_f.shape == o_s.shape and o_f.dtype == o_s.dtype == F32
    fused_layers = [i for t in ran_f if isinstance(t, tuple) for i in t[1:]]
    assert fused_layers and [t for t in ran_s if isinstance(t, tuple)] == [], "the fused forward did not run"
    stock_layers = [t for t in ran_s if not isinstance(t, tuple)]
    assert fused_layers == stock_layers, (fused_layers, stock_layers)
    misses = []
    e = _rel(o_f, o_s)
    print(f"stable encoder output rel L2 {e:.2e}")
    if not e < 1e-2:
        misses.append(("output", e))
    assert set(g_f) == set(g_s)
    for n in g_s:
        if n.endswith("k_proj.bias"):  # exactly 0 in exact arithmetic (softmax shift invariance): noise
            assert float(g_f[n].norm()) < 1e-3 * float(g_s[n.replace("bias", "weight")].norm()) + 1e-6
            continue
        e = _rel(g_f[n], g_s[n])
        print(f"stable encoder grad {n} rel L2 {e:.2e}")
        if not e < 3e-2:
            misses.append((n, e))
    if misses:
        o_r, g_r, _ = _run_encoder(hub, x, enc._triad_stock_forward, seed, autocast=False)
        report = [(n, e, "fused vs fp32 %.2e" % (_rel(o_f, o_r) if n == "output" else _rel(g_f[n], g_r[n])),
                   "stock vs fp32 %.2e" % (_rel(o_s, o_r) if n == "output" else _rel(g_s[n], g_r[n]))) for n, e in misses]
        raise AssertionError(f"bars missed (1e-2 output, 3e-2 gradients): {report}")
    return stock_layers


def test_fused_stable_encoder_matches_stock_without_dropout():
    """Fused HubertEncoderStableLayerNorm vs the stock transformers loop, 2 layers, every dropout,
    LayerDrop and SpecAugment off, (2, 16000) samples: fp32 last_hidden_state from both, output relative
    L2 < 1e-2, every parameter gradient < 3e-2."""
    hub = _stable_hubert(2).train()
    x = 0.1 * torch.randn(2, 16000, device=dev)
    assert _compare_with_stock(hub, x) == [0, 1]


def test_fused_stable_encoder_matches_stock_with_layerdrop():
    """The same with layerdrop = 0.5 over 6 layers and torch.manual_seed reset before each run: the same
    layers execute (an interior one and the last are skipped at this seed, checked on the CPU generator),
    and the same bars hold; parameters of skipped layers get no gradient in either run."""
    seed, kept = P.layerdrop_seed(6, 0.5)
    assert 5 not in kept and any(i not in kept for i in range(1, 5)) and len(kept) >= 2
    hub = _stable_hubert(6, layerdrop=0.5).train()
    x = 0.1 * torch.randn(2, 16000, device=dev)
    assert _compare_with_stock(hub, x, seed) == kept


def test_stable_encoder_routing_at_ten_seconds(monkeypatch):
    """10 s of audio, B = 2 (499 tokens): triad_preln_fwd runs 2 L + 1 times, the post-LN pass never, and
    the streaming attention forward once per layer."""
    layers = 2
    hub = _stable_hubert(layers).train()
    seen = _count_calls(monkeypatch)
    x = 0.1 * torch.randn(2, 160000, device=dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        out = hub(x).last_hidden_state
    assert out.shape == (2, 499, 256) and out.dtype == F32 and bool(torch.isfinite(out).all())
    assert seen.get("triad_preln_fwd") == 2 * layers + 1, seen
    assert "triad_dropaddln_fwd" not in seen, seen
    assert seen.get("triad_attn_long_fwd") == layers and "triad_attn_fwd_dropout" not in seen, seen
    from triad_amd import postln
    monkeypatch.setattr(postln, "STABLE_ROUTE", False)     # the gate: the stock loop, before any fused work
    seen.clear()
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        stock = hub(x).last_hidden_state
    assert "triad_preln_fwd" not in seen and seen.get("triad_attn_long_fwd") == layers, seen
    assert stock.dtype == F32 and _rel(out, stock) < 1e-2
