"""Conformance of the ViT's row kernels -- csrc/lora.hip (triad_rows_nt, triad_lora_update,
triad_lora_tn with and without its fused dt) and csrc/resid_ln.hip (triad_addln_fwd,
triad_addln_bwd, every D / y / output-type / dres instance) -- against fp64 references of the same
bf16 / fp32 operands, through the C ABI (`triad_amd._lib.call`), and of vit.LoRALinear over them.

Operands come from a seeded CPU generator (tests/vit_rows_ref.py, which also holds the references,
the bounds and their derivation; tests/test_vit_rows_checks_cpu.py shows that each bound passes an
fp32 emulation of its kernel and fails one planted error). Every output, slab and workspace buffer
is filled with NaN before the call, carries NaN guard elements or rows past its end that must still
be NaN afterwards, and is checked to be finite before it is compared. The bounds are derived from
the rounding steps of the code, per element, u = 2^-24 (nothing is fitted to what the kernels
return):

    rows_nt            2 (K + 2) u (|X| . |W|) + 2^-8 |ref|
    lora_update        2 (8 + 2) u (|y| + |T| . |Bs|) + 2^-8 |ref|
    lora_tn out fp32   2 (n + 2) u |alpha| (|Y|^T . |T|),  n = min(M + G, 32 per + ceil(G / 16) + 18)
    lora_tn dt  bf16   2 (O + 8 + 2) u (|Y| . |Wt|) + 2^-8 |ref|
    addln mean         (h + 1) u mean|v|,  h = D / 64 + 5
    addln rstd         rstd (0.5 (dm rstd)^2 + (0.5 (h + 6) + 4) u)
    addln ln           |w| rstd dm + |xhat w| (rel_rstd + 4 u) + u |ref|  [+ 2^-8 |ref| for bf16]
    addln dx           rstd (u |wd| + (h + 2) u W1 + |xhat| (h + 5) u W2 + 3 u |xhat c2| + 3 u T) + u |ref|

Bit-identities read from the code: xn == torch's unfused fp32 x + g * y.float() (__fmul_rn /
__fadd_rn); dy == (g * dx).to(bf16) of the kernel's own dx; a padded leading dimension changes no
output bit; lora_tn has no atomics and a fixed slab order, so repeats are bit-identical -- checked
three times on the two shapes that run more than one tile per block (M = 16 416: 513 tiles, 2 per
block, blocks 257 .. 511 idle and their slabs zero; M = 32 805: 1 026 tiles, 3 per block).

Largest err / bound per group on MI355X (42 cases, 644 comparisons, 1.8 - 3.1 s in all; also in
DESIGN.md section 2). bf16 outputs, where the one rounding fills its 2^-8 term: rows_nt 0.976,
lora_update 0.996, lora_tn dt 0.959, addln ln 0.996, LoRALinear y 0.888 and dx 0.854. fp32 outputs:
lora_tn out 0.122, addln ln 0.843, dx 0.332, rstd 0.146, mean 0.070. LoRALinear dA 0.0084 and dB
0.0048 are below 0.01 and stay so on purpose: their bound has to allow a bf16 rounding flip of every
element of t / dt that lies within the fp32 sum's bound of a rounding boundary, and none flips; one
row of dy or x left out of the sum still exceeds the bound 27 x at M = 1 001 and over 4 000 x at
M = 33 (tests/test_vit_rows_checks_cpu.py), and the lora_tn groups above check the same kernel
tightly. All bit-identities held, after one fix: the forward kernel had fused x + g * y into one fma
(test_addln_forward failed on every D; csrc/resid_ln.hip add_scaled_unfused).
"""
import ctypes
import functools

import pytest
import torch

from tests import vit_rows_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
EPS = 1e-6
GUARD = 64     # NaN elements past the end of a flat output
GROWS = 4      # NaN rows past row M - 1 of a row-kernel output
WORST = {}     # group -> largest err / bound of this run (printed per check; pytest -s shows them)


def _lib():
    from triad_amd import _lib
    return _lib


def _at(t, elems=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + t.element_size() * elems)


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
    assert r <= 1.0, f"{what}: err/bound {r}"


def _padded(mat, extra):
    """mat on the device as the first columns of a NaN-filled buffer of row stride width + extra."""
    buf = torch.full((mat.shape[0], mat.shape[1] + extra), NAN, dtype=mat.dtype, device=dev)
    buf[:, :mat.shape[1]] = mat.to(dev)
    return buf, mat.shape[1] + extra


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nViT row kernels, largest err/bound per group:",
          ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))


# ---- triad_rows_nt ------------------------------------------------------------------------------

def _rows_nt(Xd, ldx, M, K, Wd, J):
    L = _lib()
    out = _nan(M * J + GUARD, BF)
    L.call("triad_rows_nt", _at(Xd), ldx, M, K, _at(Wd), J, _at(out), L.stream_ptr())
    assert _all_nan(out[M * J:]), f"rows_nt {M}x{K}x{J}: wrote past out[M][J]"
    return out[:M * J].view(M, J)


@pytest.mark.parametrize("K", [32, 96, 128, 160, 768])
def test_rows_nt(K):
    """out[m][j] = sum_k X[m][k] W[j][k] at 1, 3, 4, 5 and 24 k-steps (below, at and one past the
    prefetch depth 4), row counts around the 16-row wave and the 64-row block (the clamped tail
    rows), J = 1, 8 and 16 columns; 64 NaN elements after out[M][J] stay NaN."""
    for M in (1, 15, 16, 17, 63, 64, 65, 130):
        for J in (1, 8, 16):
            X, W = R.rows_nt_case(M, K, J)
            got = _rows_nt(X.to(dev), K, M, K, W.to(dev), J)
            _check(got, *R.rows_nt_ref(X, W), "rows_nt", f"M {M} K {K} J {J}")


def test_rows_nt_padded_ldx():
    """ldx = K + 8 with NaN in the padding columns: bit-identical to the tight call."""
    M, K, J = 65, 160, 8
    X, W = R.rows_nt_case(M, K, J)
    Xp, ldx = _padded(X, 8)
    got = _rows_nt(Xp, ldx, M, K, W.to(dev), J)
    _check(got, *R.rows_nt_ref(X, W), "rows_nt", f"M {M} K {K} J {J} ldx {ldx}")
    assert torch.equal(got, _rows_nt(X.to(dev), K, M, K, W.to(dev), J))


# ---- triad_lora_update --------------------------------------------------------------------------

@pytest.mark.parametrize("O", [8, 256, 768])
def test_lora_update(O):
    """Y += T Bs^T in place with the row stride of the thread grid (1 024 row groups) above, at and
    below the row count (M = 2 500: three rows per thread); NaN after Y[M][O] stays NaN."""
    L = _lib()
    for M in (1, 7, 1024, 1025, 2500):
        Y, T, Bs = R.lora_update_case(M, O)
        buf = _nan(M * O + GUARD, BF)
        buf[:M * O] = Y.to(dev).view(-1)
        Td, Bd = T.to(dev), Bs.to(dev)
        L.call("triad_lora_update", _at(buf), O, M, O, _at(Td), _at(Bd), L.stream_ptr())
        assert _all_nan(buf[M * O:]), f"lora_update {M}x{O}: wrote past Y"
        _check(buf[:M * O].view(M, O), *R.lora_update_ref(Y, T, Bs), "lora_update", f"M {M} O {O}")


def test_lora_update_padded_ldy():
    """ldy = O + 8: the padding columns hold a bit pattern that must be unchanged; the result is
    bit-identical to the tight call."""
    L = _lib()
    M, O = 1025, 256
    Y, T, Bs = R.lora_update_case(M, O)
    Td, Bd = T.to(dev), Bs.to(dev)
    buf = torch.empty((M, O + 8), dtype=BF, device=dev)
    bits = buf.view(torch.int16)
    bits.fill_(0x7FC1)
    buf[:, :O] = Y.to(dev)
    L.call("triad_lora_update", _at(buf), O + 8, M, O, _at(Td), _at(Bd), L.stream_ptr())
    assert bool((bits[:, O:] == 0x7FC1).all()), "lora_update wrote into the padding columns"
    _check(buf[:, :O], *R.lora_update_ref(Y, T, Bs), "lora_update", f"M {M} O {O} ldy {O + 8}")
    tight = Y.to(dev).clone()
    L.call("triad_lora_update", _at(tight), O, M, O, _at(Td), _at(Bd), L.stream_ptr())
    assert torch.equal(buf[:, :O], tight)


# ---- triad_lora_tn ------------------------------------------------------------------------------

def _lora_tn(Yd, ldy, M, O, Td, Wtd, alpha):
    """One call with NaN-filled slabs, out and dt (+ guards). Returns (out [O][8], dt [M][8] or
    None, slabs [G][O][8]) on the device."""
    L = _lib()
    G = L.call("triad_lora_tn_blocks", M)
    assert G == R.tn_blocks(M)
    slabs = _nan(G * O * 8, F32)
    out = _nan(O * 8 + GUARD, F32)
    dt = None if Wtd is None else _nan(M * 8 + GUARD, BF)
    L.call("triad_lora_tn", _at(Yd), ldy, M, O, _at(Td), _at(Wtd), _at(dt), alpha, _at(slabs), _at(out),
           L.stream_ptr())
    what = f"lora_tn M {M} O {O}"
    assert _all_nan(out[O * 8:]), what + ": wrote past out"
    assert bool(torch.isfinite(slabs).all()), what + ": slab elements left unwritten"
    slabs = slabs.view(G, O, 8)
    used = -(-((M + 31) // 32) // R.tn_per(M))   # blocks that own a tile
    assert not bool(slabs[used:].any()), what + ": an idle block's slab is not zero"
    if dt is not None:
        assert _all_nan(dt[M * 8:]), what + ": wrote past dt"
        dt = dt[:M * 8].view(M, 8)
    return out[:O * 8].view(O, 8), dt, slabs


@functools.lru_cache(maxsize=2)
def _tn_problem(M, O, alpha):
    """Seeded operands (CPU) with the fp64 references and bounds of out and dt: computed once."""
    Y, T, Wt = R.lora_tn_case(M, O)
    return Y, T, Wt, R.lora_tn_out_ref(Y, T, R.f32(alpha)), R.lora_tn_dt_ref(Y, Wt)


def _tn_both(M, O, alpha, what, pad=0):
    """Both instances at one problem against the references (ldy = O + pad, NaN in the padding):
    (out with dt, dt, out without dt)."""
    Y, T, Wt, (ref, bound), dt_want = _tn_problem(M, O, alpha)
    Yd, ldy = _padded(Y, pad)
    Td, Wtd = T.to(dev), Wt.to(dev)
    out1, dt, _ = _lora_tn(Yd, ldy, M, O, Td, Wtd, alpha)
    out0, _, _ = _lora_tn(Yd, ldy, M, O, Td, None, alpha)
    _check(out1, ref, bound, "lora_tn.out", what + " with dt")
    _check(out0, ref, bound, "lora_tn.out", what + " without dt")
    _check(dt, *dt_want, "lora_tn.dt", what)
    return out1, dt, out0


@pytest.mark.parametrize("nc", R.TN_WIDTHS)
def test_lora_tn_every_width(nc):
    """Every O / 256 the entry point has an instance for, M = 33 (two tiles, the second with one
    row), alpha = 0.37, with and without the fused dt."""
    _tn_both(33, 256 * nc, 0.37, f"M 33 O {256 * nc} alpha 0.37")


@pytest.mark.parametrize("O", [256, 768])
def test_lora_tn_row_tails_and_alpha(O):
    """Row counts around the 32-row tile, alpha 1, 2 and 0.37."""
    for M in (1, 31, 32, 33, 100):
        for alpha in (1.0, 2.0, 0.37):
            _tn_both(M, O, alpha, f"M {M} O {O} alpha {alpha}")


def test_lora_tn_padded_ldy():
    """ldy = O + 8 with NaN in the padding columns: bit-identical to the tight call."""
    M, O = 100, 768
    padded = _tn_both(M, O, 0.37, f"M {M} O {O} ldy {O + 8}", pad=8)
    tight = _tn_both(M, O, 0.37, f"M {M} O {O}")
    assert all(torch.equal(p, t) for p, t in zip(padded, tight))


@pytest.mark.parametrize("M,per", [(16385 + 31, 2), (32805, 3)])
def test_lora_tn_several_tiles_per_block(M, per):
    """The only shapes whose blocks loop over more than one tile (past 512 tiles): 513 tiles at 2
    per block (blocks 257 .. 511 own no tile and must still write a zero slab over the NaN) and
    1 026 tiles at 3 per block. Both instances, each run three times: bit-identical results."""
    O = 256
    assert R.tn_per(M) == per and R.tn_blocks(M) == 512
    runs = [_tn_both(M, O, 0.37, f"M {M} O {O} run {i}") for i in range(3)]
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r, runs[0])), f"M {M}: a repeat changed the result"
    _tn_problem.cache_clear()


# ---- triad_addln_fwd / triad_addln_bwd ----------------------------------------------------------

def _rows(M, D, dt):
    return torch.full((M + GROWS, D), NAN, dtype=dt, device=dev)


def _addln_fwd(c, M, D, has_y, out_f32):
    """The forward on case c; checks the guard rows; returns device xn (None without y), ln, mean,
    rstd, each cut to M rows."""
    L = _lib()
    xn, ln = _rows(M, D, F32), _rows(M, D, F32 if out_f32 else BF)
    mean, rstd = _nan(M + GROWS, F32), _nan(M + GROWS, F32)
    L.call("triad_addln_fwd", _at(c["x"]), _at(c["y"]) if has_y else None, _at(c["g"]), _at(c["w"]), _at(c["b"]),
           EPS, M, D, _at(xn), _at(ln), int(out_f32), _at(mean), _at(rstd), L.stream_ptr())
    what = f"addln_fwd M {M} D {D} y {has_y} f32 {out_f32}"
    for t in (ln, mean, rstd):
        assert _all_nan(t[M:]), what + ": wrote past row M - 1"
    assert _all_nan(xn[M:] if has_y else xn), what + ": wrote xn rows it does not own"
    return (xn[:M] if has_y else None), ln[:M], mean[:M], rstd[:M]


@pytest.mark.parametrize("D", [256, 512, 768, 1024, 1280, 1536])
def test_addln_forward(D):
    """Every D instance x {y, y == NULL} x {bf16, fp32 ln} at M = 1, 4, 5, 131 (M % 4 tails of the
    four-rows-per-block grid). xn bit-identical to torch's x + g * y.float() and untouched when
    y == NULL; mean, rstd and ln against the fp64 LayerNorm of that exact xn. At D = 768 rows 0 .. 2
    are a mean-100 / sigma-0.1 row, a mean-0 / sigma-1e-3 row and a constant row (mean exact,
    ln == b)."""
    eps = R.f32(EPS)
    for M in (1, 4, 5, 131):
        c = R.addln_case(M, D)
        d = {k: v.to(dev) for k, v in c.items()}
        for has_y in (True, False):
            for out_f32 in (False, True):
                what = f"M {M} D {D} y {has_y} f32 {out_f32}"
                xn, ln, mean, rstd = _addln_fwd(d, M, D, has_y, out_f32)
                v = c["x"]
                if has_y:
                    v = R.addln_xn(c["x"], c["y"], c["g"])
                    assert torch.equal(xn.cpu(), v), what + ": xn != x + g * y.float()"
                want = R.addln_fwd_ref(v, c["w"], c["b"], eps, not out_f32)
                _check(mean, *want["mean"], "addln.mean", what)
                _check(rstd, *want["rstd"], "addln.rstd", what)
                _check(ln, *want["ln"], "addln.ln." + ("f32" if out_f32 else "bf16"), what)
                if D == 768 and M >= 4:
                    k = R.SPECIAL_ROWS["const"]
                    assert float(mean[k]) == R.CONST, what + ": constant row's mean"
                    assert torch.equal(ln[k].cpu().float(), c["b"].to(ln.dtype).float()), what + ": constant row ln != b"


@pytest.mark.parametrize("D", [256, 512, 768, 1024, 1280, 1536])
def test_addln_backward(D):
    """Every D instance x {bf16, fp32 dln} x {dres, dres == NULL} at M = 1, 5, 131, with xn, mean
    and rstd from the forward kernel: dx against the fp64 LayerNorm backward at those statistics,
    dy bit-identical to (g * dx).to(bf16) of the kernel's dx."""
    L = _lib()
    for M in (1, 5, 131):
        c = R.addln_case(M, D)
        d = {k: v.to(dev) for k, v in c.items()}
        xn, _, mean, rstd = _addln_fwd(d, M, D, True, False)
        xn, mean, rstd = xn.contiguous(), mean.contiguous(), rstd.contiguous()
        xc, mc, rc = xn.cpu(), mean.cpu(), rstd.cpu()
        for key in ("dln_bf16", "dln_f32"):
            for has_res in (True, False):
                what = f"M {M} D {D} {key} dres {has_res}"
                dx, dy = _rows(M, D, F32), _rows(M, D, BF)
                L.call("triad_addln_bwd", _at(d[key]), int(key == "dln_f32"), _at(d["dres"]) if has_res else None,
                       _at(xn), _at(mean), _at(rstd), _at(d["w"]), _at(d["g"]), M, D, _at(dx), _at(dy), L.stream_ptr())
                assert _all_nan(dx[M:]) and _all_nan(dy[M:]), what + ": wrote past row M - 1"
                ref, bound = R.addln_bwd_ref(c[key], c["dres"] if has_res else None, xc, mc, rc, c["w"])
                _check(dx[:M], ref, bound, "addln.dx", what)
                assert bool(torch.isfinite(dy[:M]).all()), what + ": dy not finite"
                assert torch.equal(dy[:M].cpu(), R.addln_dy(dx[:M].cpu(), c["g"])), what + ": dy != bf16(g * dx)"


# ---- vit.LoRALinear -----------------------------------------------------------------------------

HIP_LORA_CALLS = {"triad_rows_nt": 1, "triad_lora_update": 2, "triad_lora_tn": 2}


def _count_calls(monkeypatch):
    """Count vit.py's entry-point calls by name (size queries left out)."""
    from triad_amd import vit as V
    seen = {}
    real = V.call

    def counting(name, *a, **k):
        if name != "triad_lora_tn_blocks":
            seen[name] = seen.get(name, 0) + 1
        return real(name, *a, **k)
    monkeypatch.setattr(V, "call", counting)
    return seen


def _lora_module(K, O, g, b_std=0.05):
    """LoRALinear over a frozen bf16 Linear(K, O), every parameter a bf16 value; r 8, alpha 16."""
    from triad_amd.vit import LoRALinear
    base = torch.nn.Linear(K, O)
    with torch.no_grad():
        base.weight.copy_((torch.randn(O, K, generator=g) * K ** -0.5).to(BF).float())
        base.bias.copy_(torch.randn(O, generator=g).to(BF).float())
    base = base.to(dev)
    base.weight.data, base.bias.data = base.weight.data.to(BF), base.bias.data.to(BF)
    for p in base.parameters():
        p.requires_grad = False
    m = LoRALinear(base, 8, 16).to(dev)
    with torch.no_grad():
        m.lora_A.copy_((torch.randn(8, K, generator=g) * K ** -0.5).to(BF).float())
        m.lora_B.copy_((torch.randn(O, 8, generator=g) * b_std).to(BF).float())
    return m


def _train_once(m, M, K, O, g):
    x = torch.randn(M, K, generator=g).to(BF).float()
    dy = torch.randn(M, O, generator=g).to(BF).float()
    xd = x.to(dev).requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        y = m(xd)
    dx, dA, dB = torch.autograd.grad((y.float() * dy.to(dev)).sum(), (xd, m.lora_A, m.lora_B))
    return x, dy, y.detach(), dx, dA, dB


@pytest.mark.parametrize("K,O", [(768, 2304), (768, 768), (1024, 3072)])
def test_lora_linear_takes_the_hip_path(monkeypatch, K, O):
    """Forward + backward under bf16 autocast: one rows_nt, two lora_update (y, then dx) and two
    lora_tn (dB + dt, then dA) calls -- the fast path is the one that ran."""
    seen = _count_calls(monkeypatch)
    g = torch.Generator().manual_seed(K + O)
    out = _train_once(_lora_module(K, O, g), 33, K, O, g)
    assert seen == HIP_LORA_CALLS
    assert all(bool(torch.isfinite(t).all()) for t in out)


@pytest.mark.parametrize("K,O", [(384, 1152), (1280, 1280)])
def test_lora_linear_outside_the_kernels_widths_trains_on_torch(monkeypatch, K, O):
    """Widths triad_lora_tn has no instance for (384 and 1152 are no multiples of 256; 1280 / 256 =
    5 passed the old gate, ran the forward on HIP and raised TriadError in the backward): forward
    and backward succeed, make no HIP call, and match the fp64 chain to bf16 accuracy."""
    seen = _count_calls(monkeypatch)
    g = torch.Generator().manual_seed(K + O)
    m = _lora_module(K, O, g)
    x, dy, y, dx, dA, dB = _train_once(m, 33, K, O, g)
    assert seen == {}
    xr = x.double().requires_grad_(True)
    Ar, Br = m.lora_A.detach().cpu().double().requires_grad_(True), m.lora_B.detach().cpu().double().requires_grad_(True)
    ref = xr @ m.base.weight.cpu().double().t() + m.base.bias.cpu().double() + m.scaling * (xr @ Ar.t()) @ Br.t()
    rx, rA, rB = torch.autograd.grad((ref * dy.double()).sum(), (xr, Ar, Br))
    for got, want in ((y, ref.detach()), (dx, rx), (dA, rA), (dB, rB)):
        rel = float((got.cpu().double() - want).norm() / want.norm())
        assert rel < 2e-2, rel


@pytest.mark.parametrize("M", [33, 1001])
def test_lora_linear_vs_fp64(monkeypatch, M):
    """LoRALinear(768, 768) forward and backward against the fp64 x W^T + b + s (x A^T) B^T of the
    bf16 operands, t and dt rounded to bf16 as the product stores them: y, dx, dA and dB within
    vit_rows_ref.lora_linear_ref's per-element bounds."""
    K = O = 768
    seen = _count_calls(monkeypatch)
    g = torch.Generator().manual_seed(M)
    m = _lora_module(K, O, g)
    x, dy, y, dx, dA, dB = _train_once(m, M, K, O, g)
    assert seen == HIP_LORA_CALLS
    s = float(m.scaling)
    sB = (m.lora_B.detach().cpu() * s).to(BF)
    want = R.lora_linear_ref(x.to(BF), m.base.weight.cpu(), m.base.bias.cpu(), m.lora_A.detach().cpu().to(BF), sB, s,
                             dy.to(BF))
    for name, got in (("y", y), ("dx", dx), ("dA", dA), ("dB", dB)):
        _check(got, *want[name], "lora_linear." + name, f"M {M}")
