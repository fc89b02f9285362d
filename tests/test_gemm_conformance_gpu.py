"""Conformance of the bf16 GEMM entry points of csrc/gemm.hip (the 128 x 128 double buffer, the
256 x 128 three-slot ring, the 256 x 256 eight-wave tile; four operand layouts, fp32 / bf16
output, alpha, bias epilogue, split-K with optional per-XCD placement) against the fp64 product
of the same bf16 operands, through the C ABI (`triad_amd._lib.call`), and of the Python wrappers
over them.

Every output and slab buffer is filled with NaN before the call, and a result is checked to be
finite before it is compared. Bounds are derived, not measured: bf16 x bf16 products are exact
in fp32, an any-order fp32 accumulation of Kd of them errs by at most (Kd - 1) u sum|a||b| to
first order (u = 2^-24), the alpha multiply and the bias add round once each; a factor 2 covers
an MFMA accumulator that does not round like IEEE at every step:

    fp32 output: |got - ref| <= 2 (Kd + 2 + splits) 2^-24 (|alpha| (|A| . |B|) + |bias|)
    bf16 output: the same + 2^-8 |ref|   (one rounding)

per element, |A| . |B| the fp64 product of the absolute values. One dropped product of a 448-deep
contraction exceeds the fp32 bound about 40 x.

Three bit-identities are read from the code: the bf16 result is the fp32 result of the same call
cast to bf16 (both evaluate (OutT)(alpha * acc + bias) on the same fp32 value); forms 1, 2 and 4
give the same fp32 result (each feeds v_mfma_f32_32x32x16_bf16 the k order 64 kt + 16 s + 8 h + j);
split s's slab is the plain GEMM of the same form over that split's k range.

All three held on MI355X. Largest err / bound seen there per group (69 cases, 2.4 s in all):
fp32 outputs a 0.0137, b padded 0.0043, b overlapping 0.0042, d split-K 0.0036; bf16 outputs (the
2^-8 rounding term dominates) a 0.990, b 0.972 / 0.968, c bias 0.993, d 0.985, e wrappers 0.981,
weight_grad 0.950, TriadLinear / _LinearFn 0.970. (Also in DESIGN.md §2.)
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
NAN = float("nan")
LAYOUTS = [(1, 1), (1, 0), (0, 1), (0, 0)]
WORST = {}   # group -> largest err / bound of this run (printed per check; pytest -s shows them)


def _lib():
    from triad_amd import _lib
    return _lib


def _at(t, elems=0):
    """Device pointer `elems` elements past t's first."""
    return ctypes.c_void_p(t.data_ptr() + t.element_size() * elems)


def _forms(M, N):
    """The forms whose own kernel runs at (M, N) when asked for by number (launch()'s policy:
    1 always, 2 when M % 256 == 0, 4 when M % 256 == 0 and N % 256 == 0)."""
    return [1] + ([2] if M % 256 == 0 else []) + ([4] if M % 256 == 0 and N % 256 == 0 else [])


@functools.lru_cache(maxsize=None)
def _problem(M, N, Kd, seed=0):
    """Seeded bf16 operands A [M][Kd], B [N][Kd] on the device with the fp64 product A . B^T of
    those bf16 values and the product of their absolute values. Shared and never modified."""
    g = torch.Generator().manual_seed(1000 * seed + M + 7 * N + 13 * Kd)
    A = torch.randn(M, Kd, generator=g).to(BF).to(dev)
    B = torch.randn(N, Kd, generator=g).to(BF).to(dev)
    ref = A.double() @ B.double().t()
    absprod = A.double().abs() @ B.double().abs().t()
    return A, B, ref, absprod


def _lay(X, kcontig):
    """X [rows][Kd] in the asked layout: (tensor, leading dimension)."""
    if kcontig:
        return X.contiguous(), X.shape[1]
    return X.t().contiguous(), X.shape[0]


def _bound(Kd, absprod, alpha=1.0, bias=None, splits=0, ref=None):
    b = abs(alpha) * absprod
    if bias is not None:
        b = b + bias.double().abs()
    b = 2.0 * (Kd + 2 + splits) * U * b
    if ref is not None:   # bf16 output: one rounding
        b = b + 2.0 ** -8 * ref.abs()
    return b


def _check(got, ref, bound, group, what):
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (unwritten or poisoned elements)"
    ratio = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
    WORST[group] = max(WORST.get(group, 0.0), ratio)
    print(f"{group} {what}: err/bound {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: err/bound {ratio}"


def _tag(dt):
    return "bf16" if dt == BF else "fp32"


def _gemm(Ap, lda, ak, Bp, ldb, bk, M, N, Kd, alpha, Cp, ldc, out_bf16, form):
    L = _lib()
    L.call("triad_gemm_bf16_form", Ap, lda, ak, Bp, ldb, bk, M, N, Kd, L.ptr(alpha), Cp, ldc, out_bf16, form,
           L.stream_ptr())


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    _problem.cache_clear()   # the shared operands and references: not held for the rest of the session
    print("\nGEMM conformance, largest err/bound per group:",
          ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))


# ---- a. forms x layouts x short k loops ---------------------------------------------------------

@pytest.mark.parametrize("Kd", [64, 128, 192, 256, 448])
@pytest.mark.parametrize("M,N", [(128, 128), (384, 640), (256, 128), (768, 384), (256, 256), (768, 768)])
def test_forms_layouts_short_k(M, N, Kd):
    """Every tile form that (M, N) admits x the four operand layouts x {fp32 with alpha = 0.7, fp32
    with alpha = NULL, bf16} at 1, 2, 3, 4 and 7 k-steps -- k loops shorter than, equal to and
    longer than the ring's two-stage prologue and both arms of its vmcnt switch. The shapes are
    chosen from launch()'s policy so that the requested form is the one that runs: form 1 always
    runs gemm_kernel (15 tiles at 384 x 640: tile_split's remainder branch), form 2 runs
    gemm_big_kernel when M % 256 == 0 (1 and 9 tiles), form 4 runs gemm_w8_kernel when M and N are
    multiples of 256 (1 and 9 tiles). fp32 within the derived bound; bf16 equal to the fp32 result
    of the same alpha cast to bf16, bit for bit; the fp32 results of all forms bit-identical."""
    A, B, ref, absprod = _problem(M, N, Kd)
    a07 = torch.tensor([0.7], device=dev)
    alpha = float(a07.double())   # the fp32 value the kernel multiplies by
    for ak, bk in LAYOUTS:
        Al, lda = _lay(A, ak)
        Bl, ldb = _lay(B, bk)
        first = None
        for form in _forms(M, N):
            what = f"form {form} layout ({ak},{bk}) {M}x{N}x{Kd}"
            out = {}
            for name, al, dt in (("f32_a", a07, F32), ("f32", None, F32), ("bf16_a", a07, BF), ("bf16", None, BF)):
                C = torch.full((M, N), NAN, dtype=dt, device=dev)
                _gemm(_at(Al), lda, ak, _at(Bl), ldb, bk, M, N, Kd, al, _at(C), N, int(dt == BF), form)
                out[name] = C
            _check(out["f32_a"], alpha * ref, _bound(Kd, absprod, alpha), "a.fp32", what + " alpha 0.7")
            _check(out["f32"], ref, _bound(Kd, absprod), "a.fp32", what + " alpha NULL")
            _check(out["bf16"], ref, _bound(Kd, absprod, ref=ref), "a.bf16", what + " bf16")
            assert torch.equal(out["bf16"], out["f32"].to(BF)), what + ": bf16 != cast of fp32"
            assert torch.equal(out["bf16_a"], out["f32_a"].to(BF)), what + ": bf16 != cast of fp32 (alpha)"
            if first is None:
                first = out
            else:
                assert torch.equal(out["f32"], first["f32"]), what + ": differs from form 1"
                assert torch.equal(out["f32_a"], first["f32_a"]), what + ": differs from form 1 (alpha)"


# ---- b. strides and bounds ----------------------------------------------------------------------

def _padded(mat, extra, spare=16):
    """mat as a view into a NaN-filled buffer: row stride = width + extra, `spare` rows before and
    after. Returns (buffer, pointer to the view's first element, leading dimension)."""
    R, W = mat.shape
    ld = W + extra
    buf = torch.full((R + 2 * spare, ld), NAN, dtype=mat.dtype, device=dev)
    buf[spare:spare + R, :W] = mat
    return buf, _at(buf, spare * ld), ld


def _sentinel_c(M, N, dt, spare=16):
    """C as a view (ldc = N + 8, 16 spare rows either side) into a buffer of a NaN bit pattern."""
    ldc = N + 8
    buf = torch.empty((M + 2 * spare, ldc), dtype=dt, device=dev)
    bits = buf.view(torch.int32 if dt == F32 else torch.int16)
    bits.fill_(0x7FC0DEAD if dt == F32 else 0x7FC1)
    return buf, bits, bits.clone(), ldc


def _c_padding_untouched(bits, before, M, N, spare=16):
    after = bits.clone()
    after[spare:spare + M, :N] = before[spare:spare + M, :N]
    return torch.equal(after, before)


@pytest.mark.parametrize("form,M,N", [(1, 384, 640), (2, 768, 384), (4, 768, 768)])
def test_padded_strides_and_bounds(form, M, N):
    """A, B and C as views into larger buffers: row strides of A and B the tight value + 24
    elements, ldc = N + 8, 16 spare rows before and after each operand; every element of A's and
    B's padding is NaN (none may reach the result), C's padding holds a bit pattern that must be
    unchanged afterwards. Kd = 192, every layout, fp32 and bf16 output."""
    Kd = 192
    A, B, ref, absprod = _problem(M, N, Kd)
    for ak, bk in LAYOUTS:
        Abuf, Ap, lda = _padded(_lay(A, ak)[0], 24)
        Bbuf, Bp, ldb = _padded(_lay(B, bk)[0], 24)
        for dt in (F32, BF):
            what = f"form {form} layout ({ak},{bk}) {_tag(dt)} padded"
            Cbuf, bits, before, ldc = _sentinel_c(M, N, dt)
            _gemm(Ap, lda, ak, Bp, ldb, bk, M, N, Kd, None, _at(Cbuf, 16 * ldc), ldc, int(dt == BF), form)
            _check(Cbuf[16:16 + M, :N], ref, _bound(Kd, absprod, ref=ref if dt == BF else None),
                   "b.padded." + _tag(dt), what)
            assert _c_padding_untouched(bits, before, M, N), what + ": wrote outside C"


@pytest.mark.parametrize("form,M,N", [(1, 384, 640), (2, 768, 384), (4, 768, 768)])
def test_overlapping_a_rows(form, M, N):
    """The conv stack's operand (frontend._gemm_rows): k-contiguous A with lda = 128 < Kd = 192,
    row m starting at element 128 m of a flat buffer (NaN before and after it), against the product
    of the materialised as_strided matrix. C padded as above."""
    Kd, lda, spare = 192, 128, 16 * 128
    g = torch.Generator().manual_seed(form)
    n = lda * (M - 1) + Kd
    flat = torch.full((n + 2 * spare,), NAN, dtype=BF, device=dev)
    flat[spare:spare + n] = torch.randn(n, generator=g).to(BF).to(dev)
    A = flat.as_strided((M, Kd), (lda, 1), spare).contiguous()
    B = _problem(M, N, Kd)[1]
    ref = A.double() @ B.double().t()
    absprod = A.double().abs() @ B.double().abs().t()
    for bk in (1, 0):
        Bbuf, Bp, ldb = _padded(_lay(B, bk)[0], 24)
        for dt in (F32, BF):
            what = f"form {form} overlapping A, b_kcontig {bk}, {_tag(dt)}"
            Cbuf, bits, before, ldc = _sentinel_c(M, N, dt)
            _gemm(_at(flat, spare), lda, 1, Bp, ldb, bk, M, N, Kd, None, _at(Cbuf, 16 * ldc), ldc, int(dt == BF), form)
            _check(Cbuf[16:16 + M, :N], ref, _bound(Kd, absprod, ref=ref if dt == BF else None),
                   "b.overlap." + _tag(dt), what)
            assert _c_padding_untouched(bits, before, M, N), what + ": wrote outside C"


# ---- c. bias epilogue ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,Kd", [(256, 256, 128), (384, 640, 192), (8192, 1024, 64), (32768, 256, 64)])
def test_bias_epilogue(M, N, Kd):
    """triad_gemm_bf16_bias / triad_gemm_bf16_bias_bf16 (tile form by shape: 128 x 128; the ring at
    8,192 x 1,024 = 256 ring tiles; the eight-wave tile at 32,768 rows) in F.linear's layout (1, 1)
    and the input gradient's (1, 0): within the bf16 bound of fp64(A . B^T) + bias for a bias of
    the product's magnitude, the two entry points bit-identical given the same bf16 bias, and
    bias = NULL the plain product."""
    L = _lib()
    A, B, ref, absprod = _problem(M, N, Kd)
    g = torch.Generator().manual_seed(M + N + Kd)
    b16 = (torch.randn(N, generator=g) * Kd ** 0.5).to(BF).to(dev)
    b32 = b16.float()
    b32_own = (torch.randn(N, generator=g) * Kd ** 0.5).to(dev)   # an fp32 bias that is no bf16 value
    for bk in (1, 0):
        Bl, ldb = _lay(B, bk)
        what = f"bias {M}x{N}x{Kd} layout (1,{bk})"

        def run(entry, bias):
            C = torch.full((M, N), NAN, dtype=BF, device=dev)
            L.call(entry, _at(A), Kd, 1, _at(Bl), ldb, bk, M, N, Kd, L.ptr(bias), _at(C), N, L.stream_ptr())
            return C
        y16, y32 = run("triad_gemm_bf16_bias_bf16", b16), run("triad_gemm_bf16_bias", b32)
        r = ref + b16.double()
        _check(y16, r, _bound(Kd, absprod, bias=b16, ref=r), "c.bias", what + " bf16 bias")
        _check(y32, r, _bound(Kd, absprod, bias=b16, ref=r), "c.bias", what + " fp32 bias")
        assert torch.equal(y16, y32), what + ": the two entry points differ"
        r = ref + b32_own.double()
        _check(run("triad_gemm_bf16_bias", b32_own), r, _bound(Kd, absprod, bias=b32_own, ref=r), "c.bias",
               what + " own fp32 bias")
        for entry in ("triad_gemm_bf16_bias", "triad_gemm_bf16_bias_bf16"):
            _check(run(entry, None), ref, _bound(Kd, absprod, ref=ref), "c.bias", what + f" {entry} NULL bias")


# ---- d. split-K ---------------------------------------------------------------------------------

SPLITK = [(7, 3, 0), (5, 4, 0), (4, 4, 0), (2, 8, 8), (16, 8, 8), (24, 16, 8)]


@pytest.mark.parametrize("ksteps,splits,flag", SPLITK)
@pytest.mark.parametrize("form,M,N", [(1, 128, 128), (2, 256, 128), (4, 256, 256)])
def test_splitk_slabs_and_sum(form, M, N, ksteps, splits, flag):
    """triad_gemm_bf16_splitk_form with split counts that do and do not divide the k-steps (empty
    splits at (5, 4), (2, 8) and (24, 16)), in the weight gradients' layout (0, 0) and in (1, 1),
    alpha NULL / 0.5, fp32 / bf16 C: every slab element written (slabs and C start as NaN), an empty
    split's slab exactly zero, slab s bit-identical to triad_gemm_bf16_form of the same form
    (alpha NULL, fp32) over that split's k range, C within the bound with `splits` extra additions,
    and the per-XCD placement (flag 8, splits % 8 == 0) bit-identical to the default one."""
    L = _lib()
    Kd = 64 * ksteps
    kps = -(-ksteps // splits) * 64
    A, B, ref, absprod = _problem(M, N, Kd, seed=1)
    half = torch.tensor([0.5], device=dev)
    for ak, bk in ((0, 0), (1, 1)):
        Al, lda = _lay(A, ak)
        Bl, ldb = _lay(B, bk)
        want = []   # per split: the plain GEMM over its k range, or None for an empty split
        for s in range(splits):
            kbeg, kend = s * kps, min(Kd, (s + 1) * kps)
            if kbeg >= kend:
                want.append(None)
                continue
            C = torch.full((M, N), NAN, dtype=F32, device=dev)
            _gemm(_at(Al, kbeg if ak else kbeg * lda), lda, ak, _at(Bl, kbeg if bk else kbeg * ldb), ldb, bk,
                  M, N, kend - kbeg, None, _at(C), N, 0, form)
            assert bool(torch.isfinite(C).all())
            want.append(C)
        assert sum(w is None for w in want) == max(0, splits - -(-ksteps // (kps // 64)))
        for al in (None, half):
            a = 1.0 if al is None else 0.5
            for dt in (F32, BF):
                got = {}
                for fl in sorted({0, flag}):
                    what = (f"split-K form {form}+{fl} layout ({ak},{bk}) {ksteps} k-steps / {splits} splits "
                            f"alpha {a} {_tag(dt)}")
                    slabs = torch.full((splits, M, N), NAN, dtype=F32, device=dev)
                    C = torch.full((M, N), NAN, dtype=dt, device=dev)
                    L.call("triad_gemm_bf16_splitk_form", _at(Al), lda, ak, _at(Bl), ldb, bk, M, N, Kd, splits,
                           L.ptr(al), _at(slabs), _at(C), int(dt == BF), form | fl, L.stream_ptr())
                    assert bool(torch.isfinite(slabs).all()), what + ": slab elements left unwritten"
                    for s, w in enumerate(want):
                        if w is None:
                            assert not bool(slabs[s].any()), what + f": empty split {s} is not zero"
                        else:
                            assert torch.equal(slabs[s], w), what + f": slab {s} != the GEMM of its k range"
                    r = a * ref
                    _check(C, r, _bound(Kd, absprod, a, splits=splits, ref=r if dt == BF else None),
                           "d.splitk." + _tag(dt), what)
                    got[fl] = (slabs, C)
                if flag:
                    assert torch.equal(got[0][0], got[flag][0]) and torch.equal(got[0][1], got[flag][1]), \
                        what + ": per-XCD placement changed the result"


# ---- e. Python wrappers -------------------------------------------------------------------------

def _misaligned(t):
    """A contiguous copy of t whose first element lies 2 bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 2
    return v


def _wide(t):
    """t as a column slice of a tensor three times as wide (row stride 3 x width)."""
    R, W = t.shape
    w = torch.full((R, 3 * W), NAN, dtype=t.dtype, device=t.device)
    w[:, W:2 * W] = t
    return w[:, W:2 * W]


@pytest.mark.parametrize("case", ["aligned", "x_misaligned", "w_misaligned", "x_noncontiguous", "untileable"])
def test_gemm_wrappers_take_any_operand(case):
    """gemm.linear / gemm.mm: an operand 2 bytes past a 16-byte boundary (which the entry points
    refuse: the wrappers send it to torch), a non-contiguous x (copied, HIP path) and untileable
    sizes (M = 130, N = 200, K = 72: torch) all give the product within the bf16 bound."""
    from triad_amd import gemm
    M, N, K = (130, 200, 72) if case == "untileable" else (256, 256, 128)
    A, W, ref, absprod = _problem(M, N, K, seed=2)
    g = torch.Generator().manual_seed(5)
    b = (torch.randn(N, generator=g) * K ** 0.5).to(BF).to(dev)
    x = {"x_misaligned": _misaligned, "x_noncontiguous": _wide}.get(case, lambda t: t)(A)
    w = _misaligned(W) if case == "w_misaligned" else W
    r = ref + b.double()
    _check(gemm.linear(x, w, b), r, _bound(K, absprod, bias=b, ref=r), "e.wrappers", f"linear {case}")
    _check(gemm.linear(x, w), ref, _bound(K, absprod, ref=ref), "e.wrappers", f"linear {case} no bias")
    wt = W.t().contiguous()           # [K][N]: mm's second operand
    wt = _misaligned(wt) if case == "w_misaligned" else wt
    _check(gemm.mm(x, wt), ref, _bound(K, absprod, ref=ref), "e.wrappers", f"mm {case}")


def test_weight_grad_reads_column_slices_in_place():
    """linear.weight_grad with dy2 and x2 as column slices of wider tensors (stride(0) = 3 x width,
    NaN beside them): bit-identical to the result on contiguous copies, within the bf16 bound."""
    from triad_amd import linear
    M, O, K = 192, 256, 128
    g = torch.Generator().manual_seed(9)
    dy = torch.randn(M, O, generator=g).to(BF).to(dev)
    x = torch.randn(M, K, generator=g).to(BF).to(dev)
    dyw, xw = _wide(dy), _wide(x)
    assert dyw.stride(0) == 3 * O and xw.stride(0) == 3 * K
    got, tight = linear.weight_grad(dyw, xw), linear.weight_grad(dy, x)
    ref = dy.double().t() @ x.double()
    absprod = dy.double().abs().t() @ x.double().abs()
    _check(got, ref, _bound(M, absprod, splits=2, ref=ref), "e.weight_grad", "column slices")
    assert torch.equal(got, tight)


def _linear_case(M, K, O, make):
    g = torch.Generator().manual_seed(M + K + O)
    x = torch.randn(M, K, generator=g).to(BF).to(dev)
    w = (torch.randn(O, K, generator=g) * K ** -0.5).to(BF).to(dev)
    b = torch.randn(O, generator=g).to(BF).to(dev)
    dy = torch.randn(M, O, generator=g).to(BF).to(dev)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    F.linear(xr, wr, br).backward(dy.double())
    xg = x.clone().requires_grad_(True)
    out, wp, bp = make(xg, w, b)
    out.backward(dy)
    dyd, xd, wd = dy.double(), x.double(), w.double()
    ref = F.linear(xd, wd, b.double())
    what = f"({M},{K},{O})"
    _check(out.detach(), ref, _bound(K, xd.abs() @ wd.abs().t(), bias=b, ref=ref), "e.linear", what + " y")
    _check(xg.grad, xr.grad, _bound(O, dyd.abs() @ wd.abs(), ref=xr.grad), "e.linear", what + " dX")
    # (2 = linear._splits below 4,096 tokens, where the split-K GEMM runs; torch's product has none)
    _check(wp.grad, wr.grad, _bound(M, dyd.abs().t() @ xd.abs(), splits=2, ref=wr.grad), "e.linear", what + " dW")
    _check(bp.grad, br.grad, _bound(M, dyd.abs().sum(0), ref=br.grad), "e.linear", what + " db")


@pytest.mark.parametrize("M,K,O", [(256, 768, 200), (130, 200, 136)])
def test_triad_linear_at_untileable_widths(M, K, O):
    """TriadLinear forward and backward under bf16 autocast at widths the GEMMs do not tile:
    output, dX, dW and db within the bf16 bound of an fp64 F.linear of the same bf16 operands,
    and no TriadError."""
    from triad_amd.linear import TriadLinear

    def make(xg, w, b):
        lin = TriadLinear(K, O).to(dev)
        with torch.no_grad():
            lin.weight.copy_(w)
            lin.bias.copy_(b)
        with torch.autocast("cuda", dtype=BF):
            return lin(xg), lin.weight, lin.bias
    _linear_case(M, K, O, make)


@pytest.mark.parametrize("M,K,O", [(256, 768, 200), (130, 200, 136), (256, 256, 384)])
def test_linear_function_at_untileable_widths(M, K, O):
    """linear._LinearFn itself (what TriadLinear and the fused QKV projection apply) at the same
    widths and at a tileable one: its forward already fell back to torch for such shapes; its
    backward's weight gradient used to be refused by the split-K entry point (TriadError)."""
    from triad_amd.linear import _LinearFn

    def make(xg, w, b):
        wp, bp = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        return _LinearFn.apply(xg, wp, bp), wp, bp
    _linear_case(M, K, O, make)
