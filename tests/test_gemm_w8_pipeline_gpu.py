"""The pipelined main loop of gemm_w8_kernel (csrc/gemm.hip, tile form 4: LDS-DMA in flight across
raw barriers, counted waits, two wave rows staggered by one barrier) against tile form 1
(gemm_kernel, which this loop does not touch and which tests/test_gemm_conformance_gpu.py checks
against fp64), bit for bit in fp32 and bf16: both feed each accumulator the
v_mfma_f32_32x32x16_bf16 products in the k order 64 kt + 16 s + 8 h + j, so nothing may differ.
Every output starts as NaN. One direct fp64 check per layout uses that suite's derived bound,
|got - ref| <= 2 (Kd + 2) 2^-24 (|A| . |B|) for an fp32 output.

What the cases are for: k loops of 1, 2, 3 (the straight-line drain only), 4, 5 (one loop trip,
even and odd rest), 8, 12 (the workload's) and 13 k-steps; a launch of 272 tiles on 256 CUs
repeated on the same buffers (a read placed by luck rather than by the vmcnt / barrier count shows
as a repeat that differs); split-K with splits of 1 to 4 k-steps and empty splits; overlapping A
rows; padded strides; the bias entry points (which reach form 4 at M >= 32,768).
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
NAN = float("nan")
LAYOUTS = [(1, 1), (1, 0), (0, 1), (0, 0)]


def _lib():
    from triad_amd import _lib
    return _lib


def _at(t, elems=0):
    return ctypes.c_void_p(t.data_ptr() + t.element_size() * elems)


@functools.lru_cache(maxsize=None)
def _operands(M, N, Kd):
    """Seeded N(0, 1) bf16 A [M][Kd], B [N][Kd] on the device; shared, never modified."""
    g = torch.Generator().manual_seed(77 + M + 7 * N + 13 * Kd)
    return torch.randn(M, Kd, generator=g).to(BF).to(dev), torch.randn(N, Kd, generator=g).to(BF).to(dev)


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _operands.cache_clear()


def _lay(X, kcontig):
    if kcontig:
        return X.contiguous(), X.shape[1]
    return X.t().contiguous(), X.shape[0]


def _gemm(Ap, lda, ak, Bp, ldb, bk, M, N, Kd, Cp, ldc, out_bf16, form):
    L = _lib()
    L.call("triad_gemm_bf16_form", Ap, lda, ak, Bp, ldb, bk, M, N, Kd, L.ptr(None), Cp, ldc, out_bf16, form,
           L.stream_ptr())


def _run(Al, lda, ak, Bl, ldb, bk, M, N, Kd, dt, form):
    C = torch.full((M, N), NAN, dtype=dt, device=dev)
    _gemm(_at(Al), lda, ak, _at(Bl), ldb, bk, M, N, Kd, _at(C), N, int(dt == BF), form)
    return C


def _same(a, b):
    """Bit-for-bit (NaN would compare unequal: an unwritten element fails)."""
    return bool(torch.isfinite(a).all()) and torch.equal(a, b)


# ---- loop depth ---------------------------------------------------------------------------------

@pytest.mark.parametrize("ksteps", [1, 2, 3, 4, 5, 8, 12, 13])
@pytest.mark.parametrize("M,N", [(256, 256), (512, 768)])
def test_loop_depth_equals_form1(M, N, ksteps):
    Kd = 64 * ksteps
    A, B = _operands(M, N, Kd)
    for ak, bk in LAYOUTS:
        Al, lda = _lay(A, ak)
        Bl, ldb = _lay(B, bk)
        for dt in (F32, BF):
            got = _run(Al, lda, ak, Bl, ldb, bk, M, N, Kd, dt, 4)
            want = _run(Al, lda, ak, Bl, ldb, bk, M, N, Kd, dt, 1)
            assert _same(got, want), f"form 4 != form 1: {M}x{N}x{Kd} layout ({ak},{bk}) {dt}"


@pytest.mark.parametrize("ak,bk", LAYOUTS)
def test_fp64_bound_per_layout(ak, bk):
    M, N, Kd = 512, 768, 832
    A, B = _operands(M, N, Kd)
    ref = A.double() @ B.double().t()
    bound = 2.0 * (Kd + 2) * U * (A.double().abs() @ B.double().abs().t())
    Al, lda = _lay(A, ak)
    Bl, ldb = _lay(B, bk)
    got = _run(Al, lda, ak, Bl, ldb, bk, M, N, Kd, F32, 4)
    assert bool(torch.isfinite(got).all())
    ratio = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"layout ({ak},{bk}) {M}x{N}x{Kd}: err/bound {ratio:.4f}")
    assert ratio <= 1.0, ratio


# ---- a launch larger than the chip, repeated ----------------------------------------------------

@pytest.mark.parametrize("ak,bk", [(1, 1), (0, 0)])
def test_272_tiles_repeat_identical(ak, bk):
    M, N, Kd = 4096, 4352, 832
    A, B = _operands(M, N, Kd)
    Al, lda = _lay(A, ak)
    Bl, ldb = _lay(B, bk)
    want = _run(Al, lda, ak, Bl, ldb, bk, M, N, Kd, F32, 1)
    C = torch.empty((M, N), dtype=F32, device=dev)
    first = None
    for rep in range(10):
        C.fill_(NAN)
        _gemm(_at(Al), lda, ak, _at(Bl), ldb, bk, M, N, Kd, _at(C), N, 0, 4)
        if first is None:
            first = C.clone()
            assert _same(first, want), f"layout ({ak},{bk}): form 4 != form 1"
        else:
            assert _same(C, first), f"layout ({ak},{bk}): repeat {rep} differs from the first"


# ---- split-K ------------------------------------------------------------------------------------

@pytest.mark.parametrize("ksteps,splits,flag", [(7, 3, 0), (5, 4, 0), (13, 4, 0), (3, 8, 8), (26, 8, 8)])
@pytest.mark.parametrize("M,N", [(256, 256), (512, 256)])
def test_splitk_slabs(M, N, ksteps, splits, flag):
    L = _lib()
    Kd = 64 * ksteps
    per = -(-ksteps // splits)
    kps = per * 64
    A, B = _operands(M, N, Kd)
    for ak, bk in ((0, 0), (1, 1)):
        Al, lda = _lay(A, ak)
        Bl, ldb = _lay(B, bk)

        def splitk(form):
            slabs = torch.full((splits, M, N), NAN, dtype=F32, device=dev)
            C = torch.full((M, N), NAN, dtype=F32, device=dev)
            L.call("triad_gemm_bf16_splitk_form", _at(Al), lda, ak, _at(Bl), ldb, bk, M, N, Kd, splits, L.ptr(None),
                   _at(slabs), _at(C), 0, form | flag, L.stream_ptr())
            return slabs, C
        slabs, C = splitk(4)
        what = f"split-K {M}x{N} {ksteps} k-steps / {splits} splits flag {flag} layout ({ak},{bk})"
        assert bool(torch.isfinite(slabs).all()), what + ": slab elements left unwritten"
        empty = 0
        for s in range(splits):
            kbeg, kend = s * kps, min(Kd, (s + 1) * kps)
            if kbeg >= kend:
                empty += 1
                assert not bool(slabs[s].view(torch.int32).any()), what + f": empty split {s} is not +0"
                continue
            Cs = torch.full((M, N), NAN, dtype=F32, device=dev)
            _gemm(_at(Al, kbeg if ak else kbeg * lda), lda, ak, _at(Bl, kbeg if bk else kbeg * ldb), ldb, bk,
                  M, N, kend - kbeg, _at(Cs), N, 0, 1)
            assert _same(slabs[s], Cs), what + f": slab {s} != form 1 over its k range"
        assert empty == splits - -(-ksteps // per), what
        assert _same(C, splitk(1)[1]), what + ": the sum differs from form 1's"


# ---- strides ------------------------------------------------------------------------------------

def _view_in_nan(mat, ld, spare):
    """mat's rows at stride ld inside a NaN-filled flat buffer with `spare` NaNs either side."""
    R, W = mat.shape
    flat = torch.full((2 * spare + ld * (R - 1) + W,), NAN, dtype=mat.dtype, device=dev)
    flat.as_strided((R, W), (ld, 1), spare).copy_(mat)
    return flat


@pytest.mark.parametrize("bk", [1, 0])
def test_overlapping_a_rows(bk):
    """The conv stack's operand: k-contiguous A with lda = 64 < Kd = 192."""
    M, N, Kd, lda, spare = 512, 256, 192, 64, 1024
    g = torch.Generator().manual_seed(3)
    n = lda * (M - 1) + Kd
    flat = torch.full((n + 2 * spare,), NAN, dtype=BF, device=dev)
    flat[spare:spare + n] = torch.randn(n, generator=g).to(BF).to(dev)
    Bl, ldb = _lay(_operands(M, N, Kd)[1], bk)
    for dt in (F32, BF):
        out = []
        for form in (4, 1):
            C = torch.full((M, N), NAN, dtype=dt, device=dev)
            _gemm(_at(flat, spare), lda, 1, _at(Bl), ldb, bk, M, N, Kd, _at(C), N, int(dt == BF), form)
            out.append(C)
        assert _same(out[0], out[1]), f"overlapping A rows, b_kcontig {bk}, {dt}"


@pytest.mark.parametrize("ak,bk", LAYOUTS)
def test_padded_strides(ak, bk):
    """lda, ldb = the tight value + 8 and ldc = N + 8, NaN in all padding: equal to form 1, and C's
    padding untouched."""
    M, N, Kd, spare = 512, 768, 320, 4096
    A, B = _operands(M, N, Kd)
    Al, Bl = _lay(A, ak)[0], _lay(B, bk)[0]
    lda, ldb, ldc = Al.shape[1] + 8, Bl.shape[1] + 8, N + 8
    Af, Bf = _view_in_nan(Al, lda, spare), _view_in_nan(Bl, ldb, spare)
    for dt in (F32, BF):
        out = []
        for form in (4, 1):
            Cf = torch.full((2 * spare + ldc * M,), NAN, dtype=dt, device=dev)
            _gemm(_at(Af, spare), lda, ak, _at(Bf, spare), ldb, bk, M, N, Kd, _at(Cf, spare), ldc, int(dt == BF), form)
            body = Cf[spare:spare + ldc * M].view(M, ldc)
            assert bool(torch.isnan(Cf[:spare]).all()) and bool(torch.isnan(Cf[spare + ldc * M:]).all())
            assert bool(torch.isnan(body[:, N:]).all()), f"form {form} layout ({ak},{bk}) {dt}: wrote C's padding"
            out.append(body[:, :N])
        assert _same(out[0], out[1]), f"padded strides, layout ({ak},{bk}), {dt}"


# ---- bias ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,Kd", [(32768, 256, 64), (512, 768, 832)])
def test_bias_entry_points(M, N, Kd):
    """triad_gemm_bf16_bias / _bias_bf16 against form 1's fp32 product + bias, cast once. At
    M = 32,768 they run form 4."""
    L = _lib()
    A, B = _operands(M, N, Kd)
    g = torch.Generator().manual_seed(M + N + Kd)
    b16 = (torch.randn(N, generator=g) * Kd ** 0.5).to(BF).to(dev)
    b32 = (torch.randn(N, generator=g) * Kd ** 0.5).to(dev)
    for bk in (1, 0):
        Bl, ldb = _lay(B, bk)
        prod = _run(A, Kd, 1, Bl, ldb, bk, M, N, Kd, F32, 1)
        for entry, bias in (("triad_gemm_bf16_bias", b32), ("triad_gemm_bf16_bias_bf16", b16)):
            C = torch.full((M, N), NAN, dtype=BF, device=dev)
            L.call(entry, _at(A), Kd, 1, _at(Bl), ldb, bk, M, N, Kd, L.ptr(bias), _at(C), N, L.stream_ptr())
            assert _same(C, (prod + bias.float()[None, :]).to(BF)), f"{entry} {M}x{N}x{Kd} layout (1,{bk})"
