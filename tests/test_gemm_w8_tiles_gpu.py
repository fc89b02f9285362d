"""The multi-tile eight-wave GEMM (gemm_w8_tiles_kernel, csrc/gemm.hip: one workgroup runs several
256 x 256 tiles back to back, the LDS-DMA pipeline of the one-tile loop carried across the seams)
against tile form 1 (gemm_kernel through triad_gemm_bf16_form), bit for bit: the k order per
accumulator and the epilogue arithmetic are the same, so nothing may differ. Every output starts
as NaN, so an element left unwritten fails.

What the cases are for: k loops of 1 (a seam in every k-step, the prefetch two tiles ahead), 2, 3,
4, 5 (odd depths put seams on both slot parities) and 12 k-steps (the workload's) on six tiles run
by 1, 2, 4 and 6 workgroups (6 in one, 3 + 3, 2 + 2 + 1 + 1, one each); 15 tiles on 4 workgroups
(the last workgroup one tile short, the drain on another tile count); alpha, both bias types with
n0 changing inside a workgroup, padded ldc, overlapping A rows; launches repeated on the same
buffers (a read placed by luck rather than by the vmcnt / barrier count shows as a repeat that
differs); and the routing of the product path.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32
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
    g = torch.Generator().manual_seed(91 + M + 7 * N + 13 * Kd)
    return torch.randn(M, Kd, generator=g).to(BF).to(dev), torch.randn(N, Kd, generator=g).to(BF).to(dev)


@functools.lru_cache(maxsize=None)
def _laid(M, N, Kd, ak, bk):
    A, B = _operands(M, N, Kd)
    return _lay(A, ak) + _lay(B, bk)


@functools.lru_cache(maxsize=None)
def _form1(M, N, Kd, ak, bk, dt):
    """The reference: form 1 on the shared operands, computed once per case; never modified."""
    Al, lda, Bl, ldb = _laid(M, N, Kd, ak, bk)
    L = _lib()
    C = torch.full((M, N), NAN, dtype=dt, device=dev)
    L.call("triad_gemm_bf16_form", _at(Al), lda, ak, _at(Bl), ldb, bk, M, N, Kd, L.ptr(None), _at(C), N, int(dt == BF),
           1, L.stream_ptr())
    return C


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for f in (_form1, _laid, _operands):
        f.cache_clear()


def _lay(X, kcontig):
    if kcontig:
        return X.contiguous(), X.shape[1]
    return X.t().contiguous(), X.shape[0]


def _tiles(Ap, lda, ak, Bp, ldb, bk, M, N, Kd, Cp, ldc, out_bf16, wgs, alpha=None, bias=None):
    L = _lib()
    L.call("triad_gemm_bf16_tiles", Ap, lda, ak, Bp, ldb, bk, M, N, Kd, L.ptr(alpha), Cp, ldc, out_bf16, L.ptr(bias),
           int(bias is not None and bias.dtype == BF), wgs, L.stream_ptr())


def _run(M, N, Kd, ak, bk, dt, wgs, **kw):
    Al, lda, Bl, ldb = _laid(M, N, Kd, ak, bk)
    C = torch.full((M, N), NAN, dtype=dt, device=dev)
    _tiles(_at(Al), lda, ak, _at(Bl), ldb, bk, M, N, Kd, _at(C), N, int(dt == BF), wgs, **kw)
    return C


def _same(a, b):
    """Bit-for-bit (NaN would compare unequal: an unwritten element fails)."""
    return bool(torch.isfinite(a).all()) and torch.equal(a, b)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- seams per loop depth -----------------------------------------------------------------------

@pytest.mark.parametrize("wgs", [1, 2, 4, 6])
@pytest.mark.parametrize("ksteps", [1, 2, 3, 4, 5, 12])
def test_seams_per_loop_depth(ksteps, wgs):
    M, N, Kd = 512, 768, 64 * ksteps
    for ak, bk in (LAYOUTS if ksteps in (1, 3, 12) else [(1, 1), (0, 0)]):
        for dt in (F32, BF):
            got = _run(M, N, Kd, ak, bk, dt, wgs)
            assert _same(got, _form1(M, N, Kd, ak, bk, dt)), \
                f"{wgs} workgroups != form 1: {M}x{N}x{Kd} layout ({ak},{bk}) {dt}"


@pytest.mark.parametrize("ksteps", [1, 2, 5])
def test_uneven_ends(ksteps):
    """15 tiles on 4 workgroups: 4 + 4 + 4 + 3."""
    M, N, Kd = 768, 1280, 64 * ksteps
    for ak, bk in LAYOUTS:
        for dt in (F32, BF):
            got = _run(M, N, Kd, ak, bk, dt, 4)
            assert _same(got, _form1(M, N, Kd, ak, bk, dt)), f"{M}x{N}x{Kd} layout ({ak},{bk}) {dt}"


# ---- output forms -------------------------------------------------------------------------------

@pytest.mark.parametrize("wgs", [1, 4])
def test_alpha(wgs):
    """alpha scales the accumulator before the one rounding, as in form 1."""
    M, N, Kd = 512, 768, 192
    L = _lib()
    alpha = torch.tensor([0.3125 + 2.0 ** -12], dtype=F32, device=dev)
    for ak, bk in ((1, 1), (0, 0)):
        Al, lda, Bl, ldb = _laid(M, N, Kd, ak, bk)
        for dt in (F32, BF):
            want = torch.full((M, N), NAN, dtype=dt, device=dev)
            L.call("triad_gemm_bf16_form", _at(Al), lda, ak, _at(Bl), ldb, bk, M, N, Kd, L.ptr(alpha), _at(want), N,
                   int(dt == BF), 1, L.stream_ptr())
            assert _same(_run(M, N, Kd, ak, bk, dt, wgs, alpha=alpha), want), f"alpha, layout ({ak},{bk}) {dt}"


@pytest.mark.parametrize("wgs", [1, 2, 4, 6])
@pytest.mark.parametrize("ksteps", [1, 3])
def test_bias_follows_the_tile(ksteps, wgs):
    """fp32 and bf16 bias, N = 768: n0 changes between the tiles of one workgroup, and every tile must
    get its own columns' bias (form 1's fp32 product + bias, rounded once)."""
    M, N, Kd = 512, 768, 64 * ksteps
    g = torch.Generator().manual_seed(5 + ksteps)
    b32 = (torch.randn(N, generator=g) * Kd ** 0.5).to(dev)
    b16 = (torch.randn(N, generator=g) * Kd ** 0.5).to(BF).to(dev)
    for ak, bk in ((1, 1), (1, 0)):
        prod = _form1(M, N, Kd, ak, bk, F32)
        for bias in (b32, b16):
            want = prod + bias.float()[None, :]
            for dt in (F32, BF):
                got = _run(M, N, Kd, ak, bk, dt, wgs, bias=bias)
                assert _same(got, want.to(dt)), f"{bias.dtype} bias, layout ({ak},{bk}) {dt}, {wgs} workgroups"


@pytest.mark.parametrize("ak,bk", LAYOUTS)
def test_padded_ldc_is_left_untouched(ak, bk):
    M, N, Kd, spare, wgs = 512, 768, 192, 4096, 2
    ldc = N + 8
    Al, lda, Bl, ldb = _laid(M, N, Kd, ak, bk)
    for dt in (F32, BF):
        Cf = torch.full((2 * spare + ldc * M,), NAN, dtype=dt, device=dev)
        _tiles(_at(Al), lda, ak, _at(Bl), ldb, bk, M, N, Kd, _at(Cf, spare), ldc, int(dt == BF), wgs)
        body = Cf[spare:spare + ldc * M].view(M, ldc)
        assert bool(torch.isnan(Cf[:spare]).all()) and bool(torch.isnan(Cf[spare + ldc * M:]).all())
        assert bool(torch.isnan(body[:, N:]).all()), f"layout ({ak},{bk}) {dt}: wrote C's padding"
        assert _same(body[:, :N], _form1(M, N, Kd, ak, bk, dt)), f"ldc = N + 8, layout ({ak},{bk}) {dt}"


@pytest.mark.parametrize("bk", [1, 0])
def test_overlapping_a_rows(bk):
    """The conv stack's operand: k-contiguous A with lda = 64 < Kd = 192."""
    M, N, Kd, lda, spare = 512, 768, 192, 64, 1024
    L = _lib()
    g = torch.Generator().manual_seed(3)
    n = lda * (M - 1) + Kd
    flat = torch.full((n + 2 * spare,), NAN, dtype=BF, device=dev)
    flat[spare:spare + n] = torch.randn(n, generator=g).to(BF).to(dev)
    Bl, ldb = _lay(_operands(M, N, Kd)[1], bk)
    for dt in (F32, BF):
        want = torch.full((M, N), NAN, dtype=dt, device=dev)
        L.call("triad_gemm_bf16_form", _at(flat, spare), lda, 1, _at(Bl), ldb, bk, M, N, Kd, L.ptr(None), _at(want), N,
               int(dt == BF), 1, L.stream_ptr())
        for wgs in (2, 4):
            C = torch.full((M, N), NAN, dtype=dt, device=dev)
            _tiles(_at(flat, spare), lda, 1, _at(Bl), ldb, bk, M, N, Kd, _at(C), N, int(dt == BF), wgs)
            assert _same(C, want), f"overlapping A rows, b_kcontig {bk}, {dt}, {wgs} workgroups"


# ---- placement by luck --------------------------------------------------------------------------

def _repeat(launch, C, want, what):
    first = None
    for rep in range(10):
        C.fill_(NAN)
        launch(C)
        if first is None:
            first = C.clone()
            assert _same(first, want), what + ": != form 1"
        else:
            assert _same(C, first), what + f": repeat {rep} differs from the first"


@pytest.mark.parametrize("ak,bk", [(1, 1), (0, 0)])
def test_routed_272_tiles_repeat_identical(ak, bk):
    """272 tiles through the product entry point: two tiles per workgroup on 256 CUs."""
    M, N, Kd = 4096, 4352, 832
    L = _lib()
    Al, lda, Bl, ldb = _laid(M, N, Kd, ak, bk)
    C = torch.empty((M, N), dtype=F32, device=dev)
    _repeat(lambda c: L.call("triad_gemm_bf16_form", _at(Al), lda, ak, _at(Bl), ldb, bk, M, N, Kd, L.ptr(None), _at(c),
                             N, 0, 4, L.stream_ptr()),
            C, _form1(M, N, Kd, ak, bk, F32), f"routed form 4, layout ({ak},{bk})")


@pytest.mark.parametrize("ak,bk", [(1, 1), (0, 0)])
def test_nine_tiles_per_workgroup_repeat_identical(ak, bk):
    M, N, Kd = 2048, 2304, 192
    Al, lda, Bl, ldb = _laid(M, N, Kd, ak, bk)
    C = torch.empty((M, N), dtype=F32, device=dev)
    _repeat(lambda c: _tiles(_at(Al), lda, ak, _at(Bl), ldb, bk, M, N, Kd, _at(c), N, 0, 8),
            C, _form1(M, N, Kd, ak, bk, F32), f"72 tiles on 8 workgroups, layout ({ak},{bk})")


# ---- routing ------------------------------------------------------------------------------------

def test_form4_routes_to_the_rule_of_triad_gemm_w8_workgroups():
    """A form-4 call with more tiles than CUs gives the bits of triad_gemm_bf16_tiles on
    triad_gemm_w8_workgroups(tiles, cus) workgroups."""
    M, N, Kd, ak, bk = 4096, 4352, 832, 1, 1
    L = _lib()
    tiles, cus = (M // 256) * (N // 256), _cus()
    assert tiles > cus, (tiles, cus)
    wgs = L.call("triad_gemm_w8_workgroups", tiles, cus)
    assert 1 <= wgs < tiles, wgs
    Al, lda, Bl, ldb = _laid(M, N, Kd, ak, bk)
    for dt in (F32, BF):
        routed = torch.full((M, N), NAN, dtype=dt, device=dev)
        L.call("triad_gemm_bf16_form", _at(Al), lda, ak, _at(Bl), ldb, bk, M, N, Kd, L.ptr(None), _at(routed), N,
               int(dt == BF), 4, L.stream_ptr())
        assert _same(routed, _run(M, N, Kd, ak, bk, dt, wgs)), dt
