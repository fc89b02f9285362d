"""Conformance of the post-LN kernels of csrc/postln.hip -- triad_dropout_keep, triad_dropaddln_fwd /
_bwd (every D instance, the grid-stride trips past 4096 rows, dh / dhb NULL), triad_geludrop_fwd /
_bwd (table and formula, with and without dropout, past one sweep of the persistent grid),
triad_gelu_table -- through the C ABI (`triad_amd._lib.call`), of the wrappers drop_add_ln / gelu_drop
over them, and of the dropout seeds of one fused HuBERT layer.

Operands come from a seeded CPU generator (tests/postln_ref.py, which also holds the numpy definition
of the keep bits, the fp64 references, the bounds and their derivation;
tests/test_postln_checks_cpu.py shows that each bound passes an emulation of its kernel and that each
of thirteen planted errors fails one). Every output, part and table buffer is filled with NaN (0xFF
bytes for the u8 keep bits) before the call, carries a guard past its end that must be unchanged
afterwards, and is checked to be finite before it is compared. Each operand sits in its own buffer.
Keep bits always come from the numpy definition; triad_dropout_keep is itself compared with it bit for
bit (the pair index's high word, n > 2^33 elements, cannot be reached with a test-sized buffer; the
numpy side of it is pinned by a hand-worked value in the CPU file).

Bounds (u = 2^-24, h = D / 64 + 5, ez = u |z| or 0 on a row whose z are fp32 values; derivations in
tests/postln_ref.py; nothing is fitted to what the kernels return):
    mean    (h + 1) u mean|z| + mean ez
    rstd    rstd (0.5 (dm rstd)^2 + (0.5 (h + 6) + 4) u + 0.5 rstd^2 (2 mean(|z - m| ez) + mean ez^2))
    h       |w| rstd (dm + ez) + |xhat w| (rel_rstd + 4 u) + u |ref|          [hb: + 2^-8 |ref|]
    dres    rstd (e_wd + e_c1 + e_xh |c2| + |xh| e_c2 + u |xh c2| + 3 u T) + (u + rel_r) |ref|
    part    sum_rows (edl |xh| + |dl| e_xh) + (trips + 3) u sum_rows |dl xh|   (dbeta: without xh)
    total   the partials' bounds summed (the wrapper's: + triad_sum_slabs' depth)
    gelu    absolute, from an ASSUMED erff 4 ulp / expf 1 ulp (doubled), + the bf16 roundings
Identities asserted exactly: hb == bf16(h); dy == bf16(bf16(dres) keep scale); a constant row gives
h == b; both gradients NULL give exact zeros; repeats are bit-identical; table == NULL and the table
give identical bits; geludrop_fwd at p == bf16(g keep scale) of its own p = 0 output; aten gelu /
gelu_backward bit for bit on the same mask.

Largest err / bound per group on MI355X (35 cases, 570 bound comparisons, 8 s in all, of which 3 s
build the HubertModel of the layer test; also in DESIGN.md section 2). bf16 outputs, where the one
rounding fills its 2^-8 term: fwd hb 0.995, gelu fwd 0.975 / bwd 0.985, table value 0.975, wrapper hb
0.996 / gelu v 0.880 / du 0.996. fp32 outputs: fwd h 0.482, mean 0.078, rstd 0.135; bwd dres 0.399,
part dgamma 0.879, part dbeta 0.548, total 0.879 (the one-block shapes, where total == part); chained
dres 0.157, part 0.492, total 0.064; table slope 0.666; wrapper h 0.453, dres 0.226, dgamma / dbeta
0.192. No group is below 0.01. The fp32 groups sit where the CPU emulation of the same case sits (bwd
0.3989 / 0.8786 / 0.5481 to four digits): the emulation has the kernel's grouping. Every bit-identity
held, the keep bits equal the numpy definition on all 240 (n, p, seed) combinations, and no kernel or
wrapper defect was found. The fused layer against the fp32 restatement on the recorded masks: output
4.4e-4, parameter gradients 1.0e-7 .. 6.2e-3 relative L2 (bars 1e-2 / 3e-2).
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import postln_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
EPS = R.EPS
GUARD = 64     # NaN elements past the end of a flat output
GROWS = 4      # NaN rows past row M - 1 of a row-kernel output
WORST = {}     # group -> largest err / bound of this run (printed per check; pytest -s shows them)


def _lib():
    from triad_amd import _lib
    return _lib


def _at(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _nan(n, dt):
    return torch.full((n,), NAN, dtype=dt, device=dev)


def _rows(M, D, dt):
    return torch.full((M + GROWS, D), NAN, dtype=dt, device=dev)


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
    print("\npost-LN kernels, largest err/bound per group:",
          ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))


@functools.lru_cache(maxsize=4)
def _case(M, D):
    """Seeded operands on the CPU and, each in its own buffer, on the device."""
    c = R.postln_case(M, D)
    return c, {k: v.to(dev) for k, v in c.items()}


# ---- triad_dropout_keep ---------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 12345, 2 ** 31, 2 ** 32 - 1])
def test_keep_bits_equal_the_numpy_definition(seed):
    """n around the 256-thread block and up to 2^20, every p of the CPU file's threshold list: bit for
    bit; nothing kept at thr = 65536, everything at thr = 0; 0xFF guard bytes intact. (The high word
    of the pair index needs n > 2^33 and is not reachable here.)"""
    L = _lib()
    for n in (1, 2, 7, 255, 256, 257, 65537, 1 << 20):
        for p in R.P_LIST:
            out = torch.full((n + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
            L.call("triad_dropout_keep", n, p, seed, _at(out), L.stream_ptr())
            got = out.cpu().numpy()
            what = f"n {n} p {p} seed {seed}"
            assert (got[n:] == 0xFF).all(), what + ": wrote past out[n]"
            assert np.array_equal(got[:n], R.keep_bits(n, p, seed).astype(np.uint8)), what
            if R.drop_thr(p) == 65536:
                assert not got[:n].any(), what
            if R.drop_thr(p) == 0:
                assert got[:n].all(), what


# ---- triad_dropaddln_fwd --------------------------------------------------------------------------------

def _fwd(d, M, D, p, seed):
    L = _lib()
    h, hb = _rows(M, D, F32), _rows(M, D, BF)
    mean, rstd = _nan(M + GROWS, F32), _nan(M + GROWS, F32)
    L.call("triad_dropaddln_fwd", _at(d["res"]), _at(d["y"]), _at(d["w"]), _at(d["b"]), EPS, M, D, p, seed, _at(h),
           _at(hb), _at(mean), _at(rstd), L.stream_ptr())
    for t in (h, hb, mean, rstd):
        assert _all_nan(t[M:]), f"dropaddln_fwd M {M} D {D}: wrote past row M - 1"
    return h[:M], hb[:M], mean[:M], rstd[:M]


@pytest.mark.parametrize("D", R.FWD_DS)
def test_dropaddln_forward(D):
    """Every D instance x M = 1, 3, 4, 5, 9, 130 (one wave, a partial block, a full block, one past it)
    x p = 0, 0.1, 0.5 with a seed >= 2^31: mean, rstd, h, hb per element against fp64; hb == bf16(h);
    rows >= M stay NaN. At D = 768, M >= 4: the mean-100 row (z exact in fp32, asserted), the tiny row,
    the constant row (mean exact, h == b, rstd = 1 / sqrt(eps) to 6 u)."""
    eps = R.f32(EPS)
    for M in R.FWD_MS:
        c, d = _case(M, D)
        for p in R.FWD_PS:
            what = f"M {M} D {D} p {p}"
            h, hb, mean, rstd = _fwd(d, M, D, p, R.SEED_HI)
            want = R.dropaddln_fwd_ref(c["res"], c["y"], c["w"], c["b"], eps, p, R.SEED_HI)
            _check(mean, *want["mean"], "fwd.mean", what)
            _check(rstd, *want["rstd"], "fwd.rstd", what)
            _check(h, *want["h"], "fwd.h", what)
            _check(hb, *want["hb"], "fwd.hb", what)
            assert torch.equal(hb, h.to(BF)), what + ": hb != bf16(h)"
            if D == 768 and M >= 4:
                assert bool(want["exact"][R.SPECIAL_ROWS["mean100"]]), "the mean-100 row's z must be exact in fp32"
                k = R.SPECIAL_ROWS["const"]
                assert float(mean[k]) == R.CONST, what + ": constant row's mean"
                assert torch.equal(h[k].cpu(), c["b"]), what + ": constant row h != b"
                assert abs(float(rstd[k]) - eps ** -0.5) <= 6 * R.U * eps ** -0.5, what + ": constant row's rstd"


# ---- triad_dropaddln_bwd --------------------------------------------------------------------------------

def _bwd(d, M, D, p, seed, mean, rstd, use_dh=True, use_dhb=True):
    """One call with NaN-filled dres, dy, part (+ guards): (dres, dy, part [blocks][2][D]) on the device."""
    L = _lib()
    G = L.call("triad_dropaddln_bwd_blocks", M)
    assert G == R.bwd_blocks(M)
    dres, dy = _rows(M, D, F32), _rows(M, D, BF)
    part = _nan(G * 2 * D + GUARD, F32)
    L.call("triad_dropaddln_bwd", _at(d["dh"]) if use_dh else None, _at(d["dhb"]) if use_dhb else None, _at(d["res"]),
           _at(d["y"]), _at(mean), _at(rstd), _at(d["w"]), M, D, p, seed, _at(dres), _at(dy), _at(part), L.stream_ptr())
    what = f"dropaddln_bwd M {M} D {D}"
    assert _all_nan(dres[M:]) and _all_nan(dy[M:]), what + ": wrote past row M - 1"
    assert _all_nan(part[G * 2 * D:]), what + ": wrote past part[blocks][2][D]"
    assert bool(torch.isfinite(part[:G * 2 * D]).all()), what + ": part elements left unwritten"
    return dres[:M], dy[:M], part[:G * 2 * D].view(G, 2, D)


@functools.lru_cache(maxsize=4)
def _ref_stats(M, D, p, seed):
    """The fp64 statistics rounded to fp32 (CPU, device): the backward's operands, independent of the
    forward kernel."""
    c, _ = _case(M, D)
    want = R.dropaddln_fwd_ref(c["res"], c["y"], c["w"], c["b"], R.f32(EPS), p, seed)
    m, r = want["mean"][0].to(F32), want["rstd"][0].to(F32)
    return m, r, m.to(dev), r.to(dev)


def _check_bwd(c, got, want, p, seed, what):
    dres, dy, part = got
    _check(dres, *want["dres"], "bwd.dres", what)
    ref, bound = want["part"]
    _check(part[:, 0], ref[:, 0], bound[:, 0], "bwd.part.dgamma", what)
    _check(part[:, 1], ref[:, 1], bound[:, 1], "bwd.part.dbeta", what)
    _check(part.double().sum(0), *want["total"], "bwd.total", what)
    assert bool(torch.isfinite(dy).all()), what + ": dy not finite"
    keep = R.keep_mask(c["res"].shape, p, seed)
    assert torch.equal(dy.cpu(), R.dy_of(dres.cpu(), keep, R.drop_scale(p))), what + ": dy != bf16(bf16(dres) keep scale)"


def _bwd_case(M, D, p, use_dh=True, use_dhb=True):
    c, d = _case(M, D)
    m, r, md, rd = _ref_stats(M, D, p, R.SEED_HI)
    got = _bwd(d, M, D, p, R.SEED_HI, md, rd, use_dh, use_dhb)
    want = R.dropaddln_bwd_ref(c["dh"] if use_dh else None, c["dhb"] if use_dhb else None, c["res"], c["y"], m, r,
                               c["w"], p, R.SEED_HI)
    _check_bwd(c, got, want, p, R.SEED_HI, f"M {M} D {D} p {p} dh {use_dh} dhb {use_dhb}")
    return got


@pytest.mark.parametrize("D", R.FWD_DS)
def test_dropaddln_backward(D):
    """The forward's D x M grid at p = 0 and 0.1, mean / rstd from the fp64 reference rounded to fp32:
    dres, every one of the blocks x 2 x D partials against its own block's rows, the fp64-summed
    totals, and the dy identity; part is written for exactly triad_dropaddln_bwd_blocks(M) blocks."""
    for M in R.FWD_MS:
        for p in (0.0, 0.1):
            _bwd_case(M, D, p)


@pytest.mark.parametrize("M,D", R.BWD_BIG)
def test_dropaddln_backward_past_one_trip(M, D):
    """M = 4101 and 8197 at D = 256, M = 4101 at D = 1024: rows from 4096 on are a block's second (and
    third) trip of the grid-stride loop, the last trip partial (2 blocks of 1024 own a row in it)."""
    assert R.bwd_trips(M) == (3 if M == 8197 else 2)
    _bwd_case(M, D, 0.1)


@pytest.mark.parametrize("M,D", [(5, 256), (130, 768), (4101, 256)])
def test_dropaddln_backward_optional_gradients(M, D):
    """dh only, dhb only, both, and both NULL (dres, dy and the partials exactly zero)."""
    c, d = _case(M, D)
    for use_dh, use_dhb in ((True, False), (False, True), (True, True)):
        _bwd_case(M, D, 0.1, use_dh, use_dhb)
    _, _, md, rd = _ref_stats(M, D, 0.1, R.SEED_HI)
    dres, dy, part = _bwd(d, M, D, 0.1, R.SEED_HI, md, rd, False, False)
    assert not bool(dres.any()) and not bool(dy.float().any()) and not bool(part.any())


def test_dropaddln_bwd_blocks():
    L = _lib()
    got = [L.call("triad_dropaddln_bwd_blocks", M) for M in (1, 4, 5, 4095, 4096, 4097, 1 << 20)]
    assert got == [1, 1, 2, 1024, 1024, 1024, 1024]


@pytest.mark.parametrize("D", R.FWD_DS)
def test_dropaddln_chained(D):
    """Forward, then backward on the forward's own mean / rstd, with and without dropout, against the
    fp64 chain that keeps the fp64 statistics: the backward bounds widened by the forward's dm and
    rel_rstd (e_xh + rstd dm + rel_r |xh|, dres + rel_r |ref|)."""
    M = 130
    c, d = _case(M, D)
    for p in (0.0, 0.1):
        h, hb, mean, rstd = _fwd(d, M, D, p, R.SEED_HI)
        fw = R.dropaddln_fwd_ref(c["res"], c["y"], c["w"], c["b"], R.f32(EPS), p, R.SEED_HI)
        got = _bwd(d, M, D, p, R.SEED_HI, mean.contiguous(), rstd.contiguous())
        want = R.dropaddln_bwd_ref(c["dh"], c["dhb"], c["res"], c["y"], fw["mean"][0], fw["rstd"][0], c["w"], p,
                                   R.SEED_HI, dm=fw["dm"], rel_r=fw["rel_r"])
        dres, dy, part = got
        what = f"chained M {M} D {D} p {p}"
        _check(dres, *want["dres"], "chained.dres", what)
        _check(part, *want["part"], "chained.part", what)
        _check(part.double().sum(0), *want["total"], "chained.total", what)
        keep = R.keep_mask(c["res"].shape, p, R.SEED_HI)
        assert torch.equal(dy.cpu(), R.dy_of(dres.cpu(), keep, R.drop_scale(p))), what


# ---- GELU table and passes ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _table():
    """triad_gelu_table into a 0xFF-filled buffer (NaN in both halves) with a guard: exactly
    triad_gelu_table_bytes() bytes are written."""
    L = _lib()
    nbytes = int(L.call("triad_gelu_table_bytes"))
    assert nbytes == R.GL_BYTES
    buf = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    L.call("triad_gelu_table", _at(buf), L.stream_ptr())
    torch.cuda.synchronize()
    assert bool((buf[nbytes:] == 0xFF).all()), "gelu_table wrote past its bytes"
    return buf


def test_gelu_table_entries():
    """Each entry's slope (fp32) and value (bf16) inside the fp64 bound of the argument it stands for
    (the host restatement of gl_index, inverted)."""
    buf = _table()
    slope = buf[:R.GL_N * 4].view(F32)
    val = buf[R.GL_N * 4:R.GL_BYTES].view(BF)
    x = torch.from_numpy(R.gl_pattern(np.arange(R.GL_N)).astype(np.int32)).to(torch.int16).view(BF)
    (g, gb), (s, sb) = R.gelu_table_ref(x)
    _check(val, g, gb, "gelu.table.value", "all entries")
    _check(slope, s, sb, "gelu.table.slope", "all entries")


def _gelu_fwd(u, p, seed, table):
    L = _lib()
    n = u.numel()
    v = _nan(n + GUARD, BF)
    L.call("triad_geludrop_fwd", _at(u), n, p, seed, _at(table), _at(v), L.stream_ptr())
    assert _all_nan(v[n:]), f"geludrop_fwd n {n}: wrote past v[n]"
    return v[:n]


def _gelu_bwd(u, dv, p, seed, table):
    L = _lib()
    n = u.numel()
    du = _nan(n + GUARD, BF)
    L.call("triad_geludrop_bwd", _at(u), _at(dv), n, p, seed, _at(table), _at(du), L.stream_ptr())
    assert _all_nan(du[n:]), f"geludrop_bwd n {n}: wrote past du[n]"
    return du[:n]


def _same_bits(a, b):
    """Bit-identical, NaN patterns equal as NaN."""
    a, b = a.cpu(), b.cpu()
    return bool(((a.view(torch.int16) == b.view(torch.int16)) | (torch.isnan(a) & torch.isnan(b))).all())


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gelu_passes_every_bf16_pattern(p):
    """All 65 536 patterns at even and odd positions, forward and backward, table and table == NULL:
    identical bits; both inside the fp64 bound on every finite pattern whose result bf16 can hold (x
    scale of the largest 47 overflows at p = 0.1); v == bf16(g keep scale) of the p = 0 output; keep
    bits from the numpy definition."""
    seed = 1234
    u = R.all_patterns()
    dv = R.gelu_case(u.numel(), 1)[1]
    ud, dvd = u.to(dev), dv.to(dev)
    keep, scale = R.keep_mask(u.shape, p, seed), R.drop_scale(p)
    fin = torch.isfinite(u.float())
    v_t, v_f = _gelu_fwd(ud, p, seed, _table()), _gelu_fwd(ud, p, seed, None)
    du_t, du_f = _gelu_bwd(ud, dvd, p, seed, _table()), _gelu_bwd(ud, dvd, p, seed, None)
    assert _same_bits(v_t, v_f), "forward: table and formula differ"
    assert _same_bits(du_t, du_f), "backward: table and formula differ"
    vref, vbound = R.geludrop_fwd_ref(u, keep, scale)
    ok = fin & R.in_range(vref, vbound)
    assert int((fin & ~ok).sum()) <= 64
    _check(v_f[ok.to(dev)], vref[ok], vbound[ok], "gelu.fwd", f"p {p}")
    dref, dbound = R.geludrop_bwd_ref(u, dv, keep, scale)
    _check(du_f[fin.to(dev)], dref[fin], dbound[fin], "gelu.bwd", f"p {p}")
    g0 = _gelu_fwd(ud, 0.0, 0, None).cpu()
    want = torch.where(keep, (g0.float() * torch.tensor(scale, dtype=F32)).to(BF), torch.zeros_like(g0))
    assert _same_bits(v_f.cpu()[fin], want[fin]), "v != bf16(g keep scale) of the p = 0 output"


def _aten_on_mask(u, dv, keep, scale):
    """aten gelu / gelu_backward on the device with the given mask, as tests/test_postln_gpu.py forms them."""
    s = torch.tensor(scale, dtype=F32, device=dev)
    v = torch.where(keep, (F.gelu(u).float() * s).to(BF), torch.zeros_like(u))
    dg = torch.where(keep, (dv.float() * s).to(BF), torch.zeros_like(dv))
    return v, torch.ops.aten.gelu_backward(dg, u)


@pytest.mark.parametrize("table", [True, False])
def test_gelu_drop_past_one_sweep(table):
    """n = 2 CUs 4096 + 4096 + 8: a second sweep of the persistent grid with one full block and a last
    lone thread, and n = 8; the DROP instances (p = 0.1), bit-identical to aten on the numpy mask."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tb = _table() if table else None
    for n in (2 * cus * 4096 + 4096 + 8, 8):
        u, dv = R.gelu_case(n, 2)
        ud, dvd = u.to(dev), dv.to(dev)
        keep = R.keep_mask(u.shape, 0.1, R.SEED_HI).to(dev)
        v, du = _gelu_fwd(ud, 0.1, R.SEED_HI, tb), _gelu_bwd(ud, dvd, 0.1, R.SEED_HI, tb)
        av, adu = _aten_on_mask(ud, dvd, keep, R.drop_scale(0.1))
        assert torch.equal(v, av), f"n {n}: forward differs from aten"
        assert torch.equal(du, adu), f"n {n}: backward differs from aten"


# ---- repeats ----------------------------------------------------------------------------------------------

def test_repeats_are_bit_identical():
    M, D, p = 4101, 256, 0.1
    _, d = _case(M, D)
    _, _, md, rd = _ref_stats(M, D, p, R.SEED_HI)
    f = [_fwd(d, M, D, p, R.SEED_HI) for _ in range(3)]
    b = [_bwd(d, M, D, p, R.SEED_HI, md, rd) for _ in range(3)]
    u, dv = R.gelu_case(1 << 17, 3)
    ud, dvd = u.to(dev), dv.to(dev)
    gf = [(_gelu_fwd(ud, p, 5, _table()),) for _ in range(3)]
    gb = [(_gelu_bwd(ud, dvd, p, 5, _table()),) for _ in range(3)]
    for runs in (f, b, gf, gb):
        for r in runs[1:]:
            assert all(torch.equal(x, y) for x, y in zip(r, runs[0])), "a repeat changed the result"


# ---- wrappers (triad_amd/postln.py) -----------------------------------------------------------------------

def _count_calls(monkeypatch, seen=None, record=None):
    """Count postln.py's entry-point calls by name (size queries and the table build left out)."""
    from triad_amd import postln
    seen = {} if seen is None else seen
    real = postln.call

    def counting(name, *a, **k):
        if name not in ("triad_dropaddln_bwd_blocks", "triad_gelu_table_bytes", "triad_gelu_table"):
            seen[name] = seen.get(name, 0) + 1
            if record is not None:
                record.append((name, a))
        return real(name, *a, **k)
    monkeypatch.setattr(postln, "call", counting)
    return seen


def _offset_view(t, elems):
    """t's values as a contiguous view `elems` elements into a fresh buffer."""
    buf = torch.empty(t.numel() + elems, dtype=t.dtype, device=t.device)
    v = buf[elems:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == elems * t.element_size()
    return v


def _run_drop_add_ln(d, norm, p, seed, res, y):
    from triad_amd import postln
    norm.zero_grad(set_to_none=True)
    rf, yf = res.detach().requires_grad_(True), y.detach().requires_grad_(True)
    h, hb = postln.drop_add_ln(rf, yf, norm, p, seed)
    ((h * d["dh"]).sum() + (hb.float() * d["dhb"].float()).sum()).backward()
    return h.detach(), hb.detach(), rf.grad, yf.grad, norm.weight.grad.clone(), norm.bias.grad.clone()


@pytest.mark.parametrize("M,D", [(4101, 256), (5, 768)])
def test_drop_add_ln_wrapper_vs_fp64(monkeypatch, M, D):
    """drop_add_ln forward and backward per element against the fp64 chain (bounds of the chained
    test; dgamma / dbeta through triad_sum_slabs: + its depth in u over the summed |partials|); one
    forward, one backward and one slab-sum HIP call; a y at a 2-byte and a res at a 4-byte offset give
    the same bits as aligned copies."""
    p, seed = 0.1, R.SEED_HI
    seen = _count_calls(monkeypatch)
    c, d = _case(M, D)
    norm = torch.nn.LayerNorm(D, eps=EPS).to(dev)
    with torch.no_grad():
        norm.weight.copy_(d["w"])
        norm.bias.copy_(d["b"])
    got = _run_drop_add_ln(d, norm, p, seed, d["res"], d["y"])
    assert seen == {"triad_dropaddln_fwd": 1, "triad_dropaddln_bwd": 1, "triad_sum_slabs": 1}
    h, hb, dres, dy, dw, db = got
    fw = R.dropaddln_fwd_ref(c["res"], c["y"], c["w"], c["b"], R.f32(EPS), p, seed)
    want = R.dropaddln_bwd_ref(c["dh"], c["dhb"], c["res"], c["y"], fw["mean"][0], fw["rstd"][0], c["w"], p, seed,
                               dm=fw["dm"], rel_r=fw["rel_r"])
    what = f"drop_add_ln M {M} D {D}"
    _check(h, *fw["h"], "wrapper.h", what)
    _check(hb, *fw["hb"], "wrapper.hb", what)
    _check(dres, *want["dres"], "wrapper.dres", what)
    keep = R.keep_mask(c["res"].shape, p, seed)
    assert torch.equal(dy.cpu(), R.dy_of(dres.cpu(), keep, R.drop_scale(p))), what
    tref, tbound = want["total"]
    pref, pbound = want["part"]
    tbound = tbound + R.sum_slabs_depth(R.bwd_blocks(M)) * R.U * (pref.abs() + pbound).sum(0)
    _check(torch.stack([dw, db]), tref, tbound, "wrapper.dgamma_dbeta", what)
    shifted = _run_drop_add_ln(d, norm, p, seed, _offset_view(d["res"], 1), _offset_view(d["y"], 1))
    assert all(torch.equal(a, b) for a, b in zip(shifted, got)), what + ": offset views changed the result"


@pytest.mark.parametrize("n", [2 * 4101 * 256, 5 * 8])
def test_gelu_drop_wrapper_vs_fp64(monkeypatch, n):
    """gelu_drop forward and backward per element against the fp64 reference on the numpy mask; one
    HIP call each way; u and dv at a 2-byte offset give the same bits as aligned copies."""
    from triad_amd import postln
    p, seed = 0.1, R.SEED_HI
    seen = _count_calls(monkeypatch)
    u, dv = R.gelu_case(n, 4)
    ud, dvd = u.to(dev), dv.to(dev)

    def run(uu, dd):
        uf = uu.detach().requires_grad_(True)
        v = postln.gelu_drop(uf, p, seed)
        v.backward(dd)
        return v.detach(), uf.grad

    v, du = run(ud, dvd)
    assert seen == {"triad_geludrop_fwd": 1, "triad_geludrop_bwd": 1}
    keep, scale = R.keep_mask(u.shape, p, seed), R.drop_scale(p)
    _check(v, *R.geludrop_fwd_ref(u, keep, scale), "wrapper.gelu.v", f"n {n}")
    _check(du, *R.geludrop_bwd_ref(u, dv, keep, scale), "wrapper.gelu.du", f"n {n}")
    v2, du2 = run(_offset_view(ud, 1), _offset_view(dvd, 1))
    assert torch.equal(v2, v) and torch.equal(du2, du), f"n {n}: offset views changed the result"


# ---- seeds of one fused HuBERT layer ------------------------------------------------------------------------

P_HIDDEN, P_ACT = 0.1, 0.2
SEED_ARGS = {"triad_dropaddln_fwd": (7, 8), "triad_dropaddln_bwd": (9, 10), "triad_geludrop_fwd": (2, 3),
             "triad_geludrop_bwd": (3, 4)}     # positions of (p, seed)


def _layer():
    from triad_amd import model as Mdl
    torch.manual_seed(0)
    over = dict(hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=512,
                hidden_dropout=P_HIDDEN, activation_dropout=P_ACT, attention_dropout=0.0, layerdrop=0.0,
                feat_proj_dropout=0.0, mask_time_prob=0.0)
    hub = Mdl.hubert_execution_tweaks(Mdl._hf_model("HubertModel", "none/none", over)).to(dev)
    return hub.encoder.layers[0]


def _layer_pass(layer, res, gy, seeds, record):
    from triad_amd import postln
    del record[:]
    layer.zero_grad(set_to_none=True)
    r = res.detach().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        h2, _ = postln.fused_layer(layer, r, r.detach().to(BF), seeds)
    if r.requires_grad and torch.is_grad_enabled():
        (h2 * gy).sum().backward()
    calls = [(n, float(a[SEED_ARGS[n][0]]), int(a[SEED_ARGS[n][1]])) for n, a in record if n in SEED_ARGS]
    grads = {n: q.grad.float().cpu().clone() for n, q in layer.named_parameters() if q.grad is not None}
    return h2.detach().float().cpu(), grads, calls


def _layer_restatement(layer, res, gy, masks):
    """The layer in plain fp32 torch on the CPU with the given (mask, scale) per dropout."""
    ref = copy.deepcopy(layer).cpu().float()
    at, ff = ref.attention, ref.feed_forward
    B, N, E = res.shape
    H = at.num_heads

    def heads(t):
        return t.view(B, N, H, E // H).transpose(1, 2)
    q, k, v = (heads(F.linear(res, m.weight, m.bias)) for m in (at.q_proj, at.k_proj, at.v_proj))
    a = torch.softmax(q @ k.transpose(-1, -2) * at.scaling, -1) @ v
    a = F.linear(a.transpose(1, 2).reshape(B, N, E), at.out_proj.weight, at.out_proj.bias)
    (m1, s1), (m2, s2), (m3, s3) = masks
    ln1, ln2 = ref.layer_norm, ref.final_layer_norm
    h1 = F.layer_norm(res + a * m1 * s1, (E,), ln1.weight, ln1.bias, ln1.eps)
    g = F.gelu(F.linear(h1, ff.intermediate_dense.weight, ff.intermediate_dense.bias)) * m2 * s2
    f = F.linear(g, ff.output_dense.weight, ff.output_dense.bias)
    h2 = F.layer_norm(h1 + f * m3 * s3, (E,), ln2.weight, ln2.bias, ln2.eps)
    (h2 * gy).sum().backward()
    return h2.detach(), {n: q.grad.clone() for n, q in ref.named_parameters() if q.grad is not None}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


def test_fused_layer_dropout_seeds(monkeypatch):
    """One fused HuBERT layer (hidden 256, 4 heads of 64, intermediate 512, 2 x 24 tokens), dropout on,
    training mode, twice: the three post-LN seeds of a pass are pairwise distinct and differ between
    the passes, forward and backward of a pass use the same seed, every p is the module's; in eval
    mode every p is 0; and the output and parameter gradients match a plain fp32 torch restatement
    that applies the numpy masks of the recorded seeds (1e-2 / 3e-2 relative L2, the bars of the fused
    encoder test in tests/test_postln_gpu.py)."""
    from triad_amd import postln
    record = []
    _count_calls(monkeypatch, record=record)
    layer = _layer().train()
    B, N, E, I = 2, 24, 256, 512
    g = torch.Generator().manual_seed(11)
    res = torch.randn(B, N, E, generator=g)
    gy = torch.randn(B, N, E, generator=g)
    seeds = postln._Seeds()
    passes = [_layer_pass(layer, res.to(dev), gy.to(dev), seeds, record) for _ in range(2)]
    want_p = [P_HIDDEN, P_ACT, P_HIDDEN]
    all_seeds = []
    for out, grads, calls in passes:
        assert [c[0] for c in calls] == ["triad_dropaddln_fwd", "triad_geludrop_fwd", "triad_dropaddln_fwd",
                                         "triad_dropaddln_bwd", "triad_geludrop_bwd", "triad_dropaddln_bwd"]
        fwd, bwd = calls[:3], calls[3:][::-1]
        assert [c[2] for c in fwd] == [c[2] for c in bwd], "backward seeds differ from the forward's"
        for (_, p, _), (_, pb, _), wp in zip(fwd, bwd, want_p):
            assert p == pb == wp
        assert len({c[2] for c in fwd}) == 3, "two dropouts of one pass share a seed"
        all_seeds += [c[2] for c in fwd]
    assert len(set(all_seeds)) == 6, "the second pass reused a seed"
    # the last pass against the restatement on its masks
    out, grads, calls = passes[1]
    shapes = [(B, N, E), (B, N, I), (B, N, E)]
    masks = [(R.keep_mask(s, p, sd).float(), R.drop_scale(p)) for (_, p, sd), s in zip(calls[:3], shapes)]
    ref_out, ref_grads = _layer_restatement(layer, res, gy, masks)
    r = _rel(out, ref_out)
    print(f"fused layer output rel L2 {r:.2e}")
    assert r < 1e-2, r
    assert set(grads) == set(ref_grads)
    for n in ref_grads:
        if n.endswith("k_proj.bias"):   # exactly 0 in exact arithmetic (softmax shift invariance): noise
            continue
        r = _rel(grads[n], ref_grads[n])
        print(f"fused layer grad {n} rel L2 {r:.2e}")
        assert r < 3e-2, (n, r)
    layer.eval()
    with torch.no_grad():
        _, _, calls = _layer_pass(layer, res.to(dev), gy.to(dev), seeds, record)
    assert [c[0] for c in calls] == ["triad_dropaddln_fwd", "triad_geludrop_fwd", "triad_dropaddln_fwd"]
    assert all(c[1] == 0.0 for c in calls), "eval mode must not drop"
