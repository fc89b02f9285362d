"""Conformance of the attention kernels of csrc/attention.hip -- triad_attn_fwd / triad_attn_bwd, their
_dropout forms (every NKT = 1 .. 10 x DROP instance of the forward, dq and dk / dv kernels) and
triad_attn_dropmask -- against fp64 references of the same bf16 operands, through the C ABI
(`triad_amd._lib.call`) at B = 2, H = 3, and of the attention.py wrappers over them.

Operands come from a seeded CPU generator (tests/attention_ref.py, which also holds the input
families, the references, the bounds and their derivation; tests/test_attention_checks_cpu.py shows
that every bound passes an fp32 / bf16 emulation of its kernel and fails ten planted errors). Every
tensor sits in its own NaN-filled buffer with its own row stride sN = H * 64 + 8 j, a gap between the
samples (sB), and NaN guards before and after; out, dq, dk, dv, lse and delta must leave every gap
and guard NaN and be finite inside before they are compared; no element is left out of a comparison.
The backward kernels are tested on their own (o = bf16(reference out), lse = fp32(reference lse), so a
forward error can neither mask nor fake a backward one) and chained to the forward (bounds widened by
the forward's bounds as input errors). Under dropout the reference uses the mask the kernel drew
(seed >= 2^31), which test_dropmask_* pin to triad_dropout_keep's bit of element (bh N + q) N + key.
The `selector` family has answers known exactly and is compared bit for bit.

Bounds (per element, u = 2^-24, r = 2^-8; derivation in tests/attention_ref.py, nothing fitted):

    out    pre + r (|out| + pre), pre = sum_k P w |v| (eps + r) + 2 (32 nkt + 2) u sum_k P w |v|
                                       + |out| (sum_k P eps + (16 nkt + 4) u) + FLUSH sum_k |v|
    lse    2 u |m scale| + sum_k P eps + (16 nkt + 1) u + LOG |log l| + u |lse|
    delta  (64 + 1) u sum_d |dO o|
    dq/dk  pre + r (|ref| + pre), pre = scale (sum e_dS |X| + 2 (32 nkt + 2) u sum |dS| |X|) + u |ref|
    dv     pre + r (|ref| + pre), pre = sum_q (p w (eta + u + r) + FLUSH w) |dO| + 2 (32 nkt + 2) u sum_q p w |dO|

Not covered: element indices past 2^32 in the mask hash (that needs a 0.5 GB mask; the largest
index here is 6 * 320 * 320).

Largest err / bound per group on MI355X (112 cases, 1 449 bound comparisons, 7 s in all, the slowest
case 0.8 s; also in DESIGN.md section 2; `pytest -s` prints every figure). Without / with dropout:
out 0.708 / 0.844, lse 0.015 / 0.015, delta 0.029 / 0.023, dq 0.829 / 0.849, dk 0.837 / 0.884, dv
0.850 / 0.900. Chained: delta 0.210, dq 0.703, dk 0.689, dv 0.849. Through attention_bnhd: out 0.550,
dq 0.169, dk 0.161, dv 0.639. The bf16 outputs sit where the CPU emulation of the same rounding
points does (0.5 - 0.87 there): the bf16 roundings of P / dS and of the store fill their r terms.
Every exact check (selector, mask,
repeats, guards) held on the first run and no bound was missed, so neither a kernel nor a derivation
was changed after the run. Found while writing the wrapper checks, on the host side only:
`_as_bnhd` used `.contiguous()`, which returns a contiguous view at an 8-byte storage offset as it
is; such views are now cloned (tests/test_attention_checks_cpu.py::test_wrapper_gates).
"""
import ctypes
import functools
import math

import pytest
import torch

from tests import attention_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
B, H, HD = 2, 3, 64
SCALE = R.f32(R.SCALE)
ALL_N = (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 256, 257, 288, 289, 319, 320)
FAMILY_N = (5, 33, 96, 199, 261, 320)
DROP_N = (32, 33, 65, 97, 129, 161, 193, 225, 257, 289, 320)   # every NKT, one past each tile boundary
OTHERS = tuple(f for f in R.FAMILIES if f != "gauss")
SENTINEL = 0x5A5A5A5A
J = dict(k=1, v=2, q=3, o=4, do=5, out=6, dq=7, dk=8, dv=9)   # sN = H * 64 + 8 j: no two alike
WORST = {}


def _lib():
    from triad_amd import _lib
    return _lib


def _at(t, elems=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + t.element_size() * elems)


class Rows:
    """A (B, N, H, 64) bf16 tensor inside its own NaN-filled device buffer: row stride sN = H * 64 +
    8 j, sample stride sB = N * sN + 8 (j + 1) (a gap), 8 (j % 3 + 1) guard elements in front and 64
    behind; all 16-byte aligned."""

    def __init__(self, N, name, src=None):
        j = J[name]
        self.name = name
        self.sN = H * HD + 8 * j
        self.sB = N * self.sN + 8 * (j + 1)
        self.off = 8 * (j % 3 + 1)
        self.flat = torch.full((self.off + B * self.sB + 64,), NAN, dtype=BF, device=dev)
        self.shape, self.strides = (B, N, H, HD), (self.sB, self.sN, HD, 1)
        self.view = self.flat.as_strided(self.shape, self.strides, self.off)
        if src is not None:
            self.view.copy_(src.to(dev))
        assert self.view.data_ptr() % 16 == 0 and self.sB % 8 == 0 and self.sN % 8 == 0

    @property
    def args(self):
        return _at(self.flat, self.off), self.sB, self.sN

    def result(self, what):
        """The written tensor (contiguous, on the host) after checking that everything outside it is
        still NaN and everything inside is finite."""
        inside = torch.zeros(self.flat.shape, dtype=torch.bool, device=dev)
        inside.as_strided(self.shape, self.strides, self.off).fill_(True)
        assert bool(torch.isnan(self.flat[~inside]).all()), f"{what}: {self.name} wrote into a gap or a guard"
        assert bool(torch.isfinite(self.view).all()), f"{what}: {self.name} has unwritten or non-finite elements"
        return self.view.cpu().contiguous()


class Stat:
    """lse / delta: (B, H, N) fp32 with 4 NaN guard elements in front and 16 behind."""

    def __init__(self, N, name, src=None):
        self.name, self.n = name, B * H * N
        self.flat = torch.full((4 + self.n + 16,), NAN, dtype=F32, device=dev)
        self.view = self.flat[4:4 + self.n].view(B, H, N)
        if src is not None:
            self.view.copy_(src.to(dev))

    @property
    def ptr(self):
        return _at(self.flat, 4)

    def result(self, what):
        assert bool(torch.isnan(self.flat[:4]).all()) and bool(torch.isnan(self.flat[4 + self.n:]).all()), \
            f"{what}: {self.name} wrote past its ends"
        assert bool(torch.isfinite(self.view).all()), f"{what}: {self.name} has unwritten or non-finite elements"
        return self.view.cpu()


def _check(got, ref, bound, group, what):
    r = R.ratio(got, ref, bound)
    WORST[group] = max(WORST.get(group, 0.0), r) if r == r else NAN
    print(f"{group} {what}: err/bound {r:.4f}")
    assert r <= 1.0, f"{group} {what}: err/bound {r}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nattention kernels, largest err/bound per group:",
          ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))


# ---- the calls ----------------------------------------------------------------------------------

def run_fwd(c, N, what, mask=None, p=0.0):
    """-> (out (B, N, H, 64) bf16, lse (B, H, N) fp32) on the host, guards checked."""
    L = _lib()
    q, k, v = (Rows(N, n, c[n]) for n in ("q", "k", "v"))
    out, lse = Rows(N, "out"), Stat(N, "lse")
    if mask is None:
        L.call("triad_attn_fwd", *q.args, *k.args, *v.args, B, H, N, HD, SCALE, *out.args, lse.ptr, L.stream_ptr())
    else:
        L.call("triad_attn_fwd_dropout", *q.args, *k.args, *v.args, B, H, N, HD, SCALE, _at(mask.wq), p, *out.args,
               lse.ptr, L.stream_ptr())
    return out.result(what), lse.result(what)


def run_bwd(c, N, o, lse, what, mask=None, p=0.0):
    """o (B, N, H, 64) bf16, lse (B, H, N) fp32 (host) -> dict of dq, dk, dv, delta on the host."""
    L = _lib()
    q, k, v, do = (Rows(N, n, c[n]) for n in ("q", "k", "v", "do"))
    ob, ls = Rows(N, "o", o), Stat(N, "lse", lse)
    dq, dk, dv, delta = Rows(N, "dq"), Rows(N, "dk"), Rows(N, "dv"), Stat(N, "delta")
    if mask is None:
        L.call("triad_attn_bwd", *q.args, *k.args, *v.args, *ob.args, *do.args, ls.ptr, B, H, N, HD, SCALE, *dq.args,
               *dk.args, *dv.args, delta.ptr, L.stream_ptr())
    else:
        L.call("triad_attn_bwd_dropout", *q.args, *k.args, *v.args, *ob.args, *do.args, ls.ptr, B, H, N, HD, SCALE,
               _at(mask.wq), _at(mask.wk), p, *dq.args, *dk.args, *dv.args, delta.ptr, L.stream_ptr())
    return {"dq": dq.result(what), "dk": dk.result(what), "dv": dv.result(what), "delta": delta.result(what)}


class Mask:
    """triad_attn_dropmask at (N, p, seed) into sentinel-filled word buffers with 32 sentinel words
    behind. keep_q / keep_k: the (B, H, N, 32 nkt) bits of the query-major words [b, h, q, key] and
    of the key-major words [b, h, key, q], on the host."""

    def __init__(self, N, p, seed):
        L = _lib()
        self.N, self.nkt = N, R.nkt(N)
        self.words = B * H * N * self.nkt
        self.wq = torch.full((self.words + 32,), SENTINEL, dtype=torch.int32, device=dev)
        self.wk = self.wq.clone()
        L.call("triad_attn_dropmask", B, H, N, p, seed, _at(self.wq), _at(self.wk), L.stream_ptr())
        self.keep_q, self.keep_k = self._unpack(self.wq), self._unpack(self.wk)

    def _unpack(self, w):
        w = w[:self.words].cpu().to(torch.int64).view(B, H, self.N, self.nkt, 1) & 0xFFFFFFFF
        return ((w >> torch.arange(32)) & 1).bool().view(B, H, self.N, self.nkt * 32)

    @property
    def keep(self):
        """(B, H, N, N) [b, h, q, key] from the query-major words."""
        return self.keep_q[..., :self.N]


def pack_words(keep):
    """(B, H, N, M) bool -> (B, H, N, ceil(M / 32)) words as int64, bit j of word t = column 32 t + j."""
    n, m = keep.shape[2], keep.shape[3]
    pad = torch.zeros(B, H, n, R.nkt(m) * 32, dtype=torch.int64)
    pad[..., :m] = keep
    return (pad.view(B, H, n, -1, 32) << torch.arange(32)).sum(-1)


@functools.lru_cache(maxsize=4)
def _problem(family, N):
    """Seeded case with its no-dropout references, computed once per (family, N) and not modified:
    (case, forward reference, o = bf16(ref out), lse = fp32(ref lse), backward reference at o, lse)."""
    c = R.case(family, B, H, N, N)
    fw = R.fwd_ref(c["q"], c["k"], c["v"], SCALE)
    o, lse = fw["out"][0].to(F32).to(BF), fw["lse"][0].to(F32)
    return c, fw, o, lse, R.bwd_ref(c["q"], c["k"], c["v"], o, lse, c["do"], SCALE)


def _fwd_case(family, N, mask=None, p=0.0):
    c = R.case(family, B, H, N, N)
    what = f"{family} N {N} p {p}"
    fw = _problem(family, N)[1] if mask is None else R.fwd_ref(c["q"], c["k"], c["v"], SCALE, mask.keep, p)
    out, lse = run_fwd(c, N, what, mask, p)
    tag = ".drop" if mask is not None else ""
    _check(out, *fw["out"], "fwd.out" + tag, what)
    _check(lse, *fw["lse"], "fwd.lse" + tag, what)
    return fw, out, lse


def _bwd_case(family, N, mask=None, p=0.0):
    c = R.case(family, B, H, N, N)
    what = f"{family} N {N} p {p}"
    if mask is None:
        _, _, o, lse, bw = _problem(family, N)
    else:
        fw = R.fwd_ref(c["q"], c["k"], c["v"], SCALE, mask.keep, p)
        o, lse = fw["out"][0].to(F32).to(BF), fw["lse"][0].to(F32)
        bw = R.bwd_ref(c["q"], c["k"], c["v"], o, lse, c["do"], SCALE, mask.keep, p)
    got = run_bwd(c, N, o, lse, what, mask, p)
    tag = ".drop" if mask is not None else ""
    for name in ("delta", "dq", "dk", "dv"):
        _check(got[name], *bw[name], f"bwd.{name}{tag}", what)


def _chain_case(family, N, mask=None, p=0.0):
    """The forward's own out and lse into the backward, against the backward of the fp64 out and
    lse with the forward's bounds as input errors."""
    c = R.case(family, B, H, N, N)
    what = f"{family} N {N} p {p}"
    keep = None if mask is None else mask.keep
    fw = R.fwd_ref(c["q"], c["k"], c["v"], SCALE, keep, p)
    out, lse = run_fwd(c, N, what, mask, p)
    bw = R.bwd_ref(c["q"], c["k"], c["v"], fw["out"][0], fw["lse"][0], c["do"], SCALE, keep, p,
                   lse_err=fw["lse"][1], o_err=fw["out"][1])
    got = run_bwd(c, N, out, lse, what, mask, p)
    for name in ("delta", "dq", "dk", "dv"):
        _check(got[name], *bw[name], f"chain.{name}", what)


# ---- forward, backward, chained -------------------------------------------------------------------

@pytest.mark.parametrize("N", ALL_N)
def test_forward_every_tile_count(N):
    """Every NKT at its first and last size (nlast == 32 skips the tail mask), `gauss`."""
    _fwd_case("gauss", N)


@pytest.mark.parametrize("N", ALL_N)
def test_backward_every_tile_count(N):
    """The dq and dk / dv kernels on their own, fed the reference's o and lse."""
    _bwd_case("gauss", N)


@pytest.mark.parametrize("N", FAMILY_N)
def test_forward_input_regimes(N):
    """Peaked rows, a large common offset (row max and lse of a few hundred, both signs), exact
    ties, one-hot rows."""
    for family in OTHERS:
        _fwd_case(family, N)


@pytest.mark.parametrize("N", FAMILY_N)
def test_backward_input_regimes(N):
    for family in OTHERS:
        _bwd_case(family, N)


@pytest.mark.parametrize("N", [33, 199, 261])
def test_chained(N):
    for family in R.FAMILIES:
        _chain_case(family, N)


@pytest.mark.parametrize("N", DROP_N)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout(N, p):
    """Every NKT of the DROP instances, every input family: forward, backward on its own, and
    chained, on the mask the kernel drew for a seed >= 2^31."""
    mask = Mask(N, p, 2 ** 31 + 977 * N + int(100 * p))
    for family in R.FAMILIES:
        _fwd_case(family, N, mask, p)
        _bwd_case(family, N, mask, p)
        _chain_case(family, N, mask, p)


# ---- exact answers --------------------------------------------------------------------------------

def _used_key(row, table):
    """Which row of table (N, 64) the 64-vector `row` equals (or is nearest to): for a failure report."""
    d = (table.float() - row.float()).abs().sum(-1)
    return int(d.argmin()), float(d.min())


def _assert_rows_equal(got, want, table_of, what):
    """got, want (B, N, H, 64) bit for bit; on a mismatch name the first row and the key it holds."""
    bad = (got.view(torch.int16) != want.view(torch.int16)).any(-1)
    if bool(bad.any()):
        b, n, h = (int(x) for x in bad.nonzero()[0])
        key, dist = _used_key(got[b, n, h], table_of(b, h))
        raise AssertionError(f"{what}: row (b {b}, n {n}, h {h}) is not the expected one; it is nearest to row {key} "
                             f"of the source (L1 distance {dist}); {int(bad.sum())} rows differ")


@pytest.mark.parametrize("N", [5, 33, 96, 261, 320])
def test_selector_exact(N):
    """One-hot attention: out[q] == V[perm[q]] and dv[perm[q]] == dO[q] bit for bit."""
    c, _, o, lse, _ = _problem("selector", N)
    out, _ = run_fwd(c, N, f"selector N {N}")
    _assert_rows_equal(out, R.selected_rows(c["v"], c["perm"]), lambda b, h: c["v"][b, :, h], f"out N {N}")
    got = run_bwd(c, N, o, lse, f"selector N {N}")
    _assert_rows_equal(R.selected_rows(got["dv"], c["perm"]), c["do"], lambda b, h: c["do"][b, :, h], f"dv N {N}")


@pytest.mark.parametrize("N", [5, 33, 96, 261, 320])
def test_selector_exact_under_dropout(N):
    """p = 0.5: out[q] == 2 V[perm[q]] where the keep bit of (q, perm[q]) is set and |out| < 1e-6
    where it is not; dv[perm[q]] == 2 dO[q] or ~0 by the same bit read from the key-major words."""
    c = R.case("selector", B, H, N, N)
    perm = c["perm"]
    mask = Mask(N, 0.5, 2 ** 31 + N)
    what = f"selector N {N} p 0.5"
    out, _ = run_fwd(c, N, what, mask, 0.5)
    kept = torch.gather(mask.keep_q, -1, perm[..., None]).squeeze(-1).permute(0, 2, 1)[..., None]   # (B, N, H, 1) by q
    want = (2 * R.selected_rows(c["v"], perm).float()).to(BF)
    sel = kept.expand_as(out)
    _assert_rows_equal(torch.where(sel, out, want), want, lambda b, h: 2 * c["v"][b, :, h].float(), "out " + what)
    assert float((out.float() * ~sel).abs().max()) < 1e-6, "out " + what + ": a dropped selection is not ~0"
    fw = R.fwd_ref(c["q"], c["k"], c["v"], SCALE, mask.keep, 0.5)
    got = run_bwd(c, N, fw["out"][0].to(F32).to(BF), fw["lse"][0].to(F32), what, mask, 0.5)
    # key-major words: bit of (key = perm[q], query q), gathered per q
    kk = torch.gather(mask.keep_k, 2, perm[..., None].expand(B, H, N, mask.keep_k.shape[-1]))      # rows key = perm[q]
    kept_k = torch.gather(kk, -1, torch.arange(N).view(1, 1, N, 1).expand(B, H, N, 1)).squeeze(-1)
    kept_k = kept_k.permute(0, 2, 1)[..., None]
    dv_q = R.selected_rows(got["dv"], perm)
    want = (2 * c["do"].float()).to(BF)
    sel = kept_k.expand_as(dv_q)
    _assert_rows_equal(torch.where(sel, dv_q, want), want, lambda b, h: 2 * c["do"][b, :, h].float(), "dv " + what)
    assert float((dv_q.float() * ~sel).abs().max()) < 1e-6, "dv " + what + ": a dropped selection is not ~0"


# ---- the dropout mask -----------------------------------------------------------------------------

def _keep_bits(n, p, seed):
    L = _lib()
    out = torch.full((n + 64,), 7, dtype=torch.uint8, device=dev)
    L.call("triad_dropout_keep", n, p, seed, _at(out), L.stream_ptr())
    assert bool((out[n:] == 7).all())
    return out[:n].cpu().bool()


@pytest.mark.parametrize("N", [1, 31, 33, 64, 199, 320])
def test_dropmask_is_the_hash_of_the_element_index(N):
    """Bit (bh, q, key) of the query-major words == triad_dropout_keep's bit of element
    (bh N + q) N + key (odd N: odd and even element offsets of a row), the key-major words hold its
    transpose, bits of keys / queries >= N are 0, every word inside B H N nkt is written (the
    buffers start as a sentinel pattern) and none after it."""
    p, seed = 0.3, 2 ** 31 + 12345 + N
    mask = Mask(N, p, seed)
    dense = _keep_bits(B * H * N * N, p, seed).view(B, H, N, N)
    for name, w, want in (("wq", mask.wq, dense), ("wk", mask.wk, dense.transpose(-1, -2))):
        words = (w[:mask.words].cpu().to(torch.int64) & 0xFFFFFFFF).view(B, H, N, mask.nkt)
        assert torch.equal(words, pack_words(want)), f"{name} N {N}: words differ from the packed hash bits"
        assert bool((w[mask.words:] == SENTINEL).all()), f"{name} N {N}: wrote past B H N nkt words"
    assert not bool(mask.keep_q[..., N:].any()) and not bool(mask.keep_k[..., N:].any())
    assert torch.equal(mask.keep, dense) and torch.equal(mask.keep_k[..., :N], dense.transpose(-1, -2))


def test_dropmask_p0_seeds_and_repeats():
    """p = 0 keeps everything in range; one seed twice gives equal words, two seeds different ones."""
    N = 97
    full = Mask(N, 0.0, 2 ** 31 + 5)
    assert bool(full.keep.all()) and bool(full.keep_k[..., :N].all())
    assert not bool(full.keep_q[..., N:].any()) and not bool(full.keep_k[..., N:].any())
    a, b, c = Mask(N, 0.5, 2 ** 31 + 5), Mask(N, 0.5, 2 ** 31 + 5), Mask(N, 0.5, 2 ** 31 + 6)
    assert torch.equal(a.wq, b.wq) and torch.equal(a.wk, b.wk)
    assert not torch.equal(a.wq, c.wq) and not torch.equal(a.wk, c.wk)
    frac = float(a.keep.float().mean())
    assert abs(frac - 0.5) < 5 * 0.5 / math.sqrt(B * H * N * N), frac   # five standard deviations


def test_bit_stable_repeats():
    """No atomics in these kernels: three runs at N = 261 with dropout are bit-identical."""
    N, p = 261, 0.1
    c = R.case("gauss", B, H, N, N)
    mask = Mask(N, p, 2 ** 31 + 261)
    runs = []
    for i in range(3):
        out, lse = run_fwd(c, N, f"repeat {i}", mask, p)
        g = run_bwd(c, N, out, lse, f"repeat {i}", mask, p)
        runs.append((out, lse, g["dq"], g["dk"], g["dv"], g["delta"]))
    for r in runs[1:]:
        assert all(torch.equal(x.view(torch.int16) if x.dtype == BF else x, y.view(torch.int16) if y.dtype == BF else y)
                   for x, y in zip(r, runs[0])), "a repeat changed a result bit"


# ---- rejected calls ---------------------------------------------------------------------------------

def _fwd_args(tokens, **over):
    """Argument list of triad_attn_fwd over NaN-filled outputs; `over` replaces entries by name."""
    t = {name: Rows(tokens, name, torch.zeros(B, tokens, H, HD, dtype=BF)) for name in ("q", "k", "v")}
    out, lse = Rows(tokens, "out"), Stat(tokens, "lse")
    a = {name: t[name].args for name in t}
    a.update(B=B, H=H, N=tokens, D=HD, scale=SCALE, out=out.args, lse=lse.ptr)
    a.update(over)
    args = (*a["q"], *a["k"], *a["v"], a["B"], a["H"], a["N"], a["D"], a["scale"], *a["out"], a["lse"])
    return args, [out.flat, lse.flat]


def _bwd_args(tokens, **over):
    t = {name: Rows(tokens, name, torch.zeros(B, tokens, H, HD, dtype=BF)) for name in ("q", "k", "v", "o", "do")}
    outs = {name: Rows(tokens, name) for name in ("dq", "dk", "dv")}
    lse, delta = Stat(tokens, "lse", torch.zeros(B, H, tokens)), Stat(tokens, "delta")
    a = {name: t[name].args for name in t}
    a.update({name: outs[name].args for name in outs})
    a.update(B=B, H=H, N=tokens, D=HD, scale=SCALE, lse=lse.ptr, delta=delta.ptr)
    a.update(over)
    args = (*a["q"], *a["k"], *a["v"], *a["o"], *a["do"], a["lse"], a["B"], a["H"], a["N"], a["D"], a["scale"],
            *a["dq"], *a["dk"], *a["dv"], a["delta"])
    return args, [outs[name].flat for name in outs] + [delta.flat]


def _shift(args, bytes_=0, dsB=0, dsN=0):
    p, sB, sN = args
    return ctypes.c_void_p(p.value + bytes_), sB + dsB, sN + dsN


def _rejected(name, args, outputs, why):
    from triad_amd._lib import TriadError
    L = _lib()
    with pytest.raises(TriadError, match="invalid argument"):
        L.call(name, *args, L.stream_ptr())
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outputs), f"{name} ({why}): an output was written"


def test_unsafe_calls_are_rejected_before_any_launch():
    """TRIAD_EINVAL (a TriadError) by status alone, the NaN-filled outputs still all NaN: nothing
    misaligned and no non-positive scale is ever launched."""
    N = 33
    bad_scales = (0.0, -0.125, math.inf, -math.inf, NAN)
    for name, make, tensors in (("triad_attn_fwd", _fwd_args, ("q", "k", "v", "out")),
                                ("triad_attn_bwd", _bwd_args, ("q", "k", "v", "o", "do", "dq", "dk", "dv"))):
        args, outs = make(N)
        L = _lib()
        L.call(name, *args, L.stream_ptr())      # the unmodified argument list is a valid call
        torch.cuda.synchronize()
        for s in bad_scales:
            _rejected(name, *make(N, scale=s), f"scale {s}")
        _rejected(name, *make(N, B=257, H=256), "B * H = 65792")
        _rejected(name, *make(N, N=321), "N = 321")
        _rejected(name, *make(N, D=32), "D = 32")
        _rejected(name, *make(N, lse=None), "null lse")
        for t in tensors:
            ref = Rows(N, t).args   # a valid (pointer, sB, sN) of this tensor, spoilt one way at a time
            for why, kw in (("8-byte offset", dict(bytes_=8)), ("2-byte offset", dict(bytes_=2)),
                            ("sB + 4", dict(dsB=4)), ("sN + 4", dict(dsN=4)), ("sN + 1", dict(dsN=1))):
                _rejected(name, *make(N, **{t: _shift(ref, **kw)}), f"{t}: {why}")
            _rejected(name, *make(N, **{t: (None, ref[1], ref[2])}), f"{t}: null")
    _rejected("triad_attn_bwd", *_bwd_args(N, delta=None), "null delta")
    # the _dropout forms share the checks
    m = Mask(N, 0.5, 2 ** 31)
    args, outs = _fwd_args(N, scale=-0.125)
    _rejected("triad_attn_fwd_dropout", (*args[:14], _at(m.wq), 0.5, *args[14:]), outs, "dropout forward, scale < 0")
    args, outs = _bwd_args(N, scale=-0.125)
    _rejected("triad_attn_bwd_dropout", (*args[:21], _at(m.wq), _at(m.wk), 0.5, *args[21:]), outs,
              "dropout backward, scale < 0")


# ---- attention.py -------------------------------------------------------------------------------------

def _math(q, k, v, scale=None, mask=None, causal=False):
    """fp32 softmax(q k^T scale + mask) v for (B, H, N, d)."""
    q, k, v = q.float(), k.float(), v.float()
    s = (q @ k.transpose(-1, -2)) * (q.shape[-1] ** -0.5 if scale is None else scale)
    if mask is not None:
        s = s + mask.float()
    if causal:
        n = s.shape[-1]
        s = s.masked_fill(torch.ones(n, n, dtype=torch.bool, device=s.device).triu(1), -math.inf)
    return torch.softmax(s, -1) @ v


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _bhnd(N, d=64, dtype=BF, seed=0):
    g = torch.Generator().manual_seed(1000 + N + d + seed)
    return [(torch.randn(B, H, N, d, generator=g) * 1.5).to(dtype).to(dev) for _ in range(3)]


def _forbid_kernels(monkeypatch):
    from triad_amd import attention as A

    def boom(*a, **k):
        raise AssertionError("the HIP forward was called for an unsupported input")
    monkeypatch.setattr(A, "_fwd", boom)   # the forward of both families
    # N = 321 belongs to the streaming kernels by default (tests/test_attention_long_conformance_gpu.py);
    # with their route closed it is PyTorch's, like everything else the whole-sequence kernels refuse
    monkeypatch.setattr(A, "LONG_ROUTE", (A.MAX_TOKENS_LONG + 1, A.MAX_TOKENS_LONG))


@pytest.mark.parametrize("why,N,d,dtype,scale", [("N = 321", 321, 64, BF, None), ("head dim 32", 40, 32, BF, None),
                                                 ("fp32 input", 40, 64, F32, None), ("scale < 0", 40, 64, BF, -0.125)])
def test_sdpa_falls_back_to_pytorch(monkeypatch, why, N, d, dtype, scale):
    from triad_amd import attention as A
    _forbid_kernels(monkeypatch)
    q, k, v = _bhnd(N, d, dtype)
    got = A.sdpa(q, k, v, scale=scale)
    assert got.shape == q.shape and got.dtype == dtype
    assert _rel(got, _math(q, k, v, scale)) < (1e-3 if dtype == F32 else 1e-2), why


def _module(training=False, causal=False):
    m = torch.nn.Module()
    m.is_causal = causal
    m.train(training)
    return m


@pytest.mark.parametrize("why", ["N = 321", "head dim 32", "fp32 input", "attention mask", "is_causal", "scale < 0"])
def test_hf_attention_forward_falls_back_to_pytorch(monkeypatch, why):
    from triad_amd import attention as A
    _forbid_kernels(monkeypatch)
    N = 321 if why == "N = 321" else 40
    d = 32 if why == "head dim 32" else 64
    dtype = F32 if why == "fp32 input" else BF
    q, k, v = _bhnd(N, d, dtype, seed=7)
    mask = None
    if why == "attention mask":
        mask = torch.zeros(B, 1, N, N, dtype=dtype, device=dev)
        mask[..., N - 7:] = -math.inf          # the last 7 keys padded away
    scaling = -0.125 if why == "scale < 0" else d ** -0.5
    got, weights = A.hf_attention_forward(_module(causal=why == "is_causal"), q, k, v, mask, scaling=scaling)
    assert weights is None and got.shape == (B, N, H, d)
    want = _math(q, k, v, scaling, mask, causal=why == "is_causal").transpose(1, 2)
    assert _rel(got, want) < (1e-3 if dtype == F32 else 1e-2), why


def test_wrappers_take_the_kernels_for_supported_input(monkeypatch):
    """The counterpart of the fall-back tests: the same entry points at a supported shape do call
    the HIP forward (counted), and match fp32 math."""
    from triad_amd import attention as A
    calls = []
    real = A._fwd
    monkeypatch.setattr(A, "_fwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    q, k, v = _bhnd(40)
    assert _rel(A.sdpa(q, k, v), _math(q, k, v)) < 1e-2
    got, _ = A.hf_attention_forward(_module(), q, k, v, None, scaling=0.125)
    assert _rel(got, _math(q, k, v).transpose(1, 2)) < 1e-2
    assert len(calls) == 2


def _wrapper_matches(q, k, v, do, what):
    """attention_bnhd on (B, N, H, 64) views against the fp64 reference's bounds (out, then dq, dk,
    dv of the chain)."""
    from triad_amd import attention as A
    qd, kd, vd = (t.detach().requires_grad_(True) for t in (q, k, v))
    out = A.attention_bnhd(qd, kd, vd, SCALE)
    out.backward(do)
    qc, kc, vc, dc = (t.detach().cpu().contiguous() for t in (q, k, v, do))
    fw = R.fwd_ref(qc, kc, vc, SCALE)
    _check(out.detach().cpu(), *fw["out"], "wrapper.out", what)
    bw = R.bwd_ref(qc, kc, vc, fw["out"][0], fw["lse"][0], dc, SCALE, lse_err=fw["lse"][1], o_err=fw["out"][1])
    for name, t in (("dq", qd), ("dk", kd), ("dv", vd)):
        _check(t.grad.cpu(), *bw[name], "wrapper." + name, what)


def test_wrapper_copies_transposed_and_misaligned_views():
    """A (B, H, N, 64)-contiguous tensor passed transposed, a view at a storage offset of 4 elements
    (8 bytes) and one whose sN is not a multiple of 8 are copied by _as_bnhd and give the right
    answer (forward and backward)."""
    N = 45
    c = R.case("gauss", B, H, N, N)
    do = c["do"].to(dev)
    # (B, H, N, 64) storage, passed as its (B, N, H, 64) transpose: stride(2) != 64
    tr = [c[n].to(dev).permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for n in ("q", "k", "v")]
    assert tr[0].stride(2) != HD
    _wrapper_matches(*tr, do, "transposed")
    # storage offset of 4 elements
    off = []
    for n in ("q", "k", "v"):
        buf = torch.zeros(4 + B * N * H * HD, dtype=BF, device=dev)
        buf[4:] = c[n].to(dev).reshape(-1)
        off.append(buf[4:].view(B, N, H, HD))
    assert off[0].data_ptr() % 16 == 8
    _wrapper_matches(*off, do, "offset 4")
    # sN = H * 64 + 4
    odd = []
    for n in ("q", "k", "v"):
        buf = torch.zeros(B, N, H * HD + 4, dtype=BF, device=dev)
        buf[:, :, :H * HD] = c[n].to(dev).reshape(B, N, H * HD)
        odd.append(buf[:, :, :H * HD].view(B, N, H, HD))
    assert odd[0].stride(1) % 8 == 4
    _wrapper_matches(*odd, do, "sN + 4")
    # the fused-projection entry at a storage offset of 4 elements
    from triad_amd import attention as A
    qkv = torch.cat([c[n].reshape(B, N, H * HD) for n in ("q", "k", "v")], -1).to(dev)
    buf = torch.zeros(4 + qkv.numel(), dtype=BF, device=dev)
    buf[4:] = qkv.reshape(-1)
    got = A.attention_qkv(buf[4:].view(B, N, 3 * H * HD), H, SCALE)
    fw = R.fwd_ref(c["q"], c["k"], c["v"], SCALE)
    _check(got.view(B, N, H, HD).cpu(), *fw["out"], "wrapper.out", "fused qkv at offset 4")
