"""Conformance of the streaming attention kernels of csrc/attention_long.hip -- triad_attn_long_fwd,
triad_attn_long_bwd (forward, dq and dk / dv kernels, with and without dropout) and
triad_attn_long_dropmask, 321 <= N <= 2048 -- against fp64 references of the same bf16 operands,
through the C ABI (`triad_amd._lib.call`), and of the attention.py / vit.py wrappers over them.

The method is that of tests/test_attention_conformance_gpu.py: seeded CPU operands
(tests/attention_ref.py and, for the `rising` family, the forward's online-softmax bound and the
keep-word layout, tests/attention_long_ref.py; tests/test_attention_long_checks_cpu.py shows that the
bounds pass a chunked emulation of each kernel and fail ten planted errors). Every tensor sits in
its own NaN-filled buffer with its own row stride sN = H * 64 + 8 j, a gap between the samples and
NaN guards; outputs must be finite inside and leave every gap and guard NaN. The backward is tested
on its own (o = bf16(reference out), lse = fp32(reference lse)) and chained to the forward (bounds
widened through lse_err / o_err). Under dropout the reference uses the mask the kernel drew, which
test_dropmask_* pin to triad_dropout_keep's bit of element (bh N + q) N + key. B = 2, H = 3 below
N = 1374, B = 1, H = 2 from there.

Sizes, with KC = 64 keys per chunk and 128 queries per workgroup: the ends of the range, the workload's
499 and 1374, 351 .. 353 (a 32-tile boundary inside a chunk), m KC - 1, m KC, m KC + 1 for m = 6, 7, 8
(the first chunk counts past 320; 128 m +- 1 for m = 3, 4 are among them).

Largest err / bound per group on MI355X (66 cases, 756 bound comparisons, 13 s in all, the slowest
case 1.5 s at N = 2048; also in DESIGN.md section 2; `pytest -s` prints every figure). Without / with
dropout: out 0.710 / 0.789, lse 0.098 / 0.042, delta 0.022 / 0.021, dq 0.824 / 0.832, dk 0.863 / 0.874,
dv 0.874 / 0.899. Chained: delta 0.195, dq 0.628, dk 0.594, dv 0.879. Through attention_bnhd /
attention_qkv: out 0.524, dq 0.243, dk 0.167, dv 0.643. Every check held on the first run; neither a
kernel nor a bound was changed after it.
"""
import ctypes
import functools
import math

import pytest
import torch

from tests import attention_long_ref as LR
from tests import attention_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
HD = 64
SCALE = R.f32(R.SCALE)
ALL_N = (321, 351, 352, 353, 383, 384, 385, 447, 448, 449, 499, 511, 512, 513, 1374, 2047, 2048)
FAMILY_N = (321, 499, 1374)
OTHERS = tuple(f for f in R.FAMILIES if f != "gauss")   # peaked, offset, ties, selector
SENTINEL = 0x5A5A5A5A
J = dict(k=1, v=2, q=3, o=4, do=5, out=6, dq=7, dk=8, dv=9)   # sN = H * 64 + 8 j: no two alike
WORST = {}


def _bh(N):
    return (2, 3) if N < 1374 else (1, 2)


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
        B, H = _bh(N)
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
        inside = torch.zeros(self.flat.shape, dtype=torch.bool, device=dev)
        inside.as_strided(self.shape, self.strides, self.off).fill_(True)
        assert bool(torch.isnan(self.flat[~inside]).all()), f"{what}: {self.name} wrote into a gap or a guard"
        assert bool(torch.isfinite(self.view).all()), f"{what}: {self.name} has unwritten or non-finite elements"
        return self.view.cpu().contiguous()


class Stat:
    """lse / delta: (B, H, N) fp32 with 4 NaN guard elements in front and 16 behind."""

    def __init__(self, N, name, src=None):
        B, H = _bh(N)
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
    print("\nstreaming attention kernels, largest err/bound per group:",
          ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))


# ---- the calls ----------------------------------------------------------------------------------

def run_fwd(c, N, what, mask=None, p=0.0):
    """-> (out (B, N, H, 64) bf16, lse (B, H, N) fp32) on the host, guards checked."""
    L = _lib()
    B, H = _bh(N)
    q, k, v = (Rows(N, n, c[n]) for n in ("q", "k", "v"))
    out, lse = Rows(N, "out"), Stat(N, "lse")
    L.call("triad_attn_long_fwd", *q.args, *k.args, *v.args, B, H, N, HD, SCALE, _at(mask.wq) if mask else None, p,
           *out.args, lse.ptr, L.stream_ptr())
    return out.result(what), lse.result(what)


def run_bwd(c, N, o, lse, what, mask=None, p=0.0):
    """o (B, N, H, 64) bf16, lse (B, H, N) fp32 (host) -> dict of dq, dk, dv, delta on the host."""
    L = _lib()
    B, H = _bh(N)
    q, k, v, do = (Rows(N, n, c[n]) for n in ("q", "k", "v", "do"))
    ob, ls = Rows(N, "o", o), Stat(N, "lse", lse)
    dq, dk, dv, delta = Rows(N, "dq"), Rows(N, "dk"), Rows(N, "dv"), Stat(N, "delta")
    L.call("triad_attn_long_bwd", *q.args, *k.args, *v.args, *ob.args, *do.args, ls.ptr, B, H, N, HD, SCALE,
           _at(mask.wq) if mask else None, _at(mask.wk) if mask else None, p, *dq.args, *dk.args, *dv.args, delta.ptr,
           L.stream_ptr())
    return {"dq": dq.result(what), "dk": dk.result(what), "dv": dv.result(what), "delta": delta.result(what)}


class Mask:
    """triad_attn_long_dropmask at (N, p, seed) into sentinel-filled word buffers with 32 sentinel
    words behind. keep_q / keep_k: the (B, H, N, 32 wpr) bits of the query-major words [b, h, q, key]
    and of the key-major words [b, h, key, q], on the host."""

    def __init__(self, N, p, seed):
        L = _lib()
        self.B, self.H = _bh(N)
        self.N, self.wpr = N, LR.wpr(N)
        self.words = self.B * self.H * N * self.wpr
        self.wq = torch.full((self.words + 32,), SENTINEL, dtype=torch.int32, device=dev)
        self.wk = self.wq.clone()
        L.call("triad_attn_long_dropmask", self.B, self.H, N, p, seed, _at(self.wq), _at(self.wk), L.stream_ptr())
        self.keep_q, self.keep_k = self._unpack(self.wq), self._unpack(self.wk)

    def _unpack(self, w):
        w = w[:self.words].cpu().to(torch.int64).view(self.B, self.H, self.N, self.wpr, 1) & 0xFFFFFFFF
        return ((w >> torch.arange(32)) & 1).bool().view(self.B, self.H, self.N, self.wpr * 32)

    @property
    def keep(self):
        """(B, H, N, N) [b, h, q, key] from the query-major words."""
        return self.keep_q[..., :self.N]


@functools.lru_cache(maxsize=4)
def _problem(family, N):
    """Seeded case with its no-dropout references, computed once per (family, N) and not modified:
    (case, forward reference, o = bf16(ref out), lse = fp32(ref lse), backward reference at o, lse)."""
    c = LR.case(family, *_bh(N), N, N)
    fw = LR.fwd_ref(c["q"], c["k"], c["v"], SCALE)
    o, lse = fw["out"][0].to(F32).to(BF), fw["lse"][0].to(F32)
    return c, fw, o, lse, LR.bwd_ref(c["q"], c["k"], c["v"], o, lse, c["do"], SCALE)


def _all_three(family, N, mask=None, p=0.0, chain=True):
    """Forward, backward on its own, and (chain) the backward fed the forward's own out and lse."""
    what = f"{family} N {N} p {p}"
    tag = ".drop" if mask is not None else ""
    if mask is None:
        c, fw, o, lse, bw = _problem(family, N)
        keep = None
    else:
        c, keep = LR.case(family, *_bh(N), N, N), mask.keep
        fw = LR.fwd_ref(c["q"], c["k"], c["v"], SCALE, keep, p)
        o, lse = fw["out"][0].to(F32).to(BF), fw["lse"][0].to(F32)
        bw = LR.bwd_ref(c["q"], c["k"], c["v"], o, lse, c["do"], SCALE, keep, p)
    out, ls = run_fwd(c, N, what, mask, p)
    _check(out, *fw["out"], "fwd.out" + tag, what)
    _check(ls, *fw["lse"], "fwd.lse" + tag, what)
    got = run_bwd(c, N, o, lse, what, mask, p)
    for name in ("delta", "dq", "dk", "dv"):
        _check(got[name], *bw[name], f"bwd.{name}{tag}", what)
    if chain:
        bw = LR.bwd_ref(c["q"], c["k"], c["v"], fw["out"][0], fw["lse"][0], c["do"], SCALE, keep, p,
                        lse_err=fw["lse"][1], o_err=fw["out"][1])
        got = run_bwd(c, N, out, ls, what, mask, p)
        for name in ("delta", "dq", "dk", "dv"):
            _check(got[name], *bw[name], f"chain.{name}", what)


# ---- forward, backward, chained -------------------------------------------------------------------

@pytest.mark.parametrize("N", ALL_N)
@pytest.mark.parametrize("family", ["gauss", "rising"])
def test_forward_backward_chained_every_size(family, N):
    _all_three(family, N)


@pytest.mark.parametrize("N", FAMILY_N)
@pytest.mark.parametrize("family", OTHERS)
def test_input_regimes(family, N):
    """Peaked rows, a large common offset (row max and lse of a few hundred, both signs), exact
    ties, one-hot rows."""
    _all_three(family, N)


@pytest.mark.parametrize("N", FAMILY_N)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout(N, p):
    """Forward, backward and chained on the mask the kernel drew for a seed >= 2^31: every family at
    N = 321 and 499, `gauss` and `rising` at 1374."""
    mask = Mask(N, p, 2 ** 31 + 977 * N + int(100 * p))
    for family in (LR.FAMILIES if N < 1374 else ("gauss", "rising")):
        _all_three(family, N, mask, p)


# ---- exact answers --------------------------------------------------------------------------------

def _assert_rows_equal(got, want, what):
    bad = (got.view(torch.int16) != want.view(torch.int16)).any(-1)
    if bool(bad.any()):
        b, n, h = (int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"{what}: row (b {b}, n {n}, h {h}) is not the expected one; {int(bad.sum())} rows differ")


@pytest.mark.parametrize("N", FAMILY_N)
def test_selector_exact(N):
    """One-hot attention: out[q] == V[perm[q]] and dv[perm[q]] == dO[q] bit for bit; under p = 0.5,
    2 V[perm[q]] (2 dO[q]) where the keep bit of (q, perm[q]) is set and ~0 where it is not, the
    forward by the query-major words and dv by the key-major ones."""
    B, H = _bh(N)
    c, _, o, lse, _ = _problem("selector", N)
    perm = c["perm"]
    out, _ = run_fwd(c, N, f"selector N {N}")
    _assert_rows_equal(out, R.selected_rows(c["v"], perm), f"out N {N}")
    got = run_bwd(c, N, o, lse, f"selector N {N}")
    _assert_rows_equal(R.selected_rows(got["dv"], perm), c["do"], f"dv N {N}")

    mask = Mask(N, 0.5, 2 ** 31 + N)
    what = f"selector N {N} p 0.5"
    out, _ = run_fwd(c, N, what, mask, 0.5)
    kept = torch.gather(mask.keep_q, -1, perm[..., None]).squeeze(-1).permute(0, 2, 1)[..., None]   # (B, N, H, 1) by q
    want = (2 * R.selected_rows(c["v"], perm).float()).to(BF)
    sel = kept.expand_as(out)
    _assert_rows_equal(torch.where(sel, out, want), want, "out " + what)
    assert float((out.float() * ~sel).abs().max()) < 1e-6, "out " + what + ": a dropped selection is not ~0"
    fw = LR.fwd_ref(c["q"], c["k"], c["v"], SCALE, mask.keep, 0.5)
    got = run_bwd(c, N, fw["out"][0].to(F32).to(BF), fw["lse"][0].to(F32), what, mask, 0.5)
    kk = torch.gather(mask.keep_k, 2, perm[..., None].expand(B, H, N, mask.keep_k.shape[-1]))      # rows key = perm[q]
    kept_k = torch.gather(kk, -1, torch.arange(N).view(1, 1, N, 1).expand(B, H, N, 1)).squeeze(-1)
    kept_k = kept_k.permute(0, 2, 1)[..., None]
    dv_q = R.selected_rows(got["dv"], perm)
    want = (2 * c["do"].float()).to(BF)
    sel = kept_k.expand_as(dv_q)
    _assert_rows_equal(torch.where(sel, dv_q, want), want, "dv " + what)
    assert float((dv_q.float() * ~sel).abs().max()) < 1e-6, "dv " + what + ": a dropped selection is not ~0"


# ---- the dropout mask -----------------------------------------------------------------------------

def _keep_bits(n, p, seed):
    L = _lib()
    out = torch.full((n + 64,), 7, dtype=torch.uint8, device=dev)
    L.call("triad_dropout_keep", n, p, seed, _at(out), L.stream_ptr())
    assert bool((out[n:] == 7).all())
    return out[:n].cpu().bool()


def _pack(keep, words):
    """(B, H, N, M) bool -> (B, H, N, words) int64, bit j of word t = column 32 t + j, zero past M."""
    B, H, n, m = keep.shape
    pad = torch.zeros(B, H, n, words * 32, dtype=torch.int64)
    pad[..., :m] = keep
    return (pad.view(B, H, n, words, 32) << torch.arange(32)).sum(-1)


@pytest.mark.parametrize("N", [321, 353, 499, 1374, 2048])
def test_dropmask_is_the_hash_of_the_element_index(N):
    """Bit (bh, q, key) of the query-major words == triad_dropout_keep's bit of element
    (bh N + q) N + key, the key-major words hold its transpose, both in 2 ceil(N / 64) words per row
    with every bit past N zero (the padding word of an odd tile count included), every word inside
    B H N wpr written (the buffers start as a sentinel pattern) and none after it."""
    B, H = _bh(N)
    p, seed = 0.3, 2 ** 31 + 12345 + N
    mask = Mask(N, p, seed)
    dense = _keep_bits(B * H * N * N, p, seed).view(B, H, N, N)
    for name, w, want in (("wq", mask.wq, dense), ("wk", mask.wk, dense.transpose(-1, -2))):
        words = (w[:mask.words].cpu().to(torch.int64) & 0xFFFFFFFF).view(B, H, N, mask.wpr)
        assert torch.equal(words, _pack(want, mask.wpr)), f"{name} N {N}: words differ from the packed hash bits"
        assert bool((w[mask.words:] == SENTINEL).all()), f"{name} N {N}: wrote past B H N wpr words"
    assert not bool(mask.keep_q[..., N:].any()) and not bool(mask.keep_k[..., N:].any())
    frac = float(dense.float().mean())
    assert abs(frac - 0.7) < 5 * math.sqrt(0.21 / dense.numel()), frac


def test_bit_stable_repeats():
    """No atomics, no hand-off: three runs of forward + backward are bit-identical, at N = 1374 without
    dropout and at N = 499 with p = 0.1."""
    for N, p in ((1374, 0.0), (499, 0.1)):
        c = LR.case("gauss", *_bh(N), N, N)
        mask = Mask(N, p, 2 ** 31 + N) if p else None
        runs = []
        for i in range(3):
            out, lse = run_fwd(c, N, f"repeat {i}", mask, p)
            g = run_bwd(c, N, out, lse, f"repeat {i}", mask, p)
            runs.append((out, lse, g["dq"], g["dk"], g["dv"], g["delta"]))
        for r in runs[1:]:
            assert all(torch.equal(x.view(torch.int16) if x.dtype == BF else x,
                                   y.view(torch.int16) if y.dtype == BF else y)
                       for x, y in zip(r, runs[0])), f"N {N}: a repeat changed a result bit"


# ---- rejected calls ---------------------------------------------------------------------------------

def _fwd_args(tokens, **over):
    """Argument list of triad_attn_long_fwd over NaN-filled outputs (buffers sized for `tokens`)."""
    B, H = _bh(tokens)
    t = {name: Rows(tokens, name, torch.zeros(B, tokens, H, HD, dtype=BF)) for name in ("q", "k", "v")}
    out, lse = Rows(tokens, "out"), Stat(tokens, "lse")
    a = {name: t[name].args for name in t}
    a.update(B=B, H=H, N=tokens, D=HD, scale=SCALE, out=out.args, lse=lse.ptr)
    a.update(over)
    args = (*a["q"], *a["k"], *a["v"], a["B"], a["H"], a["N"], a["D"], a["scale"], None, 0.0, *a["out"], a["lse"])
    return args, [out.flat, lse.flat]


def _bwd_args(tokens, **over):
    B, H = _bh(tokens)
    t = {name: Rows(tokens, name, torch.zeros(B, tokens, H, HD, dtype=BF)) for name in ("q", "k", "v", "o", "do")}
    outs = {name: Rows(tokens, name) for name in ("dq", "dk", "dv")}
    lse, delta = Stat(tokens, "lse", torch.zeros(B, H, tokens)), Stat(tokens, "delta")
    a = {name: t[name].args for name in t}
    a.update({name: outs[name].args for name in outs})
    a.update(B=B, H=H, N=tokens, D=HD, scale=SCALE, lse=lse.ptr, delta=delta.ptr)
    a.update(over)
    args = (*a["q"], *a["k"], *a["v"], *a["o"], *a["do"], a["lse"], a["B"], a["H"], a["N"], a["D"], a["scale"], None,
            None, 0.0, *a["dq"], *a["dk"], *a["dv"], a["delta"])
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
    """TRIAD_EINVAL by status alone, the NaN-filled outputs still all NaN (buffers are sized for 2049
    tokens, so nothing here could write out of bounds even if it were launched)."""
    T = 2049
    for name, make, tensors in (("triad_attn_long_fwd", _fwd_args, ("q", "k", "v", "out")),
                                ("triad_attn_long_bwd", _bwd_args, ("q", "k", "v", "o", "do", "dq", "dk", "dv"))):
        _rejected(name, *make(T), "N = 2049")
        _rejected(name, *make(T, N=320), "N = 320")
        for s in (0.0, -0.125, math.inf, NAN):
            _rejected(name, *make(T, N=499, scale=s), f"scale {s}")
        _rejected(name, *make(T, N=499, D=32), "D = 32")
        _rejected(name, *make(T, N=499, lse=None), "null lse")
        for t in tensors:
            ref = Rows(T, t).args
            for why, kw in (("8-byte offset", dict(bytes_=8)), ("sB + 4", dict(dsB=4)), ("sN + 4", dict(dsN=4))):
                _rejected(name, *make(T, N=499, **{t: _shift(ref, **kw)}), f"{t}: {why}")


# ---- attention.py, vit.py -----------------------------------------------------------------------------

def _math(q, k, v, scale=None):
    """fp32 softmax(q k^T scale) v for (B, H, N, d)."""
    q, k, v = q.float(), k.float(), v.float()
    s = (q @ k.transpose(-1, -2)) * (q.shape[-1] ** -0.5 if scale is None else scale)
    return torch.softmax(s, -1) @ v


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _count_long(monkeypatch):
    """Counts the streaming forwards (triad_attn_long_fwd) that reach attention.call."""
    from triad_amd import attention as A
    calls = []
    real = A.call

    def call(name, *a, **k):
        if name == "triad_attn_long_fwd":
            calls.append(1)
        return real(name, *a, **k)
    monkeypatch.setattr(A, "call", call)
    return calls


@pytest.mark.parametrize("N,p", [(499, 0.1), (1374, 0.0)])
def test_attention_bnhd_and_qkv(monkeypatch, N, p):
    """attention_bnhd and attention_qkv, forward and backward through autograd, against the fp64 bounds
    of the chain (under dropout: on the mask regenerated from the seed the wrapper drew)."""
    from triad_amd import attention as A
    B, H = _bh(N)
    calls = _count_long(monkeypatch)
    c = LR.case("gauss", B, H, N, N)
    seed = 2 ** 31 + 4242 + N
    monkeypatch.setattr(A, "_SEEDS", lambda: seed)
    keep = Mask(N, p, seed).keep if p else None
    fw = LR.fwd_ref(c["q"], c["k"], c["v"], SCALE, keep, p)
    bw = LR.bwd_ref(c["q"], c["k"], c["v"], fw["out"][0], fw["lse"][0], c["do"], SCALE, keep, p,
                    lse_err=fw["lse"][1], o_err=fw["out"][1])
    qd, kd, vd = (c[n].to(dev).requires_grad_(True) for n in ("q", "k", "v"))
    out = A.attention_bnhd(qd, kd, vd, SCALE, dropout=p)
    out.backward(c["do"].to(dev))
    what = f"attention_bnhd N {N} p {p}"
    _check(out.detach().cpu(), *fw["out"], "wrapper.out", what)
    for name, t in (("dq", qd), ("dk", kd), ("dv", vd)):
        _check(t.grad.cpu(), *bw[name], "wrapper." + name, what)
    qkv = torch.cat([c[n].reshape(B, N, H * HD) for n in ("q", "k", "v")], -1).to(dev).requires_grad_(True)
    out = A.attention_qkv(qkv, H, SCALE, dropout=p)
    out.backward(c["do"].reshape(B, N, H * HD).to(dev))
    what = f"attention_qkv N {N} p {p}"
    _check(out.detach().view(B, N, H, HD).cpu(), *fw["out"], "wrapper.out", what)
    g = qkv.grad.view(B, N, 3, H, HD).cpu()
    for i, name in enumerate(("dq", "dk", "dv")):
        _check(g[:, :, i].contiguous(), *bw[name], "wrapper." + name, what)
    assert len(calls) == 2


def _bhnd(N, seed=0):
    g = torch.Generator().manual_seed(2000 + N + seed)
    return [(torch.randn(1, 2, N, 64, generator=g) * 1.5).to(BF).to(dev) for _ in range(3)]


def _module():
    m = torch.nn.Module()
    m.is_causal = False
    m.eval()
    return m


@pytest.mark.parametrize("N", [1374, 2049])
def test_sdpa_hf_and_vit_take_the_streaming_kernels_up_to_2048(monkeypatch, N):
    """sdpa, hf_attention_forward and vit.Attention (dim 128, 2 heads) at N = 1374 each call
    triad_attn_long_fwd once (if LONG_ROUTE holds 1374) and match fp32 math to 1e-2 relative L2; at N = 2049 none calls
    it and all still match."""
    from triad_amd import attention as A
    from triad_amd import vit
    calls = _count_long(monkeypatch)
    q, k, v = _bhnd(N)
    assert _rel(A.sdpa(q, k, v), _math(q, k, v)) < 1e-2
    got, weights = A.hf_attention_forward(_module(), q, k, v, None, scaling=0.125)
    assert weights is None and got.shape == (1, N, 2, 64)
    assert _rel(got, _math(q, k, v).transpose(1, 2)) < 1e-2
    torch.manual_seed(5)
    att = vit.Attention(128, 2).to(dev).to(BF)
    x = torch.randn(1, N, 128, device=dev).to(BF)
    with torch.no_grad():   # the same bf16 qkv and proj on both sides: only the attention differs
        qkv = att.qkv(x).view(1, N, 3, 2, 64).permute(2, 0, 3, 1, 4)
        want = att.proj(_math(qkv[0], qkv[1], qkv[2]).transpose(1, 2).reshape(1, N, 128).to(BF))
        got = att(x)
    assert _rel(got, want) < 1e-2
    routed = A.LONG_ROUTE[0] <= N <= A.LONG_ROUTE[1]
    assert len(calls) == (3 if routed else 0), (N, len(calls))
