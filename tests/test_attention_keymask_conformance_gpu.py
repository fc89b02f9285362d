"""Conformance of the key-padding mask of the attention kernels of csrc/attention.hip --
triad_attn_fwd_keymask / triad_attn_bwd_keymask (every NKT = 1 .. 10 x DROP instance of the MASK forward,
dq and dk / dv kernels) and triad_attn_keymask_pack -- through the C ABI at B = 3, H = 2 (two heads: a
word row taken by (sample, head) instead of by sample reads another sample's mask), then of the
attention.py / postln.py / model.py layers over them.

The reference is tests/attention_ref.py's fp64 reference on each sample's compacted key set
(tests/attention_keymask_ref.py: nothing new is derived or fitted; tests/test_attention_keymask_checks_cpu.py
shows that the bounds pass an emulation of the masked kernels and fail eight planted errors). Buffers as in
tests/test_attention_conformance_gpu.py: every tensor in its own NaN-filled buffer with its own row stride
sN = H * 64 + 8 j, a gap between samples, NaN guards that must survive, outputs finite inside (lse = -inf
exactly where a sample has no key). K / V rows of cleared keys hold N(0, 1) * 100: finite, and loud if
read. The words handed to the kernels have the bits past N set.

Mask families (tests/attention_keymask_ref.py::masks): full; prefix (lengths N, 1, ceil(N / 2), every
32 j and 32 j + 1 below N, three per call); scattered; single (only key N - 1); empty (sample 1 has no key).

Exact checks, no tolerance: `full` against the unmasked entry points on all six outputs; `prefix` of
length L against the unmasked call at N = L (out, lse, dq on queries < L; dk, dv on keys < L with dO = 0
on queries >= L); out == V[N - 1] for `single`; the zeros and -inf of `empty`; +0 in the dk / dv rows of
cleared keys (every masked backward here); bits past N flipped; three repeats. For `single` the issue
also lists dq == 0: the reference dq is exactly 0, but the kernel forms dS = p (dP - delta) from two fp32
sums of the same 64 products in different orders (an MFMA and an fma chain), so its dq is a rounding
residue; it is held to the dq bound around 0, which is what that cancellation is given in the derivation.

Largest err / bound per group on MI355X: see `_report` (printed with -s) and DESIGN.md section 2.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import attention_keymask_ref as KM
from tests import attention_ref as R

pytestmark = pytest.mark.gpu

dev = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
B, H, HD = 3, 2, 64
SCALE = R.f32(R.SCALE)
# every NKT at its first and last size
ALL_N = (1, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 256, 257, 288, 289, 320)
FAMILY_N = (33, 128, 199)          # all five input families
OTHERS = tuple(f for f in R.FAMILIES if f != "gauss")
CASES = [("gauss", N) for N in sorted(set(ALL_N) | set(FAMILY_N))] + [(f, N) for N in FAMILY_N for f in OTHERS]
SENTINEL = 0x5A5A5A5A
J = dict(k=1, v=2, q=3, o=4, do=5, out=6, dq=7, dk=8, dv=9)   # sN = H * 64 + 8 j: no two alike
WORST = {}


def _lib():
    from triad_amd import _lib
    return _lib


def _at(t, elems=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + t.element_size() * elems)


class Rows:
    """A (nb, N, H, 64) bf16 tensor inside its own NaN-filled device buffer: row stride sN = H * 64 + 8 j,
    sample stride sB = N * sN + 8 (j + 1) (a gap), 8 (j % 3 + 1) guard elements in front and 64 behind."""

    def __init__(self, N, name, src=None, nb=B):
        j = J[name]
        self.name = name
        self.sN = H * HD + 8 * j
        self.sB = N * self.sN + 8 * (j + 1)
        self.off = 8 * (j % 3 + 1)
        self.flat = torch.full((self.off + nb * self.sB + 64,), NAN, dtype=BF, device=dev)
        self.shape, self.strides = (nb, N, H, HD), (self.sB, self.sN, HD, 1)
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
    """lse / delta: (nb, H, N) fp32 with 4 NaN guard elements in front and 16 behind. `neginf`: the samples
    whose values must be -inf exactly (lse of a sample with no key); everything else finite."""

    def __init__(self, N, name, src=None, nb=B):
        self.name, self.n = name, nb * H * N
        self.flat = torch.full((4 + self.n + 16,), NAN, dtype=F32, device=dev)
        self.view = self.flat[4:4 + self.n].view(nb, H, N)
        if src is not None:
            self.view.copy_(src.to(dev))

    @property
    def ptr(self):
        return _at(self.flat, 4)

    def result(self, what, neginf=None):
        assert bool(torch.isnan(self.flat[:4]).all()) and bool(torch.isnan(self.flat[4 + self.n:]).all()), \
            f"{what}: {self.name} wrote past its ends"
        got = self.view.cpu()
        want_inf = torch.zeros(got.shape, dtype=torch.bool)
        if neginf is not None:
            want_inf[neginf] = True
        assert bool((got[want_inf] == -math.inf).all()), f"{what}: {self.name} of a sample with no key is not -inf"
        assert bool(torch.isfinite(got[~want_inf]).all()), f"{what}: {self.name} has unwritten or non-finite elements"
        return got


class Words:
    """Key-mask words of a (B, N) mask on the device, between sentinel words; the bits past N are `past_n`."""

    def __init__(self, mask, past_n=1):
        w = KM.words_tensor(KM.pack_words(mask, past_n)).reshape(-1)
        self.flat = torch.full((3 + w.numel() + 8,), SENTINEL, dtype=torch.int32, device=dev)
        self.flat[3:3 + w.numel()] = w.to(dev)     # 12 bytes in: 4-byte aligned only
        self.n = w.numel()

    @property
    def ptr(self):
        return _at(self.flat, 3)


class Drop:
    """triad_attn_dropmask at (N, p, seed) for nb samples; keep (nb, H, N, N) [b, h, q, key] on the host."""

    def __init__(self, N, p, seed, nb=B):
        L = _lib()
        nkt = R.nkt(N)
        n = nb * H * N * nkt
        self.p = p
        self.wq = torch.full((n + 32,), SENTINEL, dtype=torch.int32, device=dev)
        self.wk = self.wq.clone()
        L.call("triad_attn_dropmask", nb, H, N, p, seed, _at(self.wq), _at(self.wk), L.stream_ptr())
        w = self.wq[:n].cpu().to(torch.int64).view(nb, H, N, nkt, 1) & 0xFFFFFFFF
        self.keep = ((w >> torch.arange(32)) & 1).bool().view(nb, H, N, nkt * 32)[..., :N]


def _check(got, ref, bound, group, what):
    r = KM.ratio(got, ref, bound)
    WORST[group] = max(WORST.get(group, 0.0), r) if r == r else NAN
    print(f"{group} {what}: err/bound {r:.4f}")
    assert r <= 1.0, f"{group} {what}: err/bound {r}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nkey-masked attention kernels, largest err/bound per group:",
          ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))


# ---- the calls ----------------------------------------------------------------------------------------------

def run_fwd(c, N, what, words=None, drop=None, nb=B, neginf=None, entry="triad_attn_fwd_keymask"):
    """-> (out (nb, N, H, 64) bf16, lse (nb, H, N) fp32) on the host, guards checked."""
    L = _lib()
    q, k, v = (Rows(N, n, c[n], nb) for n in ("q", "k", "v"))
    out, lse = Rows(N, "out", None, nb), Stat(N, "lse", None, nb)
    head = (*q.args, *k.args, *v.args, nb, H, N, HD, SCALE)
    tail = (*out.args, lse.ptr, L.stream_ptr())
    wq, p = (None, 0.0) if drop is None else (_at(drop.wq), drop.p)
    if entry == "triad_attn_fwd_keymask":
        L.call(entry, *head, wq, p, None if words is None else words.ptr, *tail)
    elif entry == "triad_attn_fwd_dropout":
        L.call(entry, *head, wq, p, *tail)
    else:
        L.call("triad_attn_fwd", *head, *tail)
    return out.result(what), lse.result(what, neginf)


def run_bwd(c, N, o, lse, what, words=None, drop=None, nb=B, entry="triad_attn_bwd_keymask"):
    """o (nb, N, H, 64) bf16, lse (nb, H, N) fp32 (host) -> dict of dq, dk, dv, delta on the host."""
    L = _lib()
    q, k, v, do = (Rows(N, n, c[n], nb) for n in ("q", "k", "v", "do"))
    ob, ls = Rows(N, "o", o, nb), Stat(N, "lse", lse, nb)
    dq, dk, dv, delta = Rows(N, "dq", None, nb), Rows(N, "dk", None, nb), Rows(N, "dv", None, nb), Stat(N, "delta", None, nb)
    head = (*q.args, *k.args, *v.args, *ob.args, *do.args, ls.ptr, nb, H, N, HD, SCALE)
    tail = (*dq.args, *dk.args, *dv.args, delta.ptr, L.stream_ptr())
    wq, wk, p = (None, None, 0.0) if drop is None else (_at(drop.wq), _at(drop.wk), drop.p)
    if entry == "triad_attn_bwd_keymask":
        L.call(entry, *head, wq, wk, p, None if words is None else words.ptr, *tail)
    elif entry == "triad_attn_bwd_dropout":
        L.call(entry, *head, wq, wk, p, *tail)
    else:
        L.call("triad_attn_bwd", *head, *tail)
    return {"dq": dq.result(what), "dk": dk.result(what), "dv": dv.result(what), "delta": delta.result(what)}


def _loud(c, mask, N, seed):
    """The case with the K / V rows of cleared keys replaced by N(0, 1) * 100 (a copy: cases are shared)."""
    g = R._gen(13, N, seed)
    cleared = ~mask[:, :, None, None].expand(B, N, H, HD)
    out = dict(c)
    for n in ("k", "v"):
        out[n] = torch.where(cleared, (torch.randn(B, N, H, HD, generator=g) * 100).to(BF), c[n])
    return out


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _assert_cleared_rows_plus_zero(got, mask, what):
    cleared = ~mask[:, :, None, None].expand(got["dk"].shape)
    for n in ("dk", "dv"):
        assert not bool(_bits(got[n])[cleared].any()), f"{what}: {n} of a cleared key is not +0"


def _masked_case(family, N, mask, drop, tag):
    """Forward, the backward alone (from the fp64 out / lse rounded to bf16 / fp32) and chained, within the bounds
    of the compacted reference; cleared dk / dv rows +0; an empty sample's zeros and -inf exact."""
    c = _loud(R.case(family, B, H, N, N), mask, N, N)
    p = 0.0 if drop is None else drop.p
    keep = None if drop is None else drop.keep
    what = f"{family} N {N} p {p} {tag}"
    words = Words(mask)
    empty = (~mask.any(1)).nonzero().squeeze(-1)
    grp = ".drop" if drop is not None else ""
    fw = KM.fwd_ref(c["q"], c["k"], c["v"], SCALE, mask, keep, p)
    out, lse = run_fwd(c, N, what, words, drop, neginf=empty)
    _check(out, *fw["out"], "fwd.out" + grp, what)
    _check(lse, *fw["lse"], "fwd.lse" + grp, what)
    assert not bool(_bits(out)[empty].any()), f"{what}: out of a sample with no key is not +0"
    o, ls = fw["out"][0].to(F32).to(BF), fw["lse"][0].to(F32)
    bw = KM.bwd_ref(c["q"], c["k"], c["v"], o, ls, c["do"], SCALE, mask, keep, p)
    got = run_bwd(c, N, o, ls, what, words, drop)
    for name in ("delta", "dq", "dk", "dv"):
        _check(got[name], *bw[name], f"bwd.{name}{grp}", what)
    _assert_cleared_rows_plus_zero(got, mask, what)
    bwc = KM.bwd_ref(c["q"], c["k"], c["v"], fw["out"][0], fw["lse"][0], c["do"], SCALE, mask, keep, p,
                     lse_err=fw["lse"][1], o_err=fw["out"][1])
    got = run_bwd(c, N, out, lse, what + " chained", words, drop)
    for name in ("delta", "dq", "dk", "dv"):
        _check(got[name], *bwc[name], f"chain.{name}{grp}", what)
    _assert_cleared_rows_plus_zero(got, mask, what + " chained")
    for name in ("dq", "dk", "dv"):
        assert not bool((got[name][empty].float() != 0).any()), f"{what}: {name} of a sample with no key is not 0"


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("family,N", CASES)
def test_masked_attention_within_bounds(family, N, p):
    """Every mask family (every prefix length) at this size, input family and dropout rate."""
    drop = None if p == 0.0 else Drop(N, p, 2 ** 31 + 977 * N + int(100 * p))
    for mf in KM.MASK_FAMILIES:
        for i, mask in enumerate(KM.masks(mf, B, N, N)):
            _masked_case(family, N, mask, drop, f"{mf}[{i}]")


# ---- exact answers ----------------------------------------------------------------------------------------------

def _six(c, N, words, drop, fwd_entry, bwd_entry, what, nb=B):
    out, lse = run_fwd(c, N, what, words, drop, nb=nb, entry=fwd_entry)
    g = run_bwd(c, N, out, lse, what, words, drop, nb=nb, entry=bwd_entry)
    return dict(out=out, lse=lse, **g)


def _assert_same_bits(a, b, what):
    for n in a:
        assert torch.equal(_bits(a[n]), _bits(b[n])), f"{what}: {n} differs in some bit"


@pytest.mark.parametrize("N", [1, 33, 128, 199, 320])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_full_mask_equals_the_unmasked_entry_points(N, p):
    c = R.case("gauss", B, H, N, N)
    drop = None if p == 0.0 else Drop(N, p, 2 ** 31 + N)
    masked = _six(c, N, Words(KM.masks("full", B, N)[0]), drop, "triad_attn_fwd_keymask", "triad_attn_bwd_keymask",
                  f"full N {N} p {p}")
    plain = _six(c, N, None, drop, "triad_attn_fwd_dropout", "triad_attn_bwd_dropout", f"unmasked N {N} p {p}")
    _assert_same_bits(masked, plain, f"full mask N {N} p {p} against the _dropout entry points")
    if p == 0.0:
        plain = _six(c, N, None, None, "triad_attn_fwd", "triad_attn_bwd", f"unmasked N {N}")
        _assert_same_bits(masked, plain, f"full mask N {N} against triad_attn_fwd / _bwd")
        null = _six(c, N, None, None, "triad_attn_fwd_keymask", "triad_attn_bwd_keymask", f"km null N {N}")
        _assert_same_bits(null, plain, f"km = NULL N {N}")


@pytest.mark.parametrize("N", [33, 97, 199, 320])
def test_prefix_mask_equals_the_unmasked_call_at_its_length(N):
    """Sample b with the first L keys set, dO = 0 on queries >= L, against the unmasked call on its first L
    tokens alone: the cleared keys add exact zeros, so out, lse, dq on queries < L and dk, dv on keys < L
    agree bit for bit."""
    base = R.case("gauss", B, H, N, N)
    for i, mask in enumerate(KM.masks("prefix", B, N, N)):
        lens = [int(x) for x in mask.sum(1)]
        c = _loud(base, mask, N, N)
        c["do"] = torch.where(mask[:, :, None, None].expand(B, N, H, HD), base["do"], torch.zeros((), dtype=BF))
        got = _six(c, N, Words(mask), None, "triad_attn_fwd_keymask", "triad_attn_bwd_keymask", f"prefix[{i}] N {N}")
        for b, L in enumerate(lens):
            one = {n: c[n][b:b + 1, :L].contiguous() for n in ("q", "k", "v", "do")}
            ref = _six(one, L, None, None, "triad_attn_fwd", "triad_attn_bwd", f"unmasked N {L}", nb=1)
            for n in ("out", "dq", "dk", "dv"):
                assert torch.equal(_bits(got[n][b, :L]), _bits(ref[n][0])), \
                    f"prefix[{i}] N {N}: {n} of sample {b} (length {L}) differs from the unmasked call at N = {L}"
            for n in ("lse", "delta"):
                assert torch.equal(_bits(got[n][b, :, :L]), _bits(ref[n][0])), \
                    f"prefix[{i}] N {N}: {n} of sample {b} (length {L}) differs from the unmasked call at N = {L}"


@pytest.mark.parametrize("N", [1, 33, 128, 199, 320])
def test_single_key(N):
    """Only key N - 1: out[q] == V[N - 1] bit for bit; dv[N - 1] == sum_q dO[q] within the dv bound; the
    reference dq is exactly 0 and the kernel's is inside the dq bound around it (see the module docstring)."""
    mask = KM.masks("single", B, N)[0]
    c = _loud(R.case("gauss", B, H, N, N), mask, N, N)
    out, lse = run_fwd(c, N, f"single N {N}", Words(mask))
    assert torch.equal(_bits(out), _bits(c["v"][:, N - 1:N].expand(B, N, H, HD).contiguous())), "out != V[N - 1]"
    fw = KM.fwd_ref(c["q"], c["k"], c["v"], SCALE, mask)
    o, ls = fw["out"][0].to(F32).to(BF), fw["lse"][0].to(F32)
    bw = KM.bwd_ref(c["q"], c["k"], c["v"], o, ls, c["do"], SCALE, mask)
    got = run_bwd(c, N, o, ls, f"single N {N}", Words(mask))
    # (the fp64 reference itself: p = exp(S - fp32(lse)) is 1 to 1e-7, dP - delta two fp64 sums of the same products)
    assert float(bw["dq"][0].abs().max()) < 1e-12, "the reference dq is not 0"
    _check(got["dv"][:, N - 1], c["do"].double().sum(1), bw["dv"][1][:, N - 1], "single.dv", f"N {N}: sum_q dO[q]")
    _check(got["dv"], *bw["dv"], "single.dv", f"N {N}")
    _check(got["dq"], *bw["dq"], "single.dq", f"N {N}")
    _assert_cleared_rows_plus_zero(got, mask, f"single N {N}")


@pytest.mark.parametrize("N", [33, 199, 289])
def test_bits_past_n_are_ignored(N):
    c = R.case("gauss", B, H, N, N)
    mask = KM.masks("scattered", B, N, N)[0]
    drop = Drop(N, 0.1, 2 ** 31 + 3 * N)
    runs = [_six(c, N, Words(mask, past_n), drop, "triad_attn_fwd_keymask", "triad_attn_bwd_keymask",
                 f"past_n {past_n} N {N}") for past_n in (1, 0)]
    _assert_same_bits(runs[0], runs[1], f"N {N}: the bits past N changed a result")


def test_bit_stable_repeats():
    N = 261
    c = R.case("gauss", B, H, N, N)
    mask = KM.masks("empty", B, N, N)[0]
    drop = Drop(N, 0.1, 2 ** 31 + 261)
    words = Words(mask)
    runs = []
    for i in range(3):
        out, lse = run_fwd(c, N, f"repeat {i}", words, drop, neginf=[1])
        runs.append(dict(out=out, lse=lse, **run_bwd(c, N, out, lse, f"repeat {i}", words, drop)))
    for r in runs[1:]:
        _assert_same_bits(r, runs[0], "a repeat")


# ---- the packing kernel -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 31, 32, 33, 320])
@pytest.mark.parametrize("kind", ["bool", "uint8"])
def test_keymask_pack_equals_the_host_packing(N, kind):
    """From bool and from uint8 values other than 0 / 1; the words past B ceil(N / 32) keep their sentinel."""
    L = _lib()
    g = R._gen(17, N)
    m = torch.rand(B, N, generator=g) < 0.5
    m[0, N - 1], m[2, 0] = True, True
    src = m if kind == "bool" else torch.where(m, torch.randint(1, 256, (B, N), generator=g), 0).to(torch.uint8)
    n = B * R.nkt(N)
    words = torch.full((2 + n + 16,), SENTINEL, dtype=torch.int32, device=dev)
    buf = torch.zeros(3 + B * N + 5, dtype=src.dtype)            # the mask at a 3-byte offset: no alignment needed
    buf[3:3 + B * N] = src.reshape(-1)
    buf = buf.to(dev)
    L.call("triad_attn_keymask_pack", _at(buf, 3), B, N, _at(words, 2), L.stream_ptr())
    got = words.cpu()
    assert bool((got[:2] == SENTINEL).all()) and bool((got[2 + n:] == SENTINEL).all()), "wrote outside B ceil(N / 32) words"
    assert np.array_equal(got[2:2 + n].numpy().view(np.uint32).reshape(B, -1), KM.pack_words(m))
    from triad_amd import attention as A
    assert np.array_equal(A.pack_key_mask(src.to(dev)).cpu().numpy().view(np.uint32), KM.pack_words(m))
    assert np.array_equal(A.pack_key_mask(m.long().to(dev)).cpu().numpy().view(np.uint32), KM.pack_words(m))


# ---- rejected calls ---------------------------------------------------------------------------------------------

def _rejected(name, args, outputs, why):
    from triad_amd._lib import TriadError
    L = _lib()
    with pytest.raises(TriadError, match="invalid argument"):
        L.call(name, *args, L.stream_ptr())
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outputs), f"{name} ({why}): an output was written"


def test_unsafe_calls_are_rejected_before_any_launch():
    """TRIAD_EINVAL by status, the NaN-filled outputs still all NaN."""
    N = 33
    z = torch.zeros(B, N, H, HD, dtype=BF)
    words = Words(KM.masks("scattered", B, N, N)[0])

    def fwd(**over):
        t = {n: Rows(N, n, z) for n in ("q", "k", "v")}
        out, lse = Rows(N, "out"), Stat(N, "lse")
        a = {n: t[n].args for n in t}
        a.update(B=B, H=H, N=N, D=HD, scale=SCALE, wq=None, p=0.0, km=words.ptr, out=out.args, lse=lse.ptr)
        a.update(over)
        return ((*a["q"], *a["k"], *a["v"], a["B"], a["H"], a["N"], a["D"], a["scale"], a["wq"], a["p"], a["km"],
                 *a["out"], a["lse"]), [out.flat, lse.flat])

    def bwd(**over):
        t = {n: Rows(N, n, z) for n in ("q", "k", "v", "o", "do")}
        outs = {n: Rows(N, n) for n in ("dq", "dk", "dv")}
        lse, delta = Stat(N, "lse", torch.zeros(B, H, N)), Stat(N, "delta")
        a = {n: t[n].args for n in t}
        a.update({n: outs[n].args for n in outs})
        a.update(B=B, H=H, N=N, D=HD, scale=SCALE, wq=None, wk=None, p=0.0, km=words.ptr, lse=lse.ptr, delta=delta.ptr)
        a.update(over)
        return ((*a["q"], *a["k"], *a["v"], *a["o"], *a["do"], a["lse"], a["B"], a["H"], a["N"], a["D"], a["scale"],
                 a["wq"], a["wk"], a["p"], a["km"], *a["dq"], *a["dk"], *a["dv"], a["delta"]),
                [outs[n].flat for n in outs] + [delta.flat])

    L = _lib()
    for name, make, tensors in (("triad_attn_fwd_keymask", fwd, ("q", "k", "v", "out")),
                                ("triad_attn_bwd_keymask", bwd, ("q", "k", "v", "o", "do", "dq", "dk", "dv"))):
        args, _ = make()
        L.call(name, *args, L.stream_ptr())      # the unmodified argument list is a valid call
        torch.cuda.synchronize()
        for off in (1, 2, 3):
            _rejected(name, *make(km=ctypes.c_void_p(words.ptr.value + off)), f"km + {off} bytes")
        for s in (0.0, -0.125, math.inf, NAN):
            _rejected(name, *make(scale=s), f"scale {s}")
        _rejected(name, *make(N=321), "N = 321")
        _rejected(name, *make(D=32), "D = 32")
        _rejected(name, *make(B=257, H=256), "B * H = 65792")
        _rejected(name, *make(p=1.0), "p = 1")
        _rejected(name, *make(lse=None), "null lse")
        for t in tensors:
            ptr, sB, sN = Rows(N, t).args
            _rejected(name, *make(**{t: (ctypes.c_void_p(ptr.value + 8), sB, sN)}), f"{t}: 8-byte offset")
            _rejected(name, *make(**{t: (ptr, sB, sN + 4)}), f"{t}: sN + 4")
            _rejected(name, *make(**{t: (None, sB, sN)}), f"{t}: null")
    drop = Drop(N, 0.5, 2 ** 31)
    _rejected("triad_attn_bwd_keymask", *bwd(wq=_at(drop.wq), wk=None, p=0.5), "wq without wk")
    _rejected("triad_attn_bwd_keymask", *bwd(delta=None), "null delta")
    out = torch.full((64,), SENTINEL, dtype=torch.int32, device=dev)
    src = torch.ones(B, N, dtype=torch.uint8, device=dev)
    from triad_amd._lib import TriadError
    for args in ((None, B, N, _at(out)), (_at(src), B, N, None), (_at(src), B, 321, _at(out)), (_at(src), 0, N, _at(out))):
        with pytest.raises(TriadError, match="invalid argument"):
            L.call("triad_attn_keymask_pack", *args, L.stream_ptr())
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- attention.py -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("entry", ["bnhd", "qkv"])
def test_wrappers_with_a_key_mask(monkeypatch, entry, p):
    """attention_bnhd / attention_qkv with key_mask through autograd at N = 33, with and without dropout,
    against the same reference (the chained bounds; the keep bits are those of the seed the call drew)."""
    from triad_amd import attention as A
    N, seed = 33, 2 ** 31 + 4242
    monkeypatch.setattr(A, "_SEEDS", lambda: seed)
    mask = KM.masks("empty", B, N, N)[0]
    c = _loud(R.case("gauss", B, H, N, N), mask, N, N)
    keep = None if p == 0.0 else A.dropout_keep_dense(B, H, N, p, seed, dev)[0].cpu()
    do = c["do"].to(dev)
    if entry == "bnhd":
        leaves = [c[n].to(dev).requires_grad_(True) for n in ("q", "k", "v")]
        out = A.attention_bnhd(*leaves, SCALE, dropout=p, key_mask=mask.to(dev))
        out.backward(do)
        grads = [t.grad.cpu() for t in leaves]
    else:
        qkv = torch.cat([c[n].reshape(B, N, H * HD) for n in ("q", "k", "v")], -1).to(dev).requires_grad_(True)
        out = A.attention_qkv(qkv, H, SCALE, dropout=p, key_mask=A.pack_key_mask(mask.to(dev)))   # packed words
        out.backward(do.view(B, N, H * HD))
        grads = [g.reshape(B, N, H, HD).contiguous() for g in qkv.grad.cpu().view(B, N, 3, H * HD).unbind(2)]
        out = out.view(B, N, H, HD)
    fw = KM.fwd_ref(c["q"], c["k"], c["v"], SCALE, mask, keep, p)
    _check(out.detach().cpu(), *fw["out"], "wrapper.out", f"{entry} p {p}")
    bw = KM.bwd_ref(c["q"], c["k"], c["v"], fw["out"][0], fw["lse"][0], c["do"], SCALE, mask, keep, p,
                    lse_err=fw["lse"][1], o_err=fw["out"][1])
    for name, g in zip(("dq", "dk", "dv"), grads):
        _check(g, *bw[name], "wrapper." + name, f"{entry} p {p}")


def test_wrappers_refuse_a_mask_on_the_streaming_kernels():
    from triad_amd import attention as A
    from triad_amd._lib import TriadError
    N = 321
    q, k, v = ((torch.randn(1, N, H, HD) * 1.5).to(BF).to(dev) for _ in range(3))
    mask = torch.ones(1, N, dtype=torch.bool, device=dev)
    with pytest.raises(TriadError):
        A.attention_bnhd(q, k, v, SCALE, key_mask=mask)
    with pytest.raises(TriadError):
        A.attention_qkv(torch.cat([t.reshape(1, N, H * HD) for t in (q, k, v)], -1), H, SCALE, key_mask=mask)


# ---- postln.py / model.py -------------------------------------------------------------------------------------------

LENGTHS = (32, 17, 1, 9)
SMALL = dict(n_layers=2, dim=256, n_heads=4, hidden_dim=512, dropout=0.0, attention_dropout=0.0)
DEFAULT = dict(n_layers=2, dropout=0.0, attention_dropout=0.0)      # dim 768, 12 heads, hidden_dim 3072


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _distilbert(cfg):
    from triad_amd import model as Mdl
    from triad_amd import postln
    torch.manual_seed(0)
    enc = Mdl._hf_model("DistilBertModel", "none/none", dict(cfg))
    return postln.install_fused_distilbert(enc).to(dev).train()


def _count_calls(monkeypatch):
    """Entry points launched through attention.call, by name."""
    from triad_amd import attention as A
    seen = {}
    real = A.call

    def counting(name, *a, **k):
        seen[name] = seen.get(name, 0) + 1
        return real(name, *a, **k)
    monkeypatch.setattr(A, "call", counting)
    return seen


def _forbid_stock(monkeypatch, tr):
    def boom(*a, **k):
        raise AssertionError("the stock transformer forward was entered")
    monkeypatch.setattr(tr, "_triad_stock_forward", boom)


def _ragged(Bt=4, Nt=32):
    ids = torch.randint(1000, 30000, (Bt, Nt), generator=torch.Generator().manual_seed(3))
    mask = (torch.arange(Nt)[None] < torch.tensor(LENGTHS)[:, None]).long()
    return ids, mask


@pytest.mark.parametrize("cfg", [SMALL, DEFAULT], ids=["dim256", "dim768"])
def test_fused_distilbert_with_a_key_mask_matches_stock(monkeypatch, cfg):
    """Padded batch (lengths 32, 17, 1, 9 of 32) under bf16 autocast, dropout off: output and parameter
    gradients of the fused forward agree with the stock forward on the same mask at the bars of
    tests/test_postln_gpu.py; the fused run launches exactly one masked attention forward per layer and
    does not enter the stock forward."""
    enc = _distilbert(cfg)
    tr = enc.transformer
    ids, mask = (t.to(dev) for t in _ragged())

    def run(fwd):
        enc.zero_grad(set_to_none=True)
        tr.forward = fwd
        with torch.autocast("cuda", dtype=torch.bfloat16), enc.triad_key_mask(mask):
            out = enc(input_ids=ids, attention_mask=mask).last_hidden_state
        gy = torch.linspace(-1, 1, out.numel(), device=dev).view_as(out)
        (out.float() * gy).sum().backward()
        return out.detach().float(), {n: q.grad.float().clone() for n, q in enc.named_parameters() if q.grad is not None}

    fused_fwd, stock = tr.forward, tr._triad_stock_forward
    try:
        o_s, g_s = run(stock)
        seen = _count_calls(monkeypatch)
        _forbid_stock(monkeypatch, tr)
        o_f, g_f = run(fused_fwd)
    finally:
        tr.forward = fused_fwd
    assert seen.get("triad_attn_fwd_keymask", 0) == cfg["n_layers"], seen
    assert seen.get("triad_attn_bwd_keymask", 0) == cfg["n_layers"], seen
    assert seen.get("triad_attn_keymask_pack", 0) == 1, seen
    assert "triad_attn_fwd_dropout" not in seen and "triad_attn_fwd" not in seen, seen
    assert bool(torch.isfinite(o_f).all())
    assert _rel(o_f, o_s) < 1e-2, _rel(o_f, o_s)
    assert set(g_f) == set(g_s)
    for n in g_s:
        if n.endswith("k_lin.bias"):  # exactly 0 in exact arithmetic: noise
            continue
        assert _rel(g_f[n], g_s[n]) < 3e-2, (n, _rel(g_f[n], g_s[n]))


def test_a_4d_mask_without_a_key_mask_reaches_the_stock_forward(monkeypatch):
    """The transformer handed a 4-D mask directly (no key-mask context, or one of another shape) does not
    guess: it runs the stock forward, as before."""
    enc = _distilbert(SMALL)
    tr = enc.transformer
    entered = []
    real = tr._triad_stock_forward
    monkeypatch.setattr(tr, "_triad_stock_forward", lambda *a, **k: (entered.append(1), real(*a, **k))[1])
    seen = _count_calls(monkeypatch)
    _, mask = _ragged()
    m4 = mask.bool().to(dev)[:, None, None, :].expand(4, 1, 32, 32)
    h = torch.randn(4, 32, 256, device=dev)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        tr(h, attention_mask=m4)
        assert len(entered) == 1
        with enc.triad_key_mask(mask.to(dev)[:, :16]):       # a key mask of another shape
            tr(h, attention_mask=m4)
        assert len(entered) == 2
        with enc.triad_key_mask(mask):                       # a host mask
            tr(h, attention_mask=m4)
        assert len(entered) == 3
    assert "triad_attn_fwd_keymask" not in seen, seen


def _text_embedder(monkeypatch):
    from triad_amd import model as Mdl
    real = Mdl._hf_model
    monkeypatch.setattr(Mdl, "_hf_model", lambda kind, name, cfg=None: real("DistilBertModel", "none/none", dict(SMALL)))
    torch.manual_seed(0)
    return Mdl.TextEmbedder(model_name="none/distilbert").to(dev).train()


@pytest.mark.parametrize("where", ["host", "device"])
def test_text_embedder_takes_the_masked_kernels_for_a_padded_batch(monkeypatch, where):
    """TextEmbedder.forward with a padded batch (mask on the host or on the device): one masked attention
    forward per layer, the stock transformer forward not entered, features finite with gradients."""
    emb = _text_embedder(monkeypatch)
    ids, mask = _ragged()
    if where == "device":
        ids, mask = ids.to(dev), mask.to(dev)
    seen = _count_calls(monkeypatch)
    _forbid_stock(monkeypatch, emb.encoder.transformer)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        feats, m = emb({"input_ids": ids, "attention_mask": mask})
    feats.float().square().sum().backward()
    assert seen.get("triad_attn_fwd_keymask", 0) == SMALL["n_layers"], seen
    assert seen.get("triad_attn_bwd_keymask", 0) == SMALL["n_layers"], seen
    assert "triad_attn_fwd_dropout" not in seen, seen
    assert feats.shape == (4, 32, 512) and bool(torch.isfinite(feats).all())
    assert m.is_cuda and torch.equal(m.cpu(), _ragged()[1])
    assert getattr(emb.encoder.transformer, "_triad_key_mask", None) is None      # the context is closed


def test_text_embedder_drops_a_host_mask_without_padding(monkeypatch):
    """As before: a host mask of ones is dropped, the unmasked kernels run, no masked launch, no packing."""
    emb = _text_embedder(monkeypatch)
    ids, _ = _ragged()
    seen = _count_calls(monkeypatch)
    _forbid_stock(monkeypatch, emb.encoder.transformer)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        feats, m = emb({"input_ids": ids, "attention_mask": torch.ones(4, 32, dtype=torch.long)})
    assert seen.get("triad_attn_fwd_dropout", 0) == SMALL["n_layers"], seen
    assert "triad_attn_fwd_keymask" not in seen and "triad_attn_keymask_pack" not in seen, seen
    assert bool(torch.isfinite(feats).all()) and m.is_cuda
