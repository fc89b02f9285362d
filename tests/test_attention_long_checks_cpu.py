"""CPU checks for the streaming attention kernels of csrc/attention_long.hip (321 <= N <= 2048):

* every TRIAD_EINVAL rule of triad_attn_long_fwd / _bwd / _dropmask, one assertion per rule
  (tests/attention_abi.py: the library validates before it launches, so no device is needed);
* attention.supported_long, LONG_ROUTE and the routing of the wrappers at N = 320, 321, 2048, 2049;
* the checks of tests/test_attention_long_conformance_gpu.py bite: the chunked fp32 / bf16 emulations
  of the three kernels (tests/attention_long_ref.py) pass every per-element bound on the five input
  families of attention_ref and on `rising`, and the same emulations with one planted error push at
  least one element of `gauss` past a bound. Run with -s for the err / bound figures.
B = 2, H = 3 up to N = 499; B = 1, H = 2 at N = 1374 (the fp64 references stay under a second)."""
import pytest
import torch

from tests import attention_abi as ABI
from tests import attention_long_ref as LR
from tests import attention_ref as R

SCALE = R.f32(R.SCALE)
SIZES = (321, 499, 1374)
CLEAN, PLANTED = {}, {}


def _bh(N):
    return (2, 3) if N < 1000 else (1, 2)


# ---- the entry points' argument checks -------------------------------------------------------------

@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_forward_and_backward_reject_bad_arguments(which):
    ABI.forward_or_backward_rejects_bad_arguments("long", which)


def test_dropmask_rejects_bad_arguments():
    ABI.dropmask_rejects_bad_arguments("long")


def test_new_entry_points_are_backbone_only():
    """bench.TRACKED (the hot-path entry points) stays what it was."""
    from triad_amd import _lib
    names = {"triad_attn_long_fwd", "triad_attn_long_bwd", "triad_attn_long_dropmask"}
    assert names <= set(_lib.SIGNATURES) and names <= _lib.BACKBONE_ENTRY_POINTS
    assert not names & set(_lib.hot_path_entry_points())


# ---- the wrappers' gates and routing ------------------------------------------------------------------

class Dev:   # supported*() read only these
    is_cuda, dtype = True, torch.bfloat16


def test_supported_long_and_route():
    from triad_amd import attention as A
    x = Dev()
    assert A.LONG_ROUTE[0] >= 321 and A.LONG_ROUTE[1] <= A.MAX_TOKENS_LONG == 2048 and A.MAX_TOKENS == 320
    lo, hi = A.LONG_ROUTE
    assert A.supported_long(x, lo, 64) and A.supported_long(x, hi, 64, 0.125, 65535)
    assert not A.supported_long(x, 320, 64) and not A.supported_long(x, 2049, 64)
    assert not A.supported_long(x, lo - 1, 64) and not A.supported_long(x, hi + 1, 64)
    assert not A.supported_long(x, lo, 32) and not A.supported_long(x, lo, 64, 0.125, 65536)
    for scale in (0.0, -0.125, float("inf"), float("nan")):
        assert not A.supported_long(x, lo, 64, scale)

    class F32Dev:
        is_cuda, dtype = True, torch.float32

    class Cpu:
        is_cuda, dtype = False, torch.bfloat16
    assert not A.supported_long(F32Dev(), lo, 64) and not A.supported_long(Cpu(), lo, 64)
    assert not A.supported(x, 321, 64)   # the short gate is what it was


class _Stub(torch.Tensor):
    """A CPU bf16 tensor that says it is on the device (the gates read is_cuda and dtype)."""
    @property
    def is_cuda(self):
        return True


@pytest.mark.parametrize("N,want", [(320, "short"), (321, "long"), (2048, "long"), (2049, "torch")])
def test_routing(monkeypatch, N, want):
    """sdpa, hf_attention_forward and vit.Attention with the library call patched (every entry point
    that reaches attention.call is recorded): 320 tokens take the whole-sequence forward, 321 and 2048
    the streaming one (if LONG_ROUTE holds them), 2049 PyTorch; one forward per call, nothing else."""
    from triad_amd import attention as A
    from triad_amd import vit
    if want == "long" and not A.LONG_ROUTE[0] <= N <= A.LONG_ROUTE[1]:
        want = "torch"
    calls = []
    family = {"triad_attn_fwd_dropout": "short", "triad_attn_long_fwd": "long"}
    monkeypatch.setattr(A, "call", lambda name, *args: calls.append(family.get(name, name)))
    monkeypatch.setattr(A, "ptr", lambda t: None)
    monkeypatch.setattr(A, "stream_ptr", lambda device=None: None)
    monkeypatch.setattr(A.F, "scaled_dot_product_attention",
                        lambda q, k, v, **kw: (calls.append("torch"), torch.zeros_like(q))[1])
    monkeypatch.setattr(A, "_as_bnhd", lambda t: t)
    q = torch.zeros(1, 2, N, 64, dtype=torch.bfloat16).as_subclass(_Stub)
    assert q.is_cuda
    A.sdpa(q, q, q)
    assert calls == [want], ("sdpa", N, calls)
    del calls[:]
    att = vit.Attention(128, 2).to(torch.bfloat16)

    class QKV(torch.nn.Module):
        def forward(self, x):
            return torch.zeros(1, N, 384, dtype=torch.bfloat16).as_subclass(_Stub)
    att.qkv = QKV()
    att(torch.zeros(1, N, 128, dtype=torch.bfloat16))
    assert calls == [want], ("vit.Attention", N, calls)
    del calls[:]
    try:
        import transformers.integrations.sdpa_attention as S
    except ImportError:
        return
    monkeypatch.setattr(S, "sdpa_attention_forward",
                        lambda m, q, k, v, mask, **kw: (calls.append("torch"), (q.transpose(1, 2), None))[1])
    mod = torch.nn.Module()
    mod.is_causal = False
    mod.eval()
    A.hf_attention_forward(mod, q, q, q, None, scaling=0.125)
    assert calls == [want], ("hf_attention_forward", N, calls)


# ---- the bounds against the emulations ------------------------------------------------------------------

@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nclean emulation, largest err/bound:", ", ".join(f"{k} {v:.3f}" for k, v in sorted(CLEAN.items())))
    print("planted errors on gauss, smallest over N of the largest err/bound:")
    for k, v in PLANTED.items():
        print(f"  {k}: {v:.3g}")


def _keep(N, p):
    return None if p == 0.0 else R.cpu_keep(*_bh(N), N, p, N)


@pytest.fixture(scope="module")
def problems():
    """(family, N, p) -> (case, keep, forward reference, backward inputs o / lse, backward reference):
    built on first use, shared, never modified."""
    made = {}

    def get(family, N, p=0.0):
        key = (family, N, p)
        if key not in made:
            c = LR.case(family, *_bh(N), N, N)
            keep = _keep(N, p)
            fw = LR.fwd_ref(c["q"], c["k"], c["v"], SCALE, keep, p)
            o, lse = fw["out"][0].to(R.F32).to(R.BF), fw["lse"][0].to(R.F32)
            bw = LR.bwd_ref(c["q"], c["k"], c["v"], o, lse, c["do"], SCALE, keep, p)
            made[key] = (c, keep, fw, o, lse, bw)
        return made[key]
    return get


def _fwd_ratios(c, keep, p, fw, **plant):
    out, lse = LR.emul_fwd(c["q"], c["k"], c["v"], SCALE, keep, p, **plant)
    return {"out": R.ratio(out, *fw["out"]), "lse": R.ratio(lse, *fw["lse"])}


def _bwd_ratios(c, keep, p, o, lse, bw, **plant):
    got = LR.emul_bwd(c["q"], c["k"], c["v"], o, lse, c["do"], SCALE, keep, p, **plant)
    return {n: R.ratio(t, *bw[n]) for n, t in zip(("dq", "dk", "dv", "delta"), got)}


def _ok(r):
    return all(v == v and v <= 1.0 for v in r.values())


def _fmt(r):
    return " ".join(f"{k} {v:.3g}" for k, v in r.items())


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("family", LR.FAMILIES)
def test_clean_emulation_is_inside_every_bound(problems, family, N):
    for p in (0.0, 0.1, 0.5):
        c, keep, fw, o, lse, bw = problems(family, N, p)
        rf = _fwd_ratios(c, keep, p, fw)
        rb = _bwd_ratios(c, keep, p, o, lse, bw)
        print(f"clean {family} N {N} p {p}: {_fmt(rf)} {_fmt(rb)}")
        for k, v in {**rf, **rb}.items():
            CLEAN[k] = max(CLEAN.get(k, 0.0), v)
        assert _ok(rf) and _ok(rb), (family, N, p, rf, rb)


def test_the_online_terms_add_a_few_per_cent_at_most():
    """The streaming bound against attention_ref's on the same reference: never smaller, and the out
    bound grows by under 3 % (the bf16 r terms still dominate); `rising` does rise chunk by chunk."""
    for family in ("gauss", "rising", "offset"):
        c = LR.case(family, 1, 2, 1374, 1374)
        long_, short = LR.fwd_ref(c["q"], c["k"], c["v"], SCALE), R.fwd_ref(c["q"], c["k"], c["v"], SCALE)
        g = long_["out"][1] / short["out"][1]
        assert float(g.min()) >= 1.0 and float(g.max()) < 1.03, (family, float(g.min()), float(g.max()))
        assert bool((long_["lse"][1] >= short["lse"][1]).all())
    c = LR.case("rising", 1, 2, 1374, 1374)
    n = LR.rises(c["q"], c["k"], SCALE)
    print(f"rising N 1374: the running max rises in {n:.1f} of {LR.nch(1374) - 1} later chunks on average")
    assert n > 0.8 * (LR.nch(1374) - 1)


FWD_PLANTS = {
    "a skipped rescale": lambda N: dict(skip_rescale=LR.nch(N) // 2),
    "O rescaled but not l": lambda N: dict(l_not_rescaled=True),
    "the last chunk left out": lambda N: dict(drop_last_chunk=True),
    "the last chunk's padded keys counted in l": lambda N: dict(count_pad_keys=True),
    "chunk c of K with chunk c - 1 of V": lambda N: dict(v_lag=True),
}
BWD_PLANTS = {
    "dkv reads lse / delta of query chunk 0": (dict(stat_chunk0=True), 0.0),
    "drop_scale missing from dV": (dict(dv_no_drop_scale=True), 0.1),
    "dq without the final scale": (dict(dq_no_scale=True), 0.0),
}


def _planted(name, r):
    worst = max((v if v == v else float("inf")) for v in r.values())
    PLANTED[name] = min(PLANTED.get(name, float("inf")), worst)


@pytest.mark.parametrize("name", list(FWD_PLANTS))
def test_forward_bounds_see_a_planted_error(problems, name):
    for N in SIZES:   # none is a multiple of 64: every size has padded keys
        c, keep, fw, *_ = problems("gauss", N)
        r = _fwd_ratios(c, keep, 0.0, fw, **FWD_PLANTS[name](N))
        print(f"{name}: gauss N {N}: {_fmt(r)}")
        _planted(name, r)
        assert not _ok(r), (name, N, r)


@pytest.mark.parametrize("name", list(BWD_PLANTS))
def test_backward_bounds_see_a_planted_error(problems, name):
    plant, p = BWD_PLANTS[name]
    for N in SIZES:
        c, keep, _, o, lse, bw = problems("gauss", N, p)
        r = _bwd_ratios(c, keep, p, o, lse, bw, **plant)
        print(f"{name}: gauss N {N}: {_fmt(r)}")
        _planted(name, r)
        assert not _ok(r), (name, N, r)


def test_bounds_see_keep_words_indexed_with_the_short_forms_words_per_row(problems):
    """2 ceil(N / 64) words per row against ceil(N / 32): they differ where the tile count is odd
    (N = 321: 12 / 11, N = 1374: 44 / 43), and there the forward and the backward both fail; at
    N = 499 (16 / 16) the two layouts are one."""
    assert LR.wpr(499) == R.nkt(499)
    for N in (321, 1374):
        assert LR.wpr(N) == R.nkt(N) + 1
        c, keep, fw, o, lse, bw = problems("gauss", N, 0.5)
        rf = _fwd_ratios(c, keep, 0.5, fw, short_words=True)
        rb = _bwd_ratios(c, keep, 0.5, o, lse, bw, short_words=True)
        print(f"short words: gauss N {N}: {_fmt(rf)} {_fmt(rb)}")
        _planted("keep words with the short form's words per row (fwd)", rf)
        _planted("keep words with the short form's words per row (bwd)", rb)
        assert not _ok(rf) and not _ok(rb), (N, rf, rb)
