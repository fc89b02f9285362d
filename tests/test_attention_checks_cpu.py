"""The checks of tests/test_attention_conformance_gpu.py bite: a plain-torch fp32 / bf16 emulation of
the three kernels of csrc/attention.hip with their rounding points (bf16 P and dS, fp32 sums,
exp2-based probabilities, fp32 lse and delta; tests/attention_ref.py) passes every per-element bound
of the fp64 reference on every input family, and the same emulation with one planted error pushes at
least one element past a bound or breaks an exact check. No device. Run with -s for the err / bound
figures."""
import pytest
import torch

from tests import attention_abi as ABI
from tests import attention_ref as R

B, H = 2, 3
SCALE = R.f32(R.SCALE)
SIZES = (1, 5, 33, 96, 261, 320)
S_TRUE, S_WRONG = H * 64 + 16, H * 64 + 8   # v's and k's row strides in the conformance test's buffers
CLEAN, PLANTED = {}, {}   # worst err / bound of the clean emulation; weakest detection of each planted error


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nclean emulation, largest err/bound:", ", ".join(f"{k} {v:.3f}" for k, v in sorted(CLEAN.items())))
    print("planted errors on gauss, smallest over N of the largest err/bound:")
    for k, v in PLANTED.items():
        print(f"  {k}: {v:.3g}")


def _note_clean(r, prefix=""):
    for k, v in r.items():
        CLEAN[prefix + k] = max(CLEAN.get(prefix + k, 0.0), v)


def _note_planted(name, r):
    worst = max((v if v == v else float("inf")) for v in r.values())
    PLANTED[name] = min(PLANTED.get(name, float("inf")), worst)


def _keep(N, p):
    return None if p == 0.0 else R.cpu_keep(B, H, N, p, N)


@pytest.fixture(scope="module")
def problems():
    """(family, N, p) -> (case, keep, forward reference, backward inputs o / lse, backward
    reference): built on first use, shared by the tests, never modified."""
    made = {}

    def get(family, N, p=0.0):
        key = (family, N, p)
        if key not in made:
            c = R.case(family, B, H, N, N)
            keep = _keep(N, p)
            fw = R.fwd_ref(c["q"], c["k"], c["v"], SCALE, keep, p)
            o, lse = fw["out"][0].to(R.F32).to(R.BF), fw["lse"][0].to(R.F32)
            bw = R.bwd_ref(c["q"], c["k"], c["v"], o, lse, c["do"], SCALE, keep, p)
            made[key] = (c, keep, fw, o, lse, bw)
        return made[key]
    return get


def _fwd_ratios(c, keep, p, fw, **plant):
    out, lse = R.emul_fwd(c["q"], c["k"], c["v"], SCALE, keep, p, **plant)
    return {"out": R.ratio(out, *fw["out"]), "lse": R.ratio(lse, *fw["lse"])}


def _bwd_ratios(c, keep, p, o, lse, bw, **plant):
    got = R.emul_bwd(c["q"], c["k"], c["v"], o, lse, c["do"], SCALE, keep, p, **plant)
    return {n: R.ratio(t, *bw[n]) for n, t in zip(("dq", "dk", "dv", "delta"), got)}


def _ok(r):
    return all(v == v and v <= 1.0 for v in r.values())


def _fmt(r):
    return " ".join(f"{k} {v:.3g}" for k, v in r.items())


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_clean_emulation_is_inside_every_bound(problems, family, p):
    for N in SIZES:
        c, keep, fw, o, lse, bw = problems(family, N, p)
        rf = _fwd_ratios(c, keep, p, fw)
        rb = _bwd_ratios(c, keep, p, o, lse, bw)
        print(f"clean {family} N {N} p {p}: {_fmt(rf)} {_fmt(rb)}")
        _note_clean(rf)
        _note_clean(rb)
        assert _ok(rf) and _ok(rb), (family, N, p, rf, rb)


@pytest.mark.parametrize("N", [33, 199, 261])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_clean_chain_is_inside_the_widened_bounds(N, p):
    """The emulated forward's own out and lse into the emulated backward, against the backward of
    the fp64 out and lse with the forward's bounds as input errors."""
    for family in R.FAMILIES:
        c, keep = R.case(family, B, H, N, N), _keep(N, p)
        fw = R.fwd_ref(c["q"], c["k"], c["v"], SCALE, keep, p)
        out, lse = R.emul_fwd(c["q"], c["k"], c["v"], SCALE, keep, p)
        bw = R.bwd_ref(c["q"], c["k"], c["v"], fw["out"][0], fw["lse"][0], c["do"], SCALE, keep, p,
                       lse_err=fw["lse"][1], o_err=fw["out"][1])
        r = _bwd_ratios(c, keep, p, out, lse, bw)
        print(f"chain {family} N {N} p {p}: {_fmt(r)}")
        _note_clean(r, "chain.")
        assert _ok(r), (family, N, p, r)


def test_selector_answers_are_exact_in_the_emulation(problems):
    """case() asserts the two selector conditions for every N; the emulation then returns V[perm[q]]
    and dO[q] bit for bit, and 2 V[perm[q]] or ~0 under p = 0.5 by the keep bit of (q, perm[q])."""
    for N in SIZES:
        c, _, fw, o, lse, _ = problems("selector", N)
        out, _ = R.emul_fwd(c["q"], c["k"], c["v"], SCALE)
        assert torch.equal(out, R.selected_rows(c["v"], c["perm"])), N
        dv = R.emul_bwd(c["q"], c["k"], c["v"], o, lse, c["do"], SCALE)[2]
        assert torch.equal(R.selected_rows(dv, c["perm"]), c["do"]), N
        keep = R.cpu_keep(B, H, N, 0.5, N)
        kept = torch.gather(keep, -1, c["perm"][..., None]).squeeze(-1).permute(0, 2, 1)[..., None]   # (B, N, H, 1)
        out, _ = R.emul_fwd(c["q"], c["k"], c["v"], SCALE, keep, 0.5)
        want = 2 * R.selected_rows(c["v"], c["perm"]).float()
        assert torch.equal(out.float()[kept.expand_as(out)], want[kept.expand_as(out)]), N
        assert float((out.float() * ~kept).abs().max()) < 1e-6, N


FWD_PLANTS = {
    "last valid key left out of the softmax": (lambda N: dict(drop_last_key=True), lambda N: N > 1),
    "zero-padded key N counted in l": (lambda N: dict(count_pad_key=True), lambda N: N % 32 != 0),
    "two keys swapped in a 16-key chunk of PV": (lambda N: dict(swap_keys=(N - 5, N - 1) if N < 16 else (17, 21)),
                                                 lambda N: N >= 5),
    "k_sN used for v": (lambda N: dict(v_stride=(S_TRUE, S_WRONG)), lambda N: N > 1),
    "head index off by one": (lambda N: dict(head_shift=1), lambda N: True),
    "lse missing log(l)": (lambda N: dict(lse_no_log=True), lambda N: N > 1),
}
BWD_PLANTS = {
    "delta from 32 of the 64 dims": (dict(delta_half=True), 0.0),
    "dropout bit read at (key, q) in dK/dV": (dict(mask_transposed_dkv=True), 0.5),
    "drop_scale missing from the dV operand": (dict(dv_no_drop_scale=True), 0.1),
    "dq missing the final scale": (dict(dq_no_scale=True), 0.0),
}


@pytest.mark.parametrize("name", list(FWD_PLANTS))
def test_forward_bounds_see_a_planted_error(problems, name):
    """On `gauss` at every N the error applies to (and, printed, on the other families)."""
    plant, applies = FWD_PLANTS[name]
    for N in SIZES:
        if not applies(N):
            continue
        for family in R.FAMILIES:
            c, keep, fw, *_ = problems(family, N)
            r = _fwd_ratios(c, keep, 0.0, fw, **plant(N))
            print(f"{name}: {family} N {N}: {_fmt(r)}")
            if family == "gauss":
                _note_planted(name, r)
                assert not _ok(r), (name, N, r)


@pytest.mark.parametrize("name", list(BWD_PLANTS))
def test_backward_bounds_see_a_planted_error(problems, name):
    plant, p = BWD_PLANTS[name]
    for N in SIZES:
        if N == 1 and "dq" in name:
            continue   # N = 1: dq is 0 with or without the scale
        if N == 1 and "(key, q)" in name:
            continue   # a 1 x 1 mask is its own transpose
        for family in R.FAMILIES:
            c, keep, _, o, lse, bw = problems(family, N, p)
            r = _bwd_ratios(c, keep, p, o, lse, bw, **plant)
            print(f"{name}: {family} N {N}: {_fmt(r)}")
            if family == "gauss":
                _note_planted(name, r)
                assert not _ok(r), (name, N, r)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("family", ["short", "short, no dropout"])
def test_forward_and_backward_reject_bad_arguments(family, which):
    """Every TRIAD_EINVAL rule of triad_attn_fwd_dropout / _bwd_dropout and of triad_attn_fwd / _bwd
    (tests/attention_abi.py; validation comes before any launch, so no device is needed). That this
    family accepts keep words at a 4-byte offset cannot be shown here: an accepted call launches."""
    ABI.forward_or_backward_rejects_bad_arguments(family, which)


def test_dropmask_rejects_bad_arguments():
    """triad_attn_dropmask: the sizes, p (NaN included) and a null wq or wk."""
    ABI.dropmask_rejects_bad_arguments("short")


def test_wrapper_gates():
    """attention.supported and _as_bnhd apply the entry points' rules: a scale that is not finite
    or <= 0 and more than 65535 sequences are unsupported; a view whose base is not 16-byte aligned
    or whose sB / sN is not a multiple of 8 elements is copied, an aligned one is passed as it is."""
    from triad_amd import attention as A

    class Dev:   # supported() reads only these
        is_cuda, dtype = True, torch.bfloat16
    x = Dev()
    assert A.supported(x, 320, 64) and A.supported(x, 1, 64, 0.125, 65535)
    for scale in (0.0, -0.125, float("inf"), float("nan")):
        assert not A.supported(x, 32, 64, scale)
    assert not A.supported(x, 32, 64, 0.125, 65536)
    assert not A.supported(x, 321, 64) and not A.supported(x, 32, 32)
    buf = torch.zeros(4 + 2 * 5 * 3 * 64 + 64, dtype=torch.bfloat16)
    good = buf[:2 * 5 * 192].view(2, 5, 3, 64)
    assert A._as_bnhd(good).data_ptr() == good.data_ptr()
    off = buf[4:4 + 2 * 5 * 192].view(2, 5, 3, 64)                  # storage offset of 4 elements
    assert buf.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 8
    got = A._as_bnhd(off)
    assert got.data_ptr() % 16 == 0 and torch.equal(got, off)
    odd = torch.zeros(2, 5, 3 * 64 + 4, dtype=torch.bfloat16)[:, :, :192].view(2, 5, 3, 64)   # sN = 196
    got = A._as_bnhd(odd)
    assert got.stride(1) % 8 == 0 and got.stride(0) % 8 == 0 and torch.equal(got, odd)
    assert A._as_bnhd(good.transpose(1, 2).contiguous().transpose(1, 2)).is_contiguous()   # (B, H, N, 64) storage
