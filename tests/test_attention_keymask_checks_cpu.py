"""The checks of tests/test_attention_keymask_conformance_gpu.py bite: the fp32 / bf16 emulation of the
three masked kernels (tests/attention_keymask_ref.py; the kernels' rounding points, selects and guards,
fed the packed words with the bits past N set) passes every bound of the compacted fp64 reference on
every mask family, and the same emulation with one planted error pushes an element past a bound,
breaks an exact zero or returns something non-finite. Then the TRIAD_EINVAL rules of the three new
entry points, with fake pointers and no device. Run with -s for the err / bound figures."""
import numpy as np
import pytest
import torch

from tests import attention_abi as ABI
from tests import attention_keymask_ref as KM
from tests import attention_ref as R

B, H = 3, 2
SCALE = R.f32(R.SCALE)
SIZES = (1, 33, 96, 199, 320)
CLEAN, PLANTED = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nclean masked emulation, largest err/bound:", ", ".join(f"{k} {v:.3f}" for k, v in sorted(CLEAN.items())))
    print("planted errors, smallest over the detecting cases of the largest err/bound (nan = non-finite output):")
    for k, v in PLANTED.items():
        print(f"  {k}: {v:.3g}")


@pytest.fixture(scope="module")
def problems():
    """(mask family, variant, N, p) -> (case, mask, words, keep, forward reference, o, lse, backward
    reference): built on first use, shared, never modified."""
    made = {}

    def get(family, i, N, p=0.0):
        key = (family, i, N, p)
        if key not in made:
            c = R.case("gauss", B, H, N, N)
            mask = KM.masks(family, B, N, N)[i]
            keep = None if p == 0.0 else R.cpu_keep(B, H, N, p, N)
            fw = KM.fwd_ref(c["q"], c["k"], c["v"], SCALE, mask, keep, p)
            o, lse = fw["out"][0].to(R.F32).to(R.BF), fw["lse"][0].to(R.F32)
            bw = KM.bwd_ref(c["q"], c["k"], c["v"], o, lse, c["do"], SCALE, mask, keep, p)
            made[key] = (c, mask, KM.pack_words(mask, past_n=1), keep, fw, o, lse, bw)
        return made[key]
    return get


def _ratios(prob, p, plant=None):
    c, mask, words, keep, fw, o, lse, bw = prob
    out, ls = KM.emul_fwd(c["q"], c["k"], c["v"], SCALE, words, keep, p, plant)
    got = KM.emul_bwd(c["q"], c["k"], c["v"], o, lse, c["do"], SCALE, words, keep, p, plant)
    r = {"out": KM.ratio(out, *fw["out"]), "lse": KM.ratio(ls, *fw["lse"])}
    r.update({n: KM.ratio(t, *bw[n]) for n, t in zip(("dq", "dk", "dv", "delta"), got)})
    # the exact part: rows of cleared keys are +0 bit for bit
    cleared = ~mask[:, :, None, None].expand(B, mask.shape[1], H, 64)
    for n, t in (("dk", got[1]), ("dv", got[2])):
        if bool((t.view(torch.int16)[cleared] != 0).any()):
            r[n] = float("nan")
    return r


def _ok(r):
    return all(v == v and v <= 1.0 for v in r.values())


def _fmt(r):
    return " ".join(f"{k} {v:.3g}" for k, v in r.items())


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("family", KM.MASK_FAMILIES)
def test_clean_emulation_is_inside_every_bound(problems, family, p):
    for N in SIZES:
        for i in range(len(KM.masks(family, B, N, N))):
            r = _ratios(problems(family, i, N, p), p)
            print(f"clean {family}[{i}] N {N} p {p}: {_fmt(r)}")
            for k, v in r.items():
                CLEAN[k] = max(CLEAN.get(k, 0.0), v)
            assert _ok(r), (family, i, N, p, r)


def test_packing_restatement():
    """Bit j of word kt is key 32 kt + j; bits past N are the given filler; any non-zero byte keeps."""
    m = torch.zeros(2, 33, dtype=torch.uint8)
    m[0, 0], m[0, 31], m[1, 32], m[1, 5] = 1, 7, 255, 2
    w = KM.pack_words(m)
    assert w.dtype == np.uint32 and w.shape == (2, 2)
    assert w.tolist() == [[0x80000001, 0], [1 << 5, 1]]
    assert KM.pack_words(m, past_n=1).tolist() == [[0x80000001, 0xFFFFFFFE], [1 << 5, 0xFFFFFFFF]]
    assert KM.words_tensor(w).tolist() == [[-(2 ** 31) + 1, 0], [32, 1]]


# plant -> (mask family, p, the sizes it applies to)
WHERE = {
    "mask ignored": ("scattered", 0.0, lambda N: N > 1),
    "word row taken by bh instead of b": ("scattered", 0.0, lambda N: N > 1),
    "bit order reversed within a word": ("prefix", 0.0, lambda N: N > 1),
    "bits past N honoured": ("scattered", 0.0, lambda N: N % 32 != 0),
    "a cleared key counted in l": ("scattered", 0.0, lambda N: N > 1),
    "dkv kernel reads the query's bit": ("scattered", 0.5, lambda N: N > 1),
    "dk / dv of a cleared key not zeroed": ("prefix", 0.0, lambda N: N > 1),
    "empty sample produces NaN": ("empty", 0.0, lambda N: True),
}


@pytest.mark.parametrize("plant", KM.PLANTS)
def test_bounds_see_a_planted_error(problems, plant):
    family, p, applies = WHERE[plant]
    for N in SIZES:
        if not applies(N):
            continue
        seen = []
        for i in range(len(KM.masks(family, B, N, N))):
            r = _ratios(problems(family, i, N, p), p, plant)
            print(f"{plant}: {family}[{i}] N {N}: {_fmt(r)}")
            seen.append(r)
        # prefix has variants whose lengths are all N or fall on no boundary the error needs: one must see it
        bad = [r for r in seen if not _ok(r)]
        assert bad, (plant, N, seen)
        worst = max(max((v if v == v else float("inf")) for v in r.values()) for r in bad)
        PLANTED[plant] = min(PLANTED.get(plant, float("inf")), worst)


# ---- TRIAD_EINVAL, before any launch: fake pointers, no device ------------------------------------------------

def _fwd(**over):
    a = dict(q=ABI.ROWS, k=ABI.ROWS, v=ABI.ROWS, B=B, H=H, N=199, D=64, scale=0.125, wq=None, p=0.0, km=ABI.FAKE,
             out=ABI.ROWS, lse=ABI.FAKE)
    a.update(over)
    return ABI.lib().triad_attn_fwd_keymask(*a["q"], *a["k"], *a["v"], a["B"], a["H"], a["N"], a["D"], a["scale"],
                                            a["wq"], a["p"], a["km"], *a["out"], a["lse"], None)


def _bwd(**over):
    a = dict(q=ABI.ROWS, k=ABI.ROWS, v=ABI.ROWS, o=ABI.ROWS, do=ABI.ROWS, dq=ABI.ROWS, dk=ABI.ROWS, dv=ABI.ROWS,
             lse=ABI.FAKE, delta=ABI.FAKE, B=B, H=H, N=199, D=64, scale=0.125, wq=None, wk=None, p=0.0, km=ABI.FAKE)
    a.update(over)
    return ABI.lib().triad_attn_bwd_keymask(*a["q"], *a["k"], *a["v"], *a["o"], *a["do"], a["lse"], a["B"], a["H"],
                                            a["N"], a["D"], a["scale"], a["wq"], a["wk"], a["p"], a["km"], *a["dq"],
                                            *a["dk"], *a["dv"], a["delta"], None)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_keymask_entry_points_reject_bad_arguments(which):
    """Every rule of the _dropout forms, with a key mask present, and a km that is not 4-byte aligned."""
    f = _fwd if which == "fwd" else _bwd
    tensors = ("q", "k", "v", "out") if which == "fwd" else ("q", "k", "v", "o", "do", "dq", "dk", "dv")
    E = ABI.EINVAL
    for N in (0, 321, 2049):
        assert f(N=N) == E, N
    assert f(D=32) == E
    assert f(D=128) == E
    assert f(B=0) == E
    assert f(H=0) == E
    assert f(B=-1) == E
    assert f(H=-1) == E
    assert f(B=257, H=256) == E
    for s in (0.0, -0.125, float("inf"), float("-inf"), float("nan")):
        assert f(scale=s) == E, s
    for t in tensors:
        assert f(**{t: (None, 1 << 20, 192)}) == E, t
        assert f(**{t: (ABI.FAKE + 8, 1 << 20, 192)}) == E, t
        assert f(**{t: (ABI.FAKE + 2, 1 << 20, 192)}) == E, t
        assert f(**{t: (ABI.FAKE, (1 << 20) + 4, 192)}) == E, t
        assert f(**{t: (ABI.FAKE, 1 << 20, 196)}) == E, t
        assert f(**{t: (ABI.FAKE, 1 << 20, 193)}) == E, t
    assert f(lse=None) == E
    if which == "bwd":
        assert f(delta=None) == E
        assert f(wq=ABI.FAKE, wk=None, p=0.1) == E
        assert f(wq=None, wk=ABI.FAKE, p=0.1) == E
    for p in (-0.1, 1.0, 1.5, float("nan")):
        assert f(p=p) == E, p
        assert f(p=p, wq=ABI.FAKE, wk=ABI.FAKE) == E if which == "bwd" else f(p=p, wq=ABI.FAKE) == E, p
    assert f(km=ABI.FAKE + 2) == E
    assert f(km=ABI.FAKE + 1) == E
    assert f(km=ABI.FAKE + 3) == E


def test_keymask_pack_rejects_bad_arguments():
    pack = ABI.lib().triad_attn_keymask_pack
    E = ABI.EINVAL
    assert pack(None, 3, 33, ABI.FAKE, None) == E          # null mask
    assert pack(ABI.FAKE, 3, 33, None, None) == E          # null words
    assert pack(ABI.FAKE, 3, 33, ABI.FAKE + 2, None) == E  # words off 4 bytes
    assert pack(ABI.FAKE, 0, 33, ABI.FAKE, None) == E
    assert pack(ABI.FAKE, -1, 33, ABI.FAKE, None) == E
    assert pack(ABI.FAKE, 3, 0, ABI.FAKE, None) == E
    assert pack(ABI.FAKE, 3, 321, ABI.FAKE, None) == E


def test_wrappers_refuse_a_mask_past_320_tokens():
    """attention._key_words is the gate of attention_bnhd / attention_qkv: a mask with N > 320 raises before
    anything touches a device; None passes through."""
    from triad_amd import attention as A
    from triad_amd._lib import TriadError
    assert A._key_words(None, 2, 321) is None
    with pytest.raises(TriadError, match="take no mask"):
        A._key_words(torch.ones(2, 321, dtype=torch.bool), 2, 321)
    with pytest.raises(TriadError, match="expected"):
        A._key_words(torch.ones(2, 40, dtype=torch.bool), 2, 33)
