"""The TRIAD_EINVAL rules of the attention entry points, one assertion per rule, for both kernel families
(csrc/attention.hip: 1 .. 320 tokens; csrc/attention_long.hip: 321 .. 2048). The library validates
before it launches and every call here fails validation, so the fake pointers are never dereferenced
and no device is needed. Used by tests/test_attention_checks_cpu.py and
tests/test_attention_long_checks_cpu.py."""
EINVAL = 1001
FAKE = 4096   # 16-byte aligned, never dereferenced: validation fails first
ROWS = (FAKE, 1 << 20, 192)

# family -> entry points, a valid N, the N just outside the range (and 0), whether the forward / backward
# take (wq, wk, p), whether the kernels read two keep words at a time (8-byte aligned masks)
FAMILIES = {
    "short": dict(fwd="triad_attn_fwd_dropout", bwd="triad_attn_bwd_dropout", mask="triad_attn_dropmask", N=199,
                  bad_N=(0, 321, 2049), drop=True, word_pairs=False),
    "short, no dropout": dict(fwd="triad_attn_fwd", bwd="triad_attn_bwd", mask=None, N=199, bad_N=(0, 321, 2049),
                              drop=False, word_pairs=False),
    "long": dict(fwd="triad_attn_long_fwd", bwd="triad_attn_long_bwd", mask="triad_attn_long_dropmask", N=499,
                 bad_N=(320, 2049, 0), drop=True, word_pairs=True),
}


def lib():
    from triad_amd import _lib
    return _lib.load()


def fwd(family, **over):
    F = FAMILIES[family]
    a = dict(q=ROWS, k=ROWS, v=ROWS, B=2, H=3, N=F["N"], D=64, scale=0.125, wq=None, p=0.0, out=ROWS, lse=FAKE)
    a.update(over)
    drop = (a["wq"], a["p"]) if F["drop"] else ()
    return getattr(lib(), F["fwd"])(*a["q"], *a["k"], *a["v"], a["B"], a["H"], a["N"], a["D"], a["scale"], *drop,
                                    *a["out"], a["lse"], None)


def bwd(family, **over):
    F = FAMILIES[family]
    a = dict(q=ROWS, k=ROWS, v=ROWS, o=ROWS, do=ROWS, dq=ROWS, dk=ROWS, dv=ROWS, lse=FAKE, delta=FAKE, B=2, H=3,
             N=F["N"], D=64, scale=0.125, wq=None, wk=None, p=0.0)
    a.update(over)
    drop = (a["wq"], a["wk"], a["p"]) if F["drop"] else ()
    return getattr(lib(), F["bwd"])(*a["q"], *a["k"], *a["v"], *a["o"], *a["do"], a["lse"], a["B"], a["H"], a["N"],
                                    a["D"], a["scale"], *drop, *a["dq"], *a["dk"], *a["dv"], a["delta"], None)


def mask(family, B=2, H=3, N=None, p=0.1, wq=FAKE, wk=FAKE):
    F = FAMILIES[family]
    return getattr(lib(), F["mask"])(B, H, F["N"] if N is None else N, p, 7, wq, wk, None)


def forward_or_backward_rejects_bad_arguments(family, which):
    F = FAMILIES[family]
    f = (lambda **kw: fwd(family, **kw)) if which == "fwd" else (lambda **kw: bwd(family, **kw))
    tensors = ("q", "k", "v", "out") if which == "fwd" else ("q", "k", "v", "o", "do", "dq", "dk", "dv")
    for N in F["bad_N"]:
        assert f(N=N) == EINVAL, N
    assert f(D=32) == EINVAL
    assert f(D=128) == EINVAL
    assert f(B=0) == EINVAL
    assert f(H=0) == EINVAL
    assert f(B=-1) == EINVAL
    assert f(H=-1) == EINVAL
    assert f(B=257, H=256) == EINVAL                       # B * H = 65792
    for s in (0.0, -0.125, float("inf"), float("-inf"), float("nan")):
        assert f(scale=s) == EINVAL, s
    for t in tensors:
        assert f(**{t: (None, 1 << 20, 192)}) == EINVAL, t          # null
        assert f(**{t: (FAKE + 8, 1 << 20, 192)}) == EINVAL, t      # 8-byte aligned only
        assert f(**{t: (FAKE + 2, 1 << 20, 192)}) == EINVAL, t
        assert f(**{t: (FAKE, (1 << 20) + 4, 192)}) == EINVAL, t    # sB % 8
        assert f(**{t: (FAKE, 1 << 20, 196)}) == EINVAL, t          # sN % 8
        assert f(**{t: (FAKE, 1 << 20, 193)}) == EINVAL, t
    assert f(lse=None) == EINVAL
    if which == "bwd":
        assert f(delta=None) == EINVAL
    if not F["drop"]:
        return
    for p in (-0.1, 1.0, 1.5, float("nan")):
        assert f(p=p) == EINVAL, p
        assert f(p=p, wq=FAKE, wk=FAKE) == EINVAL, p
    if which == "bwd":
        assert f(wq=FAKE, wk=None, p=0.1) == EINVAL                 # one mask without the other
        assert f(wq=None, wk=FAKE, p=0.1) == EINVAL
    if F["word_pairs"]:                                             # keep words are read two at a time
        assert f(wq=FAKE + 4, wk=FAKE, p=0.1) == EINVAL
        if which == "bwd":
            assert f(wq=FAKE, wk=FAKE + 4, p=0.1) == EINVAL


def dropmask_rejects_bad_arguments(family):
    F = FAMILIES[family]
    for N in F["bad_N"]:
        assert mask(family, N=N) == EINVAL, N
    assert mask(family, B=0) == EINVAL
    assert mask(family, H=0) == EINVAL
    assert mask(family, B=-1) == EINVAL
    assert mask(family, B=257, H=256) == EINVAL
    for p in (-0.1, 1.0, 1.5, float("nan")):
        assert mask(family, p=p) == EINVAL, p
    assert mask(family, wq=None) == EINVAL
    assert mask(family, wk=None) == EINVAL
    if F["word_pairs"]:
        assert mask(family, wq=FAKE + 4) == EINVAL
        assert mask(family, wk=FAKE + 4) == EINVAL
