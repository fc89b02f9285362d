"""The projection-head conformance bounds against emulations of the kernels, no device needed
(tests/projhead_ref.py holds the references, the bounds with their derivation and the emulations):

(a) every emulation lies inside every bound at every shape tests/test_projhead_conformance_gpu.py runs,
    and the same emulation with ONE planted error falls outside a bound or breaks an identity -- each
    planted error its own test;
(b) the rejection rules of the entry points, through the loaded library with fake 16-byte-aligned
    pointers that are never dereferenced: validation returns TRIAD_EINVAL (1001) before any launch. One
    assertion per rule.
"""
import ctypes
import functools
import os

import pytest
import torch

from tests import projhead_ref as R

EINVAL = 1001
D = R.D
EPS = R.f32(R.EPS)


# ---- (a) clean emulations and planted errors ---------------------------------------------------------

def _zero_pad(t, M):
    return not bool(t[M:].float().abs().sum())


def _fwd(M, H, gemm1=None, ln=None, gemm2=None):
    """{name: inside its bound / identity holds} for the emulated forward chain, each stage referenced
    from the emulation's own previous stage; the keyword dicts plant an error in one stage."""
    c = R.head_case(M, H)
    y1 = R.emul_rowgemm(c["h"], c["W1"], c["b1"], **(gemm1 or {}))
    lnv, mean, rstd = R.emul_ln_fwd(y1[:M], c["gamma"], c["beta"], EPS, "panel", **(ln or {}))
    y = R.emul_rowgemm(lnv, c["W2"], c["b2"], **(gemm2 or {}))
    want = R.ln_fwd_ref(y1[:M], c["gamma"], c["beta"], EPS, R.H_PANEL)
    return {"y1": R.passes(y1[:M], *R.gemm_bias_ref(c["h"], c["W1"], c["b1"])),
            "mean": R.passes(mean, *want["mean"]), "rstd": R.passes(rstd, *want["rstd"]),
            "ln": R.passes(lnv, *want["ln"]),
            "y": R.passes(y[:M], *R.gemm_bias_ref(lnv, c["W2"], c["b2"])),
            "pad": _zero_pad(y1, M) and _zero_pad(y, M)}


@functools.lru_cache(maxsize=None)
def _bwd_operands(M):
    c = R.bwd_case(M)
    return c["dy"], c["W2"], c["y1"], c["mean"], c["rstd"], c["gamma"]


def _bwd(M, gemm=None, epi=None):
    dy, W2, y1, mean, rstd, gamma = _bwd_operands(M)
    W2t = W2.t().contiguous()                       # dln = dy W2 = dy (W2^T)^T
    dln = R.emul_rowgemm(dy, W2t, None, **(gemm or {}))[:M]
    dy1, part = R.emul_panel_ln_bwd(dln, y1, mean, rstd, gamma, **(epi or {}))
    want = R.ln_bwd_ref(dln, y1, mean, rstd, gamma, R.H_PANEL, R.row_groups_panel(M), dy1_got=dy1[:M])
    res = {"dln": R.passes(dln, *R.gemm_bias_ref(dy, W2t)), "dy1": R.passes(dy1[:M], *want["dy1"]),
           "pad": _zero_pad(dy1, M)}
    for i, k in enumerate(("dgamma", "dbeta", "db1")):
        res[k] = R.passes(part[:, i], *want[k])
        res["total." + k] = R.passes(part[:, i].double().sum(0), *want["total." + k])
    return res


def _all(res):
    bad = [k for k, ok in res.items() if not ok]
    assert not bad, f"outside its bound: {bad}"


@pytest.mark.parametrize("M,H", R.FWD_CASES)
def test_forward_emulation_inside_every_bound(M, H):
    _all(_fwd(M, H))


@pytest.mark.parametrize("H", R.ADDR_HS)
def test_strided_layouts_address_the_same_rows(H):
    """The four layouts of the GPU file hold the same rows under the kernel's address formula (and NaN
    everywhere else), so one reference serves them all; the emulation at their M = 150."""
    h = R.head_case(R.ADDR_M, H)["h"]
    for form in R.ADDR_FORMS:
        buf, off, lda, n_per, bstride = R.strided_rows(h, form)
        assert torch.equal(R.gather_rows(buf, off, lda, n_per, bstride, R.ADDR_M, H), h), form
        assert int(torch.isfinite(buf.float()).sum()) == h.numel(), form
        assert (2 * off) % 16 == 0 and lda % 8 == 0 and bstride % 8 == 0, form
    _all(_fwd(R.ADDR_M, H))


@pytest.mark.parametrize("M", R.BWD_MS)
def test_backward_emulation_inside_every_bound(M):
    _all(_bwd(M))


@pytest.mark.parametrize("M", R.LN_FWD_MS)
def test_ln_fwd_emulation_inside_every_bound(M):
    c = R.ln_case(M)
    ln, mean, rstd = R.emul_ln_fwd(c["y1"], c["gamma"], c["beta"], EPS, "wave")
    want = R.ln_fwd_ref(c["y1"], c["gamma"], c["beta"], EPS, R.H_WAVE)
    assert R.passes(mean, *want["mean"]) and R.passes(rstd, *want["rstd"]) and R.passes(ln, *want["ln"])


@pytest.mark.parametrize("M", R.LN_BWD3_MS)
def test_ln_bwd3_emulation_inside_every_bound(M):
    c = R.ln_case(M)
    mean, rstd = R.stats_f32(c["y1"], EPS)
    for nb in R.ln_bwd3_blocks(M):
        dy1, part = R.emul_ln_bwd3(c["dln"], c["y1"], mean, rstd, c["gamma"], nb)
        want = R.ln_bwd_ref(c["dln"], c["y1"], mean, rstd, c["gamma"], R.H_WAVE, R.row_groups_bwd3(M, nb), dy1)
        assert R.passes(dy1, *want["dy1"]), nb
        for i, k in enumerate(("dgamma", "dbeta", "db1")):
            assert R.passes(part[:, i], *want[k]), (nb, k)
            assert R.passes(part[:, i].double().sum(0), *want["total." + k]), (nb, k)
        idle = [b for b in range(nb) if 4 * b >= M]
        assert not bool(part[idle].abs().sum()), nb


@pytest.mark.parametrize("S,n", R.SLAB_CASES)
def test_sum_slabs_emulation_inside_every_bound(S, n):
    slabs, alpha = R.slab_case(S, n)
    for a in (1.0, float(alpha)):
        for ob in (0, 1):
            assert R.passes(R.emul_sum_slabs(slabs, a, ob), *R.sum_slabs_ref(slabs, a, ob)), (a, ob)


def test_sum_slabs_cases_reach_both_kernels():
    paths = {(R.slab_path(S, n), S % 4 != 0) for S, n in R.SLAB_CASES}
    assert paths == {("reduce", False), ("reduce", True), ("stream", False), ("stream", True)}
    assert R.slab_path(16, 16384) == "reduce" and R.slab_path(15, 16384) == "stream"
    assert R.slab_path(16, 16385) == "stream"


@pytest.mark.parametrize("cols", R.COLSUM_COLS)
def test_colsum_dma_emulation_inside_every_bound(cols):
    alpha = R.f32(0.37)
    for rows in R.COLSUM_ROWS:
        X = R.colsum_case(rows, cols)
        for ob in (0, 1):
            assert R.passes(R.emul_colsum_dma(X, alpha, ob), *R.colsum_ref(X, alpha, ob)), (rows, ob)


def test_colsum_dma_splits_rule():
    """The Python restatement against the library's own count (host only)."""
    L = _lib()
    for rows in R.COLSUM_ROWS + (8192, 65536):
        for cols in R.COLSUM_COLS + (768, 2304):
            assert L.triad_colsum_dma_splits(rows, cols) == R.colsum_dma_splits(rows, cols), (rows, cols)
    assert R.colsum_dma_splits(200, 256) > 1     # the GPU file's shapes reach a multi-split first pass


# planted errors: each one its own test, at shapes of the GPU file

def test_planted_last_k_tile_dropped():
    for M, H in ((129, 32), (129, 96), (129, 160), (129, 224), (300, 1024)):
        assert not _fwd(M, H, gemm1=dict(drop_last_ktile=True))["y1"], (M, H)
    assert not _fwd(129, 768, gemm2=dict(drop_last_ktile=True))["y"]
    assert not _bwd(129, gemm=dict(drop_last_ktile=True))["dln"]


def test_planted_bias_added_after_the_rounding():
    assert not _fwd(129, 768, gemm1=dict(bias_after=True))["y1"]
    assert not _fwd(129, 768, gemm2=dict(bias_after=True))["y"]


def test_planted_unbiased_variance():
    res = _fwd(129, 768, ln=dict(unbiased=True))
    assert not res["rstd"] and res["mean"]
    c = R.ln_case(130)
    _, _, rstd = R.emul_ln_fwd(c["y1"], c["gamma"], c["beta"], EPS, "wave", unbiased=True)
    assert not R.passes(rstd, *R.ln_fwd_ref(c["y1"], c["gamma"], c["beta"], EPS, R.H_WAVE)["rstd"])


def test_planted_pad_row_counted_into_dbeta():
    for M in (1, 127, 129, 300):
        res = _bwd(M, epi=dict(pad_row_in_dbeta=True))
        assert not res["dbeta"] and not res["total.dbeta"] and res["dgamma"] and res["db1"], M


def test_planted_last_row_copied_into_the_pad_rows():
    assert not _fwd(129, 768, gemm1=dict(copy_last_row_to=True))["pad"]
    assert not _bwd(129, epi=dict(copy_last_row_to_pad=True))["pad"]


def test_planted_dgamma_summed_from_g():
    for M in R.BWD_MS:
        res = _bwd(M, epi=dict(dgamma_from_g=True))
        assert not res["dgamma"] and not res["total.dgamma"] and res["dbeta"] and res["dy1"], M


def test_planted_two_columns_swapped_in_a_4_column_group():
    """One 8-byte row segment of the last valid row (the ~1e-3 relative L2 error at 130 x 512 that a
    whole-tensor bar lets through)."""
    assert not _fwd(129, 768, gemm1=dict(swap_cols=(128, 508)))["y1"]
    assert not _fwd(300, 768, gemm2=dict(swap_cols=(299, 64)))["y"]


def test_planted_statistics_of_row_r_plus_16():
    res = _fwd(129, 768, ln=dict(stat_shift=16))
    assert not res["ln"] and res["mean"] and res["rstd"]


def test_planted_sum_slabs_skips_the_remainder():
    for S, n in ((3, 65), (5, 1536), (15, 16384), (17, 16385)):
        slabs, _ = R.slab_case(S, n)
        assert R.slab_path(S, n) == "stream"
        assert not R.passes(R.emul_sum_slabs(slabs, 1.0, 0, skip_remainder=True), *R.sum_slabs_ref(slabs, 1.0, 0)), S


def test_planted_colsum_dma_sums_the_masked_lanes():
    for cols in (8, 248, 264, 520):
        X = R.colsum_case(65, cols)
        assert not R.passes(R.emul_colsum_dma(X, 1.0, 0, sum_masked=True), *R.colsum_ref(X, 1.0, 0)), cols


def test_planted_lane_pair_swapped_in_a_packed_fragment():
    W = R.weight_case(32)
    good = R.wpack_ref(W)
    assert not torch.equal(R.wpack_ref(W, swap_lanes=(2, 3)), good)
    # the formula itself, element by element at a few fragments: (kt, w, cb, l, i) of the kernel's comment
    W = R.weight_case(768)
    P = R.wpack_ref(W)
    for kt, w, cb, l, i in ((0, 0, 0, 0, 0), (23, 7, 3, 63, 7), (5, 2, 1, 37, 3), (11, 4, 2, 16, 0)):
        assert P[(((kt * 8 + w) * 4 + cb) * 64 + l) * 8 + i] == W[64 * w + 16 * cb + (l & 15), 32 * kt + 8 * (l >> 4) + i]
    assert torch.equal(P.sort().values, W.reshape(-1).sort().values)


# ---- (b) rejection rules -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _lib():
    from triad_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


FAKE = 4096        # 16-byte aligned, never dereferenced: validation fails first
NANF = float("nan")
INF = float("inf")


def test_rowpanel_entry_points_reject_unsafe_calls():
    L = _lib()

    def fused(h=FAKE, M=129, H=96, lda=96, n_per=129, bstride=0, W1p=FAKE, b1=FAKE, gamma=FAKE, beta=FAKE, eps=1e-5,
              W2p=FAKE, b2=FAKE, y1=FAKE, ln=FAKE, mean=FAKE, rstd=FAKE, y=FAKE):
        return L.triad_projhead_fwd(h, M, H, lda, n_per, bstride, W1p, b1, gamma, beta, eps, W2p, b2, y1, ln, mean,
                                    rstd, y, None)

    def half(h=FAKE, M=129, H=96, lda=96, n_per=129, bstride=0, W1p=FAKE, b1=FAKE, gamma=FAKE, beta=FAKE, eps=1e-5,
             y1=FAKE, ln=FAKE, mean=FAKE, rstd=FAKE):
        return L.triad_projhead_ln_fwd(h, M, H, lda, n_per, bstride, W1p, b1, gamma, beta, eps, y1, ln, mean, rstd, None)

    def gemm(A=FAKE, M=129, K=512, lda=512, Bp=FAKE, bias=FAKE, C=FAKE):
        return L.triad_rowgemm_bias(A, M, K, lda, Bp, bias, C, None)

    def bwd(dy=FAKE, M=129, W2p=FAKE, y1=FAKE, mean=FAKE, rstd=FAKE, gamma=FAKE, dy1=FAKE, part=FAKE):
        return L.triad_projhead_ln_bwd(dy, M, W2p, y1, mean, rstd, gamma, dy1, part, None)

    # the packed weights: 16-byte loads
    assert fused(W1p=FAKE + 8) == EINVAL
    assert fused(W2p=FAKE + 8) == EINVAL
    assert half(W1p=FAKE + 8) == EINVAL
    assert gemm(Bp=FAKE + 8) == EINVAL
    assert bwd(W2p=FAKE + 8) == EINVAL
    # the outputs: 8-byte stores
    assert fused(y1=FAKE + 4) == EINVAL
    assert fused(ln=FAKE + 4) == EINVAL
    assert fused(y=FAKE + 4) == EINVAL
    assert half(y1=FAKE + 4) == EINVAL
    assert half(ln=FAKE + 4) == EINVAL
    assert gemm(C=FAKE + 4) == EINVAL
    assert bwd(dy1=FAKE + 4) == EINVAL
    # part: f32x4 stores; the backward's y1: 16-byte LDS-DMA
    assert bwd(part=FAKE + 8) == EINVAL
    assert bwd(y1=FAKE + 8) == EINVAL
    # eps finite and >= 0
    for f in (fused, half):
        assert f(eps=-1e-5) == EINVAL
        assert f(eps=NANF) == EINVAL
        assert f(eps=INF) == EINVAL
    # the rules there were: rows 16-byte aligned, K % 32, lda, n_per, bstride, NULL pointers
    assert fused(h=FAKE + 8) == EINVAL and half(h=FAKE + 8) == EINVAL and gemm(A=FAKE + 8) == EINVAL
    assert bwd(dy=FAKE + 8) == EINVAL
    assert fused(M=0) == EINVAL and fused(H=0) == EINVAL and fused(H=100, lda=104) == EINVAL
    assert fused(lda=88) == EINVAL and fused(lda=100) == EINVAL
    assert fused(n_per=0) == EINVAL and fused(bstride=4) == EINVAL
    for k in ("h", "W1p", "b1", "gamma", "beta", "W2p", "b2", "y1", "ln", "mean", "rstd", "y"):
        assert fused(**{k: None}) == EINVAL, k
    for k in ("h", "W1p", "b1", "gamma", "beta", "y1", "ln", "mean", "rstd"):
        assert half(**{k: None}) == EINVAL, k
    for k in ("A", "Bp", "bias", "C"):
        assert gemm(**{k: None}) == EINVAL, k
    for k in ("dy", "W2p", "y1", "mean", "rstd", "gamma", "dy1", "part"):
        assert bwd(**{k: None}) == EINVAL, k


def test_ln_row_passes_reject_unsafe_calls():
    L = _lib()

    def fwd(y1=FAKE, M=5, gamma=FAKE, beta=FAKE, eps=1e-5, ln=FAKE, mean=FAKE, rstd=FAKE):
        return L.triad_ln_fwd(y1, M, gamma, beta, eps, ln, mean, rstd, None)

    def bwd(dln=FAKE, y1=FAKE, mean=FAKE, rstd=FAKE, gamma=FAKE, M=5, dy1=FAKE, part=FAKE, nblocks=2):
        return L.triad_ln_bwd3(dln, y1, mean, rstd, gamma, M, dy1, part, nblocks, None)

    for k in ("y1", "gamma", "beta", "ln", "mean", "rstd"):
        assert fwd(**{k: None}) == EINVAL, k
    assert fwd(y1=FAKE + 8) == EINVAL
    assert fwd(ln=FAKE + 8) == EINVAL
    assert fwd(M=0) == EINVAL
    for k in ("dln", "y1", "mean", "rstd", "gamma", "dy1", "part"):
        assert bwd(**{k: None}) == EINVAL, k
    assert bwd(dln=FAKE + 8) == EINVAL
    assert bwd(y1=FAKE + 8) == EINVAL
    assert bwd(dy1=FAKE + 8) == EINVAL
    assert bwd(M=0) == EINVAL
    assert bwd(nblocks=0) == EINVAL
    assert bwd(nblocks=(1 << 24)) == EINVAL       # 2^24 blocks of 256 threads: past 2^32 - 1 threads


def test_sums_reject_unsafe_calls():
    L = _lib()
    assert L.triad_sum_slabs(None, 4, 64, None, 0, FAKE, None) == EINVAL
    assert L.triad_sum_slabs(FAKE, 4, 64, None, 0, None, None) == EINVAL
    assert L.triad_sum_slabs(FAKE, 0, 64, None, 0, FAKE, None) == EINVAL
    assert L.triad_sum_slabs(FAKE, 4, 0, None, 0, FAKE, None) == EINVAL

    for name in ("triad_colsum", "triad_colsum_dma"):
        fn = getattr(L, name)

        def cs(X=FAKE, rows=64, cols=256, ld=256, part=FAKE, out=FAKE):
            return fn(X, rows, cols, ld, part, 1.0, 0, out, None)

        assert cs(X=None) == EINVAL, name
        assert cs(part=None) == EINVAL, name
        assert cs(out=None) == EINVAL, name
        assert cs(X=FAKE + 8) == EINVAL, name
        assert cs(rows=0) == EINVAL and cs(cols=0) == EINVAL and cs(cols=250, ld=256) == EINVAL, name
        assert cs(ld=252) == EINVAL and cs(ld=248) == EINVAL, name
    assert L.triad_colsum_dma(FAKE, 64, 256, 256, FAKE + 8, 1.0, 0, FAKE, None) == EINVAL    # part 16-byte aligned


def test_fake_pointer_is_what_the_rules_assume():
    assert FAKE % 16 == 0 and ctypes.sizeof(ctypes.c_void_p) == 8
