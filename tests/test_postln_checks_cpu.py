"""The checks of tests/test_postln_conformance_gpu.py bite: the numpy keep bits reproduce a vector
worked by hand, a plain-torch fp32 / bf16 emulation of each kernel of csrc/postln.hip in the code's
operation order (tests/postln_ref.py) lies inside every fp64 bound and satisfies every identity at
every shape the GPU file runs, and the same emulation with one planted error -- thirteen of them,
each its own test -- falls outside a bound or breaks an identity. No device."""
import functools

import numpy as np
import pytest
import torch

from tests import postln_ref as R

BF, F32 = R.BF, R.F32
EPS = R.f32(R.EPS)


# ---- keep bits ----------------------------------------------------------------------------------------

def test_keep_bits_reproduce_a_hand_worked_vector():
    """lowbias32 by hand (32-bit wrap-around), seed 12345. The high word of every q < 2^32 is 0:
        c = lowbias32(0 ^ 0x85ebca6b): 85ebca6b -> ^>>16 85eb4f80 -> *7feb352d bc527980 -> ^>>15 bc530124
            -> *846ca68b 1efef68c -> ^>>16 1efee872
        q = 0: x = 0 + 12345 + c = 1eff18ab -> 1eff0654 -> ba3f80c4 -> ba3ef4bb -> 9dc42389 -> 9dc4be4d:
               element 0 takes 0xbe4d = 48717, element 1 takes 0x9dc4 = 40388
        q = 1: x = 9e3779b9 + 12345 + c = bd369264 -> bd362f52 -> 98984b6a -> 98997a5a -> 66a3cade
               -> 66a3ac7d: element 2 takes 0xac7d = 44157, element 3 takes 0x66a3 = 26275
        q = 2: x = 2 * 9e3779b9 + 12345 + c = 5b6e0c1d -> ... -> 637d4c1a: 19482, 25469
    and for the high word, q = 2^32 + 1 with seed 7 gives 2998b054."""
    assert int(R.hash32(np.array([0x85ebca6b], dtype=np.uint32))[0]) == 0x1efee872
    assert R.keep_fields(6, 12345).tolist() == [48717, 40388, 44157, 26275, 19482, 25469]
    assert R.keep_fields(4, 12345, start=2).tolist() == [44157, 26275, 19482, 25469]
    assert R.keep_fields(4, 0).tolist() == [10986, 41246, 21253, 28148]
    assert R.keep_fields(2, 2 ** 32 - 1).tolist() == [32264, 30760]
    assert int(R.pair_hash(np.array([2 ** 32 + 1], dtype=np.uint64), 7)[0]) == 0x2998b054
    # thr(0.5) = 32768: 48717, 40388, 44157 kept, 26275, 19482, 25469 dropped
    assert R.keep_bits(6, 0.5, 12345).tolist() == [True, True, True, False, False, False]
    assert R.keep_bits(6, 0.5, 12345, swap_pair=True).tolist() == [True, True, False, True, False, False]


def test_thresholds_and_scales_at_the_edge_probabilities():
    """(unsigned)(p * 65536.f + 0.5f) and fl32(1 / (1 - p)) at p = 0, a p with thr == 0 but scale != 1,
    0.1, 0.5 and the two p just below 1 with thr = 65535 and 65536 (nothing kept)."""
    p0, ptiny, p01, p05, p65535, p65536 = R.P_LIST
    assert [R.drop_thr(p) for p in R.P_LIST] == [0, 0, 6554, 32768, 65535, 65536]
    assert R.drop_scale(p0) == 1.0 and R.drop_scale(ptiny) == 1.0 + 2.0 ** -18 != 1.0
    assert R.drop_scale(p01) == 1.1111111640930176 and R.drop_scale(p05) == 2.0
    assert R.drop_scale(p65535) == 65536.0 and R.drop_scale(p65536) == 2.0 ** 24
    assert all(R.f32(p) < 1.0 for p in R.P_LIST)
    n = 1 << 16
    assert R.keep_bits(n, p0, 3).all() and R.keep_bits(n, ptiny, 3).all()
    assert not R.keep_bits(n, p65536, 3).any()
    assert R.keep_bits(n, p65535, 3).sum() == (R.keep_fields(n, 3) == 65535).sum()
    assert abs(R.keep_bits(n, p01, 3).mean() - 0.9) < 5e-3


def test_gl_index_maps_every_pattern_to_its_own_entry_or_to_the_formula():
    bits = np.arange(65536)
    idx = R.gl_index(bits)
    inside = idx >= 0
    assert inside.sum() == R.GL_N and idx[inside].max() == R.GL_N - 1
    assert len(np.unique(idx[inside])) == R.GL_N
    assert (R.gl_pattern(idx[inside]) == bits[inside]).all()
    x = torch.from_numpy(bits.astype(np.int32)).to(torch.int16).view(BF).float().abs()
    want = (x >= 2.0 ** -40) & (x < 2.0 ** 6)          # NaN / inf compare false
    assert torch.equal(torch.from_numpy(inside), want)
    assert R.GL_BYTES == R.GL_N * 4 + R.GL_N * 2


# ---- clean emulations inside every bound ----------------------------------------------------------------

def _fwd_checks(c, p, seed, **planted):
    """{name: passes} of an emulated forward against the fp64 reference and the identities."""
    want = R.dropaddln_fwd_ref(c["res"], c["y"], c["w"], c["b"], EPS, p, seed)
    h, hb, mean, rstd = R.emul_dropaddln_fwd(c["res"], c["y"], c["w"], c["b"], EPS, p, seed, **planted)
    out = {n: R.passes(g, *want[n]) for n, g in (("mean", mean), ("rstd", rstd), ("h", h), ("hb", hb))}
    out["hb==bf16(h)"] = torch.equal(hb, h.to(BF))
    return out, want, (h, hb, mean, rstd)


@pytest.mark.parametrize("D", R.FWD_DS)
def test_forward_emulation_inside_every_bound(D):
    for M in R.FWD_MS:
        c = R.postln_case(M, D)
        for p in R.FWD_PS:
            ok, want, (h, hb, mean, rstd) = _fwd_checks(c, p, R.SEED_HI)
            assert all(ok.values()), (M, D, p, ok)
            if D == 768 and M >= 4:
                k = R.SPECIAL_ROWS["const"]
                assert bool(want["exact"][R.SPECIAL_ROWS["mean100"]]), "the mean-100 row's z must be exact in fp32"
                assert float(mean[k]) == R.CONST and torch.equal(h[k], c["b"])
                assert abs(float(rstd[k]) - EPS ** -0.5) <= 6 * R.U * EPS ** -0.5


def _stats32(c, p, seed):
    want = R.dropaddln_fwd_ref(c["res"], c["y"], c["w"], c["b"], EPS, p, seed)
    return want["mean"][0].to(F32), want["rstd"][0].to(F32)


def _bwd_checks(c, p, seed, use_dh=True, use_dhb=True, **planted):
    dh, dhb = (c["dh"] if use_dh else None), (c["dhb"] if use_dhb else None)
    mean, rstd = _stats32(c, p, seed)
    want = R.dropaddln_bwd_ref(dh, dhb, c["res"], c["y"], mean, rstd, c["w"], p, seed)
    dres, dy, part = R.emul_dropaddln_bwd(dh, dhb, c["res"], c["y"], mean, rstd, c["w"], p, seed, **planted)
    keep = R.keep_mask(c["res"].shape, p, seed)
    out = {"dres": R.passes(dres, *want["dres"]), "part": R.passes(part, *want["part"]),
           "total": R.passes(part.double().sum(0), *want["total"]),
           "dy": torch.equal(dy, R.dy_of(dres, keep, R.drop_scale(p)))}
    return out, want, (dres, dy, part)


@pytest.mark.parametrize("D", R.FWD_DS)
def test_backward_emulation_inside_every_bound(D):
    for M in R.FWD_MS:
        c = R.postln_case(M, D)
        for p in (0.0, 0.1):
            ok, _, _ = _bwd_checks(c, p, R.SEED_HI)
            assert all(ok.values()), (M, D, p, ok)
        if M in (5, 130):
            for use_dh, use_dhb in ((True, False), (False, True)):
                ok, _, _ = _bwd_checks(c, 0.1, R.SEED_HI, use_dh, use_dhb)
                assert all(ok.values()), (M, D, use_dh, use_dhb, ok)


@pytest.mark.parametrize("M", [4101, 8197])
def test_backward_emulation_inside_every_bound_past_one_trip(M):
    """M > 4096: blocks run a second and a third trip (D = 256 suffices here; the GPU file also runs
    M = 4101 at D = 1024)."""
    assert R.bwd_blocks(M) == 1024 and R.bwd_trips(M) == (2 if M == 4101 else 3)
    ok, _, _ = _bwd_checks(R.postln_case(M, 256), 0.1, R.SEED_HI)
    assert all(ok.values()), ok


@pytest.mark.parametrize("D", R.FWD_DS)
def test_chained_emulation_inside_the_widened_bounds(D):
    """Backward on the emulated forward's own fp32 mean / rstd against the chain that keeps the fp64
    statistics: inside the bounds widened by the forward's dm and rel_rstd."""
    c = R.postln_case(130, D)
    for p in (0.0, 0.1):
        fw = R.dropaddln_fwd_ref(c["res"], c["y"], c["w"], c["b"], EPS, p, R.SEED_HI)
        _, _, mean, rstd = R.emul_dropaddln_fwd(c["res"], c["y"], c["w"], c["b"], EPS, p, R.SEED_HI)
        dres, _, part = R.emul_dropaddln_bwd(c["dh"], c["dhb"], c["res"], c["y"], mean, rstd, c["w"], p, R.SEED_HI)
        want = R.dropaddln_bwd_ref(c["dh"], c["dhb"], c["res"], c["y"], fw["mean"][0], fw["rstd"][0], c["w"], p,
                                   R.SEED_HI, dm=fw["dm"], rel_r=fw["rel_r"])
        assert R.passes(dres, *want["dres"]) and R.passes(part, *want["part"]), (D, p)
        assert R.passes(part.double().sum(0), *want["total"]), (D, p)


def test_bwd_blocks_restatement():
    assert [R.bwd_blocks(M) for M in (1, 4, 5, 4095, 4096, 4097, 1 << 20)] == [1, 1, 2, 1024, 1024, 1024, 1024]
    assert R.row_block(8197)[[0, 3, 4, 4095, 4096, 4100, 8192, 8196]].tolist() == [0, 0, 1, 1023, 0, 1, 0, 1]


@functools.lru_cache(maxsize=None)
def _gelu_all():
    u = R.all_patterns()
    dv = R.gelu_case(u.numel(), 1)[1]
    return u, dv, torch.isfinite(u.float())


def _gelu_checks(p, seed, fwd_planted={}, bwd_planted={}):
    u, dv, fin = _gelu_all()
    keep, scale = R.keep_mask(u.shape, p, seed), R.drop_scale(p)
    v = R.emul_geludrop_fwd(u, p, seed, **fwd_planted)
    g0 = R.emul_geludrop_fwd(u, 0.0, 0)
    du = R.emul_geludrop_bwd(u, dv, p, seed, **bwd_planted)
    want_v = torch.where(keep, (g0.float() * torch.tensor(scale, dtype=F32)).to(BF), torch.zeros_like(g0))
    vref, vbound = R.geludrop_fwd_ref(u, keep, scale)
    ok = fin & R.in_range(vref, vbound)
    assert int((fin & ~ok).sum()) <= 64          # only the largest patterns, whose x * scale overflows bf16
    return {"v": R.passes(v[ok], vref[ok], vbound[ok]),
            "du": R.passes(du[fin], *(t[fin] for t in R.geludrop_bwd_ref(u, dv, keep, scale))),
            "v==bf16(g keep scale)": torch.equal(v[fin].view(torch.int16), want_v[fin].view(torch.int16))}


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gelu_emulation_inside_every_bound_on_every_finite_pattern(p):
    ok = _gelu_checks(p, 1234)
    assert all(ok.values()), ok


def test_gelu_table_entries_inside_their_bounds_in_emulation():
    x = torch.from_numpy(R.gl_pattern(np.arange(R.GL_N)).astype(np.int32)).to(torch.int16).view(BF)
    (g, gb), (s, sb) = R.gelu_table_ref(x)
    assert R.passes(R.emul_gelu_val(x.float()).to(BF), g, gb)
    assert R.passes(R.emul_gelu_slope(x.float()), s, sb)


# ---- the thirteen planted errors --------------------------------------------------------------------------

CASE = (9, 768)     # special rows present, three blocks


def test_planted_01_keep_bits_of_a_pair_swapped():
    ok, _, _ = _fwd_checks(R.postln_case(*CASE), 0.1, R.SEED_HI, swap_pair=True)
    assert not ok["h"] and not ok["mean"]


STRICT = dict(M=9, D=256, p=0.5, seed=0)   # seed filled in below: the first with a field == thr


def _strict_seed():
    n, thr = STRICT["M"] * STRICT["D"], R.drop_thr(STRICT["p"])
    for seed in range(2 ** 31, 2 ** 31 + 4096):
        if (R.keep_fields(n, seed) == thr).any():
            return seed
    raise AssertionError("no seed with a field equal to the threshold")


def test_planted_02_threshold_compared_with_greater_than():
    M, D, p = STRICT["M"], STRICT["D"], STRICT["p"]
    seed = _strict_seed()
    hit = R.keep_fields(M * D, seed) == R.drop_thr(p)
    assert hit.any(), "precondition: one 16-bit field equals thr"
    c = R.postln_case(M, D)
    assert bool((c["y"].view(-1)[torch.from_numpy(hit)].float().abs() > 1e-2).any())
    assert all(_fwd_checks(c, p, seed)[0].values())
    ok, _, _ = _fwd_checks(c, p, seed, strict=True)
    assert not ok["h"]


def test_planted_03_dropped_term_not_rounded_to_bf16():
    ok, _, _ = _fwd_checks(R.postln_case(*CASE), 0.1, R.SEED_HI, yd_unrounded=True)
    assert not ok["h"]


def test_planted_04_scale_from_the_double_quotient():
    """p = 0.9: fl32(1 / (1 - 0.9)) = 10 but 1 - fl32(0.9) = 0.10000002384 and the kernel's scale is
    9.99999809. yd differs only where y * scale straddles a bf16 rounding boundary; row 3 of y is
    filled with the bf16 values that do (1.046875 * 10 = 10.46875 is a tie of the wrong scale)."""
    p = 0.9
    s_kernel, s_double = R.drop_scale(p), R.f32(1.0 / (1.0 - p))
    assert s_kernel != s_double
    cand = torch.arange(0x3e80, 0x4080, dtype=torch.int32).to(torch.int16).view(BF)    # [0.25, 4)
    flips = cand[(cand.float() * torch.tensor(s_kernel)).to(BF) != (cand.float() * torch.tensor(s_double)).to(BF)]
    assert flips.numel() > 0
    c = R.postln_case(*CASE)
    c["y"][3] = flips.repeat(-(-CASE[1] // flips.numel()))[:CASE[1]]
    assert bool(R.keep_mask(c["res"].shape, p, R.SEED_HI)[3].any())
    assert all(_fwd_checks(c, p, R.SEED_HI)[0].values())
    ok, _, _ = _fwd_checks(c, p, R.SEED_HI, scale_double=True)
    assert not ok["h"]


def test_planted_05_one_pass_variance_on_the_mean_100_row():
    c = R.postln_case(*CASE)
    k = R.SPECIAL_ROWS["mean100"]
    want = R.dropaddln_fwd_ref(c["res"], c["y"], c["w"], c["b"], EPS, 0.1, R.SEED_HI)
    assert bool(want["exact"][k])
    h, _, _, rstd = R.emul_dropaddln_fwd(c["res"], c["y"], c["w"], c["b"], EPS, 0.1, R.SEED_HI, one_pass=True)
    assert not R.passes(rstd[k:k + 1], want["rstd"][0][k:k + 1], want["rstd"][1][k:k + 1])
    assert not R.passes(h[k:k + 1], want["h"][0][k:k + 1], want["h"][1][k:k + 1])


def test_planted_06_backward_without_the_c2_term():
    ok, _, _ = _bwd_checks(R.postln_case(*CASE), 0.1, R.SEED_HI, no_c2=True)
    assert not ok["dres"]


def test_planted_07_dhb_ignored():
    ok, _, _ = _bwd_checks(R.postln_case(*CASE), 0.1, R.SEED_HI, ignore_dhb=True)
    assert not ok["dres"] and not ok["part"] and not ok["total"]


def test_planted_08_dh_ignored():
    ok, _, _ = _bwd_checks(R.postln_case(*CASE), 0.1, R.SEED_HI, ignore_dh=True)
    assert not ok["dres"] and not ok["part"] and not ok["total"]


def test_planted_09_dy_without_the_inner_bf16_rounding():
    ok, _, _ = _bwd_checks(R.postln_case(*CASE), 0.1, R.SEED_HI, dy_unrounded=True)
    assert ok["dres"] and not ok["dy"]


def test_planted_10_rows_from_4096_on_left_out_of_dgamma_dbeta():
    ok, want, (_, _, part) = _bwd_checks(R.postln_case(4101, 256), 0.1, R.SEED_HI, drop_later_trips=True)
    assert ok["dres"] and not ok["part"] and not ok["total"]
    ref, bound = want["part"]
    assert R.passes(part[2:], ref[2:], bound[2:]) and not R.passes(part[:2], ref[:2], bound[:2])   # blocks 0, 1 only


def test_planted_11_dgamma_accumulated_with_z_minus_mean():
    ok, want, (_, _, part) = _bwd_checks(R.postln_case(*CASE), 0.1, R.SEED_HI, gw_unnormalised=True)
    ref, bound = want["part"]
    assert not R.passes(part[:, 0], ref[:, 0], bound[:, 0]) and R.passes(part[:, 1], ref[:, 1], bound[:, 1])


def test_planted_12_gelu_slope_without_x_pdf():
    ok = _gelu_checks(0.1, 1234, bwd_planted=dict(no_xpdf=True))
    assert ok["v"] and not ok["du"]


def test_planted_13_gelu_value_rounded_after_the_dropout_scaling():
    """One rounding instead of two lies inside the value bound; it breaks the identity with the p = 0
    output of the same pass."""
    ok = _gelu_checks(0.1, 1234, fwd_planted=dict(round_after=True))
    assert not ok["v==bf16(g keep scale)"]
