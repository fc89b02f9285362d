"""The checks of tests/test_vit_rows_conformance_gpu.py bite: for each kernel of csrc/lora.hip and
csrc/resid_ln.hip a plain-torch fp32 emulation with the kernel's rounding points (fp32 sums, bf16
stores; tests/vit_rows_ref.py) passes the fp64 reference's per-element bound, and the same
emulation with one planted error fails it. No device."""
import pytest
import torch

from tests import vit_rows_ref as R

EPS = R.f32(1e-6)


@pytest.mark.parametrize("M,K,J", [(17, 96, 8), (65, 768, 16), (130, 160, 1)])
def test_rows_nt_bound_sees_a_dropped_k_step(M, K, J):
    X, W = R.rows_nt_case(M, K, J)
    ref, bound = R.rows_nt_ref(X, W)
    assert R.passes(R.emul_rows_nt(X, W), ref, bound)
    for s in (0, K // 32 - 1):
        assert not R.passes(R.emul_rows_nt(X, W, drop_kstep=s), ref, bound), f"k-step {s} dropped unseen"


@pytest.mark.parametrize("M,O", [(7, 8), (1025, 256)])
def test_lora_update_bound_sees_swapped_rank_columns(M, O):
    Y, T, Bs = R.lora_update_case(M, O)
    ref, bound = R.lora_update_ref(Y, T, Bs)
    assert R.passes(R.emul_lora_update(Y, T, Bs), ref, bound)
    for j in range(7):
        assert not R.passes(R.emul_lora_update(Y, T, Bs, swap=j), ref, bound), f"columns {j}, {j + 1} swapped unseen"


@pytest.mark.parametrize("M,O", [(100, 256), (33, 768), (16385 + 31, 256), (32805, 256)])
def test_lora_tn_bounds_see_a_dropped_tile_a_dropped_slab_and_alpha_twice(M, O):
    """Includes the two shapes with more than one tile per block, where an any-order bound over all
    M rows would be too loose to see one tile (vit_rows_ref's docstring)."""
    Y, T, Wt = R.lora_tn_case(M, O)
    alpha = R.f32(0.37)
    ref, bound = R.lora_tn_out_ref(Y, T, alpha)
    dref, dbound = R.lora_tn_dt_ref(Y, Wt)
    out, dt = R.emul_lora_tn(Y, T, Wt, alpha)
    assert R.passes(out, ref, bound) and R.passes(dt, dref, dbound)
    tiles, G = (M + 31) // 32, R.tn_blocks(M)
    for tile in (0, tiles // 2, tiles - 2):   # (the last tile may hold a single row)
        assert not R.passes(R.emul_lora_tn(Y, T, None, alpha, drop_tile=tile)[0], ref, bound), f"tile {tile}"
    for slab in (0, (tiles - 1) // R.tn_per(M)):
        assert not R.passes(R.emul_lora_tn(Y, T, None, alpha, drop_slab=slab)[0], ref, bound), f"slab {slab} of {G}"
    assert not R.passes(R.emul_lora_tn(Y, T, None, alpha, alpha_twice=True)[0], ref, bound)
    # dt with one 256-column chunk of Wt left out
    Wd = Wt.clone()
    Wd[:, :256] = 0
    assert not R.passes(R.emul_lora_tn(Y, T, Wd, alpha)[1], dref, dbound)


@pytest.mark.parametrize("D", [256, 768, 1536])
@pytest.mark.parametrize("out_bf16", [False, True])
def test_addln_forward_bound_sees_one_pass_variance(D, out_bf16):
    c = R.addln_case(5, D)
    xn, ln, mean, rstd = R.emul_addln_fwd(c["x"], c["y"], c["g"], c["w"], c["b"], EPS, out_bf16)
    assert torch.equal(xn, R.addln_xn(c["x"], c["y"], c["g"]))
    want = R.addln_fwd_ref(xn, c["w"], c["b"], EPS, out_bf16)
    for name, got in (("mean", mean), ("rstd", rstd), ("ln", ln)):
        assert R.passes(got, *want[name]), name
    if D == 768:
        k = R.SPECIAL_ROWS["const"]
        assert float(mean[k]) == R.CONST and torch.equal(ln[k].float(), c["b"].to(ln.dtype).float())
        # the mean-100 row: one-pass variance must fail on that row alone, in rstd and in ln
        k = R.SPECIAL_ROWS["mean100"]
        _, ln1, _, rstd1 = R.emul_addln_fwd(c["x"], c["y"], c["g"], c["w"], c["b"], EPS, out_bf16, one_pass=True)
        assert not R.passes(rstd1[k:k + 1], want["rstd"][0][k:k + 1], want["rstd"][1][k:k + 1])
        assert not R.passes(ln1[k:k + 1], want["ln"][0][k:k + 1], want["ln"][1][k:k + 1])


@pytest.mark.parametrize("D", [256, 768, 1536])
@pytest.mark.parametrize("dln", ["dln_bf16", "dln_f32"])
@pytest.mark.parametrize("has_res", [False, True])
def test_addln_backward_checks_see_a_missing_c2_and_an_early_dy(D, dln, has_res):
    c = R.addln_case(5, D)
    xn, _, mean, rstd = R.emul_addln_fwd(c["x"], c["y"], c["g"], c["w"], c["b"], EPS, True)
    dres = c["dres"] if has_res else None
    ref, bound = R.addln_bwd_ref(c[dln], dres, xn, mean, rstd, c["w"])
    dx, dy = R.emul_addln_bwd(c[dln], dres, xn, mean, rstd, c["w"], c["g"])
    assert R.passes(dx, ref, bound) and torch.equal(dy, R.addln_dy(dx, c["g"]))
    dx2, _ = R.emul_addln_bwd(c[dln], dres, xn, mean, rstd, c["w"], c["g"], no_c2=True)
    assert not R.passes(dx2, ref, bound)
    if has_res:
        dx3, dy3 = R.emul_addln_bwd(c[dln], dres, xn, mean, rstd, c["w"], c["g"], dy_before_dres=True)
        assert R.passes(dx3, ref, bound) and not torch.equal(dy3, R.addln_dy(dx3, c["g"]))


@pytest.mark.parametrize("M,K,O", [(33, 256, 512), (33, 768, 768), (1001, 768, 768)])
def test_lora_linear_reference_holds_for_an_emulated_chain(M, K, O):
    """lora_linear_ref's bounds against the chain built from the kernels' emulations. Planted: the
    LoRA term of y 1 % too large; one row of dy (of x) left out of dB (of dA)."""
    g = torch.Generator().manual_seed(11)
    s = 2.0
    bf = lambda *sh, k=1.0: (torch.randn(*sh, generator=g) * k).to(R.BF)
    x, W, b, A, B, dy = bf(M, K), bf(O, K, k=K ** -0.5), bf(O), bf(8, K, k=K ** -0.5), bf(O, 8, k=0.05), bf(M, O)
    sB = (B.float() * s).to(R.BF)
    want = R.lora_linear_ref(x, W, b, A, sB, s, dy)
    t = R.emul_rows_nt(x, A)
    base = (x.float() @ W.float().t() + b.float()).to(R.BF)
    y = R.emul_lora_update(base, t, sB)
    wt = torch.zeros(16, O, dtype=R.BF)
    wt[:8] = sB.t()
    dB, dt = R.emul_lora_tn(dy, t, wt, s)
    dx = R.emul_lora_update((dy.float() @ W.float()).to(R.BF), dt, A.t().contiguous())
    dAt, _ = R.emul_lora_tn(x, dt, None, 1.0)
    for name, got in (("y", y), ("dx", dx), ("dA", dAt.t()), ("dB", dB)):
        assert R.passes(got, *want[name]), name
    y_bad = (base.float() + x.float() @ A.float().t() @ sB.float().t() * 1.01).to(R.BF)
    assert not R.passes(y_bad, *want["y"])
    dy1, x1 = dy.clone(), x.clone()
    dy1[M // 2] = 0
    x1[M // 2] = 0
    assert not R.passes(R.emul_lora_tn(dy1, t, None, s)[0], *want["dB"])
    assert not R.passes(R.emul_lora_tn(x1, dt, None, 1.0)[0].t(), *want["dA"])


def test_lora_gate_admits_exactly_the_widths_lora_tn_has():
    """vit.lora_hip_shapes: K / 256 and O / 256 both among triad_lora_tn's instances (the backward
    runs it over dy and over x), rank 8; 1280 = 5 x 256 passed the old multiple-of-256 gate."""
    from triad_amd.vit import lora_hip_shapes
    for nk in range(1, 15):
        for no in range(1, 15):
            assert lora_hip_shapes(256 * nk, 256 * no, 8) == (nk in R.TN_WIDTHS and no in R.TN_WIDTHS), (nk, no)
    assert not lora_hip_shapes(384, 1152, 8) and not lora_hip_shapes(1280, 1280, 8)
    assert not lora_hip_shapes(768, 768, 4) and not lora_hip_shapes(768, 768, 16)
