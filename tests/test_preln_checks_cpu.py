"""The checks of tests/test_preln_gpu.py bite, and the host side of the pre-LN (stable layer norm) path
works without a device: a plain-torch emulation of triad_preln_fwd / _bwd in the code's operation order
(tests/preln_ref.py) lies inside every fp64 bound and satisfies every identity at every shape the GPU
file runs; the same emulation with one planted error -- six of them, each its own test -- falls outside
a bound or breaks an identity; the entry points refuse bad arguments before any launch; the LayerDrop
plan keeps the layers the stock loop keeps; install_fused_encoder swaps a stable-LN encoder's forward
and a CPU input still runs the stock code."""
import os
import types

import pytest
import torch

from tests import postln_ref as R
from tests import preln_ref as P

BF, F32 = P.BF, P.F32
EPS = R.f32(P.EPS)


# ---- clean emulations inside every bound ------------------------------------------------------------------

def _fwd_checks(c, p, seed, with_y=True, **planted):
    y = c["y"] if with_y else None
    want = P.preln_fwd_ref(c["res"], y, c["w"], c["b"], EPS, p, seed)
    zb, nb, mean, rstd = P.emul_preln_fwd(c["res"], y, c["w"], c["b"], EPS, p, seed, False, **planted)
    _, n32, _, _ = P.emul_preln_fwd(c["res"], y, c["w"], c["b"], EPS, p, seed, True, **planted)
    if with_y:   # what torch's bf16 add gives on the same mask
        keep = R.keep_mask(c["res"].shape, p, seed)
        yd = (c["y"].float() * torch.tensor(R.drop_scale(p), dtype=F32)).to(BF)
        torch_z = c["res"] + torch.where(keep, yd, torch.zeros_like(yd))
    else:
        torch_z = c["res"]
    assert torch.equal(want["z"], torch_z), "the fp64 restatement of z differs from torch's bf16 add"
    return {"res_out": torch.equal(zb, torch_z), "mean": R.passes(mean, *want["mean"]),
            "rstd": R.passes(rstd, *want["rstd"]), "n32": R.passes(n32, *want["n32"]), "nb": R.passes(nb, *want["nb"]),
            "bf16(n32)==nb": torch.equal(n32.to(BF), nb)}


@pytest.mark.parametrize("D", P.FWD_DS)
def test_forward_emulation_inside_every_bound(D):
    for M in P.FWD_MS:
        c = P.preln_case(M, D)
        for p in P.FWD_PS:
            ok = _fwd_checks(c, p, P.SEED_HI)
            assert all(ok.values()), (M, D, p, ok)
        ok = _fwd_checks(c, 0.0, 0, with_y=False)
        assert all(ok.values()), (M, D, "no y", ok)


def _bwd_checks(c, mode, p=0.1, seed=P.SEED_HI, **planted):
    z, keep, scale = P.stream(c["res"], c["y"], p, seed)
    mean, rstd = P.ref_stats(z, c["w"], c["b"], EPS)
    dz, dn = P.pick(c, mode)
    want = P.preln_bwd_ref(dz, dn, z, mean, rstd, c["w"])
    dres, dy, part = P.emul_preln_bwd(dz, dn, z, mean, rstd, c["w"], p, seed, **planted)
    return {"dres": R.passes(dres, *want["dres"]), "part": R.passes(part, *want["part"]),
            "total": R.passes(part.double().sum(0), *want["total"]),
            "dy": torch.equal(dy, R.dy_of(dres, keep, scale))}


@pytest.mark.parametrize("D", P.FWD_DS)
def test_backward_emulation_inside_every_bound(D):
    for M in P.FWD_MS:
        c = P.preln_case(M, D)
        for mode in P.BWD_MODES + (("dz", "dn32"), ("dn32",)):
            ok = _bwd_checks(c, mode)
            assert all(ok.values()), (M, D, mode, ok)


@pytest.mark.parametrize("M,D", P.BWD_BIG)
def test_backward_emulation_inside_every_bound_past_one_trip(M, D):
    assert R.bwd_blocks(M) == 1024 and R.bwd_trips(M) == (3 if M == 8197 else 2)
    c = P.preln_case(M, D)
    for mode in P.BWD_MODES:
        ok = _bwd_checks(c, mode)
        assert all(ok.values()), (M, D, mode, ok)


# ---- the six planted errors ---------------------------------------------------------------------------------

CASE = (9, 768)


def test_planted_1_z_not_rounded_to_bf16_before_the_statistics():
    ok = _fwd_checks(P.preln_case(*CASE), 0.1, P.SEED_HI, z_unrounded=True)
    assert ok["res_out"] and not ok["mean"] and not ok["n32"]


def test_planted_2_dropout_output_not_rounded():
    ok = _fwd_checks(P.preln_case(*CASE), 0.1, P.SEED_HI, yd_unrounded=True)
    assert not ok["res_out"]


def test_planted_3_dz_ignored():
    ok = _bwd_checks(P.preln_case(*CASE), ("dz", "dn"), ignore_dz=True)
    assert not ok["dres"] and ok["part"]


def test_planted_4_dn_ignored():
    ok = _bwd_checks(P.preln_case(*CASE), ("dz", "dn"), ignore_dn=True)
    assert not ok["dres"] and not ok["part"] and not ok["total"]


def test_planted_5_dy_taken_from_the_unrounded_g():
    ok = _bwd_checks(P.preln_case(*CASE), ("dz", "dn"), dy_unrounded=True)
    assert ok["dres"] and not ok["dy"]


def test_planted_6_c2_term_dropped():
    ok = _bwd_checks(P.preln_case(*CASE), ("dz", "dn"), no_c2=True)
    assert not ok["dres"] and ok["part"]


# ---- host rejection -------------------------------------------------------------------------------------------

def _lib():
    from triad_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_preln_entry_points_reject_bad_arguments():
    """TRIAD_EINVAL (1001) before any launch, so no device is needed: one assertion per rule; each
    helper's defaults are a valid call that the others differ from in one argument."""
    lib = _lib()
    fake = 4096    # 16-byte aligned, never dereferenced: validation fails first
    nan, inf = float("nan"), float("inf")

    def fwd(M=64, D=768, p=0.1, eps=1e-5, n_is_f32=0, **a):
        a = {**dict(res=fake, y=fake, w=fake, b=fake, res_out=fake, n_out=fake, mean=fake, rstd=fake), **a}
        return lib.triad_preln_fwd(a["res"], a["y"], a["w"], a["b"], eps, M, D, p, 7, a["res_out"], a["n_out"],
                                   n_is_f32, a["mean"], a["rstd"], None)

    def bwd(M=64, D=768, p=0.1, dn_is_f32=0, **a):
        a = {**dict(dz=fake, dn=fake, z=fake, mean=fake, rstd=fake, w=fake, dres=fake, dy=fake, part=fake), **a}
        return lib.triad_preln_bwd(a["dz"], a["dn"], dn_is_f32, a["z"], a["mean"], a["rstd"], a["w"], M, D, p, 7,
                                   a["dres"], a["dy"], a["part"], None)

    required = {fwd: ("res", "w", "b", "res_out", "n_out", "mean", "rstd"),
                bwd: ("z", "mean", "rstd", "w", "dres", "part")}
    for f, names in required.items():
        for n in names:
            assert f(**{n: None}) == 1001, (f.__name__, n, "NULL")
    for f in (fwd, bwd):
        for D in (0, 128, 800, 1280, -256):
            assert f(D=D) == 1001, (f.__name__, D)
        assert f(M=0) == 1001 and f(M=-4) == 1001, f.__name__
        for p in (-0.1, 1.0, 1.5, nan):
            assert f(p=p) == 1001, (f.__name__, p)
    for eps in (0.0, -1e-5, nan, inf):
        assert fwd(eps=eps) == 1001, eps
    bf16_8 = {fwd: ("res", "y", "res_out", "n_out"), bwd: ("dz", "dn", "z", "dres", "dy")}
    for f, names in bf16_8.items():
        for n in names:
            assert f(**{n: fake + 2}) == 1001 and f(**{n: fake + 4}) == 1001, (f.__name__, n, "bf16 tensor off 8 bytes")
    f32_16 = {fwd: ("w", "b"), bwd: ("w",)}
    for f, names in f32_16.items():
        for n in names:
            assert f(**{n: fake + 4}) == 1001 and f(**{n: fake + 8}) == 1001, (f.__name__, n, "fp32 vector off 16 bytes")
    assert fwd(n_is_f32=1, n_out=fake + 8) == 1001 and bwd(dn_is_f32=1, dn=fake + 8) == 1001   # the fp32 forms
    for f, names in {fwd: ("mean", "rstd"), bwd: ("mean", "rstd", "part")}.items():
        for n in names:
            assert f(**{n: fake + 2}) == 1001, (f.__name__, n, "off 4 bytes")
    assert bwd(dz=None, dn=None) == 1001                       # nothing to differentiate
    assert bwd(dy=fake + 2) == 1001 and bwd(dy=fake + 4) == 1001   # a dy that is given has y's form
    assert fwd(y=None, res_out=fake + 2) == 1001               # optional without y, but aligned when given


def test_preln_bwd_blocks():
    lib = _lib()
    got = [lib.triad_preln_bwd_blocks(M) for M in (1, 4, 5, 4095, 4096, 4097, 1 << 20)]
    assert got == [R.bwd_blocks(M) for M in (1, 4, 5, 4095, 4096, 4097, 1 << 20)] == [1, 1, 2, 1024, 1024, 1024, 1024]


# ---- LayerDrop plan ---------------------------------------------------------------------------------------------

def _fake_encoder(n_layers, layerdrop, training):
    return types.SimpleNamespace(layers=list(range(n_layers)), training=training,
                                 config=types.SimpleNamespace(layerdrop=layerdrop))


@pytest.mark.parametrize("training", [True, False])
def test_layerdrop_plan_keeps_what_the_stock_loop_keeps(training):
    """Same decisions and the same generator state afterwards as the stock loop (restated in
    preln_ref.stock_layerdrop), for 40 seeds and three rates; eval mode keeps every layer and still
    draws."""
    from triad_amd import postln
    for layerdrop in (0.0, 0.1, 0.5):
        for s in range(40):
            torch.manual_seed(s)
            want = P.stock_layerdrop(6, layerdrop, training)
            state = torch.get_rng_state()
            torch.manual_seed(s)
            got = postln.layerdrop_plan(_fake_encoder(6, layerdrop, training))
            assert got == want, (layerdrop, s)
            assert torch.equal(torch.get_rng_state(), state)
            if not training or layerdrop == 0.0:
                assert got == list(range(6))


def test_layerdrop_seed_skips_an_interior_and_the_last_layer():
    s, kept = P.layerdrop_seed()
    torch.manual_seed(s)
    assert P.stock_layerdrop(6, 0.5) == kept
    assert 5 not in kept and len(kept) >= 2 and any(i not in kept for i in range(1, 5))


# ---- install ------------------------------------------------------------------------------------------------------

def _small_stable_hubert():
    import transformers
    cfg = transformers.HubertConfig(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                                    do_stable_layer_norm=True, feat_extract_norm="layer", conv_dim=(32, 32),
                                    conv_stride=(5, 2), conv_kernel=(10, 3), num_conv_pos_embeddings=16,
                                    num_conv_pos_embedding_groups=4)
    torch.manual_seed(0)
    return transformers.HubertModel(cfg)


def test_install_swaps_the_stable_encoder_and_cpu_inputs_run_the_stock_code():
    from transformers.models.hubert.modeling_hubert import HubertEncoderStableLayerNorm
    from triad_amd import postln
    hub = _small_stable_hubert().eval()
    enc = hub.encoder
    assert type(enc) is HubertEncoderStableLayerNorm
    keys = list(hub.state_dict())
    assert postln.install_fused_encoder(hub) is hub
    assert hasattr(enc, "_triad_stock_forward") and hasattr(enc, "_triad_seeds")
    assert enc.forward.__func__ is postln._stable_encoder_forward
    assert list(hub.state_dict()) == keys
    stock = enc._triad_stock_forward
    postln.install_fused_encoder(hub)                     # a second install changes nothing
    assert enc._triad_stock_forward == stock
    x = torch.randn(2, 11, 256)
    with torch.no_grad():
        got = enc(x).last_hidden_state
        want = enc._triad_stock_forward(x).last_hidden_state
    assert got.dtype == torch.float32 and torch.equal(got, want)
