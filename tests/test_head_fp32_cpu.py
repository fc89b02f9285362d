"""CPU-only tests of the fp32-accurate head (`precision="fp32"`): the new entry points validate
their arguments before any launch, `_project` / `MultiModalModel.__init__` route use_amp=False to
the fp32 projection chain, and the chunk helper keeps the backward's working set inside ds_budget."""
import os

import pytest
import torch
import torch.nn as nn

EINVAL = 1001
fake = 4096   # 16-byte aligned, never dereferenced: validation fails first


def _lib():
    from triad_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


# The valid base of each group is never called (with a device it would launch on the fake
# pointers); every assertion changes ONE argument of it.
def test_split_pack_rejects_bad_arguments():
    f = _lib().triad_split_pack

    def pack(x=fake, B=4, N=50, N_pad=64, rows=256, hi=fake, lo=fake):
        return f(x, B, N, N_pad, rows, hi, lo, None)

    assert pack(x=None) == EINVAL and pack(hi=None) == EINVAL and pack(lo=None) == EINVAL
    assert pack(x=fake + 4) == EINVAL and pack(hi=fake + 2) == EINVAL and pack(lo=fake + 8) == EINVAL
    assert pack(B=0) == EINVAL and pack(N=0) == EINVAL
    assert pack(N_pad=48) == EINVAL            # N_pad < N
    assert pack(rows=255) == EINVAL            # rows_alloc < B * N_pad


def _fwd_args(**kw):
    a = dict(Qhi=fake, Qlo=fake, Khi=fake, Klo=fake, R=200, R_pad=256, Nq=50, Bq=4, Bk=4, Nk_pad=64, Nk_eff=60,
             D=512, temp=fake, clamp_lo=-60.0, diag=1, diag_off=0, rowmax=fake, argmax=fake, nn_part=fake,
             diagS=fake)
    a.update(kw)
    return list(a.values()) + [None]


def _ds_args(**kw):
    a = dict(Qhi=fake, Qlo=fake, Khi=fake, Klo=fake, R=200, R_pad=256, Nq=50, Bq=4, Bk=4, Nk_pad=64, Nk_eff=60,
             D=512, temp=fake, clamp_lo=-60.0, diag=1, diag_off=0, argmax=fake, dclip=fake, qw=fake, dSdiag=fake,
             coef=fake, dS_hi=fake, dS_lo=fake, CT=8, dt_part=fake)
    a.update(kw)
    return list(a.values()) + [None]


# the rules both MFMA entry points share: one argument off the valid base per case
_SHARED = [dict(Qhi=None), dict(Qlo=None), dict(Khi=None), dict(Klo=None), dict(temp=None),
           dict(D=256), dict(D=0),
           dict(R_pad=250), dict(R_pad=128), dict(R=300), dict(R_pad=0),
           dict(Nk_pad=60), dict(Nk_pad=32), dict(Nk_eff=65),
           dict(Qhi=fake + 2), dict(Qlo=fake + 8), dict(Khi=fake + 4), dict(Klo=fake + 2)]


@pytest.mark.parametrize("bad", _SHARED, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_split_entry_points_reject_shared_rules(bad):
    lib = _lib()
    assert lib.triad_pairsim_fwd_split(*_fwd_args(**bad)) == EINVAL
    assert lib.triad_pairsim_dS_split(*_ds_args(**bad)) == EINVAL


def test_pairsim_fwd_split_rejects_its_own_rules():
    f = _lib().triad_pairsim_fwd_split
    for name in ("rowmax", "argmax", "nn_part"):
        assert f(*_fwd_args(**{name: None})) == EINVAL, name
    assert f(*_fwd_args(diag_off=1)) == EINVAL and f(*_fwd_args(diag_off=-1)) == EINVAL   # diagonal outside Bk


def test_pairsim_dS_split_rejects_its_own_rules():
    f = _lib().triad_pairsim_dS_split
    for name in ("argmax", "dclip", "qw", "coef", "dS_hi", "dS_lo", "dt_part"):
        assert f(*_ds_args(**{name: None})) == EINVAL, name
    assert f(*_ds_args(dS_hi=fake + 2)) == EINVAL and f(*_ds_args(dS_lo=fake + 8)) == EINVAL
    assert f(*_ds_args(CT=4)) == EINVAL            # CT * 32 < Bk * Nk_pad
    assert f(*_ds_args(CT=10)) == EINVAL           # CT % 4
    assert f(*_ds_args(CT=0)) == EINVAL


def test_precision_is_checked_before_any_device_work():
    from triad_amd import ops
    q, k, t = torch.zeros(2, 3, 512), torch.zeros(2, 4, 512), torch.tensor(1.5)
    with pytest.raises(ValueError):
        ops.contrastive_head(ops.AV, q, k, t, precision="fp64")
    with pytest.raises(ValueError):
        ops.contrastive_heads_av_tv(q, k, q, k, t, None, precision="tf32")
    with pytest.raises(ops.TriadError, match="global negatives"):
        ops.contrastive_head(ops.AV, q, k, t, group=object(), precision="fp32")
    with pytest.raises(ops.TriadError):   # CPU tensors: no fallback in the fp32 mode either
        ops.contrastive_head(ops.AV, q, k, t, precision="fp32")


class _Holder(nn.Module):
    def __init__(self):
        super().__init__()
        self.projection1 = nn.Linear(24, 512)
        self.layer_norm = nn.LayerNorm(512)
        self.projection2 = nn.Linear(512, 512)


def test_project_takes_the_fp32_torch_chain_when_flagged(monkeypatch):
    from triad_amd import model
    torch.manual_seed(0)
    emb = _Holder()
    h = torch.randn(3, 7, 24)
    seen = []
    monkeypatch.setattr(model.ops, "projection_head", lambda *a: seen.append(a) or "fused")
    assert model._project(emb, h) == "fused" and len(seen) == 1      # without the flag: unchanged
    emb.reference_precision = True
    y = model._project(emb, h)
    assert len(seen) == 1 and y.dtype == torch.float32
    assert torch.equal(y, emb.projection2(emb.layer_norm(emb.projection1(h))))
    y.sum().backward()
    assert emb.projection1.weight.grad is not None


@pytest.mark.parametrize("use_amp", [True, False])
def test_model_flags_its_embedders_only_without_amp(use_amp, monkeypatch):
    from triad_amd import model

    class Emb(nn.Module):
        def __init__(self, *a, **kw):
            super().__init__()
            self.model = nn.Module()

    for name in ("AudioEmbedder", "TextEmbedder", "ViTLoRAEmbedder"):
        monkeypatch.setattr(model, name, Emb)
    monkeypatch.setattr(model, "store_frozen_base_bf16", lambda m: None)
    m = model.MultiModalModel(use_amp=use_amp)
    for emb in (m.audio_embedder, m.text_embedder, m.visual_embedder):
        assert getattr(emb, "reference_precision", False) is (not use_amp)
    assert m._head_precision() == ("bf16" if use_amp else "fp32")


@pytest.mark.parametrize("B,Nq,Nk", [(8, 20, 40), (6, 40, 70), (256, 199, 211), (5, 12, 70)])
def test_chunk_helper_stays_inside_the_budget(B, Nq, Nk):
    from triad_amd import ops
    g = ops.Geometry(B, Nq, B, Nk)
    whole = ops.split_working_bytes(g, B)
    assert ops.split_num_chunks(g, 1 << 50) == 1 and ops.split_chunk_samples(g, whole) == B
    small = whole - 1                                   # the GPU test's budget
    n = ops.split_num_chunks(g, small)
    assert n >= 2
    # two dS buffers and the three-fold slabs are in the accounting
    nkb = g.Nk_pad // 32
    assert whole >= 2 * (g.R_pad // 32) * B * nkb * 2048 + 3 * g.R_pad * 2048 + 3 * B * g.Nk_pad * 2048
    floor = ops.split_working_bytes(g, 1)
    for budget in (small, (small + floor) // 2, floor):
        chunk = ops.split_chunk_samples(g, budget)
        assert 1 <= chunk < B and ops.split_working_bytes(g, chunk) <= budget
        assert chunk == B - 1 or ops.split_working_bytes(g, chunk + 1) > budget   # the largest that fits
        assert ops.split_num_chunks(g, budget) == -(-B // chunk)
    with pytest.raises(ops.TriadError, match="ds_budget"):
        ops.split_chunk_samples(g, floor - 1)
