"""Multi-process (world_size 2, gloo, CPU) tests of the data-parallel collectives.

Mode G (global negatives, triad_amd.dist + ops.contrastive_head(group=...)): each rank
holds B_l triples; the sharded computation -- gather keys, local clip rows, gather clip
rows, all-reduce the regulariser sums, identical loss head, reduce-scatter key grads --
must reproduce the single-process reference loss and gradients at B_g = 2 B_l. The
per-rank compute here is the CPU oracle (the HIP kernels need a GPU; their parity is
tested on the box); the collectives are triad_amd.dist's.

Mode R: the bucketed flat-gradient all-reduce averages gradients.
"""
import os
import socket

import pytest
import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import ref_cpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _global_inputs(Bg=4, Na=9, Nv=12, seed=5):
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(Bg, Na, 512, generator=g) * 0.58).double()
    V = (torch.randn(Bg, Nv, 512, generator=g) * 0.58).double()
    V[1, 9:] = 0  # patch-dropout zero padding on one sample
    return A, V


def _mode_g_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from triad_amd import dist as tdist
        A, V = _global_inputs()
        Bg = A.shape[0]
        Bl = Bg // world
        Na, Nv = A.shape[1], V.shape[1]
        A_l = A[rank * Bl:(rank + 1) * Bl].clone().requires_grad_(True)
        V_l = V[rank * Bl:(rank + 1) * Bl].clone()
        temp = torch.tensor(1.5, dtype=torch.float64, requires_grad=True)
        # 1) all-gather the key tokens (rank-major rows)
        Vg = tdist.gather_keys(V_l.reshape(Bl * Nv, 512), Bg * Nv).reshape(Bg, Nv, 512).requires_grad_(True)
        # 2) local query rows of the similarity tensor / clip matrix
        S = torch.einsum("iqd,jvd->ijqv", A_l, Vg) * temp            # (Bl, Bg, Na, Nv)
        clip_l = S.max(dim=3).values.mean(dim=2)                      # (Bl, Bg)
        nn_sum = S.clamp(-60, 0).pow(2).sum()
        diag = torch.stack([S[i, rank * Bl + i] for i in range(Bl)])  # this rank's diagonal pairs
        d = diag[:, 1:] - diag[:, :-1]
        sm_sum = (d * d).sum()
        # 3) gather clip rows, all-reduce the regulariser sums (values only; grads flow locally)
        clip_full_val = tdist.gather_rows(clip_l.detach().contiguous())
        sums_val = tdist.allreduce_sum(torch.stack([nn_sum.detach(), sm_sum.detach()]))
        # splice the local rows back in so autograd sees this rank's contribution
        clip_full = torch.cat([clip_full_val[:rank * Bl], clip_l, clip_full_val[(rank + 1) * Bl:]])
        nn_tot = nn_sum + (sums_val[0] - nn_sum.detach())
        sm_tot = sm_sum + (sums_val[1] - sm_sum.detach())
        l_nn = nn_tot / (Bg * Bg * Na * Nv)
        l_sm = sm_tot / (Bg * (Na - 1) * Nv)
        l_cal = (-torch.log(temp)).clamp(min=0).pow(2)
        ce = ref_cpu._symmetric_ce(clip_full)
        total = ce + 20 * l_cal + 0.15 * l_nn + 0.01 * l_sm
        g_cal = torch.autograd.grad(20 * l_cal, temp, retain_graph=True)[0]
        # every rank computes the identical loss; its gradient is the full-loss gradient
        # through this rank's tensors -> key grads are reduce-scattered, the rest summed.
        total.backward()
        dV_l = tdist.reduce_scatter_rows(Vg.grad.reshape(Bg * Nv, 512), Bl * Nv).reshape(Bl, Nv, 512)
        dt = temp.grad.clone()
        # only rank 0 keeps the (replicated) l_cal contribution when gradients are summed
        if rank != 0:
            dt -= g_cal
        dt = tdist.allreduce_sum(dt.reshape(1))
        q.put((rank, float(total), A_l.grad.numpy(), dV_l.numpy(), float(dt)))
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc(), None, None))
        raise
    finally:
        dist.destroy_process_group()


def test_mode_g_global_negatives_matches_single_process():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mode_g_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert r[1] != "error", r[2]
    A, V = _global_inputs()
    Ar, Vr = A.clone().requires_grad_(True), V.clone().requires_grad_(True)
    t = torch.tensor(1.5, dtype=torch.float64, requires_grad=True)
    total, *_ = ref_cpu.av_loss(Ar, Vr, t)
    total.backward()
    Bl = A.shape[0] // world
    for rank, tot, dA, dV, dt in res:
        assert abs(tot - float(total)) < 1e-9 * abs(float(total))
        torch.testing.assert_close(torch.from_numpy(dA), Ar.grad[rank * Bl:(rank + 1) * Bl], rtol=1e-9, atol=1e-12)
        torch.testing.assert_close(torch.from_numpy(dV), Vr.grad[rank * Bl:(rank + 1) * Bl], rtol=1e-9, atol=1e-12)
        assert abs(dt - float(t.grad)) < 1e-9 * abs(float(t.grad)) + 1e-12


def _mode_r_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from triad_amd import dist as tdist
        flat = torch.arange(10, dtype=torch.float32) * (rank + 1)
        tdist.allreduce_grads(flat, bucket_elems=3, average=True)
        q.put((rank, flat.tolist()))
    finally:
        dist.destroy_process_group()


def test_mode_r_bucketed_average():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mode_r_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    for _, v in res:
        assert v == [1.5 * i for i in range(10)]


class _Net(torch.nn.Module):
    """Three layers; the middle weight is held as a bf16 'shadow' model weight (its autograd
    gradient arrives in bf16 and is folded into the flat fp32 buffer by the reducer's hook)."""

    def __init__(self):
        super().__init__()
        self.l1 = torch.nn.Linear(16, 300)
        self.w2 = torch.nn.Parameter(torch.randn(200, 300) * 0.05)
        self.l3 = torch.nn.Linear(200, 4)

    def forward(self, x, skip_w2=False):
        h = torch.relu(self.l1(x))
        # skip_w2: like a LayerDrop'd layer on one rank only -- w2 gets no gradient there
        h = h[:, :200] if skip_w2 else torch.relu(h @ self.w2.float().t())
        return self.l3(h)


def _net_inputs(rank, step):
    g = torch.Generator().manual_seed(100 * step + rank)
    return torch.randn(8, 16, generator=g), torch.randn(8, 4, generator=g)


def _skips(skip, rank, step):
    """Does `rank` skip w2 in `step`? "one": rank 1 only (a layer LayerDrop dropped on one rank),
    "both": every rank (a layer no rank used -- e.g. the idle modality of an av_focus step)."""
    return step == 1 and (skip == "both" or (skip == "one" and rank == 1))


class _PerturbedCheck:
    """A reducer whose check reference differs from what the overlapped reduction saw (its
    snapshot perturbed in one element): the gate must report it."""

    @staticmethod
    def make(tdist, *a, **kw):
        class R(tdist.GradBucketReducer):
            def _check_reference(self):
                self._snap_range(self.order[0])[0] += 1e-3
                super()._check_reference()
        return R(*a, **kw)


def _reducer_worker(rank, world, port, wire, q, skip=False, check=None):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from triad_amd import dist as tdist
        from triad_amd import optim as fo
        torch.manual_seed(0)
        net = _Net()
        params = list(net.parameters())
        space = fo.FlatParamSpace(params, "cpu", shadow=[net.w2])
        mk = _PerturbedCheck.make if check == "perturbed" else (lambda t, *a, **kw: t.GradBucketReducer(*a, **kw))
        red = mk(tdist, space, bucket_mb=0.01, wire=wire, average=True)   # ~2.6k elems per bucket
        out, checks = [], []
        for step in range(3):
            space.zero_grad(list(range(len(params))))
            x, y = _net_inputs(rank, step)
            red.check = check is not None and step == 2
            red.begin(accumulate=False)
            ((net(x, skip_w2=_skips(skip, rank, step)) - y) ** 2).mean().backward()
            launched = red.launched_in_backward
            red.finish()
            out.append((space.flat_g.numpy().copy(), launched, list(red.order), space.touched.copy()))
            checks.append(red.check_result)
            red.check_result = None
        q.put((rank, out, len(red.buckets), checks))
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("wire,skip", [("fp32", False), ("bf16", False), ("fp32", "one"), ("fp32", "both")])
def test_overlapped_bucket_reducer_averages_gradients(wire, skip):
    """GradBucketReducer (Mode R) on two gloo ranks: after each step the flat gradient buffer is
    the average of the ranks' gradients (bf16 master weight folded in by the hook); the launch
    order is fixed after the first step and identical on both ranks; from the second step on,
    buckets are launched from the gradient hooks while backward is still running. skip "one": in
    step 1 rank 1 produces no gradient for one parameter (a layer LayerDrop skipped on that rank
    only): its bucket is flushed after backward, in the same order on both ranks, the average
    counts the missing gradient as zero, and the parameter counts as having a gradient on BOTH
    ranks (rank 0 produced one). skip "both": no rank produces it -- it must count as having no
    gradient on either rank, so AdamW leaves it alone (as torch skips a .grad of None,
    SajayR/TRIAD train.py:1010-1040; ADVICE r3: av_focus must not decay the text weights)."""
    from triad_amd import optim as fo
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reducer_worker, args=(r, world, port, wire, q, skip)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert r[1] != "error", r[2]
    nb = res[0][2]
    assert nb >= 3
    # single-process reference: the average of the two ranks' gradients, same flat layout
    torch.manual_seed(0)
    net = _Net()
    space = fo.FlatParamSpace(list(net.parameters()), "cpu", shadow=[net.w2])
    tol = 1e-6 if wire == "fp32" else 8e-3
    for step in range(3):
        acc = torch.zeros_like(space.flat_g)
        for rank in range(world):
            space.zero_grad(list(range(len(space.params))))
            x, y = _net_inputs(rank, step)
            ((net(x, skip_w2=_skips(skip, rank, step)) - y) ** 2).mean().backward()
            i = space.index[id(net.w2)]   # fold the bf16 shadow gradient by hand (the HIP gather needs a GPU)
            if net.w2.grad is not None:
                space.flat_g[space.offsets[i]:space.offsets[i] + net.w2.numel()].copy_(net.w2.grad.float().view(-1))
            net.w2.grad = None
            acc += space.flat_g / world
        for rank in range(world):
            got, launched, order, touched = res[rank][1][step]
            # a parameter has a gradient on EVERY rank iff some rank produced one (the optimizer
            # then steps, counts and clips the same set everywhere)
            want = np.ones(len(space.params), dtype=bool)
            if skip == "both" and step == 1:
                want[space.index[id(net.w2)]] = False
            assert (touched == want).all(), (step, rank, touched)
            err = float((torch.from_numpy(got) - acc).abs().max() / acc.abs().max())
            assert err < tol, (wire, step, rank, err)
            assert sorted(order) == list(range(nb))
            assert order == res[0][1][step][2]
            if step == 0:
                assert launched == 0
            elif not (skip and _skips(skip, rank, step)):
                assert launched >= 1   # overlap: at least one bucket went out during backward
            # (skip, rank 1, step 1: the bucket of the missing gradient heads the launch order, so
            # that rank issues everything at the flush -- in the same order as rank 0)


@pytest.mark.parametrize("wire,check", [("fp32", "clean"), ("bf16", "clean"), ("fp32", "perturbed")])
def test_reducer_check_gate(wire, check):
    """the reducer's correctness gate (bench.py --full --gpus N > 1 prints its result).
    With `check` set for a step, every bucket's pre-reduction gradient is snapshotted, the same
    buckets are all-reduced again from the snapshots after backward, in the same order, and the
    two results are compared bit for bit (max over ranks): equal on a clean run (fp32 and bf16
    wire), and a difference in one element is reported (equal False, its size as max_abs)."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reducer_worker, args=(r, world, port, wire, q, False, check)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert r[1] != "error", r[2]
    for rank in range(world):
        checks = res[rank][3]
        assert checks[0] is None and checks[1] is None
        c = checks[2]
        assert c["world_size"] == world and c["backend"] == "gloo" and c["buckets"] == res[rank][2]
        assert c["launched_in_backward"] >= 1
        if check == "clean":
            assert c["equal"] and c["max_abs"] == 0.0, c
        else:
            assert not c["equal"] and c["max_abs"] > 0, c


# ---- world 4: per-rank LayerDrop skips and a staged unfreeze ------------------------------------
def _skip4(rank, step):
    """w2 skipped by: step 1 ranks 1 and 3 (per-rank LayerDrop draws), step 3 every rank."""
    return (step == 1 and rank in (1, 3)) or step == 3


def _frozen4(step):
    """l1 frozen before step 2, trainable from step 2 on (train.py:527-548's staged unfreeze)."""
    return step < 2


def _reducer_worker4(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from triad_amd import dist as tdist
        from triad_amd import optim as fo
        torch.manual_seed(0)
        net = _Net()
        params = list(net.parameters())
        space = fo.FlatParamSpace(params, "cpu", shadow=[net.w2])
        red = tdist.GradBucketReducer(space, bucket_mb=0.01, wire="fp32", average=True)
        out = []
        for step in range(5):
            for p in net.l1.parameters():
                p.requires_grad = not _frozen4(step)
            space.zero_grad(list(range(len(params))))
            x, y = _net_inputs(rank, step)
            red.begin(accumulate=False)
            ((net(x, skip_w2=_skip4(rank, step)) - y) ** 2).mean().backward()
            red.finish()
            out.append((space.flat_g.numpy().copy(), list(red.order), space.touched.copy()))
        q.put((rank, out))
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


def test_bucket_reducer_world4_layerdrop_and_unfreeze():
    """GradBucketReducer on FOUR gloo ranks over five steps with per-rank LayerDrop
    skips (step 1: ranks 1 and 3 produce no gradient for w2), a staged unfreeze (l1 trainable from
    step 2: the launch order is re-derived at that step, identically on every rank) and a layer
    no rank uses (step 3). Every step: the reduced buffer is the average of the four ranks'
    gradients (zeros for the ranks that skipped), identical launch order on all ranks, and the
    touched set = parameters SOME rank produced a gradient for (frozen l1 never; w2 at step 1 on
    every rank, at step 3 on none)."""
    from triad_amd import optim as fo
    world = 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reducer_worker4, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert r[1] != "error", r[2]
    torch.manual_seed(0)
    net = _Net()
    space = fo.FlatParamSpace(list(net.parameters()), "cpu", shadow=[net.w2])
    i_w2 = space.index[id(net.w2)]
    l1_ids = [space.index[id(p)] for p in net.l1.parameters()]
    for step in range(5):
        for p in net.l1.parameters():
            p.requires_grad = not _frozen4(step)
        acc = torch.zeros_like(space.flat_g)
        for rank in range(world):
            space.zero_grad(list(range(len(space.params))))
            x, y = _net_inputs(rank, step)
            ((net(x, skip_w2=_skip4(rank, step)) - y) ** 2).mean().backward()
            if net.w2.grad is not None:
                space.flat_g[space.offsets[i_w2]:space.offsets[i_w2] + net.w2.numel()].copy_(
                    net.w2.grad.float().view(-1))
            net.w2.grad = None
            acc += space.flat_g / world
        want = np.ones(len(space.params), dtype=bool)
        if _frozen4(step):
            want[l1_ids] = False
        if step == 3:
            want[i_w2] = False
        for rank in range(world):
            got, order, touched = res[rank][1][step]
            err = float((torch.from_numpy(got) - acc).abs().max() / acc.abs().max())
            assert err < 1e-6, (step, rank, err)
            assert order == res[0][1][step][1], (step, rank)
            assert (touched == want).all(), (step, rank, touched, want)
