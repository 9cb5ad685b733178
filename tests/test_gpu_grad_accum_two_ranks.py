"""Accumulated, clipped step in a data-parallel run (-m gpu): two processes share the one GPU of the test box (gloo carries
the device tensors, comm="torch", as in tests/test_gpu_dist_two_ranks.py). Each rank runs PLBertTrainer.step_accumulated over
its 2 micro-batches with max_grad_norm small enough to clip: ONE exchange after LAST, grad_scale = 1 / (world * 2), the norm
taken after the exchange. Both ranks must end bit-identical, with the same norm and coefficient, and agree with a single rank
that accumulates all 4 micro-batches (grad_scale = 1/4) within the bounds of two bf16 evaluations in another summation
order (tests/test_gpu_grad_accum.py)."""
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

MAX_NORM = 0.02
CHILD_SECONDS = 240


def _setup():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import plbert_amd

    pcfg = plbert_amd.AlbertConfig(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2,
                                   intermediate_size=256, num_hidden_layers=2, max_position_embeddings=512)
    sd = plbert_amd.deterministic_state_dict(pcfg, 188, seed=9)
    micro = [plbert_amd.synthetic_batch(2, 32, seed=50 + i) for i in range(4)]
    return plbert_amd, pcfg, sd, micro


def _trainer(pcfg, sd, **kw):
    from plbert_amd.train import PLBertTrainer
    return PLBertTrainer(pcfg, 188, max_batch=2, max_seq=32, lr=1e-3, state_dict=sd, max_grad_norm=MAX_NORM, **kw)


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _, pcfg, sd, micro = _setup()
    torch.cuda.set_device(0)
    tr = _trainer(pcfg, sd, comm="torch")
    assert tr.world == world and tr.reducer.active and tr.comm == "torch"
    mine = [tr.stage_batch(*micro[2 * rank + i]) for i in range(2)]
    loss = tr.step_accumulated(mine)
    torch.cuda.synchronize()
    assert tr.engine.status()["ln_exchange_timeouts"] == 0 and tr.step_count == 1
    out[rank] = (float(loss.item()), tr.engine.params.cpu().numpy(), tr.last_grad_norm.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_accumulate_clip_and_stay_identical():
    world = 2
    port = 29700 + (os.getpid() % 2000)
    with mp.Manager() as mgr:
        out = mgr.dict()
        ctx = mp.spawn(_worker, args=(world, port, out), nprocs=world, join=False)
        deadline = time.monotonic() + CHILD_SECONDS        # every child under a time limit of its own
        done = False
        while not done and time.monotonic() < deadline:
            done = ctx.join(timeout=5)
        if not done:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
            pytest.fail(f"a rank did not finish within {CHILD_SECONDS} s")
        res = dict(out)
    _, pcfg, sd, micro = _setup()
    (l0, p_r0, n_r0), (l1, p_r1, n_r1) = res[0], res[1]
    assert np.array_equal(p_r0.view(np.int32), p_r1.view(np.int32))                   # replicas stay bit-identical
    assert np.array_equal(n_r0[:2].view(np.int32), n_r1[:2].view(np.int32))         # one norm, one coefficient
    assert 0.0 < n_r0[1] < 1.0 and n_r0[2] == 0.0 and n_r0[3] == 0.0                # ... and it clipped
    # a single rank over the same 4 micro-batches
    one = _trainer(pcfg, sd)
    p0 = one.engine.params.clone()
    loss = one.step_accumulated([one.stage_batch(*m) for m in micro])
    torch.cuda.synchronize()
    n = one.engine.trainable
    p1 = one.engine.params.cpu().numpy()
    got_n = one.last_grad_norm.cpu().numpy()
    assert abs(0.5 * (l0 + l1) - float(loss.item())) <= 1e-4 * float(loss.item())
    rel = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b.astype(np.float64)))
    du_ranks, du_one = p_r0[:n] - p0.cpu().numpy()[:n], p1[:n] - p0.cpu().numpy()[:n]
    print(f"norm ranks {n_r0[0]!r} one {got_n[0]!r}; coef {n_r0[1]!r} / {got_n[1]!r}; update rel {rel(du_ranks, du_one):.3e}")
    assert abs(n_r0[0] - got_n[0]) <= 1.5e-2 * got_n[0] and abs(n_r0[1] - got_n[1]) <= 1.5e-2 * got_n[1]
    assert rel(du_ranks, du_one) < 1.5e-2
    assert np.abs(du_one).max() > 0.5e-3
    assert np.array_equal(p_r0[n:], p0.cpu().numpy()[n:])                           # the pooler never trains
