"""world_size-2 tests of the multi-GPU plumbing on CPU (gloo): ray sharding covers every ray
exactly once, per-ray maps are re-assembled in order on rank 0, timing takes the slowest rank."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _worker(rank, world, port, n_rays, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "danbo-pytorch_amd"))
    from core import parallel
    rb = torch.arange(n_rays * 11, dtype=torch.float32).reshape(n_rays, 11)
    cams = torch.arange(n_rays)
    mine, extra = parallel.shard_rays(rb, cams=cams, N_uniques=1)
    assert extra["N_uniques"] == 1 and extra["cams"].shape[0] == mine.shape[0]
    # a stand-in for the per-ray render result: any deterministic function of the ray
    local = dict(rgb_map=mine[:, :3] * 2.0, acc_map=mine[:, 6])
    full = parallel.gather_maps(local, n_rays, dst=0)
    slow = parallel.max_over_ranks(0.25 * (rank + 1), torch.device("cpu"))
    if rank == 0:
        ok = torch.equal(full["rgb_map"], rb[:, :3] * 2.0) and torch.equal(full["acc_map"], rb[:, 6])
        q.put((ok, slow, mine.shape[0]))
    else:
        assert full is None
        q.put((True, slow, mine.shape[0]))
    dist.destroy_process_group()


@pytest.mark.parametrize("n_rays", [64, 101])
def test_ray_sharding_and_gather_world2(n_rays):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + n_rays) % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_rays, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(r[0] for r in res)
    assert all(abs(r[1] - 0.5) < 1e-9 for r in res)          # slowest rank (rank 1: 0.5 s) everywhere
    assert sorted(r[2] for r in res) == sorted([n_rays // 2, n_rays - n_rays // 2])


def test_shard_range_partitions():
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "danbo-pytorch_amd"))
    from core.parallel import shard_range
    for n in (0, 1, 7, 262144):
        for world in (1, 2, 3, 8):
            spans = [shard_range(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            assert max(b - a for a, b in spans) - min(b - a for a, b in spans) <= 1


def _grad_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "danbo-pytorch_amd"))
    from core.trainer import allreduce_gradients
    torch.manual_seed(0)                                    # identical initial parameters on every rank
    params = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7)), torch.nn.Parameter(torch.randn(2, 2))]
    opt = torch.optim.Adam(params, lr=1e-2)
    for step in range(3):
        opt.zero_grad()
        x = torch.full((3,), float(rank + 1 + step))        # a different data shard per rank
        loss = (params[0] @ x).pow(2).sum() + (params[1] * (rank + 1)).sum()   # params[2] gets no gradient
        loss.backward()
        local = [None if p.grad is None else p.grad.clone() for p in params]
        n = allreduce_gradients(params)
        assert n == 5 * 3 + 7 + 4
        opt.step()
    q.put((rank, [p.detach().numpy().copy() for p in params], local[1].numpy(), params[1].grad.numpy().copy(),
           params[2].grad.numpy().copy()))   # numpy: torch tensors in a Queue die with the sending process
    dist.destroy_process_group()


def test_gradient_allreduce_world2_keeps_replicas_identical():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_grad_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, p0, l0, g0, z0), (_, p1, l1, g1, z1) = res
    import numpy as np
    assert np.allclose(g0, (l0 + l1) / 2) and np.array_equal(g0, g1)       # mean of the rank gradients, on both
    assert not z0.any() and not z1.any()                                   # missing gradient == zero contribution
    assert all(np.array_equal(a, b) for a, b in zip(p0, p1))               # replicas stay bit-identical


def _sync_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "danbo-pytorch_amd"))
    from run_nerf import sync_replicas
    torch.manual_seed(100 + rank)                           # ranks that (wrongly) built their networks from different streams
    net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.BatchNorm1d(5))
    net[1].running_mean.add_(float(rank))
    sync_replicas(net)
    q.put((rank, [t.detach().numpy().copy() for t in list(net.parameters()) + list(net.buffers())]))
    dist.destroy_process_group()


def test_replicas_start_identical_world2():
    """run_nerf.train seeds every rank alike while the model is built and broadcasts rank 0's parameters and buffers: without
    that, averaging gradients alone would train N different models (the advisor's finding on round 1)"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + os.getpid() % 2000
    procs = [ctx.Process(target=_sync_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    import numpy as np
    assert all(np.array_equal(a, b) for a, b in zip(res[0][1], res[1][1]))


def _fused_worker(rank, world, port, q):
    """two ranks on ONE GPU (gloo carries the collectives): the real Trainer.train_batch, fused HIP step, flat-gradient all-reduce"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(os.path.dirname(here), "danbo-pytorch_amd"), os.path.join(os.path.dirname(here), "oracle"), here):
        sys.path.insert(0, p)
    from helpers import golden
    from test_gpu_training import batch_of, build_trainer
    g = golden("danbo_perfcap_train")
    args, caster, trainer, opt = build_trainer(g, extra=["--raw_noise_std", "1.0", "--perturb", "1.0"])
    full = batch_of(g)
    n = full["rays_o"].shape[0] // world                     # whole poses per rank (4 poses, 2 ranks)
    sl = slice(rank * n, (rank + 1) * n)
    mine = {k: (v[sl] if torch.is_tensor(v) else v) for k, v in full.items()}
    mine["N_uniques"] = full["N_uniques"] // world
    torch.manual_seed(1 + rank)                              # different noise per rank, as in run_nerf.train
    losses = []
    for i in range(3):
        loss, stats = trainer.train_batch(mine, i=i, global_step=i)
        losses.append(stats["total_loss"])
    assert trainer.engine is not None, trainer.fused_reason
    torch.cuda.synchronize()
    # resume: the checkpoint holds RANK 0's (seed, counter); restored on every rank it must give each rank ITS stream back
    # at the common counter -- not rank 0's seed, not counter 0
    eng = trainer.engine
    own = eng.rng_state_dict()
    box = [own]
    dist.broadcast_object_list(box, src=0)
    eng.reseed(12345)
    eng.load_rng_state_dict(box[0])
    resumed = eng.rng_state_dict()
    q.put((rank, eng.flat_p.detach().cpu().numpy().copy(), losses, own, resumed))
    dist.destroy_process_group()


@pytest.mark.gpu
def test_fused_training_world2_on_one_gpu_keeps_replicas_bit_identical():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + os.getpid() % 2000
    procs = [ctx.Process(target=_fused_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    import numpy as np
    assert np.array_equal(res[0][1], res[1][1])              # every parameter, bit for bit, after 3 steps
    assert all(np.isfinite(l) for r in res for l in r[2]) and res[0][2] != res[1][2]    # the shards (and their losses) differ
    (own0, res0), (own1, res1) = res[0][3:5], res[1][3:5]
    assert own0["seed"] != own1["seed"] and own0["counter"] == own1["counter"] > 0
    assert res0 == own0 and res1 == own1                     # every rank continues its own stream from rank 0's checkpoint entry


def _run_bench(*flags, timeout=900):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *flags], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_gpus_flag_starts_the_ranks_itself():
    """`python bench.py --gpus 2 ...` from a shell with no RANK / WORLD_SIZE exported starts two ranks (launch_ranks) and prints ONE
    line with n_gpus = ranks_seen = 2.  --dry-run: a host no-op as the step, so the command path runs without a GPU."""
    r = _run_bench("--gpus", "2", "--dry-run", "--config", "4", "--scaling", "strong", "--steps", "4", "--warmup", "1")
    assert r["n_gpus"] == 2 and r["ranks_seen"] == 2 and r["scaling"] == "strong" and r["steps"] == 4 and r["block_steps"] == [1] * 4
    r1 = _run_bench("--dry-run", "--steps", "7", "--warmup", "0")
    assert r1["n_gpus"] == 1 and r1["ranks_seen"] == 1 and r1["block_steps"] == [2, 2, 1, 1, 1]      # --steps = the timed steps


def test_bench_value_is_units_over_the_slowest_ranks_time():
    """with UNEQUAL rank speeds (rank 0 sleeps 2 ms per step, rank 1 6 ms; gloo, world 2, no GPU) the line's
    ms_per_step is the MAX over the ranks, value = N x K x units / that time, and the line says which rank was slow:
    ms_per_step_ranks lists every rank's own time, slowest_rank_per_block names the rank behind each block's maximum."""
    r = _run_bench("--gpus", "2", "--dry-run", "--dry-run-ms", "2,6", "--steps", "50", "--warmup", "1")
    assert r["n_gpus"] == 2 and r["ranks_seen"] == 2 and len(r["block_ms"]) == 5 and r["block_steps"] == [10] * 5
    fast, slow = r["ms_per_step_ranks"]
    assert 2.0 <= fast < 4.5 and 6.0 <= slow < 8.5, r["ms_per_step_ranks"]          # each rank's OWN time (sleep + overhead)
    assert r["slowest_rank_per_block"] == [1] * 5
    assert abs(r["ms_per_step"] - slow) <= 0.05 * slow                                # the job's time is the slowest rank's
    units = r["config"]["units_per_step_and_rank"]
    assert abs(r["value"] - 2 * units / (r["ms_per_step"] * 1e-3)) <= 1e-6 * r["value"]   # whole-job units over max-over-ranks time
    assert all(b >= 6.0 for b in r["block_ms"])


@pytest.mark.gpu
def test_bench_config4_strong_scaling_on_two_ranks_of_one_gpu():
    """the real thing on the GPU box: two ranks (both on cuda:0, gloo collectives) split the reference's 16-pose / 3072-ray batch by
    whole poses; one JSON line, n_gpus = 2, 1536 rays per rank"""
    r = _run_bench("--gpus", "2", "--debug-single-device", "--config", "4", "--scaling", "strong", "--steps", "3", "--warmup", "2",
                   "--no-cpu-baseline")
    assert r["n_gpus"] == 2 and r["ranks_seen"] == 2 and r["scaling"] == "strong"
    assert r["config"]["rays"] == 3072 and r["config"]["rays_per_rank"] == 1536
    assert r["value"] > 0 and r["loss"] == r["loss"]


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["1", "4"])
def test_bench_weak_scaling_on_two_ranks_of_one_gpu(config):
    """the N > 1 path of the HEADLINE config (1: the frame, every rank its own camera view, no collective) and of
    config 4 weak (every rank its own 3072-ray batch, two in-place all-reduces per step) through the real launcher with two ranks that
    share cuda:0 (gloo carries the collectives): one line, ranks_seen = 2, per-rank lists present, and -- two ranks taking turns on one
    device -- a whole-job value close to what one rank alone reaches."""
    flags = ("--config", config, "--steps", "25", "--warmup", "1", "--no-cpu-baseline", "--no-dense", "--no-sweep", "--no-api",
             *(("--full",) if config == "4" else ()))          # --full: the collectives' events (collective_ms)
    two = _run_bench("--gpus", "2", "--debug-single-device", *flags)
    one = _run_bench("--gpus", "1", *flags)
    assert two["n_gpus"] == 2 and two["ranks_seen"] == 2 and one["n_gpus"] == 1 and two["scaling"] == "weak"
    assert len(two["ms_per_step_ranks"]) == 2 and len(two["slowest_rank_per_block"]) == 5 and all(r in (0, 1) for r in two["slowest_rank_per_block"])
    assert two["config"]["parallelism"].endswith("dp2") and two["config"]["rays"] == 2 * one["config"]["rays"] if config == "4" else True
    # the device is shared: each rank's step takes about twice as long, the job processes twice the units -> about the one-rank rate
    # for the frame; config 4's two all-reduces of the 10 MB flat gradient travel through HOST memory here (gloo: device -> host ->
    # device per step, ~3 ms against a 1.3 ms step: measured 0.46 x the one-rank rate), which the bound allows for
    lo, hi = (0.6, 3.4) if config == "1" else (0.25, 8.0)
    assert lo * one["value"] <= two["value"] <= 1.35 * one["value"], (one["value"], two["value"])
    assert 1.5 * one["ms_per_step"] <= two["ms_per_step"] <= hi * one["ms_per_step"], (one["ms_per_step"], two["ms_per_step"])
    if config == "4":
        assert two["collective_ms"] is not None and two["collective_ms"]["steps_measured"] >= 5 and "gloo" in two["collectives"]


def _nccl_world1_worker(port, q):
    """ONE rank, backend "nccl" (= RCCL on ROCm), cuda:0: the data-parallel form of Trainer.train_batch -- split step as two HIP
    graphs, the first in-place all-reduce on the comm side stream under phase 2, the second behind it, 1 / world folded into Adam --
    against the plain one-rank step of a second, identically built trainer."""
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(os.path.dirname(here), "danbo-pytorch_amd"), os.path.join(os.path.dirname(here), "oracle"), here):
        sys.path.insert(0, p)
    from helpers import golden
    from test_gpu_training import batch_of, build_trainer

    def run(parallel):
        g = golden("danbo_perfcap_train")
        args, caster, trainer, opt = build_trainer(g)         # perturb = 0, no density noise: the step is a function of the batch
        trainer.collectives_at_world_1 = parallel
        full = batch_of(g)
        grads, losses = [], []
        for i in range(4):
            loss, stats = trainer.train_batch(full, i=i, global_step=i)
            torch.cuda.synchronize()
            grads.append(trainer.engine.flat_g.detach().cpu().numpy().copy())
            losses.append(stats["total_loss"])
        eng = trainer.engine
        graphs = (eng.graph is not None, eng.graph is not None and eng.graph[4] is not None)
        return grads, losses, eng.flat_p.detach().cpu().numpy().copy(), graphs, trainer._comm_stream is not None, float(args.lrate)

    a = run(True)
    b = run(False)
    c = run(False)          # the step's own run-to-run repeatability (float atomics in the adjoints), measured the same way
    q.put((a, b, c))
    dist.destroy_process_group()


@pytest.mark.gpu
def test_fused_training_step_through_rccl_at_world_size_1():
    """Executes the nccl branch (bench.py:init_process_group("nccl"), core/trainer.py: two in-place all-reduces, one on a side
    stream between the two graph-replayed phases) -- communicator creation, stream ordering against the captured graphs and the
    in-place flat-buffer collectives, everything except the wire.  Replaces the reference's nn.DataParallel
    (core/raycasters.py:116); SURVEY 8(e).  The sum over one rank is the identity, so the gradients must equal the plain step's:
    the first step (identical parameters on both sides) within the step's own repeatability (its adjoints use float atomics:
    test_graph_replays_are_repeatable allows 1e-5 of the largest entry), the losses of every step to 1e-5 relative."""
    import numpy as np
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37500 + os.getpid() % 2000
    p = ctx.Process(target=_nccl_world1_worker, args=(port, q))
    p.start()
    (ga, la, pa, graphs_a, comm_a, lr), (gb, lb, pb, graphs_b, comm_b, _), (gc, lc, pc, _, _, _) = q.get(timeout=600)
    p.join(timeout=120)
    assert p.exitcode == 0
    assert graphs_a == (True, True) and comm_a            # two graphs (phase 1 | phase 2) and the comm stream were in use
    assert graphs_b == (True, False) and not comm_b       # the plain step: one graph, no collective
    scale = np.abs(gb[0]).max()
    noise = np.abs(gb[0] - gc[0]).max()
    assert noise <= 1e-5 * scale
    assert np.abs(ga[0] - gb[0]).max() <= max(2 * noise, 1e-6 * scale), (np.abs(ga[0] - gb[0]).max(), noise, scale)
    for x, y in zip(la, lb):
        assert np.isfinite(x) and abs(x - y) <= 1e-5 * abs(y), (la, lb)
    assert np.isfinite(pa).all() and np.abs(pa - pb).max() <= 4 * 2.5 * lr       # 4 Adam steps bound any entry's drift (|update| <~ lr)
    assert not np.array_equal(pa, np.zeros_like(pa))


@pytest.mark.gpu
def test_bench_config4_through_the_rccl_branch_at_world_1():
    """bench.py --config 4 --gpus 1 --nccl-world-1: the bench's own training loop through a one-rank nccl process group"""
    r = _run_bench("--config", "4", "--nccl-world-1", "--steps", "3", "--warmup", "2", "--no-cpu-baseline")
    assert r["n_gpus"] == 1 and "nccl" in r["collectives"] and "forced at world 1" in r["collectives"]
    assert r["value"] > 0 and r["loss"] == r["loss"] and len(r["block_ms"]) >= 3
