"""GPU (-m gpu): the N > 1 layout of the operator with the HIP path doing the compute.  Two ranks share the one GPU of the
box (transport = gloo through host staging; RCCL needs one GPU per rank), each runs ``plugin.MixQLinear(tp_size=2)`` on
its row shard of W through the C ABI, and the gathered output must equal

  * the CPU oracle of the UNSHARDED layer bit for bit on a fixture whose fp16 outlier products are exact in fp32 in any
    summation order (integer-valued outlier activations / weights), bias included, and
  * the oracle within the north-star 1e-3 on ordinary data (Qwen2-7B qkv shape, which has a bias: BASELINE configs[3]).

Covers plugin.py:137-162 (forward, bias after the collective in the reference) under SURVEY 8e's row sharding."""
import os
import socket
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def exact_fixture(M, N, K, seed, O=128):
    """Packed tensors + activations for which every fp32 partial sum of the outlier GEMM is an integer < 2^24."""
    rng = np.random.default_rng(seed)
    ind = rng.permutation(K)[:O].astype(np.int32)
    W8 = rng.integers(-127, 128, size=(N, K), dtype=np.int8)
    W8[:, ind] = 0
    sW = (rng.random(N) * 4e-4 + 4e-4).astype(np.float16)
    fpw = rng.integers(-3, 4, size=(N, O)).astype(np.float16)
    A = rng.standard_normal((M, K)).astype(np.float16)
    A[:, ind] = rng.integers(-60, 61, size=(M, O)).astype(np.float16)
    bias = (rng.standard_normal(N) * 0.5).astype(np.float16)
    packed = dict(weight=W8, weights_scaling_factor=sW, fp_weight=fpw, fp_ind=ind,
                  qweight=np.zeros((K, N), np.uint8), bias=bias)
    return A, packed


def ordinary_fixture(M, N, K, seed):
    sys.path.insert(0, ROOT)
    from mixq_tensorrt_llm_amd import pack
    rng = np.random.default_rng(seed)
    act = np.abs(rng.standard_normal(K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) * 0.02).astype(np.float16)
    A = rng.standard_normal((M, K)).astype(np.float32)
    p = pack.pack_linear_weights(torch.from_numpy(W), torch.from_numpy(act))
    A[:, p["fp_ind"]] *= 20
    p["bias"] = (rng.standard_normal(N) * 0.5).astype(np.float16)
    return A.astype(np.float16), p


CASES = [  # (name, M, N, K, exact)
    ("exact_small", 40, 512, 512, True),
    ("exact_pp_tiles", 300, 1024, 1024, True),
    ("qwen2_qkv_bias", 48, 4608, 3584, False),
    ("llama2_70b_qkv", 40, 10240, 8192, False),   # BASELINE configs[4] shapes (here sharded 2 ways; 8 ways = 1280 rows)
    ("llama2_70b_proj_decode_batch", 16, 8192, 28672, False),   # long K: the small-tile K split over workgroups per shard
]


def _worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from oracle.oracle import usable_cpus
    os.environ["OMP_NUM_THREADS"] = str(max(1, usable_cpus() // world))   # `world` oracles run side by side
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import oracle
    from conftest import elementwise_violations, prefill_slack, ulp16
    from mixq_tensorrt_llm_amd import parallel, plugin
    ok, notes = True, []
    for name, M, N, K, exact in CASES:
        A, full = exact_fixture(M, N, K, 5) if exact else ordinary_fixture(M, N, K, 6)
        mine = parallel.shard_packed(full, world, rank)
        n0, n1 = parallel.shard_bounds(N, world, rank)
        assert mine["bias"].shape == (n1 - n0,)
        Ad = torch.from_numpy(A).cuda()
        want_nb, parts = oracle.linear_prefill(A, full["weight"], full["weights_scaling_factor"], full["fp_weight"],
                                               full["fp_ind"], return_parts=True)
        slack_nb = prefill_slack(parts, A, full)
        for with_bias in (False, True):
            want, slack = want_nb, slack_nb
            if with_bias:  # plugin.py:158-160: one fp16 addition per element after the operator (one more ulp of the un-biased value)
                want = (torch.from_numpy(want_nb) + torch.from_numpy(full["bias"])).numpy()
                slack = slack_nb + ulp16(want_nb)
            for gather in (True, False):
                layer = plugin.MixQLinear(K, N, bias=with_bias, tp_size=world, tp_group=None, gather_output=gather,
                                          device="cuda:0").load(mine)
                assert layer.out_features == N // world and (layer.bias is None or layer.bias.shape == (N // world,))
                got = layer(Ad).cpu().numpy()
                ref = want if gather else want[:, n0:n1]
                sl = slack if gather else slack[:, n0:n1]
                if got.shape != ref.shape:
                    ok = False
                    notes.append(f"{name} bias={with_bias} gather={gather}: shape {got.shape} vs {ref.shape}")
                    continue
                if exact:
                    good = np.array_equal(got.view(np.uint16), ref.view(np.uint16))
                else:   # north_star's 1e-3 of the maximum AND element by element
                    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max() / np.abs(ref).max()
                    bad, _, _ = elementwise_violations(got, ref, sl)
                    good = err < 1e-3 and not bad.any()
                    if bad.any():
                        notes.append(f"{name}: {int(bad.sum())} of {bad.size} outputs outside the element-wise bound")
                if not good:
                    ok = False
                    notes.append(f"{name} bias={with_bias} gather={gather}: mismatch")
                # 3-D activations keep their leading dims through the gather
                if gather and M % 2 == 0 and with_bias:
                    g3 = layer(Ad.reshape(2, M // 2, K))
                    ok &= tuple(g3.shape) == (2, M // 2, N) and np.array_equal(
                        g3.reshape(M, N).cpu().numpy().view(np.uint16), got.view(np.uint16))
    open(os.path.join(tmp, f"ok{rank}"), "w").write("1" if ok else "0\n" + "\n".join(notes))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_mixqlinear_row_sharded_ranks_one_gpu(tmp_path, oracle, world):
    """MixQLinear(tp_size = world) over the RCCL-shaped transport (gloo staging here): 2-way and 4-way shards (the 4-way ones,
    2560 / 2048 / 1152 rows, select other kernels than the 2-way ones), with and without bias / gather.  At most four ranks: with
    the test process itself, five processes have the GPU open."""
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        res = open(tmp_path / f"ok{r}").read()
        assert res == "1", f"rank {r}: {res}"


# ------------------------------------------------------------------- peer-write all-gather (csrc/tp_kernels.hip) ---
def _peer_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mixq_tensorrt_llm_amd import parallel
    ok, notes = True, []
    try:
        max_m, N = 700, 1024
        pg = parallel.PeerGather(max_m, N, world, rank, "cuda:0")
        n_loc = N // world
        g = torch.Generator(device="cpu").manual_seed(100)          # same stream of numbers on both ranks
        for call, m in enumerate([700, 33, 256, 1, 0, 699, 700, 512, 0, 8]):  # both parities, m < max_m, EMPTY calls (flags still published)
            full = torch.randn((m, N), generator=g).to(torch.float16)
            mine = full[:, rank * n_loc:(rank + 1) * n_loc].contiguous().cuda()
            got = pg.gather(mine)
            torch.cuda.synchronize()
            if not torch.equal(got.cpu(), full):
                ok = False
                notes.append(f"call {call} m={m}: gathered tensor differs")
            # the gloo staging path must agree (same contract, different transport)
            ref = parallel.all_gather_columns(mine, None, world)
            ok &= torch.equal(ref.cpu(), full)
        ok &= not pg.timed_out()
        pg.check(sync=True)
        ok &= pg.data_kind == "finegrained" and pg.flag_kind == "uncached"   # what a remote GPU writes is never coarse-grained
        # a capturing stream is refused (host-side sequence number / parity: a replay would read stale flags)
        gr = torch.cuda.CUDAGraph()
        refused = False
        try:
            with torch.cuda.graph(gr):
                pg.gather(mine)
        except RuntimeError as e:
            refused = "not graph-capturable" in str(e)
        except Exception:  # noqa: BLE001
            pass
        ok &= refused
        if not refused:
            notes.append("gather under graph capture was not refused")
        # through the layer: MixQLinear(tp_size=2, gather_output=True) with the peer transport == the gloo transport
        from mixq_tensorrt_llm_amd import plugin
        A, full_p = exact_fixture(64, 512, 512, 5)
        mine_p = parallel.shard_packed(full_p, world, rank)
        layer = plugin.MixQLinear(512, 512, bias=True, tp_size=world, gather_output=True, device="cuda:0").load(mine_p)
        want = layer(torch.from_numpy(A).cuda()).cpu()
        layer.peer_gather = parallel.PeerGather(64, 512, world, rank, "cuda:0")
        got = layer(torch.from_numpy(A).cuda())
        torch.cuda.synchronize()
        ok &= torch.equal(got.cpu(), want)
        # the layer's result is the caller's own tensor, not a view of a buffer overwritten two calls later
        got2 = layer(torch.from_numpy(A * 0.5).cuda())
        got3 = layer(torch.from_numpy(A * 0.25).cuda())
        torch.cuda.synchronize()
        ok &= torch.equal(got.cpu(), want) and got.data_ptr() not in (got2.data_ptr(), got3.data_ptr())
        layer.peer_gather.close()
        pg.close()
    except Exception as e:  # noqa: BLE001
        import traceback
        ok = False
        notes.append(traceback.format_exc())
    open(os.path.join(tmp, f"peer{rank}"), "w").write("1" if ok else "0\n" + "\n".join(notes))
    dist.barrier()
    dist.destroy_process_group()


def test_peer_write_allgather_two_ranks_one_gpu(tmp_path, oracle):
    """One-sided peer writes + flags between two processes (IPC-mapped buffers; both ranks on the one GPU of the box, so
    the 'peer' memory is local -- the protocol, the IPC plumbing, the column placement and the double buffering are what
    is covered; xGMI itself needs a multi-GPU node)."""
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_peer_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        res = open(tmp_path / f"peer{r}").read()
        assert res == "1", f"rank {r}: {res}"


def _timeout_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mixq_tensorrt_llm_amd import parallel
    ok, notes = True, []
    try:
        pg = parallel.PeerGather(64, 256, world, rank, "cuda:0", patience_ms=300)
        x = torch.full((64, 128), float(rank + 1), dtype=torch.float16, device="cuda:0")
        got = pg.gather(x)                       # call 1: both ranks -> fine
        torch.cuda.synchronize()
        pg.check()
        ok &= bool((got[:, :128] == 1).all() and (got[:, 128:] == 2).all())
        dist.barrier()
        if rank == 0:                            # call 2: rank 1 never pushes -> rank 0's wait gives up after 300 ms
            import time
            t0 = time.perf_counter()
            pg.gather(x)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ok &= 0.25 < dt < 5.0
            raised = 0
            try:
                pg.check()
            except parallel.PeerGatherTimeout as e:
                raised += "call 2" in str(e)
            try:                                  # sticky: the next gather refuses on the host, without a device sync
                pg.gather(x)
            except parallel.PeerGatherTimeout:
                raised += 1
            ok &= raised == 2 and pg.timed_out()
            if raised != 2:
                notes.append(f"timeout not surfaced (raised={raised}, dt={dt:.2f})")
        dist.barrier()
        pg.close()
    except Exception:  # noqa: BLE001
        import traceback
        ok = False
        notes.append(traceback.format_exc())
    open(os.path.join(tmp, f"to{rank}"), "w").write("1" if ok else "0\n" + "\n".join(notes))
    dist.barrier()
    dist.destroy_process_group()


def _soak_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mixq_tensorrt_llm_amd import parallel
    ok, notes = True, []
    try:
        max_m, N, calls = 2048, 1536, (240 if world == 2 else 120)
        n_loc = N // world
        pg = parallel.PeerGather(max_m, N, world, rank, "cuda:0")
        rng = np.random.default_rng(5)                              # the same sequence of sizes and delays on both ranks
        ms = [int(m) for m in rng.integers(0, max_m + 1, calls)]
        lag = rng.integers(0, world + 2, calls)                     # who is late on call c: 0 nobody, r + 1 that rank, world + 1 everybody
        bad = torch.zeros((), dtype=torch.int64, device="cuda:0")
        cols = torch.arange(N, device="cuda:0", dtype=torch.float32)
        for c, m in enumerate(ms):
            # element (call, row, col) -> a value every rank can recompute: integers below 2048 are exact in fp16
            rows = torch.arange(m, device="cuda:0", dtype=torch.float32)
            full = ((rows[:, None] * 7 + cols[None, :] * 3 + c * 11) % 2039).to(torch.float16)
            mine = full[:, rank * n_loc:(rank + 1) * n_loc].contiguous()
            if lag[c] == rank + 1 or lag[c] == world + 1:
                torch.cuda._sleep(int(rng.integers(1, 40)) * 100000)   # this rank arrives late (device-side delay, no host sync)
            else:
                rng.integers(1, 40)                                    # (keep the two generators in step)
            got = pg.gather(mine)                                      # NO synchronisation between calls: back-to-back gathers,
            bad += (got != full).sum()                                 # both parities in flight, producers ahead of or behind consumers
        torch.cuda.synchronize()
        pg.check(sync=True)
        nbad = int(bad.item())
        if nbad or pg.timed_out():
            ok = False
            notes.append(f"{nbad} wrong elements over {calls} back-to-back gathers, timed_out={pg.timed_out()}")
        pg.close()
    except Exception:  # noqa: BLE001
        import traceback
        ok = False
        notes.append(traceback.format_exc())
    open(os.path.join(tmp, f"soak{rank}"), "w").write("1" if ok else "0\n" + "\n".join(notes))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_peer_gather_soak_back_to_back_with_skew(tmp_path, world):
    """240 (4 ranks: 120) back-to-back gathers of random sizes (0..2048 rows) with NO host synchronisation in between and
    device-side delays that make one rank, another, or all arrive late: the sequence flags (4 ranks: four producers' flag blocks
    in every consumer) and the two-buffer rotation under load, every element of every gather checked on the device.
    (All ranks on the one GPU: protocol, not link, coverage.)"""
    import torch.multiprocessing as mp
    mp.spawn(_soak_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        res = open(tmp_path / f"soak{r}").read()
        assert res == "1", f"rank {r}: {res}"


def test_lost_peer_surfaces_as_an_error_not_a_stale_tensor(tmp_path):
    """VERDICT r2 / ADVICE r2: a wait that gives up must not leave a silently stale tensor behind -- the status word is
    sticky, host-visible without a device sync, and every later gather / check raises."""
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_timeout_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        res = open(tmp_path / f"to{r}").read()
        assert res == "1", f"rank {r}: {res}"


def _slow_peer_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import time

    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mixq_tensorrt_llm_amd import parallel
    ok, notes = True, []
    try:
        pg = parallel.PeerGather(64, 256, world, rank, "cuda:0", capturable=True, patience_ms=300)
        x1 = torch.full((64, 128), float(rank + 1), dtype=torch.float16, device="cuda:0")
        got = pg.gather(x1)                      # call 1: both ranks arrive -> fine; `got` is this rank's ONE destination buffer
        torch.cuda.synchronize()
        pg.check()
        ok &= bool((got[:, :128] == 1).all() and (got[:, 128:] == 2).all())
        snapshot = got.clone()
        dist.barrier()
        x2 = torch.full((64, 128), float(10 * (rank + 1)), dtype=torch.float16, device="cuda:0")
        if rank == 0:
            # call 2: rank 1 is SLOW (it has not reached the call: it may still be reading call 1's tensor).  Rank 0's arrive gives up
            # after 300 ms; its push must then leave rank 1's buffer alone and publish nothing.
            pg.gather(x2)
            torch.cuda.synchronize()
            ok &= pg.timed_out()
            if not pg.timed_out():
                notes.append("rank 0: the arrive of call 2 did not time out")
            open(os.path.join(tmp, "slow_rank0_done"), "w").write("1")
        else:
            t0 = time.perf_counter()
            while not os.path.exists(os.path.join(tmp, "slow_rank0_done")) and time.perf_counter() - t0 < 30:
                time.sleep(0.05)                 # "reading" call 1's tensor for longer than the producer's patience
            torch.cuda.synchronize()
            same = bool((got == snapshot).all())  # the single destination buffer was NOT overwritten behind the slow reader's back
            ok &= same
            if not same:
                notes.append("rank 1: its destination buffer was overwritten although it never acknowledged call 2")
            pg.gather(x2)                        # the late call: rank 0 published nothing, so this wait times out -- an error, not a torn tensor
            torch.cuda.synchronize()
            ok &= pg.timed_out()
            if not pg.timed_out():
                notes.append("rank 1: its late call 2 did not surface the failure")
        dist.barrier()
        pg.close()
    except Exception:  # noqa: BLE001
        import traceback
        ok = False
        notes.append(traceback.format_exc())
    open(os.path.join(tmp, f"slow{rank}"), "w").write("1" if ok else "0\n" + "\n".join(notes))
    dist.barrier()
    dist.destroy_process_group()


def test_capturable_gather_does_not_overwrite_a_slow_peers_buffer(tmp_path):
    """in the capturable form every rank has ONE destination buffer whose reuse is acknowledged by `mixq_tp_arrive`.  When that
    arrive times out (a peer that is merely slow), the push that follows on the stream must not store into the peer's buffer nor publish
    its flag: the slow peer keeps a consistent tensor and gets a time-out on its own late call instead of a torn one."""
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_slow_peer_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        res = open(tmp_path / f"slow{r}").read()
        assert res == "1", f"rank {r}: {res}"


@pytest.mark.parametrize("gpus", [2, 4])
def test_bench_self_launches(tmp_path, gpus):
    """`python bench.py --gpus N ... --full` exactly as the driver types it (no torch.distributed.run in front, no WORLD_SIZE):
    bench.py spawns its own ranks; rank 0 prints the ONE JSON line; the north-star layout (tp = N, a --full leg) ran with a named
    transport and no error.  All ranks share the one GPU of the box (MIXQ_BENCH_SINGLE_GPU_RANKS=1: gloo for the
    harness collectives) -- control flow, not a measurement.  N = 4: its shard widths (3072 / 2752 / 1024 rows), four-way
    transport self-tests and the transport comparison execute here first; more ranks would put more than six processes on
    the one GPU (with the test process and the launcher)."""
    import json
    import subprocess
    env = dict(os.environ, MIXQ_BENCH_SINGLE_GPU_RANKS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    tokens = "16384" if gpus == 2 else "8192"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--tokens", tokens, "--steps", "1",
                        "--warmup", "1", "--full", "--config5-layers", "1"], capture_output=True, text=True, env=env, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == gpus and rec["value"] > 0 and rec["config"]["parallelism"].startswith(f"dp{gpus} ")
    tp = rec["tp"]
    assert rec["tp_tokens_per_s"] == tp["value"] and "replica" in rec["value_layout"]   # the row-sharded layout at the top level too
    assert "error" not in tp, tp
    assert tp["world_size"] == gpus and tp["tp"] == gpus and tp["transport"] and tp["peer_wait_timed_out"] is False
    assert tp["value"] > 0
    alts = tp.get("alternatives_one_step_each")   # the other transports of the same layout, one timed step each
    assert isinstance(alts, dict) and "error" not in alts, alts
    assert any("rccl" in k for k in alts) and all(v["ms_per_step"] > 0 for v in alts.values()), alts
    # BASELINE configs[4] (Llama-2-70B, rows of W sharded N ways WITH the all-gather; one decoder layer here): its own leg, its own
    # transport self-test on the 10240 / 28672 / 8192-wide outputs
    c5 = rec["configs"][f"llama2_70b_tp{gpus}"]
    assert "error" not in c5, c5
    assert c5["tp"] == gpus and c5["layers"] == 1 and c5["value"] > 0 and c5["transport"] and c5["peer_wait_timed_out"] is False
    assert "10240x8192" in c5["workload"] and "28672x8192" in c5["workload"] and "8192x28672" in c5["workload"]


def _fused_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import oracle
    from mixq_tensorrt_llm_amd import _lib, parallel, plugin
    lib = _lib.load()
    ok, notes = True, []
    try:
        # (M, N, K): per-rank shards of 6144 / 4096 columns that take the plain 256 x 256 ping-pong kernel; ragged last
        # tile row (2000), many flag words (M = 17000 -> 67 tile rows -> 4-row chunks -> 17 words)
        for M, N, K in ((2048, 12288, 512), (2000, 12288, 256), (17000, 8192, 256)):
            A, full = exact_fixture(M, N, K, 11 + M)
            mine = parallel.shard_packed(full, world, rank)
            assert lib.mixq_tp_fused_supported(M, N // world, K) == 1, (M, N, K)
            want = oracle.linear_prefill(A, full["weight"], full["weights_scaling_factor"], full["fp_weight"], full["fp_ind"])
            layer = plugin.MixQLinear(K, N, bias=False, tp_size=world, gather_output=True, device="cuda:0").load(mine)
            layer.peer_gather = parallel.PeerGather(M, N, world, rank, "cuda:0")
            Ad = torch.from_numpy(A).cuda()
            for call in range(3):                      # both buffer parities, flags / counters re-armed
                got = layer(Ad)
                torch.cuda.synchronize()
                layer.peer_gather.check()
                kern = lib.mixq_debug_last_gemm_kernel().decode()
                if "peer-write epilogue" not in kern:
                    ok = False
                    notes.append(f"{M}x{N}x{K}: fused path not taken ({kern})")
                if not np.array_equal(got.cpu().numpy().view(np.uint16), want.view(np.uint16)):
                    ok = False
                    notes.append(f"{M}x{N}x{K} call {call}: gathered output differs from the unsharded oracle")
            words = lib.mixq_tp_flag_words(M)
            ok &= (words == 17) if M == 17000 else (words == 2)
            ok &= int(layer.peer_gather.small.abs().sum()) == 0          # counters left zero
            # unsupported shape (few tiles): the same layer object falls back to enqueue + push, same contract
            small = layer(Ad[:40])
            torch.cuda.synchronize()
            ok &= np.array_equal(small.cpu().numpy().view(np.uint16), want[:40].view(np.uint16))
            layer.peer_gather.close()
            dist.barrier()
        # back to back: 36 calls of two sizes with NO host synchronisation in between, one rank or the other arriving late
        # (device-side delay) -- chunk flags, counters and the two destination buffers under load, every element checked
        M, N, K = 2048, 12288, 256
        A, full = exact_fixture(M, N, K, 77)
        mine = parallel.shard_packed(full, world, rank)
        want_d = torch.from_numpy(oracle.linear_prefill(A, full["weight"], full["weights_scaling_factor"], full["fp_weight"],
                                                        full["fp_ind"]).view(np.int16).copy()).cuda()
        layer = plugin.MixQLinear(K, N, bias=False, tp_size=world, gather_output=True, device="cuda:0").load(mine)
        layer.peer_gather = parallel.PeerGather(M, N, world, rank, "cuda:0")
        Ad = torch.from_numpy(A).cuda()
        bad = torch.zeros((), dtype=torch.int64, device="cuda:0")
        for c in range(36):
            m = M if c % 3 else 1800
            if c % 4 == rank + 1:
                torch.cuda._sleep(2000000 + 300000 * (c % 5))
            got = layer(Ad[:m])
            bad += (got.view(torch.int16) != want_d[:m]).sum()
        torch.cuda.synchronize()
        layer.peer_gather.check(sync=True)
        if int(bad.item()) != 0:
            ok = False
            notes.append(f"back-to-back fused gathers: {int(bad.item())} wrong elements")
        ok &= int(layer.peer_gather.small.abs().sum()) == 0
        layer.peer_gather.close()
        dist.barrier()
    except Exception:  # noqa: BLE001
        import traceback
        ok = False
        notes.append(traceback.format_exc())
    open(os.path.join(tmp, f"fused{rank}"), "w").write("1" if ok else "0\n" + "\n".join(notes))
    dist.barrier()
    dist.destroy_process_group()


def test_allgather_fused_into_the_gemm_epilogue_two_ranks_one_gpu(tmp_path, oracle):
    """the peer writes issued from the GEMM's own store path (mixq_enqueue_tp), chunk flags published
    as the M chunks retire; two processes on the one GPU (IPC-mapped fine-grained buffers), MixQLinear(tp_size=2)
    bit-exact against the UNSHARDED oracle on the exact fixture, ragged M, several flag words, three calls per shape.
    Cannot be timed here: both 'GPUs' are the same device."""
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_fused_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        res = open(tmp_path / f"fused{r}").read()
        assert res == "1", f"rank {r}: {res}"


# -------------------------------------------------------------- four ranks on the one GPU ---
# Four ranks, not eight: with the test process, at most five processes have the GPU open at once.  N is halved against
# BASELINE configs[4] (Llama-2-70B rows sharded 8 ways) so that every rank's shard keeps the 8-way width: 1280 / 3584 / 1024 rows.
FOUR_CASES = [  # (name, M, N, K, exact, fused)
    ("70b_qkv_m48", 48, 10240 // 2, 8192, False, False),
    ("70b_gate_m48", 48, 28672 // 2, 8192, True, False),
    ("70b_proj_m48", 48, 8192 // 2, 28672, True, False),
    ("fused_1280_row_shards", 6656, 10240 // 2, 1024, True, True),    # 26 x 5 tiles per rank: the plain 256 x 256 kernel -> mixq_enqueue_tp
    ("fused_3584_row_shards", 2560, 28672 // 2, 512, True, True),     # 10 x 14 tiles per rank
]


def _four_fixture(i):
    name, M, N, K, exact, fused = FOUR_CASES[i]
    return exact_fixture(M, N, K, 40 + i) if exact else ordinary_fixture(M, N, K, 40 + i)


def _four_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from conftest import elementwise_violations
    from mixq_tensorrt_llm_amd import _lib, parallel, plugin
    lib = _lib.load()
    ok, notes = True, []
    try:
        for i, (name, M, N, K, exact, fused) in enumerate(FOUR_CASES):
            A, full = _four_fixture(i)
            mine = parallel.shard_packed(full, world, rank)
            del full
            want = np.load(os.path.join(tmp, f"want{i}.npy"))
            slack = None if exact else np.load(os.path.join(tmp, f"slack{i}.npy"))
            if fused and lib.mixq_tp_fused_supported(M, N // world, K) != 1:
                ok = False
                notes.append(f"{name}: mixq_tp_fused_supported says no for the {N // world}-row shard")
            layer = plugin.MixQLinear(K, N, bias=False, tp_size=world, gather_output=True, device="cuda:0").load(mine)
            layer.peer_gather = parallel.PeerGather(M, N, world, rank, "cuda:0")
            Ad = torch.from_numpy(A).cuda()
            for call in range(3):                        # both buffer parities, flags of four producers re-armed
                if call == 1 and rank % 3 == 1:
                    torch.cuda._sleep(3000000)           # some ranks arrive late
                got = layer(Ad)
                torch.cuda.synchronize()
                layer.peer_gather.check()
                kern = lib.mixq_debug_last_gemm_kernel().decode()
                if fused and "peer-write epilogue" not in kern:
                    ok = False
                    notes.append(f"{name}: fused path not taken ({kern})")
                g = got.cpu().numpy()
                if exact:
                    good = np.array_equal(g.view(np.uint16), want.view(np.uint16))
                else:
                    err = np.abs(g.astype(np.float64) - want.astype(np.float64)).max() / np.abs(want).max()
                    bad, _, _ = elementwise_violations(g, want, slack)
                    good = err < 1e-3 and not bad.any()
                if not good:
                    ok = False
                    notes.append(f"{name} call {call} [{kern}]: gathered output differs from the unsharded oracle")
            ok &= int(layer.peer_gather.small.abs().sum()) == 0 and not layer.peer_gather.timed_out()
            layer.peer_gather.close()
            del layer, Ad, mine
            torch.cuda.empty_cache()
            dist.barrier()
    except Exception:  # noqa: BLE001
        import traceback
        ok = False
        notes.append(traceback.format_exc())
    open(os.path.join(tmp, f"four{rank}"), "w").write("1" if ok else "0\n" + "\n".join(notes))
    dist.barrier()
    dist.destroy_process_group()


def test_four_ranks_one_gpu_peer_writes_and_fused_epilogue(tmp_path, oracle):
    """ndst = 4: four processes on the one GPU (IPC-mapped fine-grained buffers, four producers' flag blocks per consumer), the
    N / 8 shard widths of Llama-2-70B (1280 / 3584 / 1024 rows: other kernels than the 2-way shards select) at a decode batch of
    48 through mixq_tp_push_columns, and two prefill-size cases whose shards take the all-gather FUSED into the GEMM's store path
    (mixq_enqueue_tp).  Gathered output against the UNSHARDED oracle: bit-exact on the exact-sum fixture, 1e-3 + element-wise on
    ordinary data.  First execution of these paths at more than two ranks; xGMI itself still needs a multi-GPU node."""
    import torch.multiprocessing as mp
    from conftest import prefill_slack
    world = 4
    for i, (name, M, N, K, exact, fused) in enumerate(FOUR_CASES):
        A, full = _four_fixture(i)
        want, parts = oracle.linear_prefill(A, full["weight"], full["weights_scaling_factor"], full["fp_weight"], full["fp_ind"],
                                            return_parts=True)
        np.save(tmp_path / f"want{i}.npy", want)
        if not exact:
            np.save(tmp_path / f"slack{i}.npy", prefill_slack(parts, A, full))
        del A, full, want, parts
    mp.spawn(_four_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        res = open(tmp_path / f"four{r}").read()
        assert res == "1", f"rank {r}: {res}"


# ------------------------------------------- a TP decode step as ONE HIP graph, four ranks (VERDICT r4 next #3b) ---
GRAPH_CASES = [("70b_qkv", 16, 10240, 8192), ("70b_gate", 16, 28672, 8192), ("70b_proj", 16, 8192, 28672)]


def _graph_fixture(i, variant):
    name, M, N, K = GRAPH_CASES[i]
    A, full = exact_fixture(M, N, K, 70 + i)
    if variant:   # second activation set (same weights): replays must follow the static input buffers, not repeat the capture
        rng = np.random.default_rng(700 + i)
        A2 = rng.standard_normal((M, K)).astype(np.float16)
        A2[:, full["fp_ind"]] = rng.integers(-60, 61, size=(M, 128)).astype(np.float16)
        A = A2
    return A, full


def _graph_worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mixq_tensorrt_llm_amd import parallel, plugin
    ok, notes = True, []
    try:
        layers, inputs, wants = [], [], []
        for i, (name, M, N, K) in enumerate(GRAPH_CASES):
            A0, full = _graph_fixture(i, 0)
            A1, _ = _graph_fixture(i, 1)
            mine = parallel.shard_packed(full, world, rank)
            del full
            layer = plugin.MixQLinear(K, N, bias=False, tp_size=world, gather_output=True, device="cuda:0").load(mine)
            layer.peer_gather = parallel.PeerGather(M, N, world, rank, "cuda:0", capturable=True, patience_ms=10000)
            layer.peer_gather_alias = True          # the gathered tensor IS the (one, fixed) IPC buffer: what a graph's consumers read
            layers.append(layer)
            inputs.append([torch.from_numpy(A0).cuda(), torch.from_numpy(A1).cuda()])
            wants.append([torch.from_numpy(np.load(os.path.join(tmp, f"gwant{i}_{v}.npy"))).cuda() for v in (0, 1)])
        static = [x[0].clone() for x in inputs]

        def step():
            return [layer(x) for layer, x in zip(layers, static)]

        def same(outs, v, what):
            good = all(torch.equal(o.view(torch.int16), w[v].view(torch.int16)) for o, w in zip(outs, wants))
            if not good:
                notes.append(f"{what}: gathered outputs differ from the unsharded oracle")
            return good

        # eager first (lazy allocations, and the reference result), twice: the single buffer is reused under acknowledgement
        for v in (0, 1):
            for s, x in zip(static, inputs):
                s.copy_(x[v])
            outs = step()
            torch.cuda.synchronize()
            ok &= same(outs, v, f"eager call, input set {v}")
        dist.barrier()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                gouts = step()                       # quantise + GEMM + arrive + push + wait, three linears: 15 launches, no host state
        torch.cuda.synchronize()
        dist.barrier()
        for it in range(100):
            v = (it // 7) & 1
            if it % 7 == 0:                          # new activations in the static buffers every 7 replays; NO host sync otherwise
                for s, x in zip(static, inputs):
                    s.copy_(x[v])
            if it % 13 == 5 and rank % 2 == 1:
                torch.cuda._sleep(2000000)           # odd ranks arrive late now and then
            g.replay()
            if it % 7 == 6 or it == 99:              # check the replay that closes a block of seven (and the last one)
                torch.cuda.synchronize()
                ok &= same(gouts, v, f"replay {it}")
            if it == 50:                             # an EAGER step between replays: captured and eager calls share the device-side call number
                outs = step()
                torch.cuda.synchronize()
                ok &= same(outs, v, "eager step between replays")
        torch.cuda.synchronize()
        for layer in layers:
            layer.peer_gather.check(sync=True)
            calls = int(layer.peer_gather.small[layer.peer_gather.FLAG_WORDS + 1].item())
            if calls != 2 + 100 + 1:                 # 2 eager calls, 100 replays, 1 eager call in between (capturing launches nothing)
                ok = False
                notes.append(f"device-side call number {calls}, expected 103")
            ok &= not layer.peer_gather.timed_out()
        for layer in layers:
            layer.peer_gather.close()
    except Exception:  # noqa: BLE001
        import traceback
        ok = False
        notes.append(traceback.format_exc())
    open(os.path.join(tmp, f"graph{rank}"), "w").write("1" if ok else "0\n" + "\n".join(notes))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_tp_decode_step_replays_as_one_hip_graph(tmp_path, oracle, world):
    """A TP decode step (the three Llama-2-70B linears at batch 16, rows of W sharded `world` ways, every output all-gathered by
    peer writes) captured as ONE HIP graph per rank and replayed 100 times on changing inputs, bit-exact against the unsharded
    oracle, with an eager step in between and ranks arriving late: `PeerGather(capturable=True)` keeps the call number in a device
    word and acknowledges the reuse of its one destination buffer, so nothing of a call is host state (the reference's collective
    is a plugin inside the engine and replays with it: tensorrt_llm/functional.py:3834-3880, plugin.py:155-156)."""
    import torch.multiprocessing as mp
    for i in range(len(GRAPH_CASES)):
        for v in (0, 1):
            A, full = _graph_fixture(i, v)
            want = oracle.linear_prefill(A, full["weight"], full["weights_scaling_factor"], full["fp_weight"], full["fp_ind"])
            np.save(tmp_path / f"gwant{i}_{v}.npy", want)
            del A, full, want
    mp.spawn(_graph_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        res = open(tmp_path / f"graph{r}").read()
        assert res == "1", f"rank {r}: {res}"
