"""GPU (-m gpu): the layer bias in the operator's epilogue (EPI_DEQUANT_BIAS, mixq_enqueue_bias / mixq_enqueue_tp_bias /
mixq_gemm_mixed_bias).  The reference adds the bias in the TensorRT graph after the plugin (plugin.py:158-160); the fused form
must give exactly the bits of mixq_enqueue followed by torch's fp16 ``x + bias``, on every kernel family mixq_enqueue can take,
with the same family chosen with and without the bias, the bias added once in every split form, against the oracle, with a
registered weight image, inside a HIP graph, through MixQLinear, and fused into the TP all-gather."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_elementwise, assert_prefill_parity, make_layer, ulp16, w8a16_slack

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

QKV = (4608, 3584)   # Qwen2-7B qkv projection (N, K): BASELINE configuration 4, biased
QKV_ROWS = [1, 2, 3, 4, 17, 40, 64, 80, 160, 320, 512, 768, 1024, 2048, 8192]   # its docs/SELECTION_TABLE.md rows


@pytest.fixture(scope="module")
def lib():
    from mixq_tensorrt_llm_amd import _lib
    lib = _lib.load()
    lib.mixq_debug_reset()
    yield lib
    lib.mixq_debug_reset()


_LAYERS = {}


def layer_for(N, K, rows):
    """A packed MixQ layer of shape [N, K] and `rows` activations (cached per shape)."""
    key = (N, K)
    if key not in _LAYERS or _LAYERS[key][0].shape[0] < rows:
        from mixq_tensorrt_llm_amd import pack, plugin
        A, W, act = make_layer(rows, N, K, seed=N + K)
        p = pack.pack_linear_weights(torch.from_numpy(W), torch.from_numpy(act))
        layer = plugin.MixQLinear(K, N, bias=True, device="cuda:0").load(p)
        _LAYERS[key] = (A, p, layer)
    return _LAYERS[key]


def special_bias(N, seed):
    """Random bias with +-0, +-65504 and subnormal columns at the front."""
    rng = np.random.default_rng(seed)
    b = (rng.standard_normal(N) * 0.5).astype(np.float16)
    sub = np.float16(2.0 ** -24)
    b[:10] = np.array([0.0, -0.0, 65504.0, -65504.0, sub, -sub, 3 * sub, np.float16(3e-5), -np.float16(6e-5), 1.0], np.float16)
    return b


def inputs_of(layer, A):
    return [A, layer.weight, layer.weights_scaling_factor, layer.fp_weight, layer.fp_ind, layer.qweight,
            layer.weights_scaling_factor]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy()


def plan(lib, M, N, K, image=False):
    buf = ctypes.create_string_buffer(256)
    assert lib.mixq_describe_plan(M, N, K, 1 if image else 0, buf, 256) == 0
    return buf.value.decode()


def family(kernel, plan_text, M):
    """Family label of one call: the kernel launch_gemm reported, refined by the plan text (tile width / weight route / split)."""
    if M <= 4:
        return "w8a16"
    if "gemm_skinny_kernel" in kernel:
        return "skinny-image" if "registered image" in plan_text else "skinny-route"
    if "mid_kernel" in kernel:
        return "mid-96" if "128x96" in plan_text else "mid-128"
    if "w8a8o16_kernel<DEEP>" in kernel:
        return "deep"
    if "pp128" in kernel:
        return "pp128"
    if "pp_kernel<SPLITK>" in kernel:
        return "pp256-split"
    if "pp_kernel" in kernel:
        return "pp256"
    if "two-barrier" in kernel:
        return "xsplit" if "workgroups per tile along K" in plan_text else "two-barrier"
    return "other:" + kernel


def run_pair(lib, layer, A, bias_t):
    """(enqueue + torch add, kernel name), (enqueue_bias, kernel name) on the same inputs."""
    from mixq_tensorrt_llm_amd import plugin
    plug = plugin.MixQPlugin.create(A.shape[0], layer.out_features, layer.in_features)
    ins = inputs_of(layer, A)
    want = plug.enqueue(ins) + bias_t
    torch.cuda.synchronize()
    k0 = lib.mixq_debug_last_gemm_kernel().decode()
    got = plug.enqueue(ins, bias=bias_t)
    torch.cuda.synchronize()
    k1 = lib.mixq_debug_last_gemm_kernel().decode()
    return want, k0, got, k1


FAMILY_CASES = [(QKV[0], QKV[1], m, False, None) for m in QKV_ROWS]
FAMILY_CASES += [(4608, 3584, 17, True, None), (4608, 3584, 40, True, None)]                     # skinny on a weight image
FAMILY_CASES += [(4096, 11008, m, False, None) for m in (65, 80, 128, 129, 160, 256, 512)]      # xsplit 65..128, mid split 129..512
FAMILY_CASES += [(11008, 4096, 2048, False, None)]                                               # 256 x 256 split K
FAMILY_CASES += [(4096, 11008, 160, False, 1421)]                                                # the round-5 deep build (forced)


def test_every_family_bit_identical_to_enqueue_plus_add(lib):
    seen, failures = set(), []
    for N, K, M, image, knob in FAMILY_CASES:
        A_np, p, layer = layer_for(N, K, 8192 if (N, K) == QKV else 2048)
        A = torch.from_numpy(A_np[:M]).cuda()
        bias_t = torch.from_numpy(special_bias(N, M)).cuda()
        img = None
        if image:
            from mixq_tensorrt_llm_amd import mixlib
            img = mixlib.WeightImage(layer.weight.view(torch.int8))
            img.verify()
        if knob is not None:
            lib.mixq_debug_set_gemm_variant(knob)
        try:
            want, k0, got, k1 = run_pair(lib, layer, A, bias_t)
            fam = family(k1, plan(lib, M, N, K, image), M)
        finally:
            if knob is not None:
                lib.mixq_debug_reset()
            if img is not None:
                img.close()
        seen.add(fam)
        if k0 != k1:
            failures.append(f"{N}x{K} M={M}: family {k0!r} without the bias, {k1!r} with it")
        if not np.array_equal(bits(got), bits(want)):
            n_bad = int((bits(got) != bits(want)).sum())
            failures.append(f"{N}x{K} M={M} ({fam}): {n_bad} elements differ from enqueue + add")
    need = {"skinny-route", "skinny-image", "two-barrier", "xsplit", "deep", "mid-128", "mid-96", "pp128", "pp256", "pp256-split"}
    assert need <= seen, f"families not reached: {sorted(need - seen)} (seen {sorted(seen)})"
    assert not failures, "\n".join(failures)


SPLIT_CASES = [  # (N, K, M, knob): the split factor forced through the debug knobs (shapes on which mixq_describe_plan shows that factor)
    (4096, 11008, 80, 62), (1024, 11008, 80, 64), (1024, 11008, 80, 68), (256, 16384, 64, 66),    # small tiles 2 / 4 / 8 / 16
    (4096, 4096, 256, 72), (4096, 4096, 256, 74), (4096, 4096, 256, 78),                          # 256 x 256 tiles 2 / 4 / 8
    (4096, 11008, 256, 1242), (4096, 11008, 256, 1243), (4096, 11008, 256, 1245), (4096, 11008, 256, 1249),  # deep 1 / 2 / 4 / 8
    (4096, 11008, 256, 1253), (4096, 11008, 256, 1273),                                           # 8-wave build / mid kernel, 2 ways
]


@pytest.mark.parametrize("N,K,M,knob", SPLIT_CASES)
def test_split_forms_add_the_bias_once(lib, N, K, M, knob):
    A_np, p, layer = layer_for(N, K, 2048)
    A = torch.from_numpy(A_np[:M]).cuda()
    bias_t = torch.from_numpy(special_bias(N, knob)).cuda()
    from mixq_tensorrt_llm_amd import plugin
    plug = plugin.MixQPlugin.create(M, N, K)
    ins = inputs_of(layer, A)
    lib.mixq_debug_set_gemm_variant(1)   # unsplit reference: the two-barrier tiles with no K split over workgroups
    lib.mixq_debug_set_gemm_variant(60)
    lib.mixq_debug_set_gemm_variant(1241)
    try:
        ref = plug.enqueue(ins, bias=bias_t)
        torch.cuda.synchronize()
        lib.mixq_debug_reset()
        lib.mixq_debug_set_gemm_variant(knob)
        got = plug.enqueue(ins, bias=bias_t)
        plain = plug.enqueue(ins)
        torch.cuda.synchronize()
        kern = lib.mixq_debug_last_gemm_kernel().decode()
    finally:
        lib.mixq_debug_reset()
    assert np.array_equal(bits(got), bits(plain + bias_t)), f"knob {knob} ({kern}): differs from the same form + add"
    assert np.array_equal(bits(got), bits(ref)), f"knob {knob} ({kern}): differs from the unsplit run with the bias"


@pytest.mark.parametrize("M", [40, 80, 300, 1024, 2048])
def test_against_the_oracle_prefill(lib, oracle, M):
    N, K = QKV
    A_np, p, layer = layer_for(N, K, 8192)
    A = A_np[:M]
    bias = special_bias(N, 7 + M)
    bias[2:4] = 0   # (the +-65504 columns overflow against any bound; they are covered bit-exactly above)
    bias_t = torch.from_numpy(bias).cuda()
    from mixq_tensorrt_llm_amd import plugin
    got = plugin.MixQPlugin.create(M, N, K).enqueue(inputs_of(layer, torch.from_numpy(A).cuda()), bias=bias_t)
    torch.cuda.synchronize()
    rows = np.unique(np.linspace(0, M - 1, 24).astype(int))
    assert_prefill_parity(oracle, got.cpu().numpy()[rows], A[rows], p, what=f"enqueue_bias M={M}", bias=bias)


@pytest.mark.parametrize("M", [80, 600, 2048])
def test_gemm_mixed_bias_against_the_oracle(lib, oracle, M):
    N, K = QKV
    A_np, p, layer = layer_for(N, K, 8192)
    A = A_np[:M]
    bias = special_bias(N, 11 + M)
    bias[2:4] = 0
    d = "cuda:0"
    Ad = torch.from_numpy(A).to(d)
    qA = torch.empty((M, K), dtype=torch.int8, device=d)
    sA = torch.empty(M, dtype=torch.float16, device=d)
    fpA = torch.empty((M, 128), dtype=torch.float16, device=d)
    ind = torch.from_numpy(p["fp_ind"].astype(np.int32)).to(d)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    v = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.mixq_quant_extract(M, K, v(Ad), v(qA), v(sA), v(fpA), v(ind), 128, 0, st) == 0
    W = torch.from_numpy(p["weight"]).to(d)
    sW = torch.from_numpy(p["weights_scaling_factor"]).to(d)
    fpW = torch.from_numpy(p["fp_weight"]).to(d)
    bias_t = torch.from_numpy(bias).to(d)
    nbytes = lib.mixq_gemm_scratch_size(M, N, K)
    scratch = torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=d)
    out = torch.empty((M, N), dtype=torch.float16, device=d)
    plain = torch.empty_like(out)
    assert lib.mixq_gemm_mixed_bias(v(qA), v(W), v(sA), v(sW), v(fpA), v(fpW), v(bias_t), v(out), M, N, K, 128,
                                    v(scratch), nbytes, st) == 0
    assert lib.mixq_gemm_mixed_scratch(v(qA), v(W), v(sA), v(sW), v(fpA), v(fpW), v(plain), M, N, K, 128, v(scratch), nbytes, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), bits(plain + bias_t))
    rows = np.unique(np.linspace(0, M - 1, 24).astype(int))
    assert_prefill_parity(oracle, out.cpu().numpy()[rows], A[rows], p, what=f"gemm_mixed_bias M={M}", bias=bias)


@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_decode_rows_against_the_w8a16_oracle(lib, oracle, M):
    N, K = QKV
    A_np, p, layer = layer_for(N, K, 8192)
    A = A_np[:M]
    bias = special_bias(N, 13 + M)
    bias[2:4] = 0
    from mixq_tensorrt_llm_amd import plugin
    got = plugin.MixQPlugin.create(M, N, K).enqueue(inputs_of(layer, torch.from_numpy(A).cuda()),
                                                    bias=torch.from_numpy(bias).cuda())
    torch.cuda.synchronize()
    q_un = np.empty((K, N), np.int8)
    lib.mixq_unprocess_weights_int8(q_un.ctypes.data, p["qweight"].ctypes.data, K, N)
    want = oracle.w8a16_gemv(A, q_un, p["weights_scaling_factor"])
    slack = w8a16_slack(A, q_un, p["weights_scaling_factor"]) + ulp16(want)
    want_b = (want.astype(np.float16) + bias[None, :]).astype(np.float16)
    assert_elementwise(got.cpu().numpy(), want_b, slack, f"w8a16 + bias M={M}")


def test_decode_rows_take_both_w8a16_forms(lib):
    """The M <= 4 path on qweight: the GEMV and the fpA_intB skinny form (forced both ways), each bit-identical to enqueue + add."""
    N, K = QKV
    A_np, p, layer = layer_for(N, K, 8192)
    bias_t = torch.from_numpy(special_bias(N, 3)).cuda()
    for knob in (306, 307):   # 1..4 tokens through the skinny form always / never
        lib.mixq_debug_set_gemm_variant(knob)
        try:
            for M in (1, 2, 3, 4):
                want, _, got, _ = run_pair(lib, layer, torch.from_numpy(A_np[:M]).cuda(), bias_t)
                assert np.array_equal(bits(got), bits(want)), f"knob {knob} M={M}"
        finally:
            lib.mixq_debug_reset()


def test_weight_image_same_bits(lib):
    N, K = QKV
    A_np, p, layer = layer_for(N, K, 8192)
    bias_t = torch.from_numpy(special_bias(N, 5)).cuda()
    from mixq_tensorrt_llm_amd import mixlib, plugin
    rows = list(range(5, 65, 7)) + [64]
    plain = {}
    for M in rows:
        plain[M] = bits(plugin.MixQPlugin.create(M, N, K).enqueue(inputs_of(layer, torch.from_numpy(A_np[:M]).cuda()), bias=bias_t))
    img = mixlib.WeightImage(layer.weight.view(torch.int8))
    try:
        img.verify()
        for M in rows:
            got = plugin.MixQPlugin.create(M, N, K).enqueue(inputs_of(layer, torch.from_numpy(A_np[:M]).cuda()), bias=bias_t)
            assert np.array_equal(bits(got), plain[M]), f"M={M}: weight image changes the bits"
    finally:
        img.close()


@pytest.mark.parametrize("M", [3, 40, 512, 2048])
def test_hip_graph_replay(lib, M):
    N, K = QKV
    A_np, p, layer = layer_for(N, K, 8192)
    from mixq_tensorrt_llm_amd import plugin
    plug = plugin.MixQPlugin.create(M, N, K)
    A_static = torch.from_numpy(A_np[:M]).cuda()
    bias_t = torch.from_numpy(special_bias(N, 17)).cuda()
    ws = plug._workspace(A_static.device, plug.workspace_size(M, N, K))
    out = torch.empty((M, N), dtype=torch.float16, device="cuda:0")
    plug.enqueue(inputs_of(layer, A_static), output=out, workspace=ws, bias=bias_t)   # warm-up outside the capture
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            plug.enqueue(inputs_of(layer, A_static), output=out, workspace=ws, bias=bias_t)
    torch.cuda.synchronize()
    rng = np.random.default_rng(M)
    for r in range(2):
        new = (rng.standard_normal((M, K)) * (1 + r)).astype(np.float16)
        A_static.copy_(torch.from_numpy(new))
        g.replay()
        torch.cuda.synchronize()
        eager = plug.enqueue(inputs_of(layer, torch.from_numpy(new).cuda()), bias=bias_t)
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), bits(eager)), f"replay {r}"


@pytest.mark.parametrize("M", [1, 4, 40, 512, 2048])
def test_mixqlinear_bias_bit_identical_to_the_separate_add(lib, M):
    N, K = QKV
    A_np, p, layer = layer_for(N, K, 8192)
    layer.bias = torch.from_numpy(special_bias(N, 19)).cuda()
    A = torch.from_numpy(A_np[:M]).cuda()
    fused = layer.forward(A)
    layer.fuse_bias = False
    try:
        separate = layer.forward(A)          # the pre-existing path: operator, then torch's fp16 add
    finally:
        layer.fuse_bias = True
    from mixq_tensorrt_llm_amd import plugin
    want = plugin.MixQPlugin.create(M, N, K).enqueue(inputs_of(layer, A)) + layer.bias.to(torch.float16)
    torch.cuda.synchronize()
    assert np.array_equal(bits(fused), bits(want))
    assert np.array_equal(bits(separate), bits(want))


# ------------------------------------------------------------------------------------- TP: bias in the fused gather ---
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _tp_worker(rank, world, port, tmp, M, N, K):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mixq_tensorrt_llm_amd import _lib, pack, parallel, plugin
    lib = _lib.load()
    ok, notes = True, []
    try:
        A, W, act = make_layer(M, N, K, seed=N + K + world)
        full = pack.pack_linear_weights(torch.from_numpy(W), torch.from_numpy(act))
        full["bias"] = special_bias(N, world)
        Ad = torch.from_numpy(A).cuda()
        whole = plugin.MixQLinear(K, N, bias=True, device="cuda:0").load(full)
        want = bits(plugin.MixQPlugin.create(M, N, K).enqueue(inputs_of(whole, Ad), bias=whole.bias))
        assert lib.mixq_tp_fused_supported(M, N // world, K) == 1, (M, N, K, world)
        mine = parallel.shard_packed(full, world, rank)
        layer = plugin.MixQLinear(K, N, bias=True, tp_size=world, gather_output=True, device="cuda:0").load(mine)
        pg = parallel.PeerGather(M, N, world, rank, "cuda:0")
        layer.peer_gather = pg
        calls = {"fused_bias": 0, "push": 0}
        raw, push = pg.enqueue_gather_raw, pg.gather

        def raw_spy(*a, **kw):
            if kw.get("bias_ptr") is not None:
                calls["fused_bias"] += 1
            return raw(*a, **kw)

        def push_spy(*a, **kw):
            calls["push"] += 1
            return push(*a, **kw)
        pg.enqueue_gather_raw, pg.gather = raw_spy, push_spy
        for call in range(2):
            got = layer(Ad)
            torch.cuda.synchronize()
            pg.check()
            kern = lib.mixq_debug_last_gemm_kernel().decode()
            if "peer-write epilogue" not in kern:
                ok = False
                notes.append(f"call {call}: fused path not taken ({kern})")
            if not np.array_equal(bits(got), want):
                ok = False
                notes.append(f"call {call}: {int((bits(got) != want).sum())} elements differ from the unsharded enqueue_bias")
        if calls["fused_bias"] != 2 or calls["push"] != 0:
            ok = False
            notes.append(f"calls: {calls}")
        pg.close()
        dist.barrier()
    except Exception:  # noqa: BLE001
        import traceback
        ok = False
        notes.append(traceback.format_exc())
    open(os.path.join(tmp, f"bias{rank}"), "w").write("1" if ok else "0\n" + "\n".join(notes))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,M", [(2, 4096), (4, 8192)])
def test_tp_bias_fused_into_the_gather(tmp_path, world, M):
    import torch.multiprocessing as mp
    N, K = QKV
    mp.spawn(_tp_worker, args=(world, _free_port(), str(tmp_path), M, N, K), nprocs=world, join=True)
    for r in range(world):
        res = open(tmp_path / f"bias{r}").read()
        assert res == "1", f"rank {r}: {res}"
