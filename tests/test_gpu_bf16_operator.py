"""GPU (-m gpu): bf16 calls of mixq_enqueue (inputDesc[0].type == MIXQ_TYPE_BF16).  The producer's qA / sA / fpA and the full output
are compared bit for bit with the numpy restatement (tests/bf16_restate.py) on every kernel family the fp16 call takes -- the bf16
call must report the same family --, random data within the stated bound, the bias, activations beyond fp16's range, a poisoned
workspace, a registered weight image, a HIP graph, MixQLinear(dtype=torch.bfloat16), a checkpoint round trip, and a plain C host."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import bf16_restate as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

QKV = (4608, 3584)
QKV_ROWS = [1, 2, 3, 4, 17, 40, 64, 80, 160, 320, 512, 768, 1024, 2048, 8192]   # docs/SELECTION_TABLE.md rows of this shape
KNOB_BLOCK_ROWS_64, KNOB_BLOCK_ROWS_ALWAYS, KNOB_QA_FRAG_OFF = 1301, 1312, 891


@pytest.fixture(scope="module")
def lib():
    from mixq_tensorrt_llm_amd import _lib
    lib = _lib.load()
    lib.mixq_debug_reset()
    yield lib
    lib.mixq_debug_reset()


def make_bf16_layer(N, K, seed, exact=True, fpw_zero=False, M=None):
    """A packed bf16 layer and matching bf16 activations.  exact: outlier columns of A and fp_weight are small integers times powers
    of two, so every order of the fp32 outlier sum is exact and the output is deterministic."""
    from mixq_tensorrt_llm_amd import pack
    rng = np.random.default_rng(seed)
    act = np.abs(rng.standard_normal(K)).astype(np.float32)
    W = torch.from_numpy((rng.standard_normal((N, K)) * 0.02).astype(np.float32)).to(torch.bfloat16)
    p = pack.pack_linear_weights(W, torch.from_numpy(act), fp_dtype=torch.bfloat16)
    ind = p["fp_ind"].astype(np.int64)
    if fpw_zero:
        p["fp_weight"] = np.zeros_like(p["fp_weight"])
    elif exact:
        p["fp_weight"] = R.bf16_rn(rng.integers(-8, 9, (N, len(ind))).astype(np.float32) * 2.0 ** -6)
    A = (rng.standard_normal((M or 1, K)) * 2).astype(np.float32)
    if exact:
        A[:, ind] = rng.integers(-16, 17, (A.shape[0], len(ind))).astype(np.float32) * 4
    else:
        A[:, ind] *= 20
    return p, R.bf16_rn(A)


def inputs(p, A_t, dev="cuda"):
    def carrier(a, shape, dt=torch.float16):
        return torch.from_numpy(np.ascontiguousarray(a)).view(dt).reshape(shape).to(dev)
    N, K = p["weight"].shape
    return [A_t, carrier(p["weight"], (N, K // 2)), carrier(p["weights_scaling_factor"], (N,)),
            R.from_bits(p["fp_weight"], dev), carrier(p["fp_ind"].astype(np.int32), (256,)), carrier(p["qweight"], (K, N // 2)),
            carrier(p["weights_scaling_factor"], (N,))]


def guarded_out(M, N, dtype=torch.bfloat16, guard=64):
    buf = torch.full((guard + M * N + guard,), 0, dtype=torch.int16, device="cuda")
    buf[:guard] = 0x5a5a
    buf[-guard:] = 0x5a5a
    return buf, buf[guard:guard + M * N].view(dtype).view(M, N)


def guards_intact(buf, guard=64):
    b = buf.cpu().numpy()
    return (b[:guard] == 0x5a5a).all() and (b[-guard:] == 0x5a5a).all()


def run(lib, p, A_bits, bias_bits=None, fp16=False, workspace=None):
    """(output bits, gemm kernel name) of one enqueue of the bf16 layer; fp16=True: the same layer as an fp16 call (for the family)."""
    from mixq_tensorrt_llm_amd import plugin
    M, K = A_bits.shape
    N = p["weight"].shape[0]
    plug = plugin.MixQPlugin.create(M, N, K)
    A_t = R.from_bits(A_bits, "cuda")
    ins = inputs(p, A_t)
    if fp16:
        ins[0] = A_t.float().clamp(-60000, 60000).half()
        ins[3] = ins[3].float().half()
        out = plug.enqueue(ins)
        torch.cuda.synchronize()
        return None, lib.mixq_debug_last_gemm_kernel().decode()
    buf, out = guarded_out(M, N)
    plug.enqueue(ins, output=out, workspace=workspace, bias=None if bias_bits is None else R.from_bits(bias_bits, "cuda"))
    torch.cuda.synchronize()
    assert guards_intact(buf), "output guard bytes were written"
    return R.to_bits(out), lib.mixq_debug_last_gemm_kernel().decode()


FAMILY_CASES = [(QKV[0], QKV[1], m, None) for m in QKV_ROWS if m > 4]
FAMILY_CASES += [(4096, 11008, m, None) for m in (65, 129, 256)]            # K split over workgroups (small tiles / mid)
FAMILY_CASES += [(11008, 4096, 2048, None)]                                  # 256 x 256 split K
FAMILY_CASES += [(4096, 11008, 160, 1421)]                                   # the round-5 deep build (forced)
FAMILY_CASES += [(1040, 1088, m, None) for m in (67, 129, 1000)]             # ragged M, N and K multiples of 16, not of tiles
FAMILY_CASES += [(12288, 4096, m, None) for m in (17, 67, 1000)]             # Llama-2-7B qkv


@pytest.mark.parametrize("fpw_zero", [True, False], ids=["fpW0", "exactP"])
def test_every_family_bit_exact_and_same_family(lib, fpw_zero):
    failures, seen = [], set()
    for N, K, M, knob in FAMILY_CASES:
        p, A_bits = make_bf16_layer(N, K, seed=N + K + M, fpw_zero=fpw_zero, M=M)
        if knob is not None:
            lib.mixq_debug_set_gemm_variant(knob)
        try:
            _, k16 = run(lib, p, A_bits, fp16=True)
            got, kbf = run(lib, p, A_bits)
        finally:
            if knob is not None:
                lib.mixq_debug_reset()
        seen.add(k16)
        if kbf != k16 + " [bf16]":
            failures.append(f"{N}x{K} M={M}: fp16 call {k16!r}, bf16 call {kbf!r}")
        want, _, _, _ = R.prefill(A_bits, p["weight"], p["weights_scaling_factor"], p["fp_weight"], p["fp_ind"].astype(np.int64))
        if not np.array_equal(got, want):
            bad = int((got != want).sum())
            failures.append(f"{N}x{K} M={M} ({k16}): {bad} of {got.size} elements differ from the restatement")
    assert not failures, "\n".join(failures)
    assert len(seen) >= 6, seen


SPLIT_CASES = [  # (N, K, M, knob): split factors forced through the debug knobs (the shapes of tests/test_gpu_bias_epilogue.py)
    (4096, 11008, 80, 62), (1024, 11008, 80, 64), (1024, 11008, 80, 68), (256, 16384, 64, 66),    # small tiles 2 / 4 / 8 / 16
    (4096, 4096, 256, 72), (4096, 4096, 256, 74), (4096, 4096, 256, 78),                          # 256 x 256 tiles 2 / 4 / 8
    (4096, 11008, 256, 1242), (4096, 11008, 256, 1243), (4096, 11008, 256, 1245), (4096, 11008, 256, 1249),  # deep 1 / 2 / 4 / 8
    (4096, 11008, 256, 1253), (4096, 11008, 256, 1273), (4096, 11008, 256, 1431),                # 8-wave build / mid kernel / 128 wide
]


@pytest.mark.parametrize("N,K,M,knob", SPLIT_CASES)
def test_forced_split_factors_bit_exact(lib, N, K, M, knob):
    p, A_bits = make_bf16_layer(N, K, seed=knob, M=M)
    lib.mixq_debug_set_gemm_variant(knob)
    try:
        got, kbf = run(lib, p, A_bits)
    finally:
        lib.mixq_debug_reset()
    want = R.prefill(A_bits, p["weight"], p["weights_scaling_factor"], p["fp_weight"], p["fp_ind"].astype(np.int64))[0]
    assert np.array_equal(got, want), kbf


def workspace_parts(ws, M, K):
    """(qA row-major int8 [M, K], sA bits [M], fpA bits [M, 128]) from the workspace carve of include/mixq.h (qA row-major only)."""
    base = (ws.data_ptr() + 127) // 128 * 128 - ws.data_ptr()
    qa_bytes = M * K
    if 4 < M <= 64:
        qa_bytes = max(qa_bytes, (M + 15) // 16 * 16 * ((K + 63) // 64 * 64))
    sa0 = (base + qa_bytes + 127) // 128 * 128
    fa0 = (sa0 + 2 * M + 127) // 128 * 128
    w = ws.cpu().numpy()
    return (w[base:base + M * K].view(np.int8).reshape(M, K), w[sa0:sa0 + 2 * M].view(np.uint16),
            w[fa0:fa0 + 2 * M * 128].view(np.uint16).reshape(M, 128))


def special_rows(M, K, ind, rng):
    A = (rng.standard_normal((M, K)) * 3).astype(np.float32)
    A_bits = R.bf16_rn(A)
    specials = {0: 0x0000, 1: 0x7fc0}
    A_bits[0] = 0                                       # zero row
    A_bits[1, ::7] = 0x7fc0                             # NaNs in a row
    A_bits[2] = 0xffc1                                  # all NaN
    A_bits[3, 5] = 0x7f80
    A_bits[3, 9] = 0xff80                               # +-inf
    A_bits[4] = R.bf16_rn(rng.uniform(-1, 1, K).astype(np.float32) * 3e38)   # up to bf16 max, beyond fp16's
    A_bits[4, 0] = 0x7f7f
    A_bits[min(5, M - 1)] = rng.integers(1, 0x80, K).astype(np.uint16) | (rng.integers(0, 2, K).astype(np.uint16) << 15)  # subnormals
    del specials
    return A_bits


@pytest.mark.parametrize("K", [1024, 1088, 2048, 4096, 8192, 16384, 32768, 33024])
@pytest.mark.parametrize("knob", [KNOB_BLOCK_ROWS_64, KNOB_BLOCK_ROWS_ALWAYS])
@pytest.mark.parametrize("O_used", [0, 1, 8, 128])
def test_producer_bit_exact(lib, K, knob, O_used):
    """qA / sA / fpA of the bf16 quantiser in every form (block-per-row knob), special rows, outlier sets including columns 0, K-1."""
    from mixq_tensorrt_llm_amd import plugin
    M, N = 67, 32
    rng = np.random.default_rng(K + knob + O_used)
    p, _ = make_bf16_layer(N, K, seed=K, M=1)
    ind = np.sort(rng.choice(np.arange(1, K - 1), 128, replace=False)).astype(np.int32)
    if O_used:   # the first O_used entries are real picks including 0 and K-1, the rest repeat column 0
        ind[:O_used] = np.sort(np.unique(np.r_[0, K - 1, rng.choice(np.arange(1, K - 1), max(O_used - 2, 0), replace=False)]))[:O_used]
        ind[O_used:] = 0
    p["fp_ind"] = ind
    A_bits = special_rows(M, K, ind, rng)
    lib.mixq_debug_set_gemm_variant(knob)
    lib.mixq_debug_set_gemm_variant(KNOB_QA_FRAG_OFF)
    try:
        plug = plugin.MixQPlugin.create(M, N, K)
        ws = torch.full((plug.workspace_size(M, N, K) + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        plug.enqueue(inputs(p, R.from_bits(A_bits, "cuda")), workspace=ws)
        torch.cuda.synchronize()
        form = lib.mixq_debug_last_producer_kernel().decode()
    finally:
        lib.mixq_debug_reset()
    assert form.endswith("[bf16]"), form
    qA, sA, fpA = workspace_parts(ws, M, K)
    wq, ws_ = R.quant_rows(A_bits)
    nan_w, nan_g = np.isnan(R.bf2f(ws_)), np.isnan(R.bf2f(sA))
    assert np.array_equal(nan_w, nan_g), form
    assert np.array_equal(sA[~nan_g], ws_[~nan_w]), form
    assert np.array_equal(qA, wq), (form, np.argwhere(qA != wq)[:5])
    assert np.array_equal(fpA, A_bits[:, ind]), form


def test_random_data_within_bound_and_decode_forms(lib):
    from mixq_tensorrt_llm_amd import _lib
    for N, K, M in [(4608, 3584, 67), (4608, 3584, 1000), (12288, 4096, 129), (1040, 1088, 17)]:
        p, A_bits = make_bf16_layer(N, K, seed=M, exact=False, M=M)
        got, _ = run(lib, p, A_bits)
        ref, P = R.prefill_reference64(A_bits, p["weight"], p["weights_scaling_factor"], p["fp_weight"], p["fp_ind"].astype(np.int64))
        err, lim = R.prefill_bound(got, ref, P)
        assert (err <= lim).all(), (N, K, M, float((err / lim).max()))
    for N, K in [(512, 4096), (12288, 4096)]:   # a narrow and a wide N: the GEMV and the fpA_intB skinny form
        for M in (1, 2, 3, 4):
            p, A_bits = make_bf16_layer(N, K, seed=N + M, exact=False, M=M)
            got, _ = run(lib, p, A_bits)
            q_un = np.empty((K, N), np.int8)
            _lib.load().mixq_unprocess_weights_int8(q_un.ctypes.data, p["qweight"].ctypes.data, K, N)
            ref, mag = R.decode64(A_bits, q_un, p["weights_scaling_factor"])
            err = np.abs(R.bf2f(got).astype(np.float64) - ref)
            lim = R.ulp_bf16(ref) + K * 2.0 ** -23 * mag    # one bf16 rounding + an fp32 accumulation bound
            assert (err <= lim).all(), (N, K, M, float((err / lim).max()))


def special_bias(N, seed):
    rng = np.random.default_rng(seed)
    b = R.bf16_rn(rng.standard_normal(N).astype(np.float32) * 0.5)
    b[:6] = [0x0000, 0x8000, 0x7f7f, 0xff7f, 0x0001, 0x8003]
    return b


def test_bias_equals_bias_free_call_plus_bf16_add(lib):
    cases = [(QKV[0], QKV[1], m) for m in (1, 3, 17, 80, 320, 2048)] + [(4096, 11008, 129), (11008, 4096, 2048), (1040, 1088, 67)]
    for N, K, M in cases:
        p, A_bits = make_bf16_layer(N, K, seed=M, exact=False, M=M)
        b = special_bias(N, M)
        plain, k0 = run(lib, p, A_bits)
        got, k1 = run(lib, p, A_bits, bias_bits=b)
        assert k0 == k1
        want = R.bias_add(plain, b)
        assert np.array_equal(got, want), (N, K, M, int((got != want).sum()))


def test_range_beyond_fp16(lib):
    """Activations of 1e5..1e30 in outlier and regular columns: finite bf16 results within the bound; the fp16 cast route gives inf."""
    from mixq_tensorrt_llm_amd import plugin
    N, K, M = 1040, 1088, 67
    p, A_bits = make_bf16_layer(N, K, seed=5, exact=False, M=M)
    rng = np.random.default_rng(5)
    A = R.bf2f(A_bits).copy()
    A *= np.exp(rng.uniform(np.log(1e5), np.log(1e30), (M, 1))).astype(np.float32)
    A_bits = R.bf16_rn(A)
    got, _ = run(lib, p, A_bits)
    ref, P = R.prefill_reference64(A_bits, p["weight"], p["weights_scaling_factor"], p["fp_weight"], p["fp_ind"].astype(np.int64))
    err, lim = R.prefill_bound(got, ref, P)
    assert np.isfinite(R.bf2f(got)).all() and (err <= lim).all()
    plug = plugin.MixQPlugin.create(M, N, K)
    ins = inputs(p, R.from_bits(A_bits, "cuda"))
    ins[0], ins[3] = ins[0].half(), ins[3].half()            # the cast route
    out16 = plug.enqueue(ins).to(torch.bfloat16)
    torch.cuda.synchronize()
    assert not torch.isfinite(out16.float()).all()


def test_other_routes_same_bits(lib, tmp_path):
    from mixq_tensorrt_llm_amd import checkpoint, mixlib, plugin
    N, K = 4608, 3584
    for M in (17, 40, 80, 1000):
        p, A_bits = make_bf16_layer(N, K, seed=M, exact=False, M=M)
        eager, _ = run(lib, p, A_bits)
        plug = plugin.MixQPlugin.create(M, N, K)
        ws = torch.full((plug.workspace_size(M, N, K),), 0xff, dtype=torch.uint8, device="cuda")   # poisoned workspace
        poisoned, _ = run(lib, p, A_bits, workspace=ws)
        assert np.array_equal(poisoned, eager), M
        layer = plugin.MixQLinear(K, N, bias=True, dtype=torch.bfloat16, device="cuda:0")
        p2 = dict(p, bias=special_bias(N, M))
        layer.load(p2)
        A_t = R.from_bits(A_bits, "cuda")
        y = layer(A_t)
        assert y.dtype == torch.bfloat16
        with_bias, _ = run(lib, p, A_bits, bias_bits=p2["bias"])
        assert np.array_equal(R.to_bits(y), with_bias), M
        if M <= 64:   # a registered weight image
            img = mixlib.WeightImage(layer.weight.view(torch.int8))
            img.verify()
            try:
                assert np.array_equal(R.to_bits(layer(A_t)), with_bias), M
            finally:
                img.close()
        # one HIP-graph capture and replay
        static_in = A_t.clone()
        layer(static_in)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                static_out = layer(static_in)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(R.to_bits(static_out), with_bias), M
        # checkpoint round trip
        d = tmp_path / f"ck{M}"
        checkpoint.save_checkpoint(str(d), {"l": p2})
        _, layers = checkpoint.load_checkpoint(str(d))
        l2 = checkpoint.load_linear(plugin.MixQLinear(K, N, bias=True, dtype=torch.bfloat16, device="cuda:0"), layers["l"])
        assert np.array_equal(R.to_bits(l2(A_t)), with_bias), M


def test_mixed_types_raise():
    from mixq_tensorrt_llm_amd import plugin
    p, A_bits = make_bf16_layer(512, 1024, seed=1, M=8)
    ins = inputs(p, R.from_bits(A_bits, "cuda"))
    ins[3] = ins[3].half()
    with pytest.raises(TypeError):
        plugin.MixQPlugin.create(8, 512, 1024).enqueue(ins)


def test_c_host_negotiates_bf16(tmp_path):
    exe = str(tmp_path / "host_bf16")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I", os.path.join(ROOT, "include"), "-I",
           "/opt/rocm/include", os.path.join(ROOT, "tests", "c_abi", "host_bf16.c"), "-o", exe, "-L",
           os.path.join(ROOT, "mixq_tensorrt_llm_amd"), "-l:libmixq_mi355x.so", "-L", "/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + os.path.join(ROOT, "mixq_tensorrt_llm_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    for M in (80, 3):
        N, K = 512, 1024
        p, A_bits = make_bf16_layer(N, K, seed=M, exact=True, M=M)
        d = tmp_path / f"d{M}"
        d.mkdir()
        A_bits.tofile(d / "A.bf16")
        np.ascontiguousarray(p["weight"]).astype(np.int8).tofile(d / "weight.i8")
        np.ascontiguousarray(p["weights_scaling_factor"]).astype(np.float16).tofile(d / "sw.f16")
        np.ascontiguousarray(p["fp_weight"]).tofile(d / "fp_weight.bf16")
        np.ascontiguousarray(p["fp_ind"]).astype(np.int32).tofile(d / "fp_ind.i32")
        np.ascontiguousarray(p["qweight"]).astype(np.uint8).tofile(d / "qweight.u8")
        r = subprocess.run([exe, str(d), str(M), str(N), str(K)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        got = np.fromfile(d / "out.bf16", dtype=np.uint16).reshape(M, N)
        want, _ = run(pytest.importorskip("mixq_tensorrt_llm_amd")._lib.load(), p, A_bits)
        assert np.array_equal(got, want), M
        assert "output type 7" in r.stdout, r.stdout
