"""GPU (-m gpu): the merged gate / up projection (mixq_gemm_mixed_gate_up_typed: one GEMM launch on (M, 2N, K) with SiLU(gate) x up in its
epilogue), fp16 and bf16, on every kernel family plan_gemm can choose.  The acceptance criterion is an identity, not a tolerance: the
bits of the library's own two launches (mixq_gemm_mixed_typed for up, mixq_gemm_mixed_act_typed epilogue 3 with mul = u for gate) on the
split layers, and the bits of the restatement (tests/gate_up_restate.py, with the device's expf).  Operands are the exact-product layers
of tests/test_gpu_silu_epilogue.py, read as MERGED layers of N = 2 x (output width) rows."""
import functools

import numpy as np
import pytest

import gate_up_restate as G
import guarded
from test_gpu_bf16_operator import FAMILY_CASES as OP_FAMILY_CASES, SPLIT_CASES, make_bf16_layer
from test_gpu_silu_epilogue import Call, bits, build_mlp, dtype_of, host_operands, stream, type_of, up

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
S = G.S

O = 128
MAX_ROWS = 2048
# (N2 = GEMM width = 2 x output width, K, M, knob, qA layout).  The family list of the bf16 operator test up to 2048 rows and its forced split
# factors, as GEMM problems; 1040 cannot be a merged width (520 % 16 != 0): the ragged shape has OUTPUT width 1040 (nothing a multiple of a
# tile, the merged width 2080 ends in the middle of a 32-column MFMA block of a 64- / 128- / 256-wide tile); a decode batch in both layouts
CASES = [(n, k, m, knob, 0) for n, k, m, knob in OP_FAMILY_CASES if m <= MAX_ROWS and n != 1040]
CASES += [(n, k, m, knob, 0) for n, k, m, knob in SPLIT_CASES]
CASES += [(2080, 1088, m, None, 0) for m in (67, 129, 1000)]
CASES += [(12288, 4096, 17, None, 1)]
assert (12288, 4096, 17, None, 0) in CASES and {n // 2 for n, *_ in CASES} >= {6144, 2048, 5504, 512, 128, 1040}
TYPED = [(c, bf) for c in CASES for bf in (True, False)]


def case_id(v):
    (n, k, m, knob, lay), bf = v
    return f"{n // 2}x{k}-M{m}" + (f"-knob{knob}" if knob is not None else "") + ("-frag" if lay else "") + ("-bf16" if bf else "-fp16")


@pytest.fixture(scope="module")
def lib():
    from mixq_tensorrt_llm_amd import _lib
    lib = _lib.load()
    lib.mixq_debug_reset()
    yield lib
    lib.mixq_debug_reset()


def device_expf(x):
    """expf as silu_f32 of mixq_device.h calls it: the device's libm expf (torch's float32 exp on the GPU is the same routine)."""
    return torch.exp(torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()).cpu().numpy()


def split_host(h):
    """Host operands of the gate and the up layer of merged host operands (pack.split_gate_up)."""
    from mixq_tensorrt_llm_amd import pack
    g, u = pack.split_gate_up(dict(weight=h["W"], weights_scaling_factor=h["sW"], fp_weight=h["fpW"], fp_ind=np.zeros(O, np.int32)))
    return [dict(h, W=np.ascontiguousarray(d["weight"]), sW=np.ascontiguousarray(d["weights_scaling_factor"]),
                 fpW=np.ascontiguousarray(d["fp_weight"])) for d in (g, u)]


def gate_up(c, n_out=None, out=None, o=O):
    """(Out [M, N2 / 2], kernel name) of mixq_gemm_mixed_gate_up_typed on the merged operands of Call c."""
    n_out = c.N // 2 if n_out is None else n_out
    out = torch.full((c.M, n_out), float("nan"), dtype=dtype_of(c.bf), device="cuda") if out is None else out
    s = c.scratch
    rc = c.lib.mixq_gemm_mixed_gate_up_typed(c.q.data_ptr(), c.W.data_ptr(), c.sA.data_ptr(), c.sW.data_ptr(), c.fpA.data_ptr() if o else None,
                                             c.fpW.data_ptr() if o else None, out.data_ptr(), c.M, n_out, c.K, o, c.layout, type_of(c.bf),
                                             None if s is None else s.data_ptr(), 0 if s is None else s.numel(), stream())
    assert rc == 0, f"mixq_gemm_mixed_gate_up_typed: rc {rc}"
    return out, c.lib.mixq_debug_last_gemm_kernel().decode()


def two_launches(lib, h, M, N2, K, bf, layout):
    """silu(gate) x up [M, N2 / 2] through the library's own two launches on the split layers."""
    hg, hu = split_host(h)
    cu, cg = Call(lib, hu, M, N2 // 2, K, bf, layout), Call(lib, hg, M, N2 // 2, K, bf, layout)
    u, ku = cu.typed()
    out, kg = cg.act(3, u)
    return out, (ku, kg)


def report(what, got, want, bf):
    bad = got != want
    steps = int(S.ulp_steps(got[bad], want[bad]).max()) if bad.any() and not (S.is_nan(got, bf) | S.is_nan(want, bf)).any() else 0
    return f"{what}: {int(bad.sum())} of {got.size} outputs differ (fraction {bad.mean():.2e}, at most {steps} steps of T)"


# -------------------------------------------------------------------------------------------- 1. every family, bit for bit ----
@pytest.mark.parametrize("case", TYPED, ids=case_id)
def test_every_family_bit_for_bit(lib, case):
    """Out equals (a) the restatement and (b) the two launches on the split layers, element for element by bit pattern; the kernel is the
    plain call's on (M, 2N, K) under the same knob."""
    (N2, K, M, knob, layout), bf = case
    h = host_operands(N2, K, M, (knob or 0) + N2 + K + M, bf)
    v = S.pre_activation(h["q"], h["sA"], h["fpA"], h["W"], h["sW"], h["fpW"], bf)
    want = G.gate_up_from_v(v, bf, device_expf)
    if knob is not None:
        lib.mixq_debug_set_gemm_variant(knob)
    try:
        c = Call(lib, h, M, N2, K, bf, layout)
        _, k_plain = c.typed()
        out, k_gu = gate_up(c)
        two, k_two = two_launches(lib, h, M, N2, K, bf, layout)
        torch.cuda.synchronize()
    finally:
        if knob is not None:
            lib.mixq_debug_reset()
    what = f"{case_id(case)} ({k_gu})"
    got, two = bits(out), bits(two)
    assert k_gu == k_plain and k_plain.endswith(" [bf16]") == bf, f"{what}: the plain call on ({M}, {N2}, {K}) reports {k_plain!r}"
    assert not S.is_nan(got, bf).any(), f"{what}: NaN or unwritten outputs"
    print(report(f"{what} vs the two launches {k_two}", got, two, bf))
    print(report(f"{what} vs the restatement", got, want, bf))
    assert np.array_equal(got, two), report(f"{what} vs the two launches {k_two}", got, two, bf)
    assert np.array_equal(got, want), report(f"{what} vs the restatement", got, want, bf)


@pytest.mark.parametrize("bf", [True, False], ids=["bf16", "fp16"])
def test_no_outlier_columns(lib, bf):
    """O == 0 (NULL fpA / fpW2): the GEMM alone, in two families."""
    for N2, K, M in ((2080, 1088, 129), (2080, 1088, 17)):
        h = host_operands(N2, K, M, 21, bf)
        want = G.gate_up_bits(h["q"], h["sA"], None, h["W"], h["sW"], None, bf, device_expf)
        c = Call(lib, h, M, N2, K, bf)
        out, name = gate_up(c, o=0)
        hg, hu = split_host(h)
        outs = []
        for hh, epi in ((hu, 0), (hg, 3)):
            cc = Call(lib, hh, M, N2 // 2, K, bf)
            o2 = cc.out()
            rc = lib.mixq_gemm_mixed_act_typed(cc.q.data_ptr(), cc.W.data_ptr(), cc.sA.data_ptr(), cc.sW.data_ptr(), None, None,
                                               outs[0].data_ptr() if epi else None, o2.data_ptr(), M, N2 // 2, K, 0, epi, 0, type_of(bf), None, 0, stream())
            assert rc == 0
            outs.append(o2)
        torch.cuda.synchronize()
        got = bits(out)
        assert np.array_equal(got, bits(outs[1])), report(f"O = 0, {M} rows ({name}) vs the two launches", got, bits(outs[1]), bf)
        assert np.array_equal(got, want), report(f"O = 0, {M} rows ({name}) vs the restatement", got, want, bf)


def test_at_least_six_families_are_covered(lib):
    seen = set()
    for N2, K, M, knob, layout in CASES:
        h = dict(q=np.zeros((M, K), np.int8), sA=np.zeros(M, np.uint16), fpA=np.zeros((M, O), np.uint16), W=np.zeros((N2, K), np.int8),
                 sW=np.zeros(N2, np.float16), fpW=np.zeros((N2, O), np.uint16))
        if knob is not None:
            lib.mixq_debug_set_gemm_variant(knob)
        try:
            seen.add(gate_up(Call(lib, h, M, N2, K, True, layout))[1])
        finally:
            if knob is not None:
                lib.mixq_debug_reset()
    torch.cuda.synchronize()
    assert len(seen) >= 6, seen


# ------------------------------------------------------------------------------------------------------------- 2. random data ----
@functools.lru_cache(maxsize=2)
def random_layer(N2, K, M):
    return make_bf16_layer(N2, K, seed=N2 + M, exact=False, M=M)


# knob 1: the two-barrier tiles, 2: the 256 x 256 kernel, 5: the 128 x 256 kernel, 1273: the deep form; None at 17 rows: the skinny kernel
@pytest.mark.parametrize("bf", [True, False], ids=["bf16", "fp16"])
@pytest.mark.parametrize("M,knob", [(129, 1), (129, 2), (129, 5), (160, 1273), (17, None)])
def test_random_outlier_weights_in_one_family(lib, M, knob, bf):
    """Ordinary random outlier weights: P depends on the summation order, so both routes are forced into the same family, which sums P in
    the same order whatever the width -- the one launch is the two launches again, bit for bit."""
    N2, K = 2080, 1088
    p, A_bits = random_layer(N2, K, M)
    A_T = A_bits if bf else S.rn(S.tof(A_bits, True), False)
    ind = p["fp_ind"].astype(np.int64)
    q, sA = S.quant_rows(A_T, bf)
    h = dict(q=q, sA=sA, fpA=np.ascontiguousarray(A_T[:, ind]), W=np.ascontiguousarray(p["weight"]).astype(np.int8),
             sW=np.ascontiguousarray(p["weights_scaling_factor"]).astype(np.float16),
             fpW=np.ascontiguousarray(p["fp_weight"] if bf else S.rn(S.tof(p["fp_weight"], True), False)))
    if knob is not None:
        lib.mixq_debug_set_gemm_variant(knob)
    try:
        out, k_gu = gate_up(Call(lib, h, M, N2, K, bf))
        two, (ku, kg) = two_launches(lib, h, M, N2, K, bf, 0)
        torch.cuda.synchronize()
    finally:
        if knob is not None:
            lib.mixq_debug_reset()
    assert ku == k_gu and kg == k_gu, f"one launch on {k_gu!r}, two launches on {ku!r} / {kg!r}"
    got, two = bits(out), bits(two)
    assert not S.is_nan(got, bf).any()
    assert np.array_equal(got, two), report(f"{M} rows, knob {knob} ({k_gu})", got, two, bf)


# -------------------------------------------------------------------------------------------------------- 3. guarded buffers ----
# (M, output width, K, knob): the ragged shape; then one per family -- skinny, two-barrier tiles, 256 x 256, 128 x 256, the mid kernel, and the
# K splits over workgroups of the small tiles, the deep form and the 256 x 256 tiles (scratch with hand-over words)
GUARDED = [(1000, 1040, 1088, None), (17, 272, 2048, None), (257, 272, 1088, 1), (257, 272, 1088, 2), (257, 272, 1088, 5), (256, 2048, 11008, 1273),
           (80, 512, 11008, 64), (256, 2048, 11008, 1245), (256, 2048, 4096, 74)]


@pytest.mark.parametrize("bf", [True, False], ids=["bf16", "fp16"])
@pytest.mark.parametrize("M,N,K,knob", GUARDED, ids=[f"M{m}-{n}x{k}" + (f"-knob{kn}" if kn else "") for m, n, k, kn in GUARDED])
def test_guarded_buffers(lib, M, N, K, knob, bf):
    """Out [M, N] in an exact-size guarded allocation, NaN-filled: every element is written, no guard byte is touched (inputs and scratch
    included), the hand-over words of the scratch are left zero and a repeat on the same scratch gives the same bits -- those of the two
    launches."""
    rng = np.random.default_rng(M + N + K)
    h = dict(q=rng.integers(-127, 128, (M, K)).astype(np.int8), sA=S.rn(rng.uniform(0.005, 0.02, M).astype(np.float32), bf),
             fpA=S.rn(rng.integers(-16, 17, (M, O)).astype(np.float32) * 4, bf), W=rng.integers(-127, 128, (2 * N, K)).astype(np.int8),
             sW=rng.uniform(0.0005, 0.002, 2 * N).astype(np.float16), fpW=S.rn(rng.integers(-8, 9, (2 * N, O)).astype(np.float32) * 2.0 ** -6, bf))
    nanfill = guarded.BF16_NAN if bf else guarded.F16_NAN
    Gd = guarded.Guarded
    g_q = Gd(M * K, guarded.I8_MAX, init=h["q"], guard=guarded.IN_GUARD, offset=16)
    g_sA = Gd(2 * M, nanfill, init=h["sA"], guard=guarded.IN_GUARD, offset=2)
    g_fpA = Gd(2 * M * O, nanfill, init=h["fpA"], guard=guarded.IN_GUARD, offset=16)
    g_W = Gd(2 * N * K, guarded.I8_MAX, init=h["W"], guard=guarded.IN_GUARD, offset=16)
    g_sW = Gd(2 * 2 * N, guarded.F16_NAN, init=h["sW"], guard=guarded.IN_GUARD, offset=16)
    g_fpW = Gd(2 * 2 * N * O, nanfill, init=h["fpW"], guard=guarded.IN_GUARD, offset=16)
    g_out = Gd(2 * M * N, nanfill, guard=guarded.out_guard(N, 2), offset=16)
    if knob is not None:
        lib.mixq_debug_set_gemm_variant(knob)
    try:
        n = int(lib.mixq_gemm_scratch_size(M, 2 * N, K))
        scratch = Gd(n, 0xA5, init=np.zeros(n, np.uint8), guard=guarded.SCRATCH_GUARD) if n else None
        runs = []
        for _ in range(2):
            g_out.set_body(None)
            rc = lib.mixq_gemm_mixed_gate_up_typed(g_q.ptr, g_W.ptr, g_sA.ptr, g_sW.ptr, g_fpA.ptr, g_fpW.ptr, g_out.ptr, M, N, K, O, 0, type_of(bf),
                                                   scratch.ptr if scratch else None, n, stream())
            torch.cuda.synchronize()
            assert rc == 0
            name = lib.mixq_debug_last_gemm_kernel().decode()
            for g, what in ((g_out, "Out"), (g_fpA, "fpA"), (g_sA, "sA"), (g_q, "qA"), (g_W, "W2"), (g_sW, "sW2"), (g_fpW, "fpW2")) + (((scratch, "scratch"),) if scratch else ()):
                guarded.assert_intact(g, f"{what} of {M} x {N} x {K} ({name})")
            runs.append(g_out.body(np.uint16, (M, N)).copy())
            if scratch:
                words = scratch.body(np.uint8, (n,))[:16384]
                assert not words.any(), f"{name}: {int(np.count_nonzero(words))} bytes of the hand-over words are left non-zero"
        two, _ = two_launches(lib, h, M, 2 * N, K, bf, 0)
        torch.cuda.synchronize()
    finally:
        if knob is not None:
            lib.mixq_debug_reset()
    if knob in (64, 1245, 74):
        assert scratch is not None, f"knob {knob} on {M} x {2 * N} x {K} ({name}) splits K over workgroups and needs scratch"
    assert not S.is_nan(runs[0], bf).any(), f"{name}: {int(S.is_nan(runs[0], bf).sum())} outputs were not written"
    assert np.array_equal(runs[0], runs[1]), f"{name}: a repeat on the same scratch gives other bits"
    assert np.array_equal(runs[0], bits(two)), report(f"{name} vs the two launches", runs[0], bits(two), bf)
    assert np.array_equal(g_q.body(np.int8, (M, K)), h["q"]) and np.array_equal(g_W.body(np.int8, (2 * N, K)), h["W"])


# ------------------------------------------------------------------------------------------------------------------ 4. Python ----
@pytest.mark.parametrize("bf", [True, False], ids=["bf16", "fp16"])
def test_fused_llama_mlp_equals_the_unfused_one_eager_and_in_a_graph(lib, bf):
    M, hidden, inter = 256, 4096, 5504
    mlp, cache, norm = build_mlp(hidden, inter, bf, seed=77)
    gen = torch.Generator(device="cpu").manual_seed(5 + int(bf))
    xs = [(2.0 * torch.randn((M, hidden), generator=gen)).to(dtype_of(bf)).cuda() for _ in range(2)]
    x = xs[0].clone()

    def step():
        norm.forward(x)
        return mlp.forward_quantised(cache.q_xcache, cache.x_scale, cache.activation_outliers, cache.q_layout)

    unfused = [None, None]
    for i in (0, 1):
        x.copy_(xs[i])
        unfused[i] = bits(step())
    assert mlp.fuse_gate_up() is mlp and mlp._gate_up is not None
    W2, sW2, fpW2 = mlp._gate_up
    assert tuple(W2.shape) == (2 * inter, hidden) and W2.dtype == torch.int8 and sW2.dtype == torch.float16 and fpW2.dtype == dtype_of(bf)
    x.copy_(xs[0])
    y = step()
    name = lib.mixq_debug_last_gemm_kernel().decode()      # (down's; the merged launch ran before it)
    torch.cuda.synchronize()
    assert y.dtype == dtype_of(bf) and tuple(y.shape) == (M, hidden) and torch.isfinite(y.float()).all()
    assert np.array_equal(bits(y), unfused[0]), f"the fused MLP differs from the unfused one ({name})"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g = step()
    for i in (1, 0):                                          # fresh producer outputs are written into the captured buffers
        x.copy_(xs[i])
        want = bits(step())
        y_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(want, unfused[i]), f"eager call {i} of the fused MLP differs from the unfused one"
        assert np.array_equal(bits(y_g), want), f"replay {i} differs from the eager call"
    mlp.fuse_gate_up(False)
    x.copy_(xs[1])
    assert mlp._gate_up is None and np.array_equal(bits(step()), unfused[1])
