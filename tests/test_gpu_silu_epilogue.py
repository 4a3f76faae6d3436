"""GPU (-m gpu): the SiLU and SiLU x up epilogues of the fused mixed GEMM (mixq_gemm_mixed_act_typed), fp16 and bf16, with the outlier
product inside the kernel, on every kernel family plan_gemm can choose.  The inputs are the exact-product layers of
tests/test_gpu_bf16_operator.py (outlier columns are small integers times powers of two: P does not depend on the summation order) and
an fp16 twin of them; the expected values come from tests/silu_restate.py."""
import functools

import numpy as np
import pytest

import guarded
import silu_restate as S
from test_gpu_bf16_operator import FAMILY_CASES as OP_FAMILY_CASES, SPLIT_CASES, make_bf16_layer

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PLAIN, SILU, SILU_MUL = 0, 1, 3
O = 128
MAX_ROWS = 2048

# (N, K, M, knob, qA layout): the family list of the bf16 operator test up to 2048 rows, its forced split factors, the ragged shape and a
# decode batch in both qA layouts
CASES = [(n, k, m, knob, 0) for n, k, m, knob in OP_FAMILY_CASES if m <= MAX_ROWS]
CASES += [(n, k, m, knob, 0) for n, k, m, knob in SPLIT_CASES]
CASES += [(12288, 4096, 17, None, 1)]
assert all(c in CASES for c in [(1040, 1088, 67, None, 0), (1040, 1088, 129, None, 0), (1040, 1088, 1000, None, 0), (12288, 4096, 17, None, 0),
                                (4608, 3584, 2048, None, 0), (11008, 4096, 2048, None, 0)])
TYPED = [(c, bf) for c in CASES for bf in (True, False)]


def case_id(v):
    (n, k, m, knob, lay), bf = v
    return f"{n}x{k}-M{m}" + (f"-knob{knob}" if knob is not None else "") + ("-frag" if lay else "") + ("-bf16" if bf else "-fp16")


@pytest.fixture(scope="module")
def lib():
    from mixq_tensorrt_llm_amd import _lib
    lib = _lib.load()
    lib.mixq_debug_reset()
    yield lib
    lib.mixq_debug_reset()


def stream():
    return torch.cuda.current_stream().cuda_stream


def type_of(bf):
    from mixq_tensorrt_llm_amd import _lib
    return _lib.MIXQ_TYPE_BF16 if bf else _lib.MIXQ_TYPE_HALF


def dtype_of(bf):
    return torch.bfloat16 if bf else torch.float16


@functools.lru_cache(maxsize=2)
def layer(N, K, M, seed):
    return make_bf16_layer(N, K, seed=seed, M=M)


def host_operands(N, K, M, seed, bf):
    """numpy operands of one call in type T: the exact-product layer, its activations quantised by T's rules, the outlier columns."""
    p, A_bits = layer(N, K, M, seed)
    A_T = A_bits if bf else S.rn(S.tof(A_bits, True), False)
    ind = p["fp_ind"].astype(np.int64)
    q, sA = S.quant_rows(A_T, bf)
    fpW = p["fp_weight"] if bf else S.rn(S.tof(p["fp_weight"], True), False)
    assert np.array_equal(S.tof(fpW, bf), S.tof(p["fp_weight"], True)) and np.array_equal(S.tof(A_T[:, ind], bf), S.tof(A_bits[:, ind], True))
    return dict(q=q, sA=sA, fpA=np.ascontiguousarray(A_T[:, ind]), W=np.ascontiguousarray(p["weight"]).astype(np.int8),
                sW=np.ascontiguousarray(p["weights_scaling_factor"]).astype(np.float16), fpW=np.ascontiguousarray(fpW))


def up(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype in (np.uint16, np.float16) else a).cuda()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def fragment_major(q, M, K):
    """Row-major int8 [M, K] -> the fragment-major image (the inverse of mixlib.qa_to_row_major; rows and K padded with zeros)."""
    tiles, steps = (M + 15) // 16, (K + 63) // 64
    pad = np.zeros((tiles * 16, steps * 64), np.int8)
    pad[:M, :K] = q
    return np.ascontiguousarray(pad.reshape(tiles, 16, steps, 4, 16).transpose(0, 2, 3, 1, 4)).reshape(-1)


class Call:
    """Device operands of one shape and type, and the calls on them."""

    def __init__(self, lib, h, M, N, K, bf, layout=0):
        from mixq_tensorrt_llm_amd import mixlib
        self.lib, self.M, self.N, self.K, self.bf, self.layout = lib, M, N, K, bf, layout
        self.q = up(fragment_major(h["q"], M, K) if layout else h["q"])
        if layout:
            assert np.array_equal(mixlib.qa_to_row_major(self.q, M, K).cpu().numpy(), h["q"])
        self.sA, self.fpA, self.W, self.sW, self.fpW = (up(h[k]) for k in ("sA", "fpA", "W", "sW", "fpW"))
        n = 0 if layout else int(lib.mixq_gemm_scratch_size(M, N, K))
        self.scratch = torch.zeros(n, dtype=torch.uint8, device="cuda") if n else None

    def out(self):
        return torch.full((self.M, self.N), float("nan"), dtype=dtype_of(self.bf), device="cuda")

    def act(self, epi, mul=None, out=None):
        """(Out, kernel name) of mixq_gemm_mixed_act_typed."""
        out = self.out() if out is None else out
        s = self.scratch
        rc = self.lib.mixq_gemm_mixed_act_typed(self.q.data_ptr(), self.W.data_ptr(), self.sA.data_ptr(), self.sW.data_ptr(), self.fpA.data_ptr(),
                                                self.fpW.data_ptr(), None if mul is None else mul.data_ptr(), out.data_ptr(), self.M, self.N,
                                                self.K, O, epi, self.layout, type_of(self.bf), None if s is None else s.data_ptr(),
                                                0 if s is None else s.numel(), stream())
        assert rc == 0, f"mixq_gemm_mixed_act_typed: rc {rc}"
        name = self.lib.mixq_debug_last_gemm_kernel().decode()
        return out, name

    def typed(self):
        """(Out, kernel name) of the plain call, mixq_gemm_mixed_typed with a NULL bias."""
        out, s = self.out(), self.scratch
        rc = self.lib.mixq_gemm_mixed_typed(self.q.data_ptr(), self.W.data_ptr(), self.sA.data_ptr(), self.sW.data_ptr(), self.fpA.data_ptr(),
                                            self.fpW.data_ptr(), None, out.data_ptr(), self.M, self.N, self.K, O, self.layout, type_of(self.bf),
                                            None if s is None else s.data_ptr(), 0 if s is None else s.numel(), stream())
        assert rc == 0, f"mixq_gemm_mixed_typed: rc {rc}"
        return out, self.lib.mixq_debug_last_gemm_kernel().decode()

    def two_launch(self, epi, y, mul=None):
        """fp16: the existing route -- the outlier product as an fp16 addend y, then the SiLU entries without outlier operands."""
        assert not self.bf
        out, s = self.out(), self.scratch
        a = (self.q.data_ptr(), self.W.data_ptr(), self.sA.data_ptr(), self.sW.data_ptr(), y.data_ptr())
        ws = None if s is None else s.data_ptr()
        if self.layout:
            rc = self.lib.mixq_int8_fused_dequantize_layout(*a, None if mul is None else mul.data_ptr(), out.data_ptr(), self.M, self.N, self.K,
                                                            epi, self.layout, ws, stream())
        elif epi == SILU:
            rc = self.lib.mixq_int8_fused_dequantize_silu(*a, out.data_ptr(), self.M, self.N, self.K, ws, stream())
        else:
            rc = self.lib.mixq_int8_fused_dequantize_silu_mul(*a, mul.data_ptr(), out.data_ptr(), self.M, self.N, self.K, ws, stream())
        assert rc == 0, f"two-launch route: rc {rc}"
        return out


def special_mul(M, N, bf, seed):
    """Random values plus rows of 0, -0, subnormals and the largest finite value."""
    rng = np.random.default_rng(seed)
    m = S.rn(rng.standard_normal((M, N)).astype(np.float32) * 1.5, bf)
    m[0], m[1] = 0x0000, 0x8000
    m[2] = rng.integers(1, 0x80 if bf else 0x400, N).astype(np.uint16) | (rng.integers(0, 2, N).astype(np.uint16) << 15)
    m[3] = np.where(rng.integers(0, 2, N) == 1, 0x7F7F if bf else 0x7BFF, 0xFF7F if bf else 0xFBFF).astype(np.uint16)
    return m


# ------------------------------------------------------------------------------- 1-3. every family: SiLU, SiLU x up, the two-launch route ----
@pytest.mark.parametrize("case", TYPED, ids=case_id)
def test_silu_and_silu_mul_on_every_family(lib, case):
    """1. SiLU is within one step of T of the restatement in fewer than 0.1 % of the elements (the last ulp of the two expf), and exact
    elsewhere; the kernel is the plain call's.  2. SiLU x up equals SiLU followed by torch's multiply in T, bit for bit.  3. fp16: the one
    launch equals mixq_int8_fused_dequantize_silu / _silu_mul fed y = fp16(P), bit for bit."""
    (N, K, M, knob, layout), bf = case
    h = host_operands(N, K, M, (knob or 0) + N + K + M, bf)
    want = S.silu_bits(S.pre_activation(h["q"], h["sA"], h["fpA"], h["W"], h["sW"], h["fpW"], bf), bf)
    mul_h = special_mul(M, N, bf, M)
    if knob is not None:
        lib.mixq_debug_set_gemm_variant(knob)
    try:
        c = Call(lib, h, M, N, K, bf, layout)
        _, k_plain = c.typed()
        g, k_silu = c.act(SILU)
        mul = up(mul_h).view(dtype_of(bf))
        gm, k_mul = c.act(SILU_MUL, mul)
        if not bf:
            y = up(S.outlier_product_bits(h["fpA"], h["fpW"], False)).view(torch.float16)
            two_silu, two_mul = c.two_launch(SILU, y), c.two_launch(SILU_MUL, y, mul)
        torch.cuda.synchronize()
    finally:
        if knob is not None:
            lib.mixq_debug_reset()
    what = f"{case_id(case)} ({k_silu})"
    assert k_silu == k_plain and k_mul == k_plain, f"{what}: the plain call reports {k_plain!r}, SiLU x up {k_mul!r}"
    assert k_plain.endswith(" [bf16]") == bf
    got = bits(g)
    assert not S.is_nan(got, bf).any(), f"{what}: NaN or unwritten outputs"
    steps = S.ulp_steps(got, want)
    frac = float((got != want).mean())
    print(f"{what}: SiLU max steps {int(steps.max())}, fraction differing {frac:.2e}")
    assert steps.max() <= 1, f"{what}: {int((steps > 1).sum())} outputs more than one step of T from the restatement"
    assert frac < 1e-3, f"{what}: {frac:.2e} of the outputs differ from the restatement"
    two_step = bits(g * mul)
    assert np.array_equal(bits(gm), two_step), f"{what}: SiLU x up differs from SiLU then torch's multiply in {int((bits(gm) != two_step).sum())} outputs"
    if not bf:
        assert np.array_equal(bits(two_silu), got), f"{what}: SiLU differs from the two-launch route in {int((bits(two_silu) != got).sum())} outputs"
        assert np.array_equal(bits(two_mul), bits(gm)), f"{what}: SiLU x up differs from the two-launch route"


def test_at_least_six_families_are_covered(lib):
    seen = set()
    for N, K, M, knob, layout in CASES:
        h = dict(q=np.zeros((M, K), np.int8), sA=np.zeros(M, np.uint16), fpA=np.zeros((M, O), np.uint16), W=np.zeros((N, K), np.int8),
                 sW=np.zeros(N, np.float16), fpW=np.zeros((N, O), np.uint16))
        if knob is not None:
            lib.mixq_debug_set_gemm_variant(knob)
        try:
            seen.add(Call(lib, h, M, N, K, True, layout).act(SILU)[1])
        finally:
            if knob is not None:
                lib.mixq_debug_reset()
    torch.cuda.synchronize()
    assert len(seen) >= 6, seen


@pytest.mark.parametrize("bf", [True, False], ids=["bf16", "fp16"])
def test_inf_and_nan_in_mul(lib, bf):
    """A second small call: infinities and NaNs in mul give NaNs where torch's multiply does and infinities of the same sign."""
    N, K, M = 1040, 1088, 67
    h = host_operands(N, K, M, 11, bf)
    c = Call(lib, h, M, N, K, bf)
    rng = np.random.default_rng(12)
    m = special_mul(M, N, bf, 12)
    inf, nan = (0x7F80, 0x7FC0) if bf else (0x7C00, 0x7E00)
    m[4], m[5], m[6] = inf, inf | 0x8000, nan
    m[7:] = np.where(rng.integers(0, 8, (M - 7, N)) == 0, rng.choice(np.array([inf, inf | 0x8000, nan, nan | 0x8001], np.uint16), (M - 7, N)), m[7:])
    mul = up(m).view(dtype_of(bf))
    g, _ = c.act(SILU)
    gm, _ = c.act(SILU_MUL, mul)
    torch.cuda.synchronize()
    got, want = bits(gm), bits(g * mul)
    nan_w = S.is_nan(want, bf)
    assert nan_w.any() and np.array_equal(S.is_nan(got, bf), nan_w)
    isinf = (want & 0x7FFF) == inf
    assert isinf.any() and np.array_equal((got & 0x7FFF) == inf, isinf) and np.array_equal(got[isinf], want[isinf])
    rest = ~nan_w & ~isinf
    assert np.array_equal(got[rest], want[rest])


# -------------------------------------------------------------------------------------------- 4. every family gives the same bits ----
GROUPS = {}
for _n, _k, _m, _knob in SPLIT_CASES:
    GROUPS.setdefault((_n, _k, _m), []).append(_knob)
GROUP_LIST = [(shape, tuple([1, 2] + knobs)) for shape, knobs in GROUPS.items()]


@pytest.mark.parametrize("bf", [True, False], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape,knobs", GROUP_LIST, ids=[f"{n}x{k}-M{m}" for (n, k, m), _ in GROUP_LIST])
def test_every_forced_family_gives_the_automatic_plans_bits(lib, shape, knobs, bf):
    """Knob 1: the two-barrier tiles; 2: the 256 x 256 kernel; the rest: the forced split factors and builds of SPLIT_CASES."""
    N, K, M = shape
    h = host_operands(N, K, M, 5, bf)
    c = Call(lib, h, M, N, K, bf)
    mul = up(special_mul(M, N, bf, 6)).view(dtype_of(bf))
    auto, k_auto = c.act(SILU)
    auto_mul, _ = c.act(SILU_MUL, mul)
    torch.cuda.synchronize()
    a, am = bits(auto), bits(auto_mul)
    assert not S.is_nan(a, bf).any()
    names = {k_auto}
    for knob in knobs:
        lib.mixq_debug_set_gemm_variant(knob)
        try:
            g, name = c.act(SILU)
            gm, _ = c.act(SILU_MUL, mul)
            torch.cuda.synchronize()
        finally:
            lib.mixq_debug_reset()
        names.add(name)
        assert np.array_equal(bits(g), a), f"knob {knob} ({name}): SiLU differs from the automatic plan ({k_auto}) in {int((bits(g) != a).sum())} outputs"
        assert np.array_equal(bits(gm), am), f"knob {knob} ({name}): SiLU x up differs from the automatic plan ({k_auto})"
    assert len(names) >= 2, names


def test_epilogue_0_is_the_typed_entry(lib):
    for bf in (True, False):
        for N, K, M, layout in ((1040, 1088, 129, 0), (4608, 3584, 17, 1)):
            c = Call(lib, host_operands(N, K, M, 3, bf), M, N, K, bf, layout)
            (a, ka), (b, kb) = c.act(PLAIN), c.typed()
            torch.cuda.synchronize()
            assert ka == kb and np.array_equal(bits(a), bits(b))


# --------------------------------------------------------------------------------------------------------- 5. buffer contract ----
@pytest.mark.parametrize("bf", [True, False], ids=["bf16", "fp16"])
@pytest.mark.parametrize("M,N,K", [(257, 272, 1088), (1000, 1040, 1088), (17, 272, 2048)])
def test_buffers_are_used_at_exactly_their_declared_sizes(lib, M, N, K, bf):
    """Out, mul, fpA, sA and qA at exactly their declared sizes and minimum alignment (16 bytes; sA 2), M and N no tile multiples."""
    rng = np.random.default_rng(M + N)
    q = rng.integers(-127, 128, (M, K)).astype(np.int8)
    sA = S.rn(rng.uniform(0.005, 0.02, M).astype(np.float32), bf)
    fpA = S.rn(rng.integers(-16, 17, (M, O)).astype(np.float32) * 4, bf)
    W = rng.integers(-127, 128, (N, K)).astype(np.int8)
    sW = rng.uniform(0.0005, 0.002, N).astype(np.float16)
    fpW = S.rn(rng.integers(-8, 9, (N, O)).astype(np.float32) * 2.0 ** -6, bf)
    mul = special_mul(M, N, bf, 1)
    nanfill = guarded.BF16_NAN if bf else guarded.F16_NAN
    G = guarded.Guarded
    g_q = G(M * K, guarded.I8_MAX, init=q, guard=guarded.IN_GUARD, offset=16)
    g_sA = G(2 * M, nanfill, init=sA, guard=guarded.IN_GUARD, offset=2)
    g_fpA = G(2 * M * O, nanfill, init=fpA, guard=guarded.IN_GUARD, offset=16)
    g_mul = G(2 * M * N, nanfill, init=mul, guard=guarded.IN_GUARD, offset=16)
    g_out = G(2 * M * N, nanfill, guard=guarded.out_guard(N, 2), offset=16)
    dW, dsW, dfpW = up(W), up(sW), up(fpW)
    n = int(lib.mixq_gemm_scratch_size(M, N, K))
    scratch = G(n, 0xA5, init=np.zeros(n, np.uint8), guard=guarded.SCRATCH_GUARD) if n else None   # (zero arrival words, patterned guards)
    v = S.pre_activation(q, sA, fpA, W, sW, fpW, bf)
    want = S.silu_bits(v, bf)
    for epi in (SILU, SILU_MUL):
        g_out.set_body(None)
        rc = lib.mixq_gemm_mixed_act_typed(g_q.ptr, dW.data_ptr(), g_sA.ptr, dsW.data_ptr(), g_fpA.ptr, dfpW.data_ptr(),
                                           g_mul.ptr if epi == SILU_MUL else None, g_out.ptr, M, N, K, O, epi, 0, type_of(bf),
                                           scratch.ptr if scratch else None, n, stream())
        torch.cuda.synchronize()
        assert rc == 0
        for g, name in ((g_out, "Out"), (g_mul, "mul"), (g_fpA, "fpA"), (g_sA, "sA"), (g_q, "qA")) + (((scratch, "scratch"),) if scratch else ()):
            guarded.assert_intact(g, f"{name} of {M}x{N}x{K} epilogue {epi}")
        got = g_out.body(np.uint16, (M, N))
        assert not S.is_nan(got, bf).any(), "unwritten outputs"
        if epi == SILU:
            silu = got
            assert S.ulp_steps(got, want).max() <= 1 and (got != want).mean() < 1e-3
        else:
            assert np.array_equal(got, S.mul_bits(silu, mul, bf))
    assert np.array_equal(g_q.body(np.int8, (M, K)), q) and np.array_equal(g_mul.body(np.uint16, (M, N)), mul)


# --------------------------------------------------------------------------------------------------------------- 6. bf16 range ----
@pytest.mark.parametrize("N,K,M", [(1040, 1088, 67), (4608, 3584, 320)])
def test_bf16_range_beyond_an_fp16_detour(lib, N, K, M):
    """Rows whose v is about +-1e20 and +-3e38 (through the row scale): finite results or signed zeros, as the restatement says."""
    h = host_operands(N, K, M, 9, True)
    h["fpA"] = np.zeros_like(h["fpA"])                       # v = acc sW sA alone, so its magnitude is the row scale's choice
    acc = h["q"].astype(np.float64) @ h["W"].astype(np.float64).T
    unit = np.abs(acc * h["sW"].astype(np.float64)[None, :]).max(axis=1)      # max |v| of a row per unit of sA
    sA = S.tof(h["sA"], True).astype(np.float64)
    for rows, target in ((slice(0, 16), 1e20), (slice(16, 32), 3e38)):
        sA[rows] = target / unit[rows]
    h["sA"] = S.rn(sA.astype(np.float32), True)
    v = S.pre_activation(h["q"], h["sA"], h["fpA"], h["W"], h["sW"], h["fpW"], True)
    assert np.isfinite(v).all() and np.abs(v[:16]).max() > 5e19 and np.abs(v[16:32]).max() > 1e38 and (v[:32] < -1e10).any() and (v[:32] > 1e10).any()
    want = S.silu_bits(v, True)
    c = Call(lib, h, M, N, K, True)
    g, _ = c.act(SILU)
    torch.cuda.synchronize()
    got = bits(g)
    big = np.abs(v) > 1e4                                       # far beyond fp16, where SiLU is v or -0 exactly
    assert np.array_equal(got[big], want[big])
    assert (got[big & (v < 0)] == 0x8000).all() and np.isfinite(S.tof(got, True)).all()
    assert (np.abs(S.tof(got[:32], True)) > 65504).any()
    assert S.ulp_steps(got, want).max() <= 1 and (got != want).mean() < 1e-3


# -------------------------------------------------------------------------------------------------------------------- 7. graph ----
def build_mlp(hidden, inter, bf, seed):
    from mixq_tensorrt_llm_amd import mixlinear, pack, plugin
    rng = np.random.default_rng(seed)
    dt = dtype_of(bf)
    act = np.abs(rng.standard_normal(hidden)).astype(np.float32)

    def packed(n, k, scales):
        Wt = torch.from_numpy((rng.standard_normal((n, k)) * 0.02).astype(np.float32)).to(dt)
        p = pack.pack_linear_weights(Wt, torch.from_numpy(scales), fp_dtype=dt) if bf else pack.pack_linear_weights(Wt, torch.from_numpy(scales))
        fpw = rng.integers(-8, 9, p["fp_weight"].shape).astype(np.float32) * 2.0 ** -6
        p["fp_weight"] = S.rn(fpw, True) if bf else fpw.astype(np.float16)
        return p

    gate, up_, down = (plugin.MixQLinear(k, n, dtype=dt, device="cuda:0").load(packed(n, k, s))
                       for n, k, s in ((inter, hidden, act), (inter, hidden, act), (hidden, inter, np.abs(rng.standard_normal(inter)).astype(np.float32))))
    mlp = plugin.MixQLlamaMLP(gate, up_, down)
    cache = mixlinear.MixLibCache(inputdim=256, device="cuda:0", dtype=dt)
    gamma = torch.from_numpy((1.0 + 0.1 * rng.standard_normal(hidden)).astype(np.float32)).to(dt).cuda()
    norm = mixlinear.FasterTransformerRMSNorm(gamma, 1e-5, cache, dtype=dt)
    norm.next_layer = gate
    return mlp, cache, norm


@pytest.mark.parametrize("bf", [True, False], ids=["bf16", "fp16"])
@pytest.mark.parametrize("M", [32, 256])
def test_llama_mlp_eager_by_hand_and_in_a_captured_graph(lib, M, bf):
    hidden, inter = 2048, 5632
    mlp, cache, norm = build_mlp(hidden, inter, bf, seed=M)
    gen = torch.Generator(device="cpu").manual_seed(M + int(bf))
    xs = [(2.0 * torch.randn((M, hidden), generator=gen)).to(dtype_of(bf)).cuda() for _ in range(2)]
    x = xs[0].clone()

    def step():
        norm.forward(x)
        return mlp.forward_quantised(cache.q_xcache, cache.x_scale, cache.activation_outliers, cache.q_layout)

    y_e = step().clone()
    torch.cuda.synchronize()
    assert cache.q_layout == lib.mixq_qa_layout(M, inter, hidden)
    if M == 32:
        assert cache.q_layout == 1, "32 x 5632 x 2048 is in the fragment-major image's domain"
    # the three calls of the class, issued by hand
    q, sc, outl, lay = cache.q_xcache, cache.x_scale, cache.activation_outliers, cache.q_layout
    u = mlp.up.forward_quantised(q, sc, outl, lay)
    g = mlp.gate.forward_quantised(q, sc, outl, lay, act="silu", mul=u)
    by_hand = mlp.down(g)
    # ... and the unfused sequence: gate, torch's silu is NOT used (another expf); SiLU in the epilogue, then torch's multiply
    g1 = mlp.gate.forward_quantised(q, sc, outl, lay, act="silu")
    torch.cuda.synchronize()
    assert y_e.dtype == dtype_of(bf) and tuple(y_e.shape) == (M, hidden) and torch.isfinite(y_e.float()).all()
    assert np.array_equal(bits(by_hand), bits(y_e)), "MixQLlamaMLP.forward_quantised differs from its three calls issued by hand"
    assert np.array_equal(bits(g), bits(g1 * u))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g = step()
    for i in (1, 0, 1):                                            # fresh producer outputs are written into the captured buffers
        x.copy_(xs[i])
        want = step().clone()
        torch.cuda.synchronize()
        y_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(y_g), bits(want)), f"replay {i} differs from the eager call"
