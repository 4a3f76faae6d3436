"""GPU (-m gpu): the fp16 P-flavour element by element -- ``mixq_gemm_fp16`` alone in guarded buffers, ``MixLinear_GEMM.forward`` through
every branch of its state machine, the gate path and ``MixLlamaMLP``, ``dequant_weight_columns`` and ``find_outliers`` at their edges.

The layers and activations come from tests/pflavour_exact.py: the outlier product is a sum of integers times one power of two, exact in
fp32 in any order (tests/test_pflavour_exact.py shows it from the oracle alone), so the outputs must equal the oracle BIT FOR BIT.
Where the data cannot be exact (random operands, the output of the norm) the bound is ``conftest.assert_elementwise`` with the side
product's order slack (``pflavour_exact.side_slack``), and SiLU outputs follow the rule of tests/test_gpu_silu_epilogue.py."""
import ctypes

import numpy as np
import pytest

import guarded
import pflavour_exact as X
from conftest import assert_elementwise, ulp16

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OK, HALF = 0, 1


@pytest.fixture(scope="module")
def lib():
    from mixq_tensorrt_llm_amd import _lib
    lib = _lib.load()
    lib.mixq_debug_reset()
    yield lib
    lib.mixq_debug_reset()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint16)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def assert_same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    if bad.size:
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} outputs differ from the oracle; first at {i}: got "
                             f"{g.view(np.float16)[i]!r} (0x{g[i]:04x}) want {w.view(np.float16)[i]!r} (0x{w[i]:04x})")


# ------------------------------------------------------------------------------------------------------ a. mixq_gemm_fp16 alone ----
def run_gemm_fp16(lib, fpA, fpW):
    """The entry in exact-size buffers: Out is 2 M N bytes at ptr % 16 == 8 (its 8-byte stores' minimum), NaN-filled, between out_guard;
    fpA / fpW at ptr % 16 == 0 for the vector path (O % 8 == 0) and at ptr % 16 == 2 for the element path."""
    (M, O), N = fpA.shape, fpW.shape[0]
    off = 0 if O % 8 == 0 else 2
    a = guarded.Guarded(2 * M * O, guarded.F16_NAN, init=fpA.copy(), guard=guarded.IN_GUARD, offset=off)
    w = guarded.Guarded(2 * N * O, guarded.F16_NAN, init=fpW.copy(), guard=guarded.IN_GUARD, offset=off)
    out = guarded.Guarded(2 * M * N, guarded.F16_NAN, guard=guarded.out_guard(N, 2), offset=8)
    assert out.ptr % 16 == 8 and a.ptr % 16 == off and w.ptr % 16 == off
    rc = lib.mixq_gemm_fp16(a.ptr, w.ptr, out.ptr, M, N, O, stream())
    torch.cuda.synchronize()
    what = f"mixq_gemm_fp16 {M}x{N}x{O}"
    assert rc == OK, f"{what}: rc {rc}"
    for g, name in ((out, "Out"), (a, "fpA"), (w, "fpW")):
        guarded.assert_intact(g, f"{what} {name}")
    assert np.array_equal(a.body(np.uint16), bits(fpA).reshape(-1)) and np.array_equal(w.body(np.uint16), bits(fpW).reshape(-1)), what + ": an input changed"
    got = out.body(np.uint16, (M, N))
    unwritten = (got & 0x7FFF) > 0x7C00
    assert not unwritten.any(), f"{what}: {int(unwritten.sum())} outputs unwritten (or NaN), first {tuple(np.argwhere(unwritten)[0])}"
    return got.view(np.float16)


@pytest.mark.parametrize("O", X.LATTICE_O)
@pytest.mark.parametrize("M,N", X.LATTICE_MN)
def test_gemm_fp16_lattice(lib, oracle, M, N, O):
    what = f"mixq_gemm_fp16 {M}x{N}x{O}"
    fpA, fpW, _ = X.exact_operands(M, N, O)
    got = run_gemm_fp16(lib, fpA, fpW)
    assert_same_bits(got, oracle.gemm_fp16(fpA, fpW), what + " exact operands")
    if O == 0:
        assert (bits(got) == 0).all(), what + ": an empty product is +0 everywhere"
        return
    rng = np.random.default_rng(M * N + O)                      # ordinary operands, as in test_fp16_side_gemm
    fa = (rng.standard_normal((M, O)) * 10).astype(np.float16)
    fw = (rng.standard_normal((N, O)) * 0.02).astype(np.float16)
    assert_elementwise(run_gemm_fp16(lib, fa, fw), oracle.gemm_fp16(fa, fw), X.side_slack(fa, fw), what + " random operands")


def test_gemm_fp16_lattice_covers_every_class():
    """Every O with two (M, N) or more; every (M, N) with each class of O (the vector path with a full and with a zero-fed upper
    half-wave, the element path, the empty product)."""
    classes = {"O % 16 == 0": lambda o: o > 0 and o % 16 == 0, "O % 16 == 8": lambda o: o % 16 == 8, "O % 8 != 0": lambda o: o % 8 != 0,
               "O == 0": lambda o: o == 0}
    assert len(X.LATTICE_MN) >= 2
    for name, f in classes.items():
        assert any(f(o) for o in X.LATTICE_O), name
    rows = {m % 32 for m, _ in X.LATTICE_MN}
    assert {0, 1, 31} <= rows and any(n % 32 == 4 for _, n in X.LATTICE_MN) and {0, 1, 7} <= set(X.LATTICE_O)


# --------------------------------------------------------------------------------------------- b. MixLinear_GEMM.forward, fp16 ----
def gpu_layer(L, stop, inputdim=304):
    from mixq_tensorrt_llm_amd import mixlinear
    cache = mixlinear.MixLibCache(inputdim=inputdim, sigma=X.SIGMA, device="cuda:0")
    cache.stop = stop
    layer = mixlinear.MixLinear_GEMM.from_linear(torch.from_numpy(L["W"]), None if L["bias"] is None else torch.from_numpy(L["bias"]),
                                                 cache=cache, dev="cuda:0")
    assert np.array_equal(layer.q_weight.cpu().numpy(), L["k"]), "from_linear: q_weight is not k"
    assert np.array_equal(bits(layer.scale_col).reshape(-1), bits(L["scale_col"])), "from_linear: scale_col is not 2^-e"
    return layer, cache


def follow_scenario(lib, oracle, name, N, K, M):
    """Every call of the scenario (pflavour_exact.scenario): the output bits, and after the call ind, weight_cache, the mutated x,
    add_outliers and cnt.  Returns the GEMM kernel name of every call."""
    kernels = []
    sc = X.scenario(name, N, K, M)
    recs = X.walk(oracle, sc)
    layer, cache = gpu_layer(sc["layer"], sc["stop"])
    for i, (x, r) in enumerate(zip(sc["calls"], recs)):
        what = f"{name} {M}x{N}x{K} call {i}"
        static = not layer.add_outliers
        xt = dev(x)
        got = layer.forward(xt, cache, True)
        kern = lib.mixq_debug_last_gemm_kernel().decode()
        torch.cuda.synchronize()
        kernels.append(kern)
        what += f" ({'static' if static else 'dynamic'} route, O = {r['ind'].size}, {kern})"
        assert tuple(got.shape) == x.shape[:-1] + (N,) and got.dtype == torch.float16, what
        assert np.array_equal(layer.ind.cpu().numpy(), r["ind"]), what + ": the outlier index set"
        assert layer.add_outliers == r["add_outliers"] and layer.cnt == r["cnt"], what + f": add_outliers / cnt {layer.add_outliers} {layer.cnt}"
        if r["ind"].size:
            assert_same_bits(layer.weight_cache, r["weight_cache"], what + " weight_cache")
            assert_same_bits(cache.activation_outliers, r["fpA"], what + " activation_outliers")
        else:
            assert layer.weight_cache is None
        assert np.array_equal(bits(xt).reshape(-1, K), bits(r["x_after"])), what + ": input mutation (zeroed outlier columns)"
        assert_same_bits(got.reshape(-1, N), r["want"], what)
    if name == "width":
        assert layer.ind.numel() == 258 and not layer.add_outliers and layer.cnt == 2, "frozen by width, not by cache.stop"
    if name == "threshold":
        print(f"threshold {M}x{N}x{K}: the oracle's sets after the calls {[r['ind'].tolist() for r in recs]}")
    return kernels


@pytest.mark.parametrize("M", X.LAYER_M)
@pytest.mark.parametrize("N,K", X.LAYER_SHAPES)
@pytest.mark.parametrize("name", X.SCENARIOS)
def test_forward_follows_the_oracle_bit_for_bit(lib, oracle, name, N, K, M):
    follow_scenario(lib, oracle, name, N, K, M)


# The selection rule by itself reaches two kernel names at these sizes (measured on an MI355X: gemm_skinny_kernel up to 17 rows -- M <= 4
# included -- and the two-barrier tiles from 70 rows on, at both shapes); the ping-pong kernels start at sizes beyond this file's limit.
# So the two ping-pong families are put under the same forwards with the measurement knobs 5 and 2.  Only forms that
# tests/test_gpu_buffer_contract.py already runs forced, at N = 272 in guarded buffers, are reached: the scenarios "width" and "odd3"
# take the dynamic route (mixq_int8_fused_dequantize with an addend) and the static route's two-step order (the addend aliasing the output).
FORCED_FAMILIES = [(5, "pp128_kernel"), (2, "pp_kernel (256x256")]


@pytest.mark.parametrize("M", [130, 300])
@pytest.mark.parametrize("N,K", X.LAYER_SHAPES)
@pytest.mark.parametrize("name", ["width", "odd3"])
@pytest.mark.parametrize("knob,expect", FORCED_FAMILIES, ids=["pp128", "pp256"])
def test_forward_on_the_ping_pong_kernels_bit_for_bit(lib, oracle, knob, expect, name, N, K, M):
    lib.mixq_debug_set_gemm_variant(knob)
    try:
        kernels = follow_scenario(lib, oracle, name, N, K, M)
    finally:
        lib.mixq_debug_reset()
    assert all(expect in k for k in kernels), kernels


def test_at_least_four_gemm_kernels_serve_these_shapes(lib):
    """Distinct names of mixq_debug_last_gemm_kernel under MixLinear_GEMM.forward at the shapes of this file: every M by the selection rule
    (two names, see above; M <= 4 runs the int8 kernels here, not the GEMV), and the two ping-pong families forced at 130 and 300 rows."""
    from mixq_tensorrt_llm_amd import mixlinear
    seen = {}
    for N, K in X.LAYER_SHAPES:
        cache = mixlinear.MixLibCache(inputdim=304, sigma=X.SIGMA, device="cuda:0")
        cache.stop = 100                                         # (the dynamic route at every M)
        layer = mixlinear.MixLinear_GEMM(K, N, False, "cuda:0", cache=cache)
        layer.q_weight.zero_()
        layer.scale_col.fill_(1.0)
        for knob, rows in [(None, X.LAYER_M)] + [(k, [130, 300]) for k, _ in FORCED_FAMILIES]:
            if knob is not None:
                lib.mixq_debug_set_gemm_variant(knob)
            try:
                for M in rows:
                    layer.forward(torch.zeros((M, K), dtype=torch.float16, device="cuda:0"), cache, True)
                    seen[(N, K, M, knob)] = lib.mixq_debug_last_gemm_kernel().decode()
            finally:
                if knob is not None:
                    lib.mixq_debug_reset()
    torch.cuda.synchronize()
    print("kernels by (N, K, M, knob):", seen)
    assert len({k for (_, _, _, knob), k in seen.items() if knob is None}) >= 2, seen
    assert len(set(seen.values())) >= 4, seen


# ----------------------------------------------------------------------------------------------------- c. gate path and the MLP ----
def test_mlp_block_element_by_element(lib, oracle):
    """The twin of test_gpu_mixlinear.test_fused_norm_and_llama_mlp_block with exact up and gate layers.  The norm's output is not exact,
    so up and the gate's pre-activation are held to assert_elementwise against the oracle evaluated on the GPU's normalised row; the
    gate's SiLU to the one-step rule; SiLU x up (fused, and unfused behind a bias) to torch's fp16 multiply bit for bit; down to
    assert_elementwise on the same input bits (its slack is derived where it is computed)."""
    from mixq_tensorrt_llm_amd import mixlib, mixlinear
    rng = np.random.default_rng(23)
    H, F, M = 512, 1024, 40
    Lu, Lg = X.layer8(F, H, 101), X.layer8(F, H, 102)
    Wd = (rng.standard_normal((H, F)) * 0.02).astype(np.float16)
    gate_bias = (rng.standard_normal(F) * 0.1).astype(np.float16)
    gamma = (0.05 * (1.0 + 0.1 * rng.standard_normal(H))).astype(np.float16)    # small rows: the exact layers' weights reach 2
    gamma[[17, 300]] = 1.0
    eps = 1e-6
    hidden = rng.standard_normal((M, H)).astype(np.float16)
    hidden[3, 17] = np.float16(60.0)        # survives the norm as |x| > sigma -> dynamic outlier column 17
    hidden[9, 300] = np.float16(-45.0)

    def build():
        cache = mixlinear.MixLibCache(inputdim=64, sigma=X.SIGMA, device="cuda:0")
        mk = lambda W, b=None: mixlinear.MixLinear_GEMM.from_linear(torch.from_numpy(W), b, cache=cache, dev="cuda:0")  # noqa: E731
        up, gate, down = mk(Lu["W"]), mk(Lg["W"]), mk(Wd)
        gate_b = mk(Lg["W"], torch.from_numpy(gate_bias))
        norm = mixlinear.FasterTransformerRMSNorm(dev(gamma), eps, cache)
        norm.next_layer = up
        return cache, norm, up, gate, gate_b, down

    cache, norm, up, gate, gate_b, down = build()
    assert np.array_equal(up.q_weight.cpu().numpy(), Lu["k"]) and np.array_equal(gate.q_weight.cpu().numpy(), Lg["k"])
    x = norm(dev(hidden))
    x_ref = x.cpu().numpy().copy()                                   # the GPU's normalised row, before up zeroes its new columns
    assert np.array_equal(cache.q_xcache.cpu().numpy(), oracle.quant_rows(x_ref)[0]), "fused norm -> int8 rows of its own output"

    # ---- the oracle on that row --------------------------------------------------------------------------------------------------
    new_ind = oracle.find_outliers(x_ref, X.SIGMA)
    assert new_ind.tolist() == [17, 300], new_ind.tolist()
    act_out = oracle.extract_outliers(x_ref, new_ind, set_zero=True)
    qx, xs = oracle.quant_rows(x_ref)
    want, slack = {}, {}
    for n, L in (("up", Lu), ("gate", Lg)):
        wc = oracle.dequant_weight_columns(L["k"], L["scale_col"], new_ind)
        acc = oracle.gemm_s8s8s32(qx, L["k"])
        P = oracle.gemm_fp16(act_out, wc)
        want[n] = oracle.dequant_epilogue(acc, xs, L["scale_col"], C=P)
        want[n + " silu"] = oracle.dequant_epilogue(acc, xs, L["scale_col"], C=P, silu=True)
        want[n + " wc"] = wc
        slack[n] = X.side_slack(act_out, wc)

    # ---- the GPU, step by step ---------------------------------------------------------------------------------------------------
    up_got = up(x, cache)
    assert np.array_equal(up.ind.cpu().numpy(), new_ind)
    assert np.array_equal(bits(x), bits(x_ref)), "the up projection zeroes its new columns in the normalised row"
    assert np.array_equal(cache.q_xcache.cpu().numpy(), qx) and np.array_equal(bits(cache.x_scale[:M]).reshape(-1), bits(xs))
    assert_same_bits(up.weight_cache, want["up wc"], "up weight_cache")
    assert_elementwise(up_got.cpu().numpy(), want["up"], slack["up"], "up")
    print(f"MLP magnitudes: |x| max {np.abs(x_ref.astype(np.float32)).max():.2f}, |up| median {np.median(np.abs(want['up'].astype(np.float32))):.3f} "
          f"max {np.abs(want['up'].astype(np.float32)).max():.2f}")

    silu_got = gate.forward_without_preconditionFusedSilu(x, cache)
    assert np.array_equal(gate.ind.cpu().numpy(), new_ind)
    assert_same_bits(gate.weight_cache, want["gate wc"], "gate weight_cache")
    y_gate = mixlinear.outlier_product(cache.activation_outliers, gate.weight_cache)
    gate_plain = mixlib.int8FusedDequantize(cache.q_xcache, gate.q_weight, cache.x_scale, gate.scale_col, y_gate, M, F, H)
    assert_elementwise(gate_plain.cpu().numpy(), want["gate"], slack["gate"], "gate before SiLU")
    X.assert_silu_rule(silu_got.cpu().numpy(), want["gate silu"], "gate SiLU (forward_without_preconditionFusedSilu)")

    # SiLU x up: fused into the epilogue without a bias, the unfused multiply behind one -- torch's fp16 ops on the same bits
    fused = gate.forward_without_preconditionFusedSilu(x, cache, mul=up_got)
    two_step = silu_got.clone()
    two_step *= up_got
    assert_same_bits(fused, two_step, "SiLU x up in the epilogue against SiLU then torch's fp16 multiply")
    biased = gate_b.forward_without_preconditionFusedSilu(x, cache, mul=up_got)
    assert_same_bits(gate_b.weight_cache, want["gate wc"], "the biased gate adopts the same columns")
    two_step_b = silu_got.clone()
    two_step_b += gate_b.bias
    two_step_b *= up_got
    assert_same_bits(biased, two_step_b, "SiLU + bias, then the unfused multiply")

    h = fused.cpu().numpy().copy()
    y_got = down(fused, None, True).cpu().numpy()
    st = oracle.MixLinearState(down.q_weight.cpu().numpy(), down.scale_col.cpu().numpy(), sigma=X.SIGMA)
    y_want = oracle.mixlinear_forward(st, h.copy())              # same input bits: isolates the down projection
    assert np.array_equal(down.ind.cpu().numpy(), st.ind)
    # down's slack (ordinary weights; its input reaches hundreds in the two rows that held the norm's outliers, so most columns turn
    # dynamic): the side product's accumulation slack, plus one fp16 step of the ROUNDED product P16 -- P is rounded to fp16 before it
    # enters the dequant FMA, and two summation orders of a wide set can land on neighbouring fp16 values of P (conftest.prefill_slack)
    d_slack = 0.0
    if st.ind.size:
        h_out = np.ascontiguousarray(h[:, st.ind])
        d_slack = X.side_slack(h_out, st.weight_cache) + ulp16(oracle.gemm_fp16(h_out, np.ascontiguousarray(st.weight_cache)))
    print(f"down: {st.ind.size} dynamic outlier columns, |h| max {np.abs(h.astype(np.float32)).max():.2f}")
    assert_elementwise(y_got, y_want, d_slack, "down")

    # ---- the packaged block gives the same bits ------------------------------------------------------------------------------------
    cache2, norm2, up2, gate2, _, down2 = build()
    y2 = mixlinear.MixLlamaMLP(gate2, down2, up2, cache2)(norm2(dev(hidden)))
    assert_same_bits(y2, y_got, "MixLlamaMLP against its steps")


# ------------------------------------------------------------------------------------------------------------- e. the small ops ----
@pytest.mark.parametrize("N", [1, 16, 1000])
def test_dequant_weight_columns_fp16_edges(lib, oracle, N):
    """fp16(int8 x scale) with one rounding, for 1 .. 264 columns (first and last included), a subnormal scale and one of 60000 (127 x
    60000 overflows to inf, as in the reference's fp16 product); Out is exactly 2 N len bytes between guards."""
    K = 4096
    rng = np.random.default_rng(N)
    W = rng.integers(-128, 128, (N, K), dtype=np.int8)
    W[0, 0], W[0, K - 1], W[N - 1, 0] = 127, -128, -1
    for extreme in (6e-8, 60000.0):
        s = (rng.random(N) * 1e-2 + 1e-4).astype(np.float16)
        s[0] = np.float16(extreme)
        if N > 2:
            s[1], s[2] = np.float16(6e-8), np.float16(60000.0)
        w_d, s_d = dev(W), dev(s.reshape(1, N))
        for n in (1, 7, 77, 264):
            ind = np.sort(rng.choice(np.arange(1, K - 1), n, replace=False)).astype(np.int32)
            ind[0] = 0
            if n > 1:
                ind[-1] = K - 1
            out = guarded.Guarded(2 * N * n, guarded.F16_NAN, guard=guarded.out_guard(n, 2))
            i_d = dev(ind)
            rc = lib.mixq_dequant_weight_columns_typed(w_d.data_ptr(), s_d.data_ptr(), i_d.data_ptr(), n, out.ptr, N, K, HALF, stream())
            torch.cuda.synchronize()
            what = f"dequant_weight_columns {N}x{K} len={n} scale[0]={extreme}"
            assert rc == OK, what
            guarded.assert_intact(out, what)
            with np.errstate(over="ignore"):
                want = oracle.dequant_weight_columns(W, s, ind)
            assert_same_bits(out.body(np.float16, (N, n)), want, what)


def test_find_outliers_across_the_chunk_hand_over(lib, oracle):
    """K = 32768 + 64: the compaction walks the mask in chunks of 1024 words (32768 columns).  Every column of the second chunk is hot and
    the first holds thousands, so the hand-over carries a large base; a capacity that ends inside the second chunk cuts the result
    there."""
    from mixq_tensorrt_llm_amd import mixlinear
    M, K = 5, 32768 + 64
    rng = np.random.default_rng(77)
    A = np.clip(rng.standard_normal((M, K)) * 0.8, -5.49, 5.49).astype(np.float16)
    first = np.arange(0, 32768, 3)
    A[rng.integers(0, M, first.size), first] = np.float16(9.5)
    A[rng.integers(0, M, 64), np.arange(32768, K)] = -X.ABOVE_SIGMA
    want = oracle.find_outliers(A, X.SIGMA)
    assert want.size == first.size + 64 and want[-64:].tolist() == list(range(32768, K))
    a_d = dev(A)
    got = mixlinear.find_outliers(a_d, X.SIGMA).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    for cap in (first.size + 20, first.size + 1, first.size, first.size + 63):
        assert np.array_equal(mixlinear.find_outliers(a_d, X.SIGMA, capacity=cap).cpu().numpy(), want[:cap]), cap
    assert np.array_equal(bits(a_d), bits(A)), "find_outliers reads only"
