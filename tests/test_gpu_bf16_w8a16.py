"""GPU (-m gpu): the weight-only (W8A16) GEMM on bf16 rows, mixq_w8a16_gemm_forward_typed(.., MIXQ_TYPE_BF16), at every token count.

Contract (include/mixq.h): S = sum_k fp32(A[m,k]) * fp32(q[k,n] - 128) in fp32, Out = bf16_rn(fp32(scale[n]) * S).  Every form of the
operator -- narrow, wide configurations 1..6 with and without a K split over workgroups and with the weights through LDS or registers,
the skinny shapes, the two routes of 1..4 tokens -- is driven with the knobs the `form` fixture of test_gpu_w8a16_gemm.py documents
and must give the SAME bits on inputs whose fp32 sums are exact; random data stays within one bf16 rounding plus the fp32 accumulation
bound.  Inputs, expected bits and the call helper: tests/w8a16_bf16_cases.py."""
import numpy as np
import pytest

import bf16_restate as R
import guarded as G
import w8a16_bf16_cases as C

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BF16_TAG = " [bf16]"


@pytest.fixture(scope="module")
def lib():
    from mixq_tensorrt_llm_amd import _lib
    lib = _lib.load()
    lib.mixq_debug_reset()
    yield lib
    lib.mixq_debug_reset()


@pytest.fixture
def knob(lib):
    """mixq_debug_set_gemm_variant; every fpA_intB knob automatic again afterwards."""
    C.reset_forms(lib)
    lib.mixq_debug_set_gemm_variant(C.SKINNY_AUTO)
    lib.mixq_debug_set_gemm_variant(C.DECODE_AUTO)
    yield lib.mixq_debug_set_gemm_variant
    lib.mixq_debug_reset()


def forms_of(M, K):
    """(label, knobs, scratch, words the reported name must hold, words it must not hold) for every forced form of an M-row call."""
    out = [("automatic, scratch", (), True, (), ()), ("automatic, no scratch", (), False, (), ()),
           ("narrow", (C.NARROW,), True, ("narrow",), ()), ("narrow, no scratch", (C.NARROW,), False, ("narrow",), ())]
    for cfg in range(1, 7):
        for rw in ((C.RW_ON, C.RW_OFF) if cfg in C.WIDE_RW else (C.RW_AUTO,)):
            for ks in (1, 2, 4, 8):
                if not C.wide_split_allowed(cfg, K, ks):
                    continue
                has = [f"wide cfg{cfg}"] + (["K split"] if ks > 1 else []) + (["registers"] if rw == C.RW_ON else [])
                lacks = ([] if ks > 1 else ["K split"]) + ([] if rw == C.RW_ON else ["registers"])
                out.append((f"wide cfg{cfg} ks {ks} rw {rw}", (C.wide_knob(cfg), C.KS_KNOB[ks], rw), True, tuple(has), tuple(lacks)))
    if M <= 64:
        for v in C.SKINNY_SHAPES + (C.SKINNY_SHAPES_16 if M <= 16 else ()):
            out.append((f"skinny {v}", (v,), True, ("skinny",), ()))
    return out


def check_bits(got, want_dev, name, what):
    if not torch.equal(got, want_dev):
        bad = torch.nonzero(got != want_dev)
        m, n = (int(x) for x in bad[0])
        raise AssertionError(f"{what} ({name}): {bad.shape[0]} of {got.numel()} elements differ, first at ({m}, {n}): "
                             f"got 0x{int(got[m, n]) & 0xffff:04x}, expected 0x{int(want_dev[m, n]) & 0xffff:04x}")


# ---- 1. bit-exact on integer data, every form ------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", C.RAGGED)
def test_every_form_gives_the_exact_bits_on_integer_data(lib, knob, M, N, K):
    """A = integers in [-4, 4] times 2^100 / 2^-100 / 1 per row, any int8 q, fp16 scales that are no powers of two, K <= 4160: S is
    exact in fp32 in every order, so the output bits are fixed (w8a16_bf16_cases.integer_case) -- and finite on the 2^100 rows, which
    fp16 could not hold.  Each call also: a name that ends in " [bf16]" and names the forced form, equal bits on a repeat with the same
    scratch, hand-over words left zero (Device.call)."""
    A_bits, _, qi, sc, want = C.integer_case(M, N, K)
    d = C.Device(lib, torch, A_bits, qi, sc)
    want_dev = torch.from_numpy(want.view(np.int16)).to("cuda:0")
    for label, knobs, scratch, has, lacks in forms_of(M, K):
        C.reset_forms(lib)
        knob(C.SKINNY_AUTO)
        for v in knobs:
            knob(v)
        got, name = d.call(scratch=scratch)
        assert name.endswith(BF16_TAG), (label, name)
        assert all(w in name for w in has) and not any(w in name for w in lacks), (label, name)
        check_bits(got, want_dev, name, f"{M}x{N}x{K} {label}")


@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_one_to_four_tokens_on_both_decode_routes(lib, knob, M):
    """The first M rows of three ragged problems through the GEMV (skinny form never) and through the skinny form (always)."""
    for shape in [(7, 130, 192), (33, 258, 320), (64, 128, 4160)]:
        A_bits, _, qi, sc, want = C.integer_case(*shape)
        d = C.Device(lib, torch, A_bits, qi, sc)
        want_dev = torch.from_numpy(want[:M].view(np.int16)).to("cuda:0")
        for route, word in ((C.DECODE_GEMV, "GEMV"), (C.DECODE_SKINNY, "skinny")):
            knob(route)
            for scratch in (False, True):
                got, name = d.call(scratch=scratch, rows=M)
                assert name.endswith(BF16_TAG) and word in name, (shape, M, route, name)
                check_bits(got, want_dev, name, f"{M} of {shape} route {route}")


@pytest.mark.parametrize("rows,shape", [(17, (33, 258, 320)), (20, (33, 258, 320)), (32, (64, 128, 4160))])
def test_seventeen_to_thirty_two_tokens_on_every_skinny_shape(lib, knob, rows, shape):
    """The two-tile builds of the skinny form (no ragged shape above has 17..32 rows): the first rows of a larger problem."""
    A_bits, _, qi, sc, want = C.integer_case(*shape)
    d = C.Device(lib, torch, A_bits, qi, sc)
    want_dev = torch.from_numpy(want[:rows].view(np.int16)).to("cuda:0")
    for v in C.SKINNY_SHAPES:
        knob(v)
        got, name = d.call(rows=rows)
        assert name.endswith(BF16_TAG) and "skinny" in name, name
        check_bits(got, want_dev, name, f"{rows} of {shape} skinny {v}")


# ---- 2. random data within the derived bound --------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,scratch", [s + (False,) for s in C.RAGGED] + [s + (True,) for s in C.RAGGED + C.SPLIT_K])
def test_random_data_within_one_rounding_plus_the_accumulation_bound(lib, knob, M, N, K, scratch):
    """|got - ref64| <= ulp_bf16(ref64) + K * 2^-23 * sum_k |a w s| on every element (automatic plan): one bf16 rounding step plus the
    fp32 accumulation bound with a factor of two -- the bound test_gpu_bf16_operator.py applies to the M <= 4 kernels."""
    A_bits, _, qi, sc, ref64, mag = C.random_case(M, N, K)
    d = C.Device(lib, torch, A_bits, qi, sc)
    got, name = d.call(scratch=scratch)
    assert name.endswith(BF16_TAG)
    if "wide" in name:     # (the two larger shapes are there for the K split over workgroups, wherever the plan takes one with scratch)
        assert ("K split" in name) == (scratch and d.size() > 0), (name, d.size())
    g = R.bf2f(got.cpu().numpy().view(np.uint16)).astype(np.float64)
    err, lim = np.abs(g - ref64), C.accumulation_bound(ref64, mag, K)
    worst = np.unravel_index(np.argmax(err - lim), err.shape)
    print(f"{M}x{N}x{K} scratch={scratch} {name}: max err/bound {np.max(err / lim):.3f}")
    assert np.isfinite(g).all() and (err <= lim).all(), f"{name}: {int((err > lim).sum())} elements over the bound, worst at {worst}: " \
                                                        f"err {err[worst]:.3e} bound {lim[worst]:.3e}"


# ---- 3. rows do not mix -----------------------------------------------------------------------------------------------------------
NAN_CASES = [("narrow", (C.NARROW,), (65, 384, 128), 32), ("wide cfg1 registers", (C.wide_knob(1), C.RW_ON), (65, 384, 128), 31),
             ("wide cfg2", (C.wide_knob(2), C.RW_OFF), (129, 640, 1088), 64), ("wide cfg3 split", (C.wide_knob(3), C.KS_KNOB[2]), (129, 640, 1088), 128),
             ("wide cfg4", (C.wide_knob(4),), (257, 256, 256), 256), ("wide cfg5 K halves", (C.wide_knob(5), C.RW_ON), (129, 640, 1088), 63),
             ("wide cfg6 K halves split", (C.wide_knob(6), C.KS_KNOB[2]), (300, 1026, 1600), 127), ("skinny 32x8", (852,), (33, 258, 320), 16),
             ("skinny 64x16", (855,), (64, 128, 4160), 47), ("automatic", (), (700, 136, 448), 511)]


@pytest.mark.parametrize("label,knobs,shape,r", NAN_CASES, ids=[c[0] for c in NAN_CASES])
def test_a_nan_stays_in_its_row(lib, knob, label, knobs, shape, r):
    """One NaN in row r of A (r next to a tile boundary of the form): row r of the output is all NaN, every other row has the bits of
    the call without it."""
    A_bits, _, qi, sc, _ = C.integer_case(*shape)
    d = C.Device(lib, torch, A_bits, qi, sc)
    for v in knobs:
        knob(v)
    clean, name = d.call()
    poisoned = A_bits.copy()
    poisoned[r, (7 * r) % shape[2]] = 0x7fc0
    got, name2 = d.call(a=R.from_bits(poisoned, "cuda:0"))
    assert name2 == name and name.endswith(BF16_TAG)
    g, c = got.cpu().numpy().view(np.uint16), clean.cpu().numpy().view(np.uint16)
    assert ((g[r] & 0x7fff) > 0x7f80).all(), f"{name}: row {r} is not all NaN"
    rest = np.arange(shape[0]) != r
    assert np.array_equal(g[rest], c[rest]), f"{name}: rows {np.unique(np.nonzero(g[rest] != c[rest])[0])[:8]} (numbered without row {r}) changed"


# ---- 4. guarded buffers -----------------------------------------------------------------------------------------------------------
BIG, MID = (300, 1026, 1600), (129, 640, 1088)     # n % 4 == 2 (output at ptr % 8 == 4) and n % 4 == 0 (ptr % 16 == 8)
GUARD_CASES = [("narrow", (C.NARROW,), BIG), ("narrow", (C.NARROW,), MID), ("automatic", (), BIG), ("automatic", (), MID)]
for _cfg in range(1, 7):
    for _ks in (1, 2):
        GUARD_CASES.append((f"wide cfg{_cfg} ks {_ks}", (C.wide_knob(_cfg), C.KS_KNOB[_ks]), BIG if (_cfg + _ks) % 2 else MID))
for _cfg in C.WIDE_RW:
    GUARD_CASES.append((f"wide cfg{_cfg} LDS weights ks 2", (C.wide_knob(_cfg), C.KS_KNOB[2], C.RW_OFF), MID if _cfg % 2 else BIG))
GUARD_CASES += [(f"skinny {v}", (v,), (33, 258, 320)) for v in C.SKINNY_SHAPES] + [(f"skinny {v}", (v,), (64, 128, 4160)) for v in (852, 854)]
GUARD_CASES += [(f"skinny {v}", (v,), (7, 130, 192)) for v in C.SKINNY_SHAPES_16]


@pytest.mark.parametrize("label,knobs,shape", GUARD_CASES, ids=[f"{c[0]} {c[2][0]}x{c[2][1]}x{c[2][2]}" for c in GUARD_CASES])
def test_exact_size_buffers_at_the_minimum_alignment(lib, knob, label, knobs, shape):
    """Output of exactly M N bf16 filled with NaN at the least alignment the entry accepts, exact-size inputs, a workspace of exactly
    mixq_w8a16_gemm_workspace_size_typed bytes: guards intact, no NaN left in the body, the bits of the same call on ordinary buffers."""
    import ctypes
    M, N, K = shape
    A_bits, _, qi, sc, want = C.integer_case(M, N, K)
    d = C.Device(lib, torch, A_bits, qi, sc)
    for v in knobs:
        knob(v)
    plain, name = d.call()
    nws = d.size()
    out = G.Guarded(M * N * 2, G.BF16_NAN, guard=G.out_guard(N, 2), offset=8 if N % 4 == 0 else 4)
    a = G.Guarded(M * K * 2, 0x5A, init=A_bits, guard=G.IN_GUARD, offset=16)
    w = G.Guarded(K * N, 0x5A, init=qi, guard=G.IN_GUARD, offset=16)
    s = G.Guarded(N * 2, G.F16_NAN, init=sc, guard=G.IN_GUARD, offset=2)
    ws = G.Guarded(nws, 0xA5, init=np.zeros(nws, np.uint8), guard=G.SCRATCH_GUARD, offset=16) if nws else None
    assert out.ptr % 256 == (8 if N % 4 == 0 else 4) and a.ptr % 256 == 16 and w.ptr % 256 == 16 and s.ptr % 256 == 2
    rc = lib.mixq_w8a16_gemm_forward_typed(a.ptr, w.ptr, s.ptr, out.ptr, M, N, K, C.BF16, ws.ptr if ws else None, nws,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and lib.mixq_debug_last_gemm_kernel().decode() == name
    for g, what in ((out, "output"), (a, "input"), (w, "weight"), (s, "scale")) + (((ws, "workspace"),) if ws else ()):
        G.assert_intact(g, f"{name}: {what}")
    got = out.body(np.uint16, (M, N))
    assert not ((got & 0x7fff) > 0x7f80).any(), f"{name}: NaN left in the output"
    assert np.array_equal(got, plain.cpu().numpy().view(np.uint16)) and np.array_equal(got, want), name
    if ws:
        assert not ws.body(np.uint8)[:16384].any(), f"{name}: hand-over words not re-armed"


def test_a_misaligned_workspace_is_ignored(lib, knob):
    """A workspace that is not 16-byte aligned is dropped: the call succeeds and reports the form of the call without scratch."""
    import ctypes
    M, N, K = 129, 640, 1088
    A_bits, _, qi, sc, want = C.integer_case(M, N, K)
    d = C.Device(lib, torch, A_bits, qi, sc)
    _, with_ws = d.call(scratch=True)
    _, without = d.call(scratch=False)
    assert "K split" in with_ws and "K split" not in without
    nws = d.size()
    ws = G.Guarded(nws, 0xA5, init=np.zeros(nws, np.uint8), guard=G.SCRATCH_GUARD, offset=8)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda:0")
    assert lib.mixq_w8a16_gemm_forward_typed(d.a.data_ptr(), d.w.data_ptr(), d.s.data_ptr(), out.data_ptr(), M, N, K, C.BF16, ws.ptr, nws,
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    assert lib.mixq_debug_last_gemm_kernel().decode() == without
    assert np.array_equal(R.to_bits(out), want) and not ws.body(np.uint8).any()
    G.assert_intact(ws, "ignored workspace")


# ---- 5. the decode routes agree with what ships ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(512, 4096), (12288, 4096), (4096, 4096)])
def test_decode_routes_are_the_fp16_calls_and_the_bits_of_a_bf16_enqueue(lib, knob, N, K):
    """M = 1..4: the typed bf16 call takes the GEMV or the skinny form exactly where the fp16 call of the shape does (w8a16_skinny_takes
    decides both), and its bits are those of the route that ships -- a bias-free bf16 mixq_enqueue of the same qweight and scales."""
    from mixq_tensorrt_llm_amd import plugin
    rng = np.random.default_rng(N + K)
    qi = rng.integers(0, 256, size=(K, N), dtype=np.uint8)        # any bytes are an interleaved image of some q
    sc = C.odd_scales(rng, N)
    A_bits = R.bf16_rn(rng.standard_normal((4, K)).astype(np.float32))
    d = C.Device(lib, torch, A_bits, qi, sc)
    dev = d.a.device
    half = lambda t, shape: t.view(torch.float16).reshape(shape)
    seen = set()
    for M in (1, 2, 3, 4):
        got, name = d.call(scratch=False, rows=M)
        _, fp16_name = d.call(scratch=False, rows=M, typ=C.HALF, a=d.a.view(torch.float16))
        assert name == fp16_name + BF16_TAG, (M, name, fp16_name)
        seen.add("skinny" if "skinny" in name else "GEMV")
        ins = [d.a[:M].contiguous(), half(torch.zeros((N, K), dtype=torch.int8, device=dev), (N, K // 2)), d.s,
               torch.zeros((N, 128), dtype=torch.bfloat16, device=dev), half(torch.zeros(128, dtype=torch.int32, device=dev), (256,)),
               half(d.w, (K, N // 2)), d.s]
        ref = plugin.MixQPlugin.create(M, N, K).enqueue(ins)
        assert torch.equal(got, ref.view(torch.int16)), f"{M}x{N}x{K} ({name}) differs from the bf16 enqueue's decode route"
    assert seen == ({"GEMV"} if N == 512 else {"skinny"} if N == 12288 else {"GEMV", "skinny"}), (N, K, seen)


# ---- 6. Python ------------------------------------------------------------------------------------------------------------------------
def test_mixlib_and_eetq_return_the_c_entrys_bits(lib, knob):
    import EETQ
    from mixq_tensorrt_llm_amd import mixlib
    for shape in [(7, 130, 192), (129, 640, 1088), (300, 1026, 1600)]:
        A_bits, _, qi, sc, want = C.integer_case(*shape)
        d = C.Device(lib, torch, A_bits, qi, sc)
        got_c, _ = d.call()
        for op in (mixlib.w8_a16_gemm, EETQ.w8_a16_gemm):
            out = op(d.a, d.w, d.s)
            assert out.dtype == torch.bfloat16 and tuple(out.shape) == shape[:2]
            assert torch.equal(out.view(torch.int16), got_c) and np.array_equal(R.to_bits(out), want), (shape, op.__module__)
        with pytest.raises(TypeError, match="scale"):
            mixlib.w8_a16_gemm(d.a, d.w, d.s.to(torch.bfloat16))
        assert mixlib.w8_a16_gemm(d.a.view(torch.float16), d.w, d.s).dtype == torch.float16      # the fp16 call keeps its path


def test_the_boundary_between_four_and_five_tokens(lib, knob):
    from mixq_tensorrt_llm_amd import mixlib
    A_bits, _, qi, sc, want = C.integer_case(33, 258, 320)
    d = C.Device(lib, torch, A_bits, qi, sc)
    o4 = mixlib.w8_a16_gemm(d.a[:4].contiguous(), d.w, d.s)
    n4 = lib.mixq_debug_last_gemm_kernel().decode()
    o5 = mixlib.w8_a16_gemm(d.a[:5].contiguous(), d.w, d.s)
    n5 = lib.mixq_debug_last_gemm_kernel().decode()
    assert n4.startswith("w8a16 GEMV") and "skinny" in n5 and n4.endswith(BF16_TAG) and n5.endswith(BF16_TAG), (n4, n5)
    assert np.array_equal(R.to_bits(o4), want[:4]) and np.array_equal(R.to_bits(o5), want[:5])


@pytest.mark.parametrize("M,N,K", [(20, 640, 1088), (300, 1032, 1600)])
def test_a_bf16_call_is_capturable_in_a_hip_graph(lib, knob, M, N, K):
    """One linear graph (no parallel branches): the replay is bit-equal to the eager call."""
    from mixq_tensorrt_llm_amd import mixlib
    A_bits, _, qi, sc, want = C.integer_case(M, N, K)
    d = C.Device(lib, torch, A_bits, qi, sc)
    eager = mixlib.w8_a16_gemm(d.a, d.w, d.s)          # (also sizes the per-stream scratch before the capture)
    torch.cuda.synchronize()
    static_a = d.a.clone()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mixlib.w8_a16_gemm(static_a, d.w, d.s)         # warm-up on the capture stream: its scratch exists before the capture
        torch.cuda.current_stream().synchronize()
        with torch.cuda.graph(g, stream=side):
            out = mixlib.w8_a16_gemm(static_a, d.w, d.s)
    torch.cuda.current_stream().wait_stream(side)
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), eager.view(torch.int16)) and np.array_equal(R.to_bits(out), want)
