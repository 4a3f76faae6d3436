"""GPU (-m gpu): every fp16 mixlib op against the NAMED fp16 entry of the C ABI, called directly on clones of the same inputs.

The named entries (``mixq_int8quant``, ``mixq_rmsnorm``, ``mixq_int8_fused_dequantize``, ``mixq_mixlinear_forward`` ...) are the typed
entries with fewer operands (csrc/mixq_api.hip), so a wrapper may reach either.  This module pins what the wrappers pass: each op must
leave exactly the bits of the direct call in every output and side effect -- the int8 rows (or image), the row scales, the outliers,
``_out``, h, the zeroed columns of ``x``, D -- and launch the same kernel form (``mixq_debug_last_producer_kernel`` /
``mixq_debug_last_gemm_kernel``: the same form is the same speed).  ``MixQPlugin.enqueue`` is compared with ``mixq_enqueue`` /
``mixq_enqueue_bias`` in the same way.  Three refusals that sit behind ``mixlib._dev``, and so need device tensors, close the module."""
import ctypes

import pytest

from conftest import make_layer

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mixq_tensorrt_llm_amd import _lib, mixlib, mixlinear, plugin  # noqa: E402

F16 = torch.float16
ROW, FRAG = mixlib.QA_ROW_MAJOR, mixlib.QA_FRAGMENT_MAJOR
EPS = 1e-5
PRODUCER_SHAPES = [(M, K) for M in (1, 5, 67) for K in (8, 264, 2048)]
GEMM_SHAPES = [(1, 16, 16), (5, 64, 272), (67, 48, 272), (16, 1024, 2048)]
GEMM_CASES = [(s, ROW) for s in GEMM_SHAPES] + [((16, 1024, 2048), FRAG)]


def counts(K):
    return [n for n in (0, 8, 128) if n <= K]


def frag_ok(M, K):
    """The producers write the fragment-major image for decode batches with 1024 < K <= 16384 (csrc: quant_frag_layout_supported)."""
    return 0 < M <= 64 and K % 8 == 0 and 1024 < K <= 16384


PRODUCER_CASES = [(M, K, n, lay) for M, K in PRODUCER_SHAPES for n in counts(K) for lay in ((ROW, FRAG) if frag_ok(M, K) else (ROW,))]


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    lib.mixq_debug_reset()
    yield lib
    lib.mixq_debug_reset()


def p(t):
    return None if t is None else t.data_ptr()


def st():
    return torch.cuda.current_stream().cuda_stream


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def rows(M, K, seed, ind=None):
    x = torch.randn((M, K), device="cuda", generator=gen(seed)).to(F16)
    if ind is not None and ind.numel():
        x[:, ind.long()] *= 20
    return x


def columns(K, n, seed):
    return torch.randperm(K, device="cuda", generator=gen(seed))[:n].sort().values.to(torch.int32)


def scales(M, fill=7.0):
    """Row scales with three spare rows: whatever a call leaves behind row M is compared too."""
    return torch.full((M + 3, 1), fill, dtype=F16, device="cuda")


def image_rows(q, M, K, layout):
    """The int8 rows a producer wrote, whichever image holds them (the padding of the fragment-major image is nobody's output)."""
    return mixlib.qa_to_row_major(q, M, K) if layout == FRAG else q


def producer(lib):
    return lib.mixq_debug_last_producer_kernel().decode()


def gemm_kernel(lib):
    return lib.mixq_debug_last_gemm_kernel().decode()


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), f"{what} differs from the direct call's"


# ------------------------------------------------------------------------------------------------ row quantiser ---
@pytest.mark.parametrize("M,K", PRODUCER_SHAPES)
def test_find_row_scale_is_mixq_int8quant(lib, M, K):
    x = rows(M, K, 1)
    x1, x2, s1, s2 = x.clone(), x.clone(), scales(M), scales(M)
    q1 = mixlib.FindRowScale(x1, s1, M, K, 8)
    k1 = producer(lib)
    q2 = torch.empty((M, K), dtype=torch.int8, device="cuda")
    _lib.check(lib.mixq_int8quant(M, K, p(x2), p(q2), p(s2), st()), "mixq_int8quant")
    assert producer(lib) == k1
    same(q1, q2, "q"), same(s1, s2, "scaleRow"), same(x1, x2, "x")


@pytest.mark.parametrize("M,K,n,layout", PRODUCER_CASES)
def test_fused_extract_is_mixq_quant_extract_layout(lib, M, K, n, layout):
    ind = columns(K, n, 2)
    x = rows(M, K, 3, ind)
    x1, x2, s1, s2 = x.clone(), x.clone(), scales(M), scales(M)
    q1, o1 = mixlib.FindRowScaleFusedExtracOutliers(x1, s1, ind, n, M, K, layout)
    k1 = producer(lib)
    q2 = torch.empty_like(q1)
    o2 = torch.empty((M, n), dtype=F16, device="cuda")
    _lib.check(lib.mixq_quant_extract_layout(M, K, p(x2), p(q2), p(s2), p(o2), p(ind) if n else None, n, 1, layout, st()), "mixq_quant_extract_layout")
    assert producer(lib) == k1
    same(image_rows(q1, M, K, layout), image_rows(q2, M, K, layout), "q"), same(o1, o2, "outliers"), same(s1, s2, "scaleRow"), same(x1, x2, "x")
    if n:
        assert not x1[:, ind.long()].any(), "the outlier columns of x are zeroed"


# ----------------------------------------------------------------------------------------------- norm producers ---
@pytest.mark.parametrize("add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("M,K", PRODUCER_SHAPES)
def test_norm_is_mixq_rmsnorm_or_mixq_add_rmsnorm(lib, M, K, add):
    x, r, g = rows(M, K, 4), rows(M, K, 5), rows(1, K, 6).reshape(K)
    out1, out2 = torch.empty_like(x), torch.empty_like(x)
    if not add:
        assert mixlib.layernorm_forward_cuda(x, g, out1, EPS) is None
        k1 = producer(lib)
        _lib.check(lib.mixq_rmsnorm(M, K, p(x), p(g), p(out2), ctypes.c_float(EPS), st()), "mixq_rmsnorm")
        assert producer(lib) == k1
        return same(out1, out2, "_out")
    for separate in (False, True):   # h in place into _residual, or into h_out
        r1, r2 = r.clone(), r.clone()
        h1 = torch.empty_like(x) if separate else None
        h = mixlib.add_layernorm_forward_cuda(x, r1, g, out1, EPS, h_out=h1)
        assert h is (h1 if separate else r1)
        k1 = producer(lib)
        h2 = torch.empty_like(x) if separate else r2
        _lib.check(lib.mixq_add_rmsnorm(M, K, p(x), p(r2), p(h2), p(g), p(out2), ctypes.c_float(EPS), st()), "mixq_add_rmsnorm")
        assert producer(lib) == k1
        same(out1, out2, "_out"), same(h, h2, "h"), same(r1, r2, "_residual")


@pytest.mark.parametrize("add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("M,K,n,layout", PRODUCER_CASES)
def test_quantising_norm_is_the_named_layout_entry(lib, M, K, n, layout, add):
    ind = columns(K, n, 7)
    x, r, g = rows(M, K, 8, ind), rows(M, K, 9), rows(1, K, 10).reshape(K)
    out1, out2, s1, s2, r1, r2 = torch.empty_like(x), torch.empty_like(x), scales(M), scales(M), r.clone(), r.clone()
    if add:
        o1, q1 = mixlib.add_layernorm_forward_cuda_extract_outliers(x, r1, g, out1, EPS, ind, s1, layout)
    else:
        o1, q1 = mixlib.layernorm_forward_cuda_extract_outliers(x, g, out1, EPS, ind, s1, layout)
    k1 = producer(lib)
    o2 = torch.zeros((M, n), dtype=F16, device="cuda")
    q2 = torch.empty_like(q1)
    if add:
        _lib.check(lib.mixq_add_rmsnorm_extract_quant_layout(M, K, p(x), p(r2), p(r2), p(g), p(out2), ctypes.c_float(EPS), p(ind), n, p(o2), p(q2),
                                                             p(s2), layout, st()), "mixq_add_rmsnorm_extract_quant_layout")
    else:
        _lib.check(lib.mixq_rmsnorm_extract_quant_layout(M, K, p(x), p(g), p(out2), ctypes.c_float(EPS), p(ind), n, p(o2), p(q2), p(s2), layout,
                                                         st()), "mixq_rmsnorm_extract_quant_layout")
    assert producer(lib) == k1
    same(image_rows(q1, M, K, layout), image_rows(q2, M, K, layout), "q"), same(o1, o2, "outliers"), same(s1, s2, "scaleRow")
    same(out1, out2, "_out"), same(r1, r2, "h")


# ----------------------------------------------------------------------------------- the fused dequantising GEMMs ---
def quantised(M, K, layout, seed, n=0):
    """(q, x_scale, outliers, ind) as a producer leaves them for a consumer of ``layout``."""
    ind = columns(K, n, seed)
    xs = scales(M)
    q, outl = mixlib.FindRowScaleFusedExtracOutliers(rows(M, K, seed + 1, ind), xs, ind, n, M, K, layout)
    return q, xs, outl, ind


def weight(N, K, seed):
    qw = torch.randint(-127, 128, (N, K), device="cuda", generator=gen(seed), dtype=torch.int32).to(torch.int8)
    sc = (torch.rand((1, N), device="cuda", generator=gen(seed + 1)) * 1e-3 + 1e-4).to(F16)
    return qw, sc


def test_the_decode_shape_is_in_the_fragment_major_domain():
    assert mixlib.qa_layout(16, 1024, 2048) == FRAG


_NAMED = {0: "mixq_int8_fused_dequantize", 1: "mixq_int8_fused_dequantize_silu", 3: "mixq_int8_fused_dequantize_silu_mul"}


@pytest.mark.parametrize("addend", [False, True], ids=["y=None", "y"])
@pytest.mark.parametrize("epi", [0, 1, 3])
@pytest.mark.parametrize("shape,layout", GEMM_CASES)
def test_fused_dequantize_ops_are_the_named_entries(lib, shape, layout, epi, addend):
    M, N, K = shape
    assert layout == ROW or mixlib.qa_layout(M, N, K) == FRAG
    q, xs, _, _ = quantised(M, K, layout, 11)
    qw, sc = weight(N, K, 13)
    y = rows(M, N, 15) if addend else None
    mul = rows(M, N, 16)
    if epi == 0:
        D1 = mixlib.int8FusedDequantize(q, qw, xs, sc, y, M, N, K, layout)
    elif epi == 1:
        D1 = mixlib.int8FusedDequantizeSilu(q, qw, xs, sc, y, M, N, K, layout)
    else:
        D1 = mixlib.int8FusedDequantizeSiluMul(q, qw, xs, sc, y, mul, M, N, K, layout)
    k1 = gemm_kernel(lib)
    D2 = torch.empty((M, N), dtype=F16, device="cuda")
    if layout == FRAG:   # (the image has had one entry for the three epilogues all along)
        rc = lib.mixq_int8_fused_dequantize_layout(p(q), p(qw), p(xs), p(sc), p(y), p(mul) if epi == 3 else None, p(D2), M, N, K, epi, layout, None, st())
    else:
        ws = p(mixlib.gemm_scratch(q, M, N, K))
        lead = (p(q), p(qw), p(xs), p(sc), p(y)) + ((p(mul),) if epi == 3 else ())
        rc = getattr(lib, _NAMED[epi])(*lead, p(D2), M, N, K, ws, st())
    _lib.check(rc, _NAMED[epi])
    assert gemm_kernel(lib) == k1
    same(D1, D2, "D")


MIXLINEAR_CASES = [(s, lay, O) for s, lay in GEMM_CASES for O in (0, 8, 12, 136) if O <= s[2] and (lay == ROW or O in (0, 8))]


@pytest.mark.parametrize("shape,layout,O", MIXLINEAR_CASES)
def test_mixlinear_forward_is_mixq_mixlinear_forward(lib, shape, layout, O):
    """O = 12 takes the two-step route (mixq_gemm_fp16 + mixq_int8_fused_dequantize), O = 136 the one above 128 columns."""
    M, N, K = shape
    ind = columns(K, O, 17)
    x = rows(M, K, 18, ind)
    qw, sc = weight(N, K, 19)
    wc = (torch.randn((N, O), device="cuda", generator=gen(21)) * 0.02).to(F16) if O else None
    x1, x2, s1, s2 = x.clone(), x.clone(), scales(M), scales(M)
    out1, q1, o1 = mixlib.mixlinear_forward(x1, ind, qw, sc, wc, s1, layout)
    k1 = (producer(lib), gemm_kernel(lib))
    out2 = torch.empty((M, N), dtype=F16, device="cuda")
    q2 = torch.empty_like(q1)
    o2 = torch.empty((M, O), dtype=F16, device="cuda")
    scr = None if layout else mixlib.gemm_scratch(x, M, N, K)
    _lib.check(lib.mixq_mixlinear_forward(M, N, K, O, p(x2), p(ind) if O else None, p(qw), p(sc), p(wc) if O else None, p(s2), p(q2),
                                          p(o2) if O else None, p(out2), layout, p(scr), scr.numel() if scr is not None else 0, st()),
               "mixq_mixlinear_forward")
    assert (producer(lib), gemm_kernel(lib)) == k1
    same(out1, out2, "out"), same(image_rows(q1, M, K, layout), image_rows(q2, M, K, layout), "q_x"), same(o1, o2, "outliers")
    same(s1, s2, "x_scale"), same(x1, x2, "x")


@pytest.mark.parametrize("variant", ["plain", "bias", "silu", "silu_mul"])
@pytest.mark.parametrize("O", [0, 8])
@pytest.mark.parametrize("shape,layout", GEMM_CASES)
def test_gemm_mixed_passes_what_the_typed_entries_take(lib, shape, layout, O, variant):
    M, N, K = shape
    q, xs, outl, _ = quantised(M, K, layout, 23, O)
    qw, sc = weight(N, K, 25)
    sW = sc.reshape(N)
    fpw = (torch.randn((N, O), device="cuda", generator=gen(27)) * 0.02).to(F16) if O else None
    bias = rows(1, N, 28).reshape(N) if variant == "bias" else None
    mul = rows(M, N, 29) if variant == "silu_mul" else None
    act = "silu" if variant.startswith("silu") else None
    D1 = mixlib.gemm_mixed(q, qw, xs, sW, outl if O else None, fpw, M, N, K, bias=bias, qa_layout=layout, act=act, mul=mul)
    k1 = gemm_kernel(lib)
    D2 = torch.empty((M, N), dtype=F16, device="cuda")
    scr = None if layout else mixlib.gemm_scratch(q, M, N, K)
    lead = (p(q), p(qw), p(xs), p(sW), p(outl) if O else None, p(fpw) if O else None)
    tail = (p(scr), scr.numel() if scr is not None else 0, st())
    if act:
        rc = lib.mixq_gemm_mixed_act_typed(*lead, p(mul), p(D2), M, N, K, O, 1 if mul is None else 3, layout, _lib.MIXQ_TYPE_HALF, *tail)
    else:
        rc = lib.mixq_gemm_mixed_typed(*lead, p(bias), p(D2), M, N, K, O, layout, _lib.MIXQ_TYPE_HALF, *tail)
    _lib.check(rc, "mixq_gemm_mixed_typed")
    assert gemm_kernel(lib) == k1
    same(D1, D2, "out")


# -------------------------------------------------------------------------------------- mixlinear's own two ops ---
@pytest.mark.parametrize("M,K", PRODUCER_SHAPES)
def test_find_outliers_is_mixq_find_outliers(lib, M, K):
    x = rows(M, K, 31, columns(K, min(8, K), 32))
    got = mixlinear.find_outliers(x, 6.0)
    k1 = producer(lib)
    ws = torch.empty((lib.mixq_find_outliers_workspace_size(K) + 3) // 4, dtype=torch.int32, device="cuda")
    ind = torch.empty(K, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.mixq_find_outliers(p(x), M, K, ctypes.c_float(6.0), p(ws), p(ind), p(cnt), K, st()), "mixq_find_outliers")
    assert producer(lib) == k1
    assert got.numel() > 0, "the case has columns above sigma"
    same(got, ind[:int(cnt.item())], "ind")


@pytest.mark.parametrize("N,K,n", [(16, 16, 8), (48, 272, 12), (1024, 2048, 128)])
def test_dequant_weight_columns_is_the_named_entry(lib, N, K, n):
    qw, sc = weight(N, K, 33)
    ind = columns(K, n, 35)
    got = mixlinear.dequant_weight_columns(qw, sc, ind)
    want = torch.empty((N, n), dtype=F16, device="cuda")
    _lib.check(lib.mixq_dequant_weight_columns(p(qw), p(sc), p(ind), n, p(want), N, K, st()), "mixq_dequant_weight_columns")
    same(got, want, "weight columns")


# ------------------------------------------------------------------------------------------- MixQPlugin.enqueue ---
@pytest.fixture(scope="module")
def small_layer():
    """The smallest layer of tests/test_gpu_bias_epilogue.py (packing refuses K = 272: the interleaved qweight wants K % 64 == 0)."""
    from mixq_tensorrt_llm_amd import pack
    N, K = 256, 16384
    A, W, act = make_layer(64, N, K, seed=N + K)
    return A, plugin.MixQLinear(K, N, bias=True, device="cuda:0").load(pack.pack_linear_weights(torch.from_numpy(W), torch.from_numpy(act)))


@pytest.mark.parametrize("with_bias", [False, True], ids=["enqueue", "enqueue_bias"])
@pytest.mark.parametrize("M", [3, 64])   # the one-launch path up to four rows, and the quantiser + GEMM above
def test_plugin_enqueue_is_the_entry_of_its_case(lib, small_layer, M, with_bias):
    A, layer = small_layer
    N, K = layer.out_features, layer.in_features
    ins = [torch.from_numpy(A[:M]).cuda(), layer.weight, layer.weights_scaling_factor, layer.fp_weight, layer.fp_ind, layer.qweight,
           layer.weights_scaling_factor]
    bias = rows(1, N, 37).reshape(N) if with_bias else None
    plug = plugin.MixQPlugin.create(M, N, K)
    got = plug.enqueue(ins, bias=bias)
    k1 = (producer(lib), gemm_kernel(lib))
    in_desc = (_lib.TensorDesc * 7)(*[_lib.TensorDesc.make(t.shape) for t in ins])
    out_desc = _lib.TensorDesc.make((M, N))
    want = torch.empty((M, N), dtype=F16, device="cuda")
    ws = torch.empty(plug.workspace_size(M, N, K), dtype=torch.uint8, device="cuda")
    in_ptrs = (ctypes.c_void_p * 7)(*[t.data_ptr() for t in ins])
    out_ptrs = (ctypes.c_void_p * 1)(want.data_ptr())
    if with_bias:
        rc = lib.mixq_enqueue_bias(plug._h, in_desc, ctypes.byref(out_desc), in_ptrs, out_ptrs, p(bias), p(ws), st())
    else:
        rc = lib.mixq_enqueue(plug._h, in_desc, ctypes.byref(out_desc), in_ptrs, out_ptrs, p(ws), st())
    _lib.check(rc, "mixq_enqueue")
    assert (producer(lib), gemm_kernel(lib)) == k1
    same(got, want, "output")


# --------------------------------------------------------------------------------- refusals behind mixlib._dev ---
def test_a_short_scale_row_is_refused():
    with pytest.raises(AssertionError):
        mixlib.FindRowScale(rows(5, 264, 41), torch.zeros((4, 1), dtype=F16, device="cuda"), 5, 264, 8)


def test_extract_and_zero_takes_int32_indices():
    with pytest.raises(AssertionError):
        mixlib.ExtractOutliersAndSetToZeros(columns(264, 8, 42).long(), rows(5, 264, 43))


def test_unpack_int4_to_int8_takes_whole_16_byte_groups():
    with pytest.raises(AssertionError):
        mixlib.unpack_int4_to_int8(torch.zeros((3, 8), dtype=torch.uint8, device="cuda"))
