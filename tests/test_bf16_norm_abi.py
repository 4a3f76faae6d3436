"""CPU: the typed entries of the norm producer and of the launcher-level GEMM (mixq_rmsnorm_typed, mixq_rmsnorm_extract_quant_typed,
mixq_gemm_mixed_typed) are exported, typed and declared, leave the ABI revision at 5, and refuse bad arguments with the codes of the
entries they mirror, in their order -- before anything is launched, so none of this needs a device (dummy integers stand in for
pointers, as in test_add_norm_abi).  Also: the Python wrappers' dtype rules on CPU tensors, and the restatement helper
(tests/bf16_norm_restate.py) against torch CPU bf16."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from mixq_tensorrt_llm_amd import _lib

OK, BADARG, SHAPE, ALIGN, E_TYPE = 0, 1, 2, 3, 7
HALF, BF16 = _lib.MIXQ_TYPE_HALF, _lib.MIXQ_TYPE_BF16
NAMES = ("mixq_rmsnorm_typed", "mixq_rmsnorm_extract_quant_typed", "mixq_gemm_mixed_typed")
EPS = ctypes.c_float(1e-5)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def P(v):
    return ctypes.c_void_p(v)


A = [0x10000 + 0x1000 * i for i in range(12)]     # distinct 16-byte aligned "pointers"
X, R, H, G, OUT, IND, OUTL, Q, SC, W, SW, BIAS = A


def plain(lib, M, K, typ, x=X, r=R, h=H, g=G, out=OUT):
    return lib.mixq_rmsnorm_typed(M, K, P(x), P(r), P(h), P(g), P(out), EPS, typ, None)


def quant8(lib, M, K, typ, x=X, r=R, h=H, g=G, out=OUT, q=Q, layout=0, n_out=8, ind=IND, outl=OUTL):
    return lib.mixq_rmsnorm_extract_quant_typed(M, K, P(x), P(r), P(h), P(g), P(out), EPS, P(ind), n_out, P(outl), P(q), P(SC), layout,
                                                typ, None)


def gemm(lib, typ, M=16, N=32, K=64, n_out=8, qa=Q, sa=SC, bias=0, layout=0, out=OUT):
    return lib.mixq_gemm_mixed_typed(P(qa), P(W), P(sa), P(SW), P(OUTL), P(G), P(bias), P(out), M, N, K, n_out, layout, typ, None, 0, None)


ENTRIES = [plain, quant8]
TYPES = [HALF, BF16]


def test_symbols_are_declared_exported_and_typed(lib):
    src = open(os.path.join(ROOT, "include", "mixq.h")).read()
    declared = set(re.findall(r"MIXQ_API\s+[\w\s\*]+?\b(\w+)\s*\(", src))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/mixq.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        fn = getattr(lib, name)
        restype, argtypes = _lib.SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    # the add forms' arguments with `type` in front of the stream
    sig = _lib.SIGNATURES
    for name, base in (("mixq_rmsnorm_typed", "mixq_add_rmsnorm"), ("mixq_rmsnorm_extract_quant_typed", "mixq_add_rmsnorm_extract_quant_layout")):
        b = list(sig[base][1])
        assert list(sig[name][1]) == b[:-1] + [ctypes.c_int] + b[-1:], name
    # mixq_gemm_mixed_bias's arguments with qa_layout and type behind O
    b = list(sig["mixq_gemm_mixed_bias"][1])
    assert list(sig["mixq_gemm_mixed_typed"][1]) == b[:12] + [ctypes.c_int, ctypes.c_int] + b[12:]


def test_abi_revision_is_still_5(lib):
    src = open(os.path.join(ROOT, "include", "mixq.h")).read()
    assert re.search(r"^#define MIXQ_ABI_VERSION 5$", src, re.M)
    assert lib.mixq_abi_version() == 5 and _lib.ABI_VERSION == 5


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda f: f.__name__)
def test_a_bad_type_is_refused_before_everything_else(lib, entry):
    for typ in (0, 2, 3, 6, 8, -1):
        assert entry(lib, 4, 64, typ) == E_TYPE
        assert entry(lib, -1, 0, typ, x=0, r=0, h=OUT) == E_TYPE      # (every other refusal at once)
        assert entry(lib, 0, 64, typ) == E_TYPE
        assert gemm(lib, typ) == E_TYPE
        assert gemm(lib, typ, M=-1, sa=0, layout=9) == E_TYPE


@pytest.mark.parametrize("typ", TYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("entry", ENTRIES, ids=lambda f: f.__name__)
def test_norm_refusals_without_a_device(lib, entry, typ):
    for add in (True, False):
        kw = {} if add else dict(r=0, h=0)
        # an empty problem is fine, whatever the pointers
        assert entry(lib, 0, 64, typ, **kw) == OK
        assert entry(lib, 0, 64, typ, x=0, r=0, h=0, out=0) == OK
        # null or negative arguments
        assert entry(lib, 4, 64, typ, **dict(kw, x=0)) == BADARG
        assert entry(lib, -1, 64, typ, **kw) == BADARG
        assert entry(lib, 4, 0, typ, **kw) == BADARG
        # rows of whole 16-byte vectors, up to 32768 elements
        assert entry(lib, 4, 12, typ, **kw) == SHAPE
        assert entry(lib, 4, 32776, typ, **kw) == SHAPE
        assert entry(lib, 4, 64, typ, **dict(kw, x=X + 8)) == ALIGN
        # BADARG before SHAPE before ALIGN
        assert entry(lib, 4, 12, typ, **dict(kw, x=0)) == BADARG
        assert entry(lib, 4, 12, typ, **dict(kw, x=X + 2)) == SHAPE
    # a residual without h, h without a residual
    assert entry(lib, 4, 64, typ, r=0) == BADARG
    assert entry(lib, 4, 64, typ, h=0) == BADARG
    # h may be x or residual, never the normalised row
    assert entry(lib, 4, 64, typ, h=OUT) == BADARG
    # x, residual and h are read and written 16 bytes at a time
    for kw in (dict(r=R + 2), dict(r=R + 8), dict(h=H + 2), dict(h=H + 8)):
        assert entry(lib, 4, 64, typ, **kw) == ALIGN
    assert entry(lib, 4, 12, typ, r=0) == BADARG
    assert entry(lib, 4, 12, typ, r=R + 2) == SHAPE


@pytest.mark.parametrize("typ", TYPES, ids=["fp16", "bf16"])
def test_quantising_entry_checks_outlier_arguments_q_and_layout(lib, typ):
    for kw in ({}, dict(r=0, h=0)):
        assert quant8(lib, 4, 64, typ, ind=0, **kw) == BADARG
        assert quant8(lib, 4, 64, typ, outl=0, **kw) == BADARG
        assert quant8(lib, 4, 64, typ, n_out=-1, **kw) == BADARG
        assert quant8(lib, 4, 64, typ, q=0, **kw) == BADARG
        # q: 8 bytes row-major, 16 bytes as a fragment-major image
        assert quant8(lib, 4, 64, typ, q=Q + 4, **kw) == ALIGN
        assert quant8(lib, 16, 2048, typ, q=Q + 8, layout=1, **kw) == ALIGN
        # the fragment-major image exists for 1..64 rows and 1024 < K <= 16384 only
        assert quant8(lib, 65, 4096, typ, layout=1, **kw) == SHAPE
        assert quant8(lib, 16, 1024, typ, layout=1, **kw) == SHAPE
        assert quant8(lib, 65, 1024, typ, layout=1, **kw) == SHAPE
        # there are two layouts
        assert quant8(lib, 16, 4096, typ, layout=7, **kw) == BADARG
        assert quant8(lib, 16, 4096, typ, layout=-1, **kw) == BADARG
        # BADARG before SHAPE before ALIGN
        assert quant8(lib, 65, 4096, typ, layout=1, q=0, **kw) == BADARG
        assert quant8(lib, 65, 4096, typ, layout=1, q=Q + 8, **kw) == SHAPE
    assert quant8(lib, 0, 4096, typ, layout=1) == OK               # an empty problem is fine in either layout


@pytest.mark.parametrize("typ", TYPES, ids=["fp16", "bf16"])
def test_gemm_entry_refusals_without_a_device(lib, typ):
    assert gemm(lib, typ, M=0) == OK
    assert gemm(lib, typ, sa=0) == BADARG
    assert gemm(lib, typ, sa=0, bias=BIAS) == BADARG
    assert gemm(lib, typ, M=-1) == BADARG
    assert gemm(lib, typ, layout=5) == BADARG
    assert gemm(lib, typ, K=40) == SHAPE                          # K % 16
    assert gemm(lib, typ, qa=Q + 8) == ALIGN
    assert gemm(lib, typ, bias=BIAS + 8) == ALIGN                 # a misaligned bias
    assert gemm(lib, typ, n_out=136, bias=BIAS) == SHAPE          # a bias takes one LDS pass of outlier columns
    if typ == BF16:
        assert gemm(lib, typ, n_out=136) == SHAPE                 # and so does a bf16 call


def test_python_wrappers_refuse_mixed_dtypes_and_bf16_int4():
    """mixlib's norm ops dispatch on _input.dtype: every row operand, gamma, _out, h_out and scaleRow must have it (a ValueError
    raised before anything reaches the library, so CPU tensors do here); the packed 4-bit ops have no bf16 form (TypeError)."""
    torch = pytest.importorskip("torch")
    from mixq_tensorrt_llm_amd import mixlib
    ind = torch.zeros(8, dtype=torch.int32)

    def operands(dt):
        return dict(x=torch.zeros((4, 64), dtype=dt), r=torch.zeros((4, 64), dtype=dt), gamma=torch.ones(64, dtype=dt),
                    out=torch.empty((4, 64), dtype=dt), sc=torch.empty((4, 1), dtype=dt))

    def calls(o, **kw):
        return [lambda: mixlib.layernorm_forward_cuda(o["x"], o["gamma"], o["out"], 1e-6),
                lambda: mixlib.layernorm_forward_cuda_extract_outliers(o["x"], o["gamma"], o["out"], 1e-6, ind, o["sc"]),
                lambda: mixlib.add_layernorm_forward_cuda(o["x"], o["r"], o["gamma"], o["out"], 1e-6, **kw),
                lambda: mixlib.add_layernorm_forward_cuda_extract_outliers(o["x"], o["r"], o["gamma"], o["out"], 1e-6, ind, o["sc"], **kw)]

    for dt, other, name in ((torch.bfloat16, torch.float16, "bf16"), (torch.float16, torch.bfloat16, "fp16")):
        for odd in ("gamma", "out", "r", "sc"):
            o = operands(dt)
            o[odd] = o[odd].to(other)
            for i, call in enumerate(calls(o)):
                if (odd == "r" and i < 2) or (odd == "sc" and i in (0, 2)):
                    continue                                  # (the op does not take that operand)
                with pytest.raises(ValueError, match=name):
                    call()
        for call in calls(operands(dt), h_out=torch.zeros((4, 64), dtype=other))[2:]:
            with pytest.raises(ValueError, match=name):
                call()
        # matching operands get as far as the device check: there is no CPU path
        for call in calls(operands(dt)):
            with pytest.raises(_lib.MixQLibraryError):
                call()
    o = operands(torch.bfloat16)
    with pytest.raises(TypeError, match="bf16"):
        mixlib.layernorm_forward_cuda_extract_outliers_int4(o["x"], o["gamma"], o["out"], 1e-6, ind, o["sc"])
    with pytest.raises(TypeError, match="bf16"):
        mixlib.add_layernorm_forward_cuda_extract_outliers_int4(o["x"], o["r"], o["gamma"], o["out"], 1e-6, ind, o["sc"])
    # gemm_mixed: one activation type for x_scale, outliers, fp_weight, bias and out; sW stays fp16
    q, Wq = torch.zeros((4, 64), dtype=torch.int8), torch.zeros((32, 64), dtype=torch.int8)
    bf, f16 = torch.bfloat16, torch.float16
    good = dict(x_scale=torch.zeros(4, dtype=bf), sW=torch.zeros(32, dtype=f16), outliers=torch.zeros((4, 8), dtype=bf),
                fp_weight=torch.zeros((32, 8), dtype=bf))
    for odd, dt in (("x_scale", f16), ("fp_weight", f16), ("sW", bf)):
        kw = dict(good)
        kw[odd] = kw[odd].to(dt)
        with pytest.raises(TypeError):
            mixlib.gemm_mixed(q, Wq, kw["x_scale"], kw["sW"], kw["outliers"], kw["fp_weight"], 4, 32, 64)
    with pytest.raises(TypeError):
        mixlib.gemm_mixed(q, Wq, good["x_scale"], good["sW"], good["outliers"], good["fp_weight"], 4, 32, 64, bias=torch.zeros(32, dtype=f16))
    with pytest.raises(_lib.MixQLibraryError):
        mixlib.gemm_mixed(q, Wq, good["x_scale"], good["sW"], good["outliers"], good["fp_weight"], 4, 32, 64)


def test_python_layers_carry_the_dtype():
    torch = pytest.importorskip("torch")
    from mixq_tensorrt_llm_amd import mixlinear, plugin
    bf = torch.bfloat16
    cache = mixlinear.MixLibCache(inputdim=8, device="cpu", dtype=bf)
    assert cache.x_scale.dtype == bf and mixlinear.MixLibCache(inputdim=8, device="cpu").x_scale.dtype == torch.float16
    norm = mixlinear.FasterTransformerRMSNorm(torch.ones(64), 1e-6, cache, dtype=bf)
    assert norm.weight.dtype == bf and mixlinear.FasterTransformerRMSNorm(torch.ones(64)).weight.dtype == torch.float16
    layer = plugin.MixQLinear(64, 32, dtype=bf, device="cpu")
    assert layer.bit == 8 and layer.add_outliers is False
    assert layer.ind.dtype == torch.int32 and layer.ind.shape == (plugin.NUM_OUTLIERS,)
    norm.next_layer = type("Int4Layer", (), dict(bit=4, ind=layer.ind, out_features=32, add_outliers=False))()
    with pytest.raises(TypeError, match="bf16"):
        norm.forward(torch.zeros((4, 64), dtype=bf))
    sharded = plugin.MixQLinear(64, 32, tp_size=2, device="cpu")
    with pytest.raises(ValueError, match="tp_size"):
        sharded.forward_quantised(torch.zeros((4, 64), dtype=torch.int8), torch.zeros(4, dtype=torch.float16),
                                  torch.zeros((4, 128), dtype=torch.float16))


def test_restatement_against_torch_cpu_bf16():
    """tests/bf16_norm_restate.py on one small case: the add is torch's bf16 add bit for bit; the norm agrees with torch's fp32
    evaluation rounded to bf16 within one bf16 ulp; extract_zero moves the columns out."""
    torch = pytest.importorskip("torch")
    import bf16_norm_restate as NR
    import bf16_restate as BR
    g = torch.Generator().manual_seed(5)
    M, K, eps = 6, 96, 1e-5
    x = (torch.randn((M, K), generator=g) * 3).to(torch.bfloat16)
    r = (torch.randn((M, K), generator=g) * 40).to(torch.bfloat16)
    r[1] = -x[1]                                                   # cancels to 0
    x[2], r[2] = 3e38, 3e38                                        # overflows to +inf
    gamma = (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16)
    h = x + r
    h_bits = NR.add_bits(BR.to_bits(x), BR.to_bits(r))
    assert np.array_equal(h_bits, BR.to_bits(h))
    assert (h_bits[1] & 0x7FFF == 0).all() and (h_bits[2] == 0x7F80).all()
    rows = [0, 1, 3, 4, 5]                                         # (row 2 is inf / inf = NaN in both)
    hf = h.float()
    want = ((hf * torch.rsqrt((hf * hf).mean(dim=1, keepdim=True) + eps)) * gamma.float()).to(torch.bfloat16)
    ref = NR.rmsnorm64(h_bits, BR.to_bits(gamma), eps)
    err = np.abs(BR.bf2f(BR.to_bits(want)).astype(np.float64) - ref)[rows]
    assert (err <= BR.ulp_bf16(ref[rows])).all()
    assert np.isnan(ref[2]).all() and (ref[1] == 0).all()
    ind = np.array([5, 90, -1, 96, 0], np.int32)
    outl, zeroed = NR.extract_zero(BR.to_bits(want), ind)
    assert np.array_equal(outl[:, [0, 1, 4]], BR.to_bits(want)[:, [5, 90, 0]]) and (outl[:, [2, 3]] == 0).all()
    assert (zeroed[:, [5, 90, 0]] == 0).all() and np.array_equal(np.delete(zeroed, [0, 5, 90], 1), np.delete(BR.to_bits(want), [0, 5, 90], 1))
    # gemm_given on exact inputs: one outlier term per output, powers of two
    q = np.array([[3, -2, 1, 0] * 4], np.int8)
    Wq = np.array([[1, 1, 1, 1] * 4, [2, 0, -1, 5] * 4], np.int8)
    sA, sW = BR.bf16_rn(np.array([0.5], np.float32)), np.array([0.25, 2.0], np.float16)
    fpA, fpW = BR.bf16_rn(np.array([[3.0, 5.0]], np.float32)), BR.bf16_rn(np.array([[2.0, 0.0], [0.0, -0.5]], np.float32))
    out = NR.gemm_given(q, sA, fpA, Wq, sW, fpW, BR.bf16_rn(np.array([1.0, 0.0], np.float32)))
    assert np.array_equal(BR.bf2f(out), np.array([[8 * 0.125 + 6.0 + 1.0, 20 * 1.0 - 2.5]], np.float32))
