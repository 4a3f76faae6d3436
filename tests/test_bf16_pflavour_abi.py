"""CPU: the typed entries of the P-flavour (mixq_quant_extract_typed, mixq_find_outliers_typed, mixq_dequant_weight_columns_typed,
mixq_mixlinear_forward_typed) are exported, typed and declared, leave the ABI revision at 5, and refuse bad arguments -- MIXQ_E_TYPE
first, then with the codes of the entries they mirror -- before anything is launched, so none of this needs a device (dummy integers
stand in for pointers, as in test_bf16_norm_abi).  Also: the Python wrappers' dtype rules on CPU tensors, and the restatement helper
(tests/bf16_pflavour_restate.py) against torch CPU bf16."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from mixq_tensorrt_llm_amd import _lib

OK, BADARG, SHAPE, ALIGN, E_TYPE = 0, 1, 2, 3, 7
HALF, BF16 = _lib.MIXQ_TYPE_HALF, _lib.MIXQ_TYPE_BF16
NAMES = ("mixq_quant_extract_typed", "mixq_find_outliers_typed", "mixq_dequant_weight_columns_typed", "mixq_mixlinear_forward_typed")
SIGMA = ctypes.c_float(6.0)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def P(v):
    return ctypes.c_void_p(v)


X, Q, SC, OUTL, IND, W, SW, WC, OUT, WS, CNT = [0x10000 + 0x1000 * i for i in range(11)]     # distinct 16-byte aligned "pointers"


def qe(lib, typ, M=4, K=64, a=X, q=Q, s=SC, f=OUTL, ind=IND, n=8, zero=1, layout=0, named=False):
    if named:
        return lib.mixq_quant_extract_layout(M, K, P(a), P(q), P(s), P(f), P(ind), n, zero, layout, None)
    return lib.mixq_quant_extract_typed(M, K, P(a), P(q), P(s), P(f), P(ind), n, zero, layout, typ, None)


def fo(lib, typ, M=4, K=64, a=X, ws=WS, ind=IND, cnt=CNT, cap=8, named=False):
    if named:
        return lib.mixq_find_outliers(P(a), M, K, SIGMA, P(ws), P(ind), P(cnt), cap, None)
    return lib.mixq_find_outliers_typed(P(a), M, K, SIGMA, P(ws), P(ind), P(cnt), cap, typ, None)


def dq(lib, typ, N=16, K=64, qw=W, sc=SW, ind=IND, n=8, out=OUT, named=False):
    if named:
        return lib.mixq_dequant_weight_columns(P(qw), P(sc), P(ind), n, P(out), N, K, None)
    return lib.mixq_dequant_weight_columns_typed(P(qw), P(sc), P(ind), n, P(out), N, K, typ, None)


def mf(lib, typ, M=16, N=32, K=64, n_out=8, x=X, ind=IND, qw=W, sc=SW, wc=WC, xs=SC, q=Q, outl=OUTL, out=OUT, layout=0, named=False):
    if named:
        return lib.mixq_mixlinear_forward(M, N, K, n_out, P(x), P(ind), P(qw), P(sc), P(wc), P(xs), P(q), P(outl), P(out), layout, None, 0, None)
    return lib.mixq_mixlinear_forward_typed(M, N, K, n_out, P(x), P(ind), P(qw), P(sc), P(wc), P(xs), P(q), P(outl), P(out), layout, typ,
                                            None, 0, None)


ENTRIES = [qe, fo, dq, mf]


def test_symbols_are_declared_exported_and_typed(lib):
    src = open(os.path.join(ROOT, "include", "mixq.h")).read()
    declared = set(re.findall(r"MIXQ_API\s+[\w\s\*]+?\b(\w+)\s*\(", src))
    sig = _lib.SIGNATURES
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/mixq.h"
        assert name in sig, f"{name} has no ctypes signature"
        fn = getattr(lib, name)
        restype, argtypes = sig[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    # the named entry's arguments with `type` directly in front of the stream
    for name, base in (("mixq_quant_extract_typed", "mixq_quant_extract_layout"), ("mixq_find_outliers_typed", "mixq_find_outliers"),
                       ("mixq_dequant_weight_columns_typed", "mixq_dequant_weight_columns")):
        b = list(sig[base][1])
        assert list(sig[name][1]) == b[:-1] + [ctypes.c_int] + b[-1:], name
    # mixq_mixlinear_forward's arguments with `type` behind q_layout, as mixq_gemm_mixed_typed has it in front of scratch / stream
    b = list(sig["mixq_mixlinear_forward"][1])
    assert list(sig["mixq_mixlinear_forward_typed"][1]) == b[:14] + [ctypes.c_int] + b[14:]
    note = src[src.index("ABI revision of THIS header"):]
    for name in NAMES:
        assert name in note, f"{name} is missing from the revision note"


def test_abi_revision_is_still_5(lib):
    src = open(os.path.join(ROOT, "include", "mixq.h")).read()
    assert re.search(r"^#define MIXQ_ABI_VERSION 5$", src, re.M)
    assert lib.mixq_abi_version() == 5 and _lib.ABI_VERSION == 5


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda f: f.__name__)
def test_a_bad_type_is_refused_before_everything_else(lib, entry):
    for typ in (0, 2, 3, 6, 8, -1):
        assert entry(lib, typ) == E_TYPE
        assert entry(lib, typ, K=0) == E_TYPE               # (another refusal at once)
        assert entry(lib, typ, K=12, ind=0) == E_TYPE
    assert mf(lib, 9, M=-1, x=0, layout=5) == E_TYPE
    assert qe(lib, 9, M=-1, a=0, layout=5) == E_TYPE


# bad arguments per entry, each refused by the named fp16 entry before anything is launched
BAD = {
    qe: [dict(M=-1), dict(K=0), dict(n=-1), dict(a=0), dict(q=0), dict(s=0), dict(f=0), dict(ind=0), dict(K=12), dict(a=X + 8), dict(q=Q + 4),
         dict(layout=7), dict(layout=-1), dict(layout=1, M=65, K=4096), dict(layout=1, M=16, K=1024), dict(layout=1, M=16, K=2048, q=Q + 8),
         dict(layout=1, M=16, K=2048, a=0), dict(K=12, a=0), dict(K=12, a=X + 2), dict(layout=1, M=0, K=2048)],
    fo: [dict(M=-1), dict(K=0), dict(cap=-1), dict(ws=0), dict(cnt=0), dict(ind=0), dict(a=0), dict(K=12), dict(a=X + 8), dict(K=12, a=0),
         dict(K=12, a=X + 2)],
    dq: [dict(N=-1), dict(K=0), dict(n=-1), dict(qw=0), dict(sc=0), dict(ind=0), dict(out=0)],
    mf: [dict(M=-1), dict(N=-1), dict(K=0), dict(n_out=-1), dict(x=0), dict(qw=0), dict(sc=0), dict(xs=0), dict(q=0), dict(out=0),
         dict(ind=0), dict(wc=0), dict(outl=0), dict(K=12), dict(x=X + 8), dict(layout=1), dict(layout=1, n_out=12),
         dict(layout=1, M=16, N=4096, K=2048, n_out=136)],
}
EXPECT_BF16 = {
    qe: [BADARG] * 8 + [SHAPE, ALIGN, ALIGN, BADARG, BADARG, SHAPE, SHAPE, ALIGN, BADARG, BADARG, SHAPE, SHAPE],
    fo: [BADARG] * 7 + [SHAPE, ALIGN, BADARG, SHAPE],
    dq: [BADARG] * 7,
    mf: [BADARG] * 13 + [SHAPE, ALIGN, SHAPE, SHAPE, SHAPE],
}


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda f: f.__name__)
def test_half_is_the_named_entry_and_bf16_keeps_its_codes(lib, entry):
    for kw, want in zip(BAD[entry], EXPECT_BF16[entry]):
        named = entry(lib, HALF, named=True, **kw)
        assert named != OK, kw
        assert entry(lib, HALF, **kw) == named, f"{entry.__name__} {kw}: MIXQ_TYPE_HALF differs from the named entry ({named})"
        assert entry(lib, BF16, **kw) == want, f"{entry.__name__} {kw}: bf16"
        if entry is not mf:
            assert named == want, f"{entry.__name__} {kw}: the bf16 code is the fp16 entry's"


@pytest.mark.parametrize("typ", [HALF, BF16], ids=["fp16", "bf16"])
def test_empty_problems_are_fine(lib, typ):
    assert mf(lib, typ, M=0) == OK and mf(lib, typ, N=0) == OK
    assert mf(lib, typ, M=0, x=0, out=0, q=0) == OK
    assert qe(lib, typ, M=0) == OK and qe(lib, typ, M=0, a=0, q=0, s=0) == OK
    assert dq(lib, typ, N=0) == OK and dq(lib, typ, n=0, qw=0) == OK


def test_bf16_mixlinear_forward_refusals_and_their_order(lib):
    assert mf(lib, BF16, n_out=12) == SHAPE                       # the bf16 epilogues have no addend form: O % 8 ...
    assert mf(lib, BF16, n_out=136) == SHAPE                      # ... and O <= 128
    assert mf(lib, BF16, out=OUT + 8) == ALIGN
    assert mf(lib, BF16, out=OUT + 2) == ALIGN
    for kw in (dict(K=40), dict(N=24), dict(K=72, N=32)):         # K % 16, N % 16
        assert mf(lib, BF16, **kw) == SHAPE, kw
    assert mf(lib, BF16, layout=1, M=16, N=32, K=64) == SHAPE      # a fragment-major image where mixq_qa_layout does not say so
    assert mf(lib, BF16, layout=3) == BADARG
    for kw in (dict(x=X + 8), dict(q=Q + 8), dict(qw=W + 8), dict(sc=SW + 2), dict(wc=WC + 8), dict(outl=OUTL + 8)):
        assert mf(lib, BF16, **kw) == ALIGN, kw
    # MIXQ_E_BADARG, then MIXQ_E_SHAPE, then MIXQ_E_ALIGN
    assert mf(lib, BF16, n_out=12, x=0) == BADARG
    assert mf(lib, BF16, n_out=12, out=OUT + 8) == SHAPE
    assert mf(lib, BF16, K=40, x=X + 8) == SHAPE
    assert mf(lib, BF16, n_out=0, ind=0, wc=0, outl=0, out=OUT + 8) == ALIGN   # (no outlier columns: their pointers may be NULL)


def test_python_dtype_rules_on_cpu_tensors():
    """A bf16 layer takes bit 8 and not weight_only; every wrapper takes one activation type (TypeError before the library is
    touched, so CPU tensors do here); matching operands get as far as the device check."""
    torch = pytest.importorskip("torch")
    from mixq_tensorrt_llm_amd import mixlib, mixlinear
    bf, f16 = torch.bfloat16, torch.float16
    with pytest.raises(TypeError, match="bf16"):
        mixlinear.MixLinear_GEMM(64, 32, False, "cpu", bit=4, dtype=bf)
    with pytest.raises(TypeError, match="bf16"):
        mixlinear.MixLinear_GEMM(64, 32, False, "cpu", weight_only=True, dtype=bf)
    with pytest.raises(TypeError):
        mixlinear.MixLinear_GEMM(64, 32, False, "cpu", dtype=torch.float32)
    with pytest.raises(TypeError, match="bf16"):
        mixlinear.MixLinear_GEMM.from_linear(torch.zeros((32, 64), dtype=bf), bit=8, weight_only=True, dev="cpu", dtype=bf)
    cache = mixlinear.MixLibCache(inputdim=8, device="cpu", dtype=bf)
    layer = mixlinear.MixLinear_GEMM(64, 32, True, "cpu", cache=cache, dtype=bf)
    assert layer.dtype == bf and layer.bias.dtype == bf and layer.q_weight.dtype == torch.int8 and layer.scale_col.dtype == f16
    assert mixlinear.MixLinear_GEMM(64, 32, True, "cpu").bias.dtype == f16
    x, ind = torch.zeros((4, 64), dtype=bf), torch.zeros(8, dtype=torch.int32)
    with pytest.raises(TypeError, match="bf16"):
        layer.forward(x.to(f16), cache, True)                              # fp16 rows into a bf16 layer
    with pytest.raises(TypeError, match="bf16"):
        layer.forward(x, mixlinear.MixLibCache(inputdim=8, device="cpu"), True)   # an fp16 cache
    layer.arch = 9
    with pytest.raises(TypeError, match="arch"):
        layer.forward(x, cache, True)
    with pytest.raises(TypeError, match="arch"):
        layer.forward_without_preconditionFusedSilu(x, cache)
    layer.arch = 0
    sc_bf, sc_16 = torch.zeros((8, 1), dtype=bf), torch.zeros((8, 1), dtype=f16)
    qw, sw = torch.zeros((32, 64), dtype=torch.int8), torch.zeros((1, 32), dtype=f16)
    wc = torch.zeros((32, 8), dtype=bf)
    with pytest.raises(TypeError, match="4-bit"):
        mixlib.FindRowScale(x, sc_bf, 4, 64, 4)
    for a, s in ((x, sc_16), (x.to(f16), sc_bf)):
        with pytest.raises(TypeError):
            mixlib.FindRowScale(a, s, 4, 64, 8)
        with pytest.raises(TypeError):
            mixlib.FindRowScaleFusedExtracOutliers(a, s, ind, 8, 4, 64)
        with pytest.raises(TypeError):
            mixlib.mixlinear_forward(a, ind, qw, sw, wc.to(a.dtype), s)
    with pytest.raises(TypeError):
        mixlib.mixlinear_forward(x, ind, qw, sw, wc.to(f16), sc_bf)         # fp16 outlier weights in a bf16 call
    with pytest.raises(TypeError):
        mixlib.mixlinear_forward(x, ind, qw, sw.to(bf), wc, sc_bf)          # the weight scales stay fp16
    with pytest.raises(TypeError):
        mixlib.ExtractOutliersAndSetToZeros(ind, x.float())
    with pytest.raises(TypeError):
        mixlib.ExtractOutliers(ind, x.float())
    with pytest.raises(TypeError):
        mixlinear.find_outliers(x.float(), 6.0)
    with pytest.raises(TypeError):
        mixlinear.dequant_weight_columns(qw, sw.to(bf), ind, dtype=bf)
    with pytest.raises(TypeError):
        mixlinear.dequant_weight_columns(qw, sw, ind, dtype=torch.float32)
    # matching operands get as far as the device check: there is no CPU path
    for call in (lambda: mixlib.FindRowScale(x, sc_bf, 4, 64, 8), lambda: mixlib.FindRowScaleFusedExtracOutliers(x, sc_bf, ind, 8, 4, 64),
                 lambda: mixlib.mixlinear_forward(x, ind, qw, sw, wc, sc_bf), lambda: mixlib.ExtractOutliersAndSetToZeros(ind, x),
                 lambda: mixlib.ExtractOutliers(ind, x)):
        with pytest.raises(_lib.MixQLibraryError):
            call()


def test_restatement_against_torch_cpu_bf16():
    torch = pytest.importorskip("torch")
    import bf16_pflavour_restate as PR
    import bf16_restate as R
    g = torch.Generator().manual_seed(11)
    M, K, N = 7, 72, 16
    A = (torch.randn((M, K), generator=g) * 3).clamp(-5, 5).to(torch.bfloat16)
    sigma = torch.tensor([[6.0]], dtype=torch.float16)
    nxt = R.from_bits(np.array([R.bf16_rn(np.float32(6.0)) + 1], np.uint16))[0]     # the next bf16 above sigma
    A[0, 3], A[1, 9], A[2, 11], A[3, 20], A[4, 33], A[5, 40], A[6, 71] = 6.0, nxt, -nxt, float("nan"), float("inf"), -float("inf"), 7.5
    # 1. FindOutliers
    want = torch.unique(torch.where(A.abs() > sigma)[1]).to(torch.int32).numpy()
    got = PR.find_outliers(R.to_bits(A), 6.0)
    assert np.array_equal(got, want) and {9, 11, 33, 40, 71} <= set(got.tolist()) and 3 not in got and 20 not in got
    # 2. the weight columns
    qw = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int8)
    sW = (torch.rand((N, 1), generator=g) * 0.02 + 0.001).to(torch.float16)
    ind = torch.tensor([0, 71, 9, 9, 40], dtype=torch.int64)
    want = (qw[:, ind].float() * sW.float()).to(torch.bfloat16)
    got = PR.dequant_columns(qw.numpy(), sW.numpy().reshape(-1), np.array([0, 71, 9, -1, 9, 40, K], np.int32))
    assert np.array_equal(got[:, [0, 1, 2, 4, 5]], R.to_bits(want)) and (got[:, [3, 6]] == 0).all()
    # 3. a bf16 quantise of a zeroed row
    idx = np.array([9, 11, -1, 33, 40, 71, 0, 0], np.int32)
    q, sA, fpA, z = PR.quant_rows_zeroed(R.to_bits(A), idx)
    Z = A.clone()
    Z[:, [9, 11, 33, 40, 71, 0]] = 0
    assert np.array_equal(z, R.to_bits(Z)) and np.array_equal(fpA[:, [0, 1, 3, 4, 5, 6, 7]], R.to_bits(A[:, [9, 11, 33, 40, 71, 0, 0]]))
    assert (fpA[:, 2] == 0).all()
    zf = Z.float()
    amax = torch.where(torch.isnan(zf), torch.zeros(()), zf.abs()).max(dim=1)[0]
    s_t = (amax / 127).to(torch.bfloat16)
    assert np.array_equal(sA, R.to_bits(s_t))
    q_t = torch.nan_to_num(torch.round(zf / s_t.float()[:, None]), nan=0.0).clamp(-127, 127).to(torch.int8)
    assert np.array_equal(q, q_t.numpy())
    assert np.abs(q).max() == 127 and (q[3, 20] == 0)
    # forward on exact inputs: one outlier term per output
    wc = np.zeros((N, idx.size), np.float32)
    wc[np.arange(N), np.arange(N) % 2] = 0.5
    out, q2, sA2, fpA2, _ = PR.forward(R.to_bits(A), idx, qw.numpy(), sW.numpy().reshape(-1), R.bf16_rn(wc))
    assert np.array_equal(q2, q) and np.array_equal(sA2, sA) and np.array_equal(fpA2, fpA)
    acc = q.astype(np.float64) @ qw.numpy().astype(np.float64).T
    s = sW.numpy().astype(np.float32).reshape(1, -1) * R.bf2f(sA)[:, None]
    P = R.bf2f(fpA)[:, np.arange(N) % 2].astype(np.float64) * 0.5
    assert np.array_equal(out[[0, 1, 2]], R.bf16_rn((acc * s + P).astype(np.float32))[[0, 1, 2]])
