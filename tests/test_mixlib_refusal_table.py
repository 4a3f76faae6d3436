"""CPU: what every mixlib op answers to CPU tensors, over a grid of operand types and options, against a recorded table.

No mixlib op has a CPU path: given CPU tensors each one ends in an exception, at the latest ``MixQLibraryError`` from ``mixlib._dev``.
Which exception, and its text, therefore shows the order of every Python-side check in front of ``_dev``: the operand types a family
accepts, the class it refuses with (``ValueError`` for the norm ops, ``TypeError`` for the P-flavour ops and ``gemm_mixed``) and which
of two wrong operands is named.  tests/golden/mixlib_refusals.json holds the outcome of every call of the grid below, recorded with
tools/record_mixlib_refusals.py from a tree whose answers are the accepted ones; this module replays the grid.  Nothing reaches a
device: the tensors are CPU tensors on every machine."""
import itertools
import json
import os

import pytest
import torch

from conftest import ROOT

from mixq_tensorrt_llm_amd import _lib, mixlib, mixlinear

FIXTURE = os.path.join(ROOT, "tests", "golden", "mixlib_refusals.json")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
TYPES = (F16, BF16, F32)
M, N, K, O = 2, 16, 16, 8
EPS = 1e-5


def t(dtype, *shape):
    return None if dtype is None else torch.zeros(shape, dtype=dtype)


def i32(*shape):
    return torch.zeros(shape, dtype=torch.int32)


def i8(*shape):
    return torch.zeros(shape, dtype=torch.int8)


def u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def strided(dtype, rows, cols):
    return torch.zeros((rows, 2 * cols), dtype=dtype)[:, ::2]


def name(v):
    return {F16: "f16", BF16: "bf16", F32: "f32", None: "none"}.get(v, str(v))


def product(**axes):
    keys = list(axes)
    return [dict(zip(keys, vs)) for vs in itertools.product(*axes.values())]


CASES = []   # (id, thunk)


def case(op, kw, fn):
    CASES.append((op + "[" + ",".join(f"{k}={name(v)}" for k, v in kw.items()) + "]", fn))


# ---------------------------------------------------------------------------------------------- row quantiser ---
for kw in product(x=TYPES, scaleRow=TYPES, bit=(8, 4)):
    case("FindRowScale", kw, lambda kw=kw: mixlib.FindRowScale(t(kw["x"], M, K), t(kw["scaleRow"], M, 1), M, K, kw["bit"]))
for dt in (F16, BF16):
    case("FindRowScale", dict(x=dt, strided=1), lambda dt=dt: mixlib.FindRowScale(strided(dt, M, K), t(dt, M, 1), M, K))
    case("FindRowScale", dict(x=dt, short_scale=1), lambda dt=dt: mixlib.FindRowScale(t(dt, M, K), t(dt, 1, 1), M, K))
for kw in product(x=TYPES, scaleRow=TYPES, len_ind=(0, O), q_layout=(0, 1)):
    case("FindRowScaleFusedExtracOutliers", kw, lambda kw=kw: mixlib.FindRowScaleFusedExtracOutliers(
        t(kw["x"], M, K), t(kw["scaleRow"], M, 1), i32(kw["len_ind"]), kw["len_ind"], M, K, kw["q_layout"]))
for dt in TYPES:
    case("ExtractOutliersAndSetToZeros", dict(input=dt), lambda dt=dt: mixlib.ExtractOutliersAndSetToZeros(i32(O), t(dt, M, K)))
    case("ExtractOutliersAndSetToZeros", dict(input=dt, ind="int64"),
         lambda dt=dt: mixlib.ExtractOutliersAndSetToZeros(torch.zeros(O, dtype=torch.int64), t(dt, M, K)))
    case("ExtractOutliers", dict(input=dt), lambda dt=dt: mixlib.ExtractOutliers(i32(O), t(dt, M, K)))
    case("Int8quantize", dict(src=dt), lambda dt=dt: mixlib.Int8quantize(t(dt, M, K), t(dt, M, 1)))

# --------------------------------------------------------------------------------------------- norm producers ---
for kw in product(_input=TYPES, _gamma=TYPES, _out=TYPES):
    case("layernorm_forward_cuda", kw, lambda kw=kw: mixlib.layernorm_forward_cuda(t(kw["_input"], M, K), t(kw["_gamma"], K), t(kw["_out"], M, K), EPS))
for dt in (F16, BF16):
    case("layernorm_forward_cuda", dict(_input=dt, strided=1), lambda dt=dt: mixlib.layernorm_forward_cuda(strided(dt, M, K), t(dt, K), t(dt, M, K), EPS))
    case("layernorm_forward_cuda", dict(_input=dt, dims=3), lambda dt=dt: mixlib.layernorm_forward_cuda(t(dt, 1, M, K), t(dt, K), t(dt, 1, M, K), EPS))
for kw in product(_input=TYPES, _gamma=TYPES, _out=TYPES, scaleRow=TYPES):
    def _norm_q(kw=kw, int4=False, **more):
        args = (t(kw["_input"], M, K), t(kw["_gamma"], K), t(kw["_out"], M, K), EPS, i32(O), t(kw["scaleRow"], M, 1))
        if int4:
            return mixlib.layernorm_forward_cuda_extract_outliers_int4(*args)
        return mixlib.layernorm_forward_cuda_extract_outliers(*args, **more)
    case("layernorm_forward_cuda_extract_outliers", kw, _norm_q)
    case("layernorm_forward_cuda_extract_outliers", dict(kw, q_layout=1), lambda f=_norm_q: f(q_layout=1))
    case("layernorm_forward_cuda_extract_outliers_int4", kw, lambda f=_norm_q: f(int4=True))
for dt in (F16, BF16):
    case("layernorm_forward_cuda_extract_outliers", dict(_input=dt, strided="_out"), lambda dt=dt: mixlib.layernorm_forward_cuda_extract_outliers(
        t(dt, M, K), t(dt, K), strided(dt, M, K), EPS, i32(O), t(dt, M, 1)))
    case("layernorm_forward_cuda_extract_outliers", dict(_input=dt, short_scale=1), lambda dt=dt: mixlib.layernorm_forward_cuda_extract_outliers(
        t(dt, M, K), t(dt, K), t(dt, M, K), EPS, i32(O), t(dt, 1, 1)))
    case("layernorm_forward_cuda_extract_outliers_int4", dict(_input=dt, strided="_input"), lambda dt=dt: mixlib.layernorm_forward_cuda_extract_outliers_int4(
        strided(dt, M, K), t(dt, K), t(dt, M, K), EPS, i32(O), t(dt, M, 1)))

H_OUT = (None,) + TYPES
_ADD = {"add_layernorm_forward_cuda": 0, "add_layernorm_forward_cuda_extract_outliers": 8, "add_layernorm_forward_cuda_extract_outliers_int4": 4}


def _add_call(op, x, r, h, g, out, scale):
    """One call of an add form on prepared tensors (``scale`` unused by the plain form)."""
    if _ADD[op] == 0:
        return mixlib.add_layernorm_forward_cuda(x, r, g, out, EPS, h_out=h)
    return getattr(mixlib, op)(x, r, g, out, EPS, i32(O), scale, h_out=h)


for op, quant in _ADD.items():
    for kw in product(_input=TYPES, _residual=TYPES, h_out=H_OUT, _gamma=TYPES, _out=TYPES, **({"scaleRow": TYPES} if quant else {})):
        case(op, kw, lambda op=op, kw=kw: _add_call(op, t(kw["_input"], M, K), t(kw["_residual"], M, K), t(kw["h_out"], M, K), t(kw["_gamma"], K),
                                                    t(kw["_out"], M, K), t(kw.get("scaleRow"), M, 1)))
    for dt in (F16, BF16):
        full = lambda dt=dt: [t(dt, M, K), t(dt, M, K), t(dt, M, K), t(dt, K), t(dt, M, K), t(dt, M, 1)]  # noqa: E731
        for what, pos, bad in (("strided_input", 0, lambda dt: strided(dt, M, K)), ("strided_residual", 1, lambda dt: strided(dt, M, K)),
                               ("strided_h_out", 2, lambda dt: strided(dt, M, K)), ("residual_shape", 1, lambda dt: t(dt, M + 1, K)),
                               ("h_out_shape", 2, lambda dt: t(dt, M, 2 * K)), ("residual_dims", 1, lambda dt: t(dt, 1, M, K)),
                               ("strided_out", 4, lambda dt: strided(dt, M, K)), ("h_out_none", 2, lambda dt: None)):
            def _one(op=op, dt=dt, pos=pos, bad=bad, full=full):
                a = full()
                a[pos] = bad(dt)
                return _add_call(op, *a)
            case(op, dict(_input=dt, **{what: 1}), _one)
        if quant:
            case(op, dict(_input=dt, short_scale=1), lambda op=op, dt=dt, full=full: _add_call(op, *(full()[:5] + [t(dt, 1, 1)])))

# ------------------------------------------------------------------------------------- fused dequantising GEMMs ---
for y in (None, F16):
    for lay in (0, 1):
        kw = dict(y=y, qa_layout=lay)
        case("int8FusedDequantize", kw, lambda y=y, lay=lay: mixlib.int8FusedDequantize(i8(M, K), i8(N, K), t(F16, M, 1), t(F16, 1, N), t(y, M, N), M, N, K, lay))
        case("int8FusedDequantizeSilu", kw, lambda y=y, lay=lay: mixlib.int8FusedDequantizeSilu(i8(M, K), i8(N, K), t(F16, M, 1), t(F16, 1, N), t(y, M, N), M, N, K, lay))
        for mul in (None, F16):
            case("int8FusedDequantizeSiluMul", dict(kw, mul=mul), lambda y=y, lay=lay, mul=mul: mixlib.int8FusedDequantizeSiluMul(
                i8(M, K), i8(N, K), t(F16, M, 1), t(F16, 1, N), t(y, M, N), t(mul, M, N), M, N, K, lay))
    for b8 in (None, 1):
        kw = dict(y=y, B_int8=b8)
        case("int4FusedDequantize", kw, lambda y=y, b8=b8: mixlib.int4FusedDequantize(u8(M, K // 2), u8(N, K // 2), t(F16, M, 1), t(F16, 1, N), t(y, M, N), M, N,
                                                                                     K // 2, i8(N, K) if b8 else None))
        case("int4FusedDequantizeSilu", kw, lambda y=y, b8=b8: mixlib.int4FusedDequantizeSilu(u8(M, K // 2), u8(N, K // 2), t(F16, M, 1), t(F16, 1, N), t(y, M, N), M,
                                                                                             N, K // 2, i8(N, K) if b8 else None))
case("int8FusedDequantize", dict(strided="A"), lambda: mixlib.int8FusedDequantize(i8(M, 2 * K)[:, ::2], i8(N, K), t(F16, M, 1), t(F16, 1, N), None, M, N, K))
case("gemm", {}, lambda: mixlib.gemm(i8(M, K), i8(N, K), M, N, K))
case("dequantizeInt8", {}, lambda: mixlib.dequantizeInt8(i32(M, N), t(F16, M, 1), t(F16, 1, N), t(F16, M, N), 8, M, N))
case("dequantizeInt8Silu", {}, lambda: mixlib.dequantizeInt8Silu(i32(M, N), t(F16, M, 1), t(F16, 1, N), t(F16, M, N), 8, M, N))
case("w8_a16_gemm", {}, lambda: mixlib.w8_a16_gemm(t(F16, M, K), u8(K, N), t(F16, N)))
case("mixq_linear", {}, lambda: mixlib.mixq_linear(t(F16, M, K), i8(N, K), t(F16, N), t(F16, N, O), i32(O)))
case("unpack_int4_to_int8", {}, lambda: mixlib.unpack_int4_to_int8(u8(N, K // 2)))
case("unpack_int4_to_int8", dict(numel=24), lambda: mixlib.unpack_int4_to_int8(u8(3, 8)))
case("unpack_int4_to_fp16", {}, lambda: mixlib.unpack_int4_to_fp16(u8(N, K // 2), i32(O)))
case("WeightImage", {}, lambda: mixlib.WeightImage(i8(N, K)))
# the ops that are plain tensor code, or host code: they return on CPU tensors
case("int_to_half", {}, lambda: mixlib.int_to_half(i32(4)))
case("int_matrix_to_half", {}, lambda: mixlib.int_matrix_to_half(i32(2, 4)))
case("int8_matrix_to_half", {}, lambda: mixlib.int8_matrix_to_half(i8(2, 4)))
case("qa_to_row_major", {}, lambda: mixlib.qa_to_row_major(i8(16 * 64), 5, 40))
case("preprocess_weights", dict(w="int8"), lambda: mixlib.preprocess_weights(i8(64, 16)))
case("preprocess_weights", dict(w="f16"), lambda: mixlib.preprocess_weights(t(F16, 64, 16)))

# ------------------------------------------------------------------------------------------------- gemm_mixed ---
OPT = (None,) + TYPES


def _gemm_mixed(x_scale=F16, outliers=F16, fp_weight=F16, bias=None, out=None, mul=None, act=None, sW=F16, q=torch.int8, W=torch.int8, o=O,
                mul_rows=M, mul_is_out=False, short_scale=False):
    out_t = t(out, M, N)
    mul_t = out_t if mul_is_out else t(mul, mul_rows, N)
    return mixlib.gemm_mixed(torch.zeros((M, K), dtype=q), torch.zeros((N, K), dtype=W), t(x_scale, 1 if short_scale else M, 1), t(sW, N),
                             t(outliers, M, o), t(fp_weight, N, o), M, N, K, bias=t(bias, N), out=out_t, act=act, mul=mul_t)


for kw in product(x_scale=TYPES, outliers=OPT, fp_weight=TYPES, bias=OPT, out=OPT):
    case("gemm_mixed", kw, lambda kw=kw: _gemm_mixed(**kw))
for kw in product(x_scale=TYPES, outliers=(F16, BF16), out=OPT, mul=OPT):
    case("gemm_mixed", dict(kw, act="silu"), lambda kw=kw: _gemm_mixed(act="silu", **kw))
for kw in (dict(act="relu"), dict(mul=F16), dict(act="silu", bias=F16), dict(act="silu", mul=F16, mul_rows=M + 1), dict(act="silu", mul=F16, out=F16, mul_is_out=True),
           dict(sW=F32), dict(sW=BF16, x_scale=BF16, outliers=BF16, fp_weight=BF16), dict(q=torch.uint8), dict(W=torch.uint8), dict(o=0),
           dict(o=0, x_scale=BF16, fp_weight=F32), dict(o=0, x_scale=F32), dict(short_scale=True), dict(act="relu", x_scale=F32), dict(mul=F32, sW=F32)):
    case("gemm_mixed", kw, lambda kw=kw: _gemm_mixed(**kw))

# ------------------------------------------------------------------------------------------ mixlinear_forward ---
for kw in product(x=TYPES, x_scale=TYPES, weight_cache=OPT, scale_col=TYPES, o=(0, O)):
    case("mixlinear_forward", kw, lambda kw=kw: mixlib.mixlinear_forward(t(kw["x"], M, K), i32(kw["o"]), i8(N, K), t(kw["scale_col"], 1, N),
                                                                         t(kw["weight_cache"], N, kw["o"]), t(kw["x_scale"], M, 1)))
for dt in (F16, BF16):
    case("mixlinear_forward", dict(x=dt, strided=1), lambda dt=dt: mixlib.mixlinear_forward(strided(dt, M, K), i32(O), i8(N, K), t(F16, 1, N), t(dt, N, O), t(dt, M, 1)))
    case("mixlinear_forward", dict(x=dt, q_layout=1), lambda dt=dt: mixlib.mixlinear_forward(t(dt, M, K), i32(O), i8(N, K), t(F16, 1, N), t(dt, N, O), t(dt, M, 1), 1))

# ------------------------------------------------------------------------------------- mixlinear's own two ops ---
for dt in TYPES:
    case("mixlinear.find_outliers", dict(activation=dt), lambda dt=dt: mixlinear.find_outliers(t(dt, M, K), 6.0))
    case("mixlinear.find_outliers", dict(activation=dt, dims=1), lambda dt=dt: mixlinear.find_outliers(t(dt, K), 6.0, capacity=4))
for kw in product(dtype=TYPES, scale_col=TYPES):
    case("mixlinear.dequant_weight_columns", kw, lambda kw=kw: mixlinear.dequant_weight_columns(i8(N, K), t(kw["scale_col"], 1, N), i32(O), dtype=kw["dtype"]))
case("mixlinear.dequant_weight_columns", dict(ind="int64"), lambda: mixlinear.dequant_weight_columns(i8(N, K), t(F16, 1, N), torch.zeros(O, dtype=torch.int64)))
case("mixlinear.dequant_weight_columns", dict(q_weight="uint8"), lambda: mixlinear.dequant_weight_columns(u8(N, K), t(F16, 1, N), i32(O)))

assert len({c[0] for c in CASES}) == len(CASES), "case ids must be unique"


def outcome(fn):
    """[exception class name, str(exception)] of one call, or ["returned", ""]."""
    try:
        fn()
    except Exception as e:  # noqa: BLE001 (the class is what is recorded)
        return [type(e).__name__, str(e)]
    return ["returned", ""]


def by_op():
    """{op: [(case id, thunk)]} in the grid's order."""
    ops = {}
    for cid, fn in CASES:
        ops.setdefault(cid.split("[")[0], []).append((cid, fn))
    return ops


def ids_digest(cases):
    import hashlib
    return hashlib.sha256("\n".join(cid for cid, _ in cases).encode()).hexdigest()[:16]


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(_lib.LIB_PATH):   # (preprocess_weights is host code of the library)
        import __graft_entry__ as g
        g.build()
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_table_holds_every_recorded_case(table):
    """Fails -- it does not skip -- when cases were dropped from the table or from the grid."""
    ops = by_op()
    assert table["count"] == sum(len(v["index"]) for v in table["ops"].values()), "the table is cut short"
    assert len(CASES) >= table["count"], "the grid lost cases that were recorded"
    assert table["count"] >= 3634, "cases left the table since it was first recorded"
    assert sorted(ops) == sorted(table["ops"])
    for op, cases in ops.items():
        assert len(cases) == len(table["ops"][op]["index"]) and ids_digest(cases) == table["ops"][op]["ids"], \
            f"{op}: the grid changed: record the table again (tools/record_mixlib_refusals.py)"
    tensor_free = {"qa_layout", "QA_ROW_MAJOR", "QA_FRAGMENT_MAJOR"}
    assert set(ops) >= set(mixlib.__all__) - tensor_free, sorted(set(mixlib.__all__) - tensor_free - set(ops))


@pytest.mark.parametrize("op", sorted(by_op()))
def test_every_call_is_answered_as_recorded(table, op):
    cases, rec = by_op()[op], table["ops"][op]
    assert len(cases) == len(rec["index"])
    wrong = []
    for (cid, fn), i in zip(cases, rec["index"]):
        got = outcome(fn)
        if got != table["outcomes"][i]:
            wrong.append((cid, table["outcomes"][i], got))
    assert not wrong, f"{len(wrong)} of {len(cases)} calls changed their answer; (case, recorded, now): {wrong[:5]}"
