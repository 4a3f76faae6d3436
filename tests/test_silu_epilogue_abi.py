"""CPU: mixq_gemm_mixed_act_typed (the fused mixed GEMM with a SiLU or SiLU x up epilogue) is exported, typed and declared, leaves the
ABI revision at 5 and refuses bad arguments by class -- type, arguments, shapes, alignment, in that order -- before anything is launched,
so none of this needs a device (dummy integers stand in for pointers, as in test_bf16_norm_abi).  Also: the Python refusals of
mixlib.gemm_mixed, MixQLinear.forward_quantised and MixQLlamaMLP on CPU tensors, and the restatement helper (tests/silu_restate.py)
against torch CPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from mixq_tensorrt_llm_amd import _lib

OK, BADARG, SHAPE, ALIGN, E_TYPE = 0, 1, 2, 3, 7
HALF, BF16 = _lib.MIXQ_TYPE_HALF, _lib.MIXQ_TYPE_BF16
NAME = "mixq_gemm_mixed_act_typed"
PLAIN, SILU, SILU_MUL = 0, 1, 3


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def P(v):
    return ctypes.c_void_p(v)


Q, W, SA, SW, FPA, FPW, MUL, OUT = [0x10000 + 0x1000 * i for i in range(8)]     # distinct 16-byte aligned "pointers"


def act(lib, typ, epi=SILU, M=16, N=32, K=64, O=8, qa=Q, w=W, sa=SA, sw=SW, fpa=FPA, fpw=FPW, mul=None, out=OUT, layout=0):
    if mul is None:
        mul = MUL if epi == SILU_MUL else 0
    return lib.mixq_gemm_mixed_act_typed(P(qa), P(w), P(sa), P(sw), P(fpa), P(fpw), P(mul), P(out), M, N, K, O, epi, layout, typ, None, 0, None)


TYPES = pytest.mark.parametrize("typ", [HALF, BF16], ids=["fp16", "bf16"])


def test_symbol_is_declared_exported_and_typed(lib):
    src = open(os.path.join(ROOT, "include", "mixq.h")).read()
    declared = set(re.findall(r"MIXQ_API\s+[\w\s\*]+?\b(\w+)\s*\(", src))
    assert NAME in declared and NAME in _lib.SIGNATURES
    fn = getattr(lib, NAME)
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    # mixq_gemm_mixed_typed's arguments with `mul` in the bias's place and `epilogue` behind O
    b = list(_lib.SIGNATURES["mixq_gemm_mixed_typed"][1])
    assert list(argtypes) == b[:12] + [ctypes.c_int] + b[12:]
    assert re.search(r"mixq_gemm_mixed_act_typed\(const int8_t\* qA, const int8_t\* W, const void\* sA, const void\* sW,\s*const void\* fpA, "
                     r"const void\* fpW,\s*const void\* mul, void\* Out, int M, int N, int K, int O, int epilogue, int qa_layout, int type,\s*"
                     r"void\* scratch, size_t scratch_bytes, void\* stream\);", src)


def test_abi_revision_is_still_5(lib):
    src = open(os.path.join(ROOT, "include", "mixq.h")).read()
    assert re.search(r"^#define MIXQ_ABI_VERSION 5$", src, re.M)
    assert lib.mixq_abi_version() == 5 and _lib.ABI_VERSION == 5
    assert NAME in src[src.index("Revision 5 adds entries only"):src.index("#define MIXQ_ABI_VERSION")]


def test_a_bad_type_is_refused_before_everything_else(lib):
    for typ in (0, 2, 3, 6, 8, -1):
        assert act(lib, typ) == E_TYPE
        assert act(lib, typ, epi=7, M=-1, sa=0, layout=9, K=40, qa=Q + 8) == E_TYPE      # (every other refusal at once)
        assert act(lib, typ, M=0) == E_TYPE


@TYPES
def test_refusals_come_by_class_in_the_stated_order(lib, typ):
    # 2. MIXQ_E_BADARG
    for epi in (2, 4, 5, 6, 8, 9, -1):
        assert act(lib, typ, epi, mul=0) == BADARG and act(lib, typ, epi, mul=MUL) == BADARG
    assert act(lib, typ, SILU_MUL, mul=0) == BADARG                                   # 3 needs mul
    assert act(lib, typ, SILU, mul=MUL) == BADARG and act(lib, typ, PLAIN, mul=MUL) == BADARG   # 0 and 1 take none
    assert act(lib, typ, SILU_MUL, mul=OUT) == BADARG                                 # Out == mul
    for kw in (dict(qa=0), dict(w=0), dict(sa=0), dict(sw=0), dict(out=0), dict(fpa=0), dict(fpw=0)):
        assert act(lib, typ, SILU, **kw) == BADARG, kw
    assert act(lib, typ, SILU, O=0, fpa=0, fpw=0, qa=0) == BADARG
    for kw in (dict(M=-1), dict(N=-1), dict(K=0), dict(K=-16), dict(O=-8)):
        assert act(lib, typ, SILU, **kw) == BADARG, kw
    for layout in (2, 5, -1):
        assert act(lib, typ, SILU, layout=layout) == BADARG
    # 3. MIXQ_E_SHAPE
    for kw in (dict(K=40), dict(N=24), dict(O=12)):
        assert act(lib, typ, SILU, **kw) == SHAPE, kw
    assert act(lib, typ, SILU, O=136) == SHAPE and act(lib, typ, SILU_MUL, O=136) == SHAPE    # one LDS pass of outlier columns
    if typ == BF16:
        assert act(lib, typ, PLAIN, O=136) == SHAPE
    assert act(lib, typ, SILU, M=80, N=4096, K=4096, O=128, layout=1) == SHAPE        # fragment-major: the skinny kernel's shapes only
    assert act(lib, typ, SILU, M=16, N=4096, K=4096, O=136, layout=1) == SHAPE
    # 4. MIXQ_E_ALIGN
    for kw in (dict(qa=Q + 8), dict(w=W + 8), dict(out=OUT + 8), dict(sw=SW + 2), dict(fpa=FPA + 8), dict(fpw=FPW + 8)):
        assert act(lib, typ, SILU, **kw) == ALIGN, kw
    for off in (2, 4, 8):
        assert act(lib, typ, SILU_MUL, mul=MUL + off) == ALIGN                        # mul is fetched 16 bytes at a time, like Out
    # BADARG before SHAPE before ALIGN
    assert act(lib, typ, 7, K=40, qa=Q + 8) == BADARG
    assert act(lib, typ, SILU_MUL, mul=0, K=40, qa=Q + 8) == BADARG
    assert act(lib, typ, SILU_MUL, mul=OUT, O=136) == BADARG
    assert act(lib, typ, SILU, sa=0, K=40) == BADARG
    assert act(lib, typ, SILU, layout=7, O=136) == BADARG
    assert act(lib, typ, SILU_MUL, K=40, mul=MUL + 8) == SHAPE
    assert act(lib, typ, SILU, O=136, qa=Q + 8) == SHAPE
    assert act(lib, typ, SILU, M=80, N=4096, K=4096, O=128, layout=1, out=OUT + 8) == SHAPE


@TYPES
def test_an_empty_problem_is_ok_and_touches_nothing(lib, typ):
    for epi in (PLAIN, SILU, SILU_MUL):
        assert act(lib, typ, epi, M=0) == OK and act(lib, typ, epi, N=0) == OK
        assert act(lib, typ, epi, M=0, qa=0, w=0, sa=0, sw=0, fpa=0, fpw=0, out=0) == OK     # whatever the operands
        assert act(lib, typ, epi, M=0, layout=1) == OK
    assert act(lib, typ, SILU_MUL, M=0, mul=0) == BADARG                               # (the epilogue's own arguments are checked first)


def test_python_refusals():
    torch = pytest.importorskip("torch")
    from mixq_tensorrt_llm_amd import mixlib, plugin
    for dt, other in ((torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16)):
        q, Wq = torch.zeros((4, 64), dtype=torch.int8), torch.zeros((32, 64), dtype=torch.int8)
        xs, sw = torch.zeros(4, dtype=dt), torch.zeros(32, dtype=torch.float16)
        outl, fpw = torch.zeros((4, 8), dtype=dt), torch.zeros((32, 8), dtype=dt)
        mul, bias = torch.zeros((4, 32), dtype=dt), torch.zeros(32, dtype=dt)

        def gm(**kw):
            return mixlib.gemm_mixed(q, Wq, xs, sw, outl, fpw, 4, 32, 64, **kw)

        with pytest.raises(ValueError, match="bias"):
            gm(act="silu", bias=bias)
        with pytest.raises(ValueError, match="mul"):
            gm(mul=mul)
        with pytest.raises(ValueError, match="act"):
            gm(act="gelu")
        with pytest.raises(TypeError, match="mul"):
            gm(act="silu", mul=mul.to(other))
        with pytest.raises(ValueError, match="mul"):
            gm(act="silu", mul=mul[:3])
        with pytest.raises(ValueError, match="mul"):
            gm(act="silu", mul=mul, out=mul)
        for kw in (dict(act="silu"), dict(act="silu", mul=mul)):     # good arguments get as far as the device check: no CPU path
            with pytest.raises(_lib.MixQLibraryError):
                gm(**kw)

        layer = plugin.MixQLinear(64, 32, dtype=dt, device="cpu")
        with_bias = plugin.MixQLinear(64, 32, bias=True, dtype=dt, device="cpu")
        o128 = torch.zeros((4, 128), dtype=dt)
        with pytest.raises(ValueError, match="bias"):
            with_bias.forward_quantised(q, xs, o128, act="silu")
        with pytest.raises(ValueError, match="mul"):
            layer.forward_quantised(q, xs, o128, mul=mul)
        with pytest.raises(ValueError, match="act"):
            layer.forward_quantised(q, xs, o128, act="relu")
        if dt == torch.float16:
            sharded = plugin.MixQLinear(64, 64, tp_size=2, device="cpu")
            with pytest.raises(ValueError, match="tp_size"):
                sharded.forward_quantised(q, xs, o128, act="silu")
        with pytest.raises(_lib.MixQLibraryError):
            layer.forward_quantised(q, xs, o128, act="silu", mul=mul)

        # MixQLlamaMLP: one producer pass feeds gate and up
        def lin(i=64, o=32, **kw):
            kw.setdefault("dtype", dt)
            return plugin.MixQLinear(i, o, device="cpu", **kw)

        down = lin(32, 64)
        mlp = plugin.MixQLlamaMLP(lin(), lin(), down)
        assert mlp.gate.out_features == 32 and mlp.down is down
        with pytest.raises(ValueError, match="dtype"):
            plugin.MixQLlamaMLP(lin(), lin(dtype=other), down)
        with pytest.raises(ValueError, match="down"):
            plugin.MixQLlamaMLP(lin(), lin(), lin(32, 64, dtype=other))
        with pytest.raises(ValueError, match="in_features"):
            plugin.MixQLlamaMLP(lin(), lin(128, 32), down)
        with pytest.raises(ValueError, match="out_features"):
            plugin.MixQLlamaMLP(lin(), lin(64, 48), down)
        odd = lin()
        odd.fp_ind = odd.fp_ind.clone()
        odd.fp_ind.view(torch.int32)[5] = 7
        with pytest.raises(ValueError, match="fp_ind"):
            plugin.MixQLlamaMLP(lin(), odd, down)
        for g, u in ((lin(bias=True), lin()), (lin(), lin(bias=True))):
            with pytest.raises(ValueError, match="bias"):
                plugin.MixQLlamaMLP(g, u, down)
        if dt == torch.float16:
            for trio in ((lin(64, 64, tp_size=2), lin(), down), (lin(), lin(64, 64, tp_size=2), down), (lin(), lin(), lin(32, 128, tp_size=2))):
                with pytest.raises(ValueError, match="tp_size"):
                    plugin.MixQLlamaMLP(*trio)


@pytest.mark.parametrize("bf", [True, False], ids=["bf16", "fp16"])
def test_restatement_against_torch_cpu(bf):
    """tests/silu_restate.py on one small exact case and on the edges: the multiply is torch's multiply in T bit for bit; SiLU agrees
    with torch's fp32 silu rounded to T within one step of T; the ends of the range give signed zeros and v itself."""
    torch = pytest.importorskip("torch")
    import silu_restate as S
    dt = torch.bfloat16 if bf else torch.float16
    # line 1 on exact inputs: acc = 8 and 20, sW sA = 0.125 and 1, one outlier term each
    q = np.array([[3, -2, 1, 0] * 4], np.int8)
    Wq = np.array([[1, 1, 1, 1] * 4, [2, 0, -1, 5] * 4], np.int8)
    sA, sW = S.rn(np.array([0.5], np.float32), bf), np.array([0.25, 2.0], np.float16)
    fpA, fpW = S.rn(np.array([[3.0, 5.0]], np.float32), bf), S.rn(np.array([[2.0, 0.0], [0.0, -0.5]], np.float32), bf)
    v = S.pre_activation(q, sA, fpA, Wq, sW, fpW, bf)
    assert v.dtype == np.float32 and np.array_equal(v, np.array([[8 * 0.125 + 6.0, 20 * 1.0 - 2.5]], np.float32))
    assert np.array_equal(S.pre_activation(q, sA, None, Wq, sW, None, bf), np.array([[1.0, 20.0]], np.float32))
    # line 2 against torch
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(4096, generator=g) * 6).float()
    want = torch.nn.functional.silu(x).to(dt).view(torch.int16).numpy().view(np.uint16)
    got = S.silu_bits(x.numpy(), bf)
    assert S.ulp_steps(got, want).max() <= 1 and (got != want).mean() < 1e-3
    big = 3e38 if bf else 6e4
    edge = np.array([0.0, -0.0, 1e20, -1e20, big, -big, 1e-30, -1e-30], np.float32)
    e = S.silu_bits(edge, bf)
    assert np.array_equal(e[:2], [0x0000, 0x8000]) and e[3] == 0x8000 and e[5] == 0x8000
    assert np.array_equal(e[[2, 4]], S.rn(edge[[2, 4]], bf)) and np.array_equal(e[6:], S.rn(edge[6:] / 2, bf))
    # line 4 against torch's multiply in T, special values included
    rng = np.random.default_rng(4)
    a = rng.integers(0, 1 << 16, 1 << 16).astype(np.uint16)
    b = np.arange(1 << 16, dtype=np.uint16)
    rng.shuffle(b)
    m, t = S.mul_bits(a, b, bf), S.torch_mul_bits(a, b, bf)
    nan = S.is_nan(t, bf)
    assert np.array_equal(S.is_nan(m, bf), nan) and np.array_equal(m[~nan], t[~nan])
    assert np.array_equal(S.ordinal(np.array([0x0000, 0x8000, 0x0001, 0x8001], np.uint16)), [0, 0, 1, -1])
    # the fp16 quantiser twin: scale = fp16(amax / 127), saturating round half to even
    A = S.rn(np.array([[127.0, -63.5, 0.5, 1.5], [0.0, 0.0, 0.0, 0.0]], np.float32), bf)
    qq, ss = S.quant_rows(A, bf)
    assert np.array_equal(qq[0], [127, -64, 0, 2]) and ss[0] == S.rn(np.array([1.0], np.float32), bf)[0]
