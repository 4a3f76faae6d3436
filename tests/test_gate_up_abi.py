"""CPU: mixq_gemm_mixed_gate_up_typed (the merged gate / up projection: one GEMM launch with a SiLU x up epilogue) is exported, typed and
declared, leaves the ABI revision at 5 and refuses bad arguments by class -- type, arguments, shapes, alignment, in that order -- before
anything is launched, so none of this needs a device (dummy integers stand in for pointers, as in test_silu_epilogue_abi).  Also: the
Python refusals of mixlib.gemm_gate_up and MixQLlamaMLP.fuse_gate_up on CPU tensors and mixed dtypes."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

from mixq_tensorrt_llm_amd import _lib

OK, BADARG, SHAPE, ALIGN, E_TYPE = 0, 1, 2, 3, 7
HALF, BF16 = _lib.MIXQ_TYPE_HALF, _lib.MIXQ_TYPE_BF16
NAME = "mixq_gemm_mixed_gate_up_typed"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def P(v):
    return ctypes.c_void_p(v)


Q, W, SA, SW, FPA, FPW, OUT = [0x10000 + 0x1000 * i for i in range(7)]     # distinct 16-byte aligned "pointers"


def gu(lib, typ, M=16, N=32, K=64, O=8, qa=Q, w=W, sa=SA, sw=SW, fpa=FPA, fpw=FPW, out=OUT, layout=0):
    return lib.mixq_gemm_mixed_gate_up_typed(P(qa), P(w), P(sa), P(sw), P(fpa), P(fpw), P(out), M, N, K, O, layout, typ, None, 0, None)


TYPES = pytest.mark.parametrize("typ", [HALF, BF16], ids=["fp16", "bf16"])


def test_symbol_is_declared_exported_and_typed(lib):
    src = open(os.path.join(ROOT, "include", "mixq.h")).read()
    declared = set(re.findall(r"MIXQ_API\s+[\w\s\*]+?\b(\w+)\s*\(", src))
    assert NAME in declared and NAME in _lib.SIGNATURES
    fn = getattr(lib, NAME)
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    # mixq_gemm_mixed_typed's arguments without the bias
    b = list(_lib.SIGNATURES["mixq_gemm_mixed_typed"][1])
    assert list(argtypes) == b[:6] + b[7:] and restype is ctypes.c_int
    assert re.search(r"int mixq_gemm_mixed_gate_up_typed\(const int8_t\* qA, const int8_t\* W2, const void\* sA, const void\* sW2, const void\* fpA,\s*"
                     r"const void\* fpW2, void\* Out, int M, int N, int K, int O, int qa_layout, int type,\s*"
                     r"void\* scratch, size_t scratch_bytes, void\* stream\);", src)
    assert "16 * (n / 8) + (n % 8)" in src                         # the layout is written into the header


def test_abi_revision_is_still_5(lib):
    src = open(os.path.join(ROOT, "include", "mixq.h")).read()
    assert re.search(r"^#define MIXQ_ABI_VERSION 5$", src, re.M)
    assert lib.mixq_abi_version() == 5 and _lib.ABI_VERSION == 5
    assert NAME in src[src.index("Revision 5 adds entries only"):src.index("#define MIXQ_ABI_VERSION")]


def test_a_bad_type_is_refused_before_everything_else(lib):
    for typ in (0, 2, 3, 6, 8, -1):
        assert gu(lib, typ) == E_TYPE
        assert gu(lib, typ, M=-1, sa=0, layout=9, K=40, N=24, O=136, qa=Q + 8) == E_TYPE      # (every other refusal at once)
        assert gu(lib, typ, M=0) == E_TYPE and gu(lib, typ, N=0) == E_TYPE


@TYPES
def test_refusals_come_by_class_in_the_stated_order(lib, typ):
    # 2. MIXQ_E_BADARG
    for kw in (dict(qa=0), dict(w=0), dict(sa=0), dict(sw=0), dict(out=0), dict(fpa=0), dict(fpw=0)):
        assert gu(lib, typ, **kw) == BADARG, kw
    assert gu(lib, typ, O=0, fpa=0, fpw=0, qa=0) == BADARG
    for kw in (dict(M=-1), dict(N=-1), dict(N=-16), dict(K=0), dict(K=-16), dict(O=-8), dict(N=2 ** 30)):
        assert gu(lib, typ, **kw) == BADARG, kw
    for layout in (2, 5, -1):
        assert gu(lib, typ, layout=layout) == BADARG
    # 3. MIXQ_E_SHAPE
    for kw in (dict(K=40), dict(N=24), dict(N=8), dict(N=40), dict(O=12), dict(O=136)):
        assert gu(lib, typ, **kw) == SHAPE, kw
    assert gu(lib, typ, M=80, N=2048, K=4096, O=128, layout=1) == SHAPE            # fragment-major: the skinny kernel's shapes only
    assert gu(lib, typ, M=16, N=2048, K=4096, O=136, layout=1) == SHAPE
    # 4. MIXQ_E_ALIGN
    for kw in (dict(qa=Q + 8), dict(w=W + 8), dict(out=OUT + 8), dict(sw=SW + 2), dict(fpa=FPA + 8), dict(fpw=FPW + 8)):
        assert gu(lib, typ, **kw) == ALIGN, kw
    assert gu(lib, typ, O=0, fpa=0, fpw=0, out=OUT + 4) == ALIGN
    # BADARG before SHAPE before ALIGN
    assert gu(lib, typ, sa=0, K=40) == BADARG and gu(lib, typ, layout=7, O=136) == BADARG and gu(lib, typ, M=-1, N=24, qa=Q + 8) == BADARG
    assert gu(lib, typ, K=40, qa=Q + 8) == SHAPE and gu(lib, typ, N=24, out=OUT + 8) == SHAPE and gu(lib, typ, O=136, w=W + 8) == SHAPE
    assert gu(lib, typ, M=80, N=2048, K=4096, O=128, layout=1, out=OUT + 8) == SHAPE


@TYPES
def test_an_empty_problem_is_ok_and_touches_nothing(lib, typ):
    assert gu(lib, typ, M=0) == OK and gu(lib, typ, N=0) == OK
    assert gu(lib, typ, M=0, qa=0, w=0, sa=0, sw=0, fpa=0, fpw=0, out=0) == OK     # whatever the operands
    assert gu(lib, typ, N=0, qa=0, w=0, sa=0, sw=0, fpa=0, fpw=0, out=0, K=40) == OK
    assert gu(lib, typ, M=0, layout=1) == OK
    assert gu(lib, typ, M=0, layout=3) == BADARG and gu(lib, typ, M=0, K=0) == BADARG   # (values are checked before emptiness)


def test_python_refusals():
    torch = pytest.importorskip("torch")
    from mixq_tensorrt_llm_amd import mixlib, plugin
    for dt, other in ((torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16)):
        q, W2 = torch.zeros((4, 64), dtype=torch.int8), torch.zeros((64, 64), dtype=torch.int8)
        xs, sw2 = torch.zeros(4, dtype=dt), torch.zeros(64, dtype=torch.float16)
        outl, fpw2 = torch.zeros((4, 8), dtype=dt), torch.zeros((64, 8), dtype=dt)

        def gg(**kw):
            a = dict(q=q, W2=W2, x_scale=xs, sW2=sw2, outliers=outl, fpW2=fpw2)
            a.update(kw)
            return mixlib.gemm_gate_up(a["q"], a["W2"], a["x_scale"], a["sW2"], a["outliers"], a["fpW2"], 4, 32, 64, **{k: v for k, v in kw.items() if k in ("out", "qa_layout")})

        with pytest.raises(TypeError, match="x_scale"):
            gg(x_scale=xs.to(other))
        with pytest.raises(TypeError, match="fpW2"):
            gg(fpW2=fpw2.to(other))
        with pytest.raises(TypeError, match="out"):
            gg(out=torch.zeros((4, 32), dtype=other))
        with pytest.raises(TypeError, match="fp16 and bf16"):
            gg(outliers=outl.float())
        with pytest.raises(TypeError, match="sW2"):
            gg(sW2=sw2.to(torch.bfloat16))
        with pytest.raises(TypeError, match="int8"):
            gg(W2=W2.to(torch.int16))
        with pytest.raises(_lib.MixQLibraryError):                 # good arguments get as far as the device check: no CPU path
            gg()
        with pytest.raises(_lib.MixQLibraryError):
            gg(outliers=None, fpW2=None)

        def lin(i=64, o=32, **kw):
            kw.setdefault("dtype", dt)
            return plugin.MixQLinear(i, o, device="cpu", **kw)

        mlp = plugin.MixQLlamaMLP(lin(), lin(), lin(32, 64))
        assert mlp._gate_up is None and mlp.fuse_gate_up(False) is mlp
        with pytest.raises(_lib.MixQLibraryError, match="CPU"):
            mlp.fuse_gate_up()
        assert mlp._gate_up is None                                 # a refused call leaves the class as it was: two launches
        mixed = plugin.MixQLlamaMLP(lin(), lin(), lin(32, 64))
        mixed.up.fp_weight = mixed.up.fp_weight.to(other)
        with pytest.raises((TypeError, _lib.MixQLibraryError)):
            mixed.fuse_gate_up()
