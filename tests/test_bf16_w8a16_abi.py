"""CPU: mixq_w8a16_gemm_forward_typed / mixq_w8a16_gemm_workspace_size_typed (the weight-only GEMM on fp16 or bf16 rows) are declared,
exported and typed, leave the ABI revision at 5 and refuse bad arguments in the documented order before anything is launched, so none
of this needs a device: distinct 16-byte aligned integers stand in for pointers, as in test_silu_epilogue_abi, and every call here
either is refused or is an empty problem.  (The two steps of the order that lie behind a launch -- the GEMV route of 1..4 tokens, which
does not check the output's alignment, and the misaligned workspace that is ignored -- are covered on the GPU, test_gpu_bf16_w8a16.)
Also: the workspace sizes of both types, and the Python refusals of mixlib.w8_a16_gemm / EETQ.w8_a16_gemm on CPU tensors."""
import ctypes
import itertools
import os
import re

import pytest

from conftest import ROOT

from mixq_tensorrt_llm_amd import _lib
import w8a16_bf16_cases as C

OK, BADARG, SHAPE, ALIGN, E_TYPE = 0, 1, 2, 3, 7
HALF, BF16 = _lib.MIXQ_TYPE_HALF, _lib.MIXQ_TYPE_BF16
FWD, SIZE = "mixq_w8a16_gemm_forward_typed", "mixq_w8a16_gemm_workspace_size_typed"
A, W, S, OUT, WS = [0x10000 + 0x1000 * i for i in range(5)]     # distinct 16-byte aligned "pointers"
TYPES = pytest.mark.parametrize("typ", [HALF, BF16], ids=["fp16", "bf16"])


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def P(v):
    return ctypes.c_void_p(v)


def fwd(lib, typ, m=8, n=32, k=64, a=A, w=W, s=S, out=OUT, ws=0, ws_bytes=0):
    return lib.mixq_w8a16_gemm_forward_typed(P(a), P(w), P(s), P(out), m, n, k, typ, P(ws), ws_bytes, None)


def fwd_named(lib, m=8, n=32, k=64, a=A, w=W, s=S, out=OUT, ws=0, ws_bytes=0):
    return lib.mixq_w8a16_gemm_forward_ws(P(a), P(w), P(s), P(out), m, n, k, P(ws), ws_bytes, None)


def test_symbols_are_declared_exported_and_typed(lib):
    src = open(os.path.join(ROOT, "include", "mixq.h")).read()
    declared = set(re.findall(r"MIXQ_API\s+[\w\s\*]+?\b(\w+)\s*\(", src))
    for name in (FWD, SIZE):
        assert name in declared and name in _lib.SIGNATURES
        fn = getattr(lib, name)
        restype, argtypes = _lib.SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    # the named entries' arguments with `type` behind k
    b = list(_lib.SIGNATURES["mixq_w8a16_gemm_forward_ws"][1])
    assert list(_lib.SIGNATURES[FWD][1]) == b[:7] + [ctypes.c_int] + b[7:]
    assert list(_lib.SIGNATURES[SIZE][1]) == list(_lib.SIGNATURES["mixq_w8a16_gemm_workspace_size"][1]) + [ctypes.c_int]
    assert _lib.SIGNATURES[SIZE][0] is ctypes.c_size_t
    assert re.search(r"size_t mixq_w8a16_gemm_workspace_size_typed\(int m, int n, int k, int type\);", src)
    assert re.search(r"int mixq_w8a16_gemm_forward_typed\(const void\* input, const uint8_t\* weight, const void\* scale_f16,\s*void\* output, "
                     r"int m, int n,\s*int k, int type,\s*void\* workspace, size_t workspace_bytes, void\* stream\);", src)


def test_abi_revision_is_still_5(lib):
    src = open(os.path.join(ROOT, "include", "mixq.h")).read()
    assert re.search(r"^#define MIXQ_ABI_VERSION 5$", src, re.M)
    assert lib.mixq_abi_version() == 5 and _lib.ABI_VERSION == 5
    comment = src[src.index("Revision 5 adds entries only"):src.index("#define MIXQ_ABI_VERSION")]
    assert FWD in comment and SIZE in comment


def test_a_bad_type_is_refused_before_everything_else(lib):
    for typ in (0, 2, 3, 6, 8, -1):
        assert fwd(lib, typ) == E_TYPE
        assert fwd(lib, typ, m=-1, n=3, k=40, a=0, w=W + 8, out=OUT + 2) == E_TYPE      # (every other refusal at once)
        assert fwd(lib, typ, m=0) == E_TYPE
        assert lib.mixq_w8a16_gemm_workspace_size_typed(2048, 8192, 4096, typ) == 0


@TYPES
def test_refusals_come_in_the_stated_order(lib, typ):
    # 1. m < 0 || n < 0 || k <= 0: MIXQ_E_BADARG, before the empty problem
    for kw in (dict(m=-1), dict(n=-2), dict(k=0), dict(k=-64), dict(m=0, k=0), dict(n=0, m=-1)):
        assert fwd(lib, typ, **kw) == BADARG, kw
    # 2. m == 0 || n == 0: MIXQ_OK, before the pointers, the shape and the alignment are looked at
    assert fwd(lib, typ, m=0) == OK and fwd(lib, typ, n=0) == OK
    assert fwd(lib, typ, m=0, a=0, w=0, s=0, out=0, k=40, n=3) == OK
    assert fwd(lib, typ, n=0, a=A + 8, k=40) == OK
    # 3. null pointers: MIXQ_E_BADARG, before the shape
    for kw in (dict(a=0), dict(w=0), dict(s=0), dict(out=0)):
        assert fwd(lib, typ, **kw) == BADARG, kw
        assert fwd(lib, typ, k=40, n=3, **kw) == BADARG, kw
    # 4. k % 64 || n % 2: MIXQ_E_SHAPE, before the alignment
    for kw in (dict(k=40), dict(k=96), dict(n=3), dict(n=33)):
        assert fwd(lib, typ, **kw) == SHAPE, kw
        assert fwd(lib, typ, a=A + 8, w=W + 4, out=OUT + 2, **kw) == SHAPE, kw
    # 5. input or weight not 16-byte aligned: MIXQ_E_ALIGN (at every m: before the route of 1..4 tokens is chosen)
    for m in (1, 4, 5, 300):
        for kw in (dict(a=A + 8), dict(a=A + 2), dict(w=W + 8), dict(w=W + 1)):
            assert fwd(lib, typ, m=m, **kw) == ALIGN, (m, kw)
    # 7. the output: four values of a row leave at once -- 8-byte aligned where n % 4 == 0, 4-byte aligned where n % 4 == 2
    for m in (5, 64, 300):
        for off in (2, 4, 6, 12):
            assert fwd(lib, typ, m=m, n=32, out=OUT + off) == ALIGN, (m, off)
        for off in (2, 6, 10):
            assert fwd(lib, typ, m=m, n=34, out=OUT + off) == ALIGN, (m, off)
    # ... and on the skinny route of 1..4 tokens as well (8192 columns and more: w8a16_skinny_takes)
    assert fwd(lib, typ, m=2, n=8192, k=64, out=OUT + 4) == ALIGN


def test_half_through_the_typed_entry_is_the_named_entry(lib):
    grid = dict(m=(-1, 0, 3, 8), n=(-2, 0, 3, 32), k=(0, 40, 64), a=(0, A, A + 8), w=(0, W, W + 8), s=(0, S), out=(0, OUT, OUT + 4, OUT + 2))
    launched = 0
    for vals in itertools.product(*grid.values()):
        kw = dict(zip(grid.keys(), vals))
        good = kw["m"] > 0 and kw["n"] > 0 and kw["n"] % 2 == 0 and kw["k"] == 64 and kw["a"] == A and kw["w"] == W and kw["s"] and kw["out"]
        if good and (kw["m"] <= 4 or kw["out"] == OUT):     # (would launch: nothing here may reach a kernel)
            launched += 1
            continue
        assert fwd(lib, HALF, **kw) == fwd_named(lib, **kw), kw
    assert launched > 0
    for shape in [(2048, 8192, 4096), (5, 2, 64), (300, 1026, 1600), (1, 4096, 4096), (4, 12288, 4096), (0, 32, 64), (8, 0, 64), (8, 32, 0)]:
        assert lib.mixq_w8a16_gemm_workspace_size_typed(*shape, HALF) == lib.mixq_w8a16_gemm_workspace_size(*shape), shape


def test_workspace_sizes(lib):
    m, n, k = 2048, 8192, 4096
    assert lib.mixq_w8a16_gemm_workspace_size_typed(m, n, k, HALF) >= 16384 + n * k * 2     # the two-pass form's weight image
    assert lib.mixq_w8a16_gemm_workspace_size_typed(m, n, k, BF16) < n * k * 2              # never: the wide form's K split at most
    # automatic plans of the GPU tests' shapes: no fp16 call of them goes two-pass, so both types ask for the same scratch
    for (m, n, k) in C.RAGGED + C.SPLIT_K + [(20, 640, 1088), (300, 1032, 1600)]:
        h, b = (lib.mixq_w8a16_gemm_workspace_size_typed(m, n, k, t) for t in (HALF, BF16))
        assert m < 1280, (m, n, k)                      # (the two-pass form starts at 1280 tokens: none of these plans it)
        assert h == b, (m, n, k)
    for m in (1, 2, 3, 4):
        for (n, k) in ((512, 4096), (12288, 4096), (130, 192)):
            assert lib.mixq_w8a16_gemm_workspace_size_typed(m, n, k, HALF) == 0 == lib.mixq_w8a16_gemm_workspace_size_typed(m, n, k, BF16)


def test_python_refusals_on_cpu_tensors():
    torch = pytest.importorskip("torch")
    import EETQ
    from mixq_tensorrt_llm_amd import mixlib
    w = torch.zeros((64, 32), dtype=torch.uint8)
    for op in (mixlib.w8_a16_gemm, EETQ.w8_a16_gemm):
        with pytest.raises(TypeError, match="scale"):
            op(torch.zeros((8, 64), dtype=torch.bfloat16), w, torch.ones(32, dtype=torch.bfloat16))
        with pytest.raises(_lib.MixQLibraryError) as fp16:
            op(torch.zeros((8, 64), dtype=torch.float16), w, torch.ones(32, dtype=torch.float16))
        with pytest.raises(_lib.MixQLibraryError) as bf16:
            op(torch.zeros((8, 64), dtype=torch.bfloat16), w, torch.ones(32, dtype=torch.float16))
        assert str(bf16.value) == str(fp16.value)
