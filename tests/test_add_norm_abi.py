"""CPU: the residual-add forms of the RMSNorm producer (mixq_add_rmsnorm, mixq_add_rmsnorm_extract_quant_layout,
mixq_add_rmsnorm_extract_quant4) are exported, typed and declared, leave the ABI revision at 5, and refuse bad arguments with the
codes of the entries they extend -- before anything is launched, so none of this needs a device (dummy integers stand in for
pointers, as in test_abi.test_enqueue_rejects_bad_arguments_without_touching_the_gpu)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

from mixq_tensorrt_llm_amd import _lib

OK, BADARG, SHAPE, ALIGN = 0, 1, 2, 3
NAMES = ("mixq_add_rmsnorm", "mixq_add_rmsnorm_extract_quant_layout", "mixq_add_rmsnorm_extract_quant4")
EPS = ctypes.c_float(1e-5)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def P(v):
    return ctypes.c_void_p(v)


A = [0x10000 + 0x1000 * i for i in range(10)]     # ten distinct 16-byte aligned "pointers"
X, R, H, G, OUT, IND, OUTL, Q, SC = A[:9]


def plain(lib, M, K, x=X, r=R, h=H, g=G, out=OUT):
    return lib.mixq_add_rmsnorm(M, K, P(x), P(r), P(h), P(g), P(out), EPS, None)


def quant8(lib, M, K, x=X, r=R, h=H, g=G, out=OUT, q=Q, layout=0, n_out=8):
    return lib.mixq_add_rmsnorm_extract_quant_layout(M, K, P(x), P(r), P(h), P(g), P(out), EPS, P(IND), n_out, P(OUTL), P(q), P(SC),
                                                     layout, None)


def quant4(lib, M, K, x=X, r=R, h=H, g=G, out=OUT, q=Q, n_out=8):
    return lib.mixq_add_rmsnorm_extract_quant4(M, K, P(x), P(r), P(h), P(g), P(out), EPS, P(IND), n_out, P(OUTL), P(q), P(SC), None)


ENTRIES = [plain, quant8, quant4]


def test_symbols_are_declared_exported_and_typed(lib):
    src = open(os.path.join(ROOT, "include", "mixq.h")).read()
    declared = set(re.findall(r"MIXQ_API\s+[\w\s\*]+?\b(\w+)\s*\(", src))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/mixq.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        fn = getattr(lib, name)
        restype, argtypes = _lib.SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    # x, residual, h in front of gamma; everything else in the order of the entry each one extends
    for name, base in zip(NAMES, ("mixq_rmsnorm", "mixq_rmsnorm_extract_quant_layout", "mixq_rmsnorm_extract_quant4")):
        b = list(_lib.SIGNATURES[base][1])
        assert list(_lib.SIGNATURES[name][1]) == b[:3] + [ctypes.c_void_p, ctypes.c_void_p] + b[3:], name


def test_abi_revision_is_still_5(lib):
    src = open(os.path.join(ROOT, "include", "mixq.h")).read()
    assert re.search(r"^#define MIXQ_ABI_VERSION 5$", src, re.M)
    assert lib.mixq_abi_version() == 5


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda f: f.__name__)
def test_refusals_without_a_device(lib, entry):
    # an empty problem is fine, whatever the pointers
    assert entry(lib, 0, 64) == OK
    assert entry(lib, 0, 64, x=0, r=0, h=0, out=0) == OK
    # null or negative arguments
    assert entry(lib, 4, 64, r=0) == BADARG
    assert entry(lib, 4, 64, h=0) == BADARG
    assert entry(lib, 4, 64, x=0) == BADARG
    assert entry(lib, -1, 64) == BADARG
    assert entry(lib, 4, 0) == BADARG
    # h may be x or residual, never the normalised row
    assert entry(lib, 4, 64, h=OUT) == BADARG
    # rows of whole 16-byte vectors, up to 32768 elements
    assert entry(lib, 4, 12) == SHAPE
    assert entry(lib, 4, 32776) == SHAPE
    # x, residual and h are read and written 16 bytes at a time
    assert entry(lib, 4, 64, r=R + 2) == ALIGN
    assert entry(lib, 4, 64, r=R + 8) == ALIGN
    assert entry(lib, 4, 64, h=H + 2) == ALIGN
    assert entry(lib, 4, 64, h=H + 8) == ALIGN
    assert entry(lib, 4, 64, x=X + 8) == ALIGN
    # the order of the entries they extend: BADARG before SHAPE before ALIGN
    assert entry(lib, 4, 12, r=0) == BADARG
    assert entry(lib, 4, 12, r=R + 2) == SHAPE


def test_quantising_entries_check_outlier_arguments_and_q(lib):
    assert lib.mixq_add_rmsnorm_extract_quant_layout(4, 64, P(X), P(R), P(H), P(G), P(OUT), EPS, None, 8, P(OUTL), P(Q), P(SC), 0,
                                                     None) == BADARG
    assert lib.mixq_add_rmsnorm_extract_quant4(4, 64, P(X), P(R), P(H), P(G), P(OUT), EPS, P(IND), 8, None, P(Q), P(SC), None) == BADARG
    assert quant8(lib, 4, 64, n_out=-1) == BADARG and quant4(lib, 4, 64, n_out=-1) == BADARG
    assert quant8(lib, 4, 64, q=0) == BADARG and quant4(lib, 4, 64, q=0) == BADARG
    # q: 8 bytes row-major, 16 bytes as a fragment-major image, 4 bytes packed int4 -- the existing rules
    assert quant8(lib, 4, 64, q=Q + 4) == ALIGN
    assert quant8(lib, 16, 2048, q=Q + 8, layout=1) == ALIGN
    assert quant4(lib, 4, 64, q=Q + 2) == ALIGN


def test_layout_argument(lib):
    # the fragment-major image exists for 1..64 rows and 1024 < K <= 16384 only
    assert quant8(lib, 65, 4096, layout=1) == SHAPE
    assert quant8(lib, 16, 1024, layout=1) == SHAPE
    assert quant8(lib, 65, 1024, layout=1) == SHAPE
    assert quant8(lib, 0, 4096, layout=1) == OK               # an empty problem is fine in either layout
    # there are two layouts
    assert quant8(lib, 16, 4096, layout=7) == BADARG
    assert quant8(lib, 0, 4096, layout=7) == BADARG
    assert quant8(lib, 16, 4096, layout=-1) == BADARG


def test_python_wrappers_refuse_mismatched_operands():
    """mixlib.add_layernorm_forward_cuda*: x, residual and h_out of one shape, fp16, contiguous -- a ValueError, not a bad pointer
    (raised before anything is handed to the library, so CPU tensors do here)."""
    torch = pytest.importorskip("torch")
    from mixq_tensorrt_llm_amd import mixlib
    f16 = torch.float16
    x, gamma, out = torch.zeros((4, 64), dtype=f16), torch.ones(64, dtype=f16), torch.empty((4, 64), dtype=f16)
    ind, sc = torch.zeros(8, dtype=torch.int32), torch.empty((4, 1), dtype=f16)
    calls = [lambda r, **kw: mixlib.add_layernorm_forward_cuda(x, r, gamma, out, 1e-6, **kw),
             lambda r, **kw: mixlib.add_layernorm_forward_cuda_extract_outliers(x, r, gamma, out, 1e-6, ind, sc, **kw),
             lambda r, **kw: mixlib.add_layernorm_forward_cuda_extract_outliers_int4(x, r, gamma, out, 1e-6, ind, sc, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="shape"):
            call(torch.zeros((2, 64), dtype=f16))
        with pytest.raises(ValueError, match="fp16"):
            call(torch.zeros((4, 64), dtype=torch.float32))
        with pytest.raises(ValueError, match="contiguous"):
            call(torch.zeros((64, 4), dtype=f16).t())
        with pytest.raises(ValueError, match="shape"):
            call(torch.zeros((4, 64), dtype=f16), h_out=torch.zeros((4, 32), dtype=f16))
        with pytest.raises(ValueError, match="fp16"):
            call(torch.zeros((4, 64), dtype=f16), h_out=torch.zeros((4, 64), dtype=torch.bfloat16))
