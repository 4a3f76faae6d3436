"""CPU: the C ABI of the layer bias in the operator's epilogue (mixq_enqueue_bias, mixq_enqueue_tp_bias, mixq_gemm_mixed_bias;
include/mixq.h revision 5).  Exported and typed, argument validation returns codes before anything touches the device, and the
headers still compile as C99 / C++11 with a host that calls the new entries.  The arithmetic is checked on the GPU
(tests/test_gpu_bias_epilogue.py)."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

OK, BADARG, SHAPE, ALIGN, WORKSPACE = 0, 1, 2, 3, 5
NEW = ("mixq_enqueue_bias", "mixq_enqueue_tp_bias", "mixq_gemm_mixed_bias")


@pytest.fixture(scope="module")
def lib():
    from mixq_tensorrt_llm_amd import _lib
    return _lib.load()


@pytest.fixture
def ptrs():
    buf = (ctypes.c_char * 8192)()
    base = (ctypes.addressof(buf) + 15) & ~15
    yield buf, ctypes.c_void_p(base), ctypes.c_void_p(base + 2)


def test_new_entries_are_exported_typed_and_versioned(lib):
    from mixq_tensorrt_llm_amd import _lib
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, name
    assert len(lib.mixq_enqueue_bias.argtypes) == 8
    assert len(lib.mixq_enqueue_tp_bias.argtypes) == 7
    assert len(lib.mixq_gemm_mixed_bias.argtypes) == 15
    assert lib.mixq_abi_version() == _lib.ABI_VERSION == 5
    header = open(os.path.join(ROOT, "include", "mixq.h")).read()
    assert "#define MIXQ_ABI_VERSION 5" in header
    for name in NEW:
        assert f"MIXQ_API int {name}(" in header, name
    assert "enqueueWithBias" in open(os.path.join(ROOT, "include", "mixq_plugin.hpp")).read()


def _descs(M, N, K):
    from mixq_tensorrt_llm_amd._lib import TensorDesc
    shapes = [(M, K), (N, K // 2), (N,), (N, 128), (256,), (K, N // 2), (N,)]
    return (TensorDesc * 7)(*[TensorDesc.make(s) for s in shapes])


def test_enqueue_bias_validates_like_enqueue(lib, ptrs):
    _, p16, odd = ptrs
    h = lib.mixq_create(0, 0, 0)
    try:
        d = _descs(64, 512, 512)
        ins = (ctypes.c_void_p * 7)(*([p16] * 7))
        outs = (ctypes.c_void_p * 1)(p16)
        # misaligned bias: MIXQ_E_ALIGN before anything (even with a workspace missing, on both paths)
        assert lib.mixq_enqueue_bias(h, d, None, ins, outs, odd, None, None) == ALIGN
        assert lib.mixq_enqueue_bias(h, _descs(2, 512, 512), None, ins, outs, odd, None, None) == ALIGN
        # null handle / inputs / a null input pointer / no workspace: the codes of mixq_enqueue
        for args in ((None, d, None, ins, outs), (h, d, None, None, outs), (h, d, None, ins, None)):
            assert lib.mixq_enqueue_bias(*args, p16, p16, None) == lib.mixq_enqueue(*args, p16, None) == BADARG
        nul = (ctypes.c_void_p * 7)(*([p16] * 6 + [None]))
        assert lib.mixq_enqueue_bias(h, d, None, nul, outs, p16, p16, None) == lib.mixq_enqueue(h, d, None, nul, outs, p16, None) == BADARG
        assert lib.mixq_enqueue_bias(h, d, None, ins, outs, p16, None, None) == lib.mixq_enqueue(h, d, None, ins, outs, None, None) == WORKSPACE
        # K not a multiple of 8: MIXQ_E_SHAPE on both
        d60 = _descs(64, 512, 60)
        assert lib.mixq_enqueue_bias(h, d60, None, ins, outs, p16, p16, None) == lib.mixq_enqueue(h, d60, None, ins, outs, p16, None) == SHAPE
        # misaligned activations: MIXQ_E_ALIGN on both
        ins_odd = (ctypes.c_void_p * 7)(*([odd] + [p16] * 6))
        assert lib.mixq_enqueue_bias(h, d, None, ins_odd, outs, p16, p16, None) == lib.mixq_enqueue(h, d, None, ins_odd, outs, p16, None) == ALIGN
        # with a bias, N / K not multiples of 16 are refused before the quantiser runs
        assert lib.mixq_enqueue_bias(h, _descs(64, 520, 512), None, ins, outs, p16, p16, None) == SHAPE
        assert lib.mixq_enqueue_bias(h, _descs(64, 512, 520), None, ins, outs, p16, p16, None) == SHAPE
        # a misaligned weight / output with a bias: refused before the quantiser runs
        ins_w = (ctypes.c_void_p * 7)(*([p16, odd] + [p16] * 5))
        assert lib.mixq_enqueue_bias(h, d, None, ins_w, outs, p16, p16, None) == ALIGN
        assert lib.mixq_enqueue_bias(h, d, None, ins, (ctypes.c_void_p * 1)(odd), p16, p16, None) == ALIGN
        # decode rows (M <= 4) with a bias: K % 64 / N % 2 as the GEMV, alignment
        assert lib.mixq_enqueue_bias(h, _descs(2, 512, 96), None, ins, outs, p16, None, None) == SHAPE
        assert lib.mixq_enqueue_bias(h, _descs(2, 512, 512), None, ins_odd, outs, p16, None, None) == ALIGN
        # M = 0: nothing to do
        assert lib.mixq_enqueue_bias(h, _descs(0, 512, 512), None, ins, outs, p16, None, None) == OK
    finally:
        lib.mixq_destroy(h)


def test_enqueue_tp_bias_validates_like_enqueue_tp(lib, ptrs):
    from mixq_tensorrt_llm_amd._lib import TpEpilogue
    _, p16, odd = ptrs
    h = lib.mixq_create(0, 0, 0)
    try:
        ins = (ctypes.c_void_p * 7)(*([p16] * 7))
        tp = TpEpilogue()
        tp.ndst, tp.n_total, tp.col0, tp.seq = 2, 1024, 0, 1
        tp.dst_bases[0] = tp.dst_bases[1] = p16.value
        tp.dst_flags[0] = tp.dst_flags[1] = p16.value
        tp.counters = p16.value
        for M, N, K in ((64, 512, 512), (4096, 8, 3584), (4096, 512, 520)):   # few tiles / N % 16 / K % 16
            d = _descs(M, N, K)
            want = lib.mixq_enqueue_tp(h, d, ins, p16, ctypes.byref(tp), None)
            assert want in (SHAPE, BADARG)
            assert lib.mixq_enqueue_tp_bias(h, d, ins, p16, p16, ctypes.byref(tp), None) == want, (M, N, K)
        d = _descs(64, 512, 512)
        assert lib.mixq_enqueue_tp_bias(h, d, ins, p16, p16, None, None) == lib.mixq_enqueue_tp(h, d, ins, p16, None, None) == BADARG
        assert lib.mixq_enqueue_tp_bias(None, d, ins, p16, p16, ctypes.byref(tp), None) == BADARG
        # a shape the fused gather serves, with a misaligned bias: MIXQ_E_ALIGN, nothing launched
        assert lib.mixq_tp_fused_supported(4096, 2304, 3584) == 1
        tp.n_total = 4608
        d = _descs(4096, 2304, 3584)
        assert lib.mixq_enqueue_tp_bias(h, d, ins, odd, p16, ctypes.byref(tp), None) == ALIGN
        assert lib.mixq_enqueue_tp_bias(h, d, ins, p16, None, ctypes.byref(tp), None) == lib.mixq_enqueue_tp(h, d, ins, None, ctypes.byref(tp), None) == WORKSPACE
    finally:
        lib.mixq_destroy(h)


def test_gemm_mixed_bias_validates(lib, ptrs):
    _, p16, odd = ptrs
    f = lib.mixq_gemm_mixed_bias
    assert f(p16, p16, p16, p16, None, None, None, p16, 8, 64, 64, 0, None, 0, None) == BADARG      # no bias
    assert f(p16, p16, p16, p16, None, None, odd, p16, 8, 64, 64, 0, None, 0, None) == ALIGN        # misaligned bias
    assert f(p16, p16, p16, p16, None, None, p16, p16, 8, 64, 40, 0, None, 0, None) == SHAPE        # K % 16
    assert f(p16, p16, p16, p16, None, None, p16, p16, 8, 60, 64, 0, None, 0, None) == SHAPE        # N % 16
    assert f(odd, p16, p16, p16, None, None, p16, p16, 8, 64, 64, 0, None, 0, None) == ALIGN        # misaligned qA
    assert f(None, p16, p16, p16, None, None, p16, p16, 8, 64, 64, 0, None, 0, None) == BADARG      # null qA
    assert f(p16, p16, p16, p16, None, None, p16, p16, 8, 64, 64, 128, None, 0, None) == BADARG     # O > 0 without operands
    assert f(p16, p16, p16, p16, p16, p16, p16, p16, 8, 64, 64, 256, None, 0, None) == SHAPE        # O > 128
    assert f(p16, p16, p16, p16, None, None, p16, p16, 0, 64, 64, 0, None, 0, None) == OK           # empty problem


def test_headers_compile_with_a_host_that_calls_the_bias_entries(tmp_path):
    inc = os.path.join(ROOT, "include")
    c_src = tmp_path / "host.c"
    c_src.write_text("""#include "mixq.h"
int run(const mixq_handle* h, const mixq_tensor_desc* d, const void* const* in, void* const* out, const void* bias,
        void* ws, const mixq_tp_epilogue* tp, void* st)
{
    int rc = mixq_enqueue_bias(h, d, d, in, out, bias, ws, st);
    if (rc == MIXQ_OK) rc = mixq_enqueue_tp_bias(h, d, in, bias, ws, tp, st);
    if (rc == MIXQ_OK) rc = mixq_gemm_mixed_bias(0, 0, 0, 0, 0, 0, bias, 0, 0, 16, 16, 0, 0, 0, st);
    return rc + (MIXQ_ABI_VERSION == 5 ? 0 : 1);
}
""")
    cpp_src = tmp_path / "host.cpp"
    cpp_src.write_text("""#include "mixq_plugin.hpp"
int run(const mixq_plugin::MixQPlugin& p, const mixq_plugin::PluginTensorDesc* d, const void* const* in, void* const* out, const void* b, void* ws, void* st)
{
    return p.enqueueWithBias(d, d, in, out, b, ws, st);
}
""")
    for compiler, std, src in (("gcc", "-std=c99", c_src), ("g++", "-std=c++11", cpp_src)):
        r = subprocess.run([compiler, std, "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-fsyntax-only", str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, f"{compiler} {std}: {r.stderr}"
