"""CPU: the bf16 call of the MixQ operator at the ABI level (include/mixq.h MIXQ_TYPE_BF16, MIXQ_E_TYPE,
mixq_get_output_data_type_for), with no GPU -- type negotiation, the refusals that return before anything is launched, the headers
compiled into C and C++ hosts that use the new entry, and the numpy restatement (tests/bf16_restate.py) against float64."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import bf16_restate as R

HALF, BF16, FLOAT = 1, 7, 0


@pytest.fixture(scope="module")
def lib():
    from mixq_tensorrt_llm_amd import _lib
    return _lib.load()


def test_bf16_type_value_in_header_and_binding():
    from mixq_tensorrt_llm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mixq.h")).read()
    assert re.search(r"MIXQ_TYPE_BF16\s*=\s*7\b", hdr)
    assert re.search(r"MIXQ_E_TYPE\s*=\s*7\b", hdr)
    assert _lib.MIXQ_TYPE_BF16 == 7 and _lib.MIXQ_E_TYPE == 7
    assert re.search(r"#define MIXQ_ABI_VERSION 5\b", hdr)


def _descs(types):
    from mixq_tensorrt_llm_amd._lib import TensorDesc
    shapes = [(67, 4096), (512, 2048), (512,), (512, 128), (256,), (4096, 256), (512,), (67, 512)]
    return (TensorDesc * 8)(*[TensorDesc.make(s, t) for s, t in zip(shapes, types)])


def _expected(pos, types):
    t = types[pos]
    if pos == 0:
        return t in (HALF, BF16)
    if pos in (3, 7):
        return t == types[0] and t in (HALF, BF16)
    return t == HALF


def test_supports_format_combination_truth_table(lib):
    h = lib.mixq_create(67, 512, 4096)
    try:
        for a in (HALF, BF16, FLOAT):
            for fpw in (HALF, BF16, FLOAT):
                for out in (HALF, BF16, FLOAT):
                    for other in (HALF, BF16):
                        types = [a, other, other, fpw, other, other, other, out]
                        d = _descs(types)
                        for pos in range(8):
                            got = lib.mixq_supports_format_combination(h, pos, d, 7, 1)
                            assert got == int(_expected(pos, types)), (types, pos, got)
        d = _descs([HALF] * 8)   # the all-HALF answers of the reference
        assert [lib.mixq_supports_format_combination(h, p, d, 7, 1) for p in range(8)] == [1] * 8
        d[3].format = 1
        assert lib.mixq_supports_format_combination(h, 3, d, 7, 1) == 0
    finally:
        lib.mixq_destroy(h)


def test_output_data_type_for(lib):
    h = lib.mixq_create(1, 2, 3)
    try:
        for t0, want in ((BF16, BF16), (HALF, HALF), (FLOAT, HALF), (2, HALF)):
            types = (ctypes.c_int32 * 7)(t0, HALF, HALF, t0, HALF, HALF, HALF)
            assert lib.mixq_get_output_data_type_for(h, 0, types, 7) == want
        assert lib.mixq_get_output_data_type_for(h, 0, None, 0) == HALF
        assert lib.mixq_get_output_data_type(h, 0) == HALF   # the reference's entry is unchanged
    finally:
        lib.mixq_destroy(h)


def _fake_call(lib, types, M=67, out_type=None, entry="enqueue"):
    """Call an enqueue entry with pointers that are never dereferenced (the type checks come first)."""
    from mixq_tensorrt_llm_amd._lib import TensorDesc, TpEpilogue
    shapes = [(M, 4096), (512, 2048), (512,), (512, 128), (256,), (4096, 256), (512,)]
    d = (TensorDesc * 7)(*[TensorDesc.make(s, t) for s, t in zip(shapes, types)])
    fake = 1 << 20
    ins = (ctypes.c_void_p * 7)(*([fake] * 7))
    outs = (ctypes.c_void_p * 1)(fake)
    od = TensorDesc.make((M, 512), out_type if out_type is not None else types[0])
    h = lib.mixq_create(M, 512, 4096)
    try:
        if entry == "enqueue":
            return lib.mixq_enqueue(h, d, ctypes.byref(od), ins, outs, ctypes.c_void_p(fake), None)
        if entry == "bias":
            return lib.mixq_enqueue_bias(h, d, ctypes.byref(od), ins, outs, ctypes.c_void_p(fake), ctypes.c_void_p(fake), None)
        if entry == "profiled":
            return lib.mixq_enqueue_profiled(h, d, ctypes.byref(od), ins, outs, ctypes.c_void_p(fake), None, None, None)
        tp = TpEpilogue()
        tp.ndst, tp.n_total, tp.col0, tp.counters = 2, 1024, 0, fake
        if entry == "tp":
            return lib.mixq_enqueue_tp(h, d, ins, ctypes.c_void_p(fake), ctypes.byref(tp), None)
        return lib.mixq_enqueue_tp_bias(h, d, ins, ctypes.c_void_p(fake), ctypes.c_void_p(fake), ctypes.byref(tp), None)
    finally:
        lib.mixq_destroy(h)


@pytest.mark.parametrize("entry", ["enqueue", "bias", "profiled"])
@pytest.mark.parametrize("M", [67, 3])
def test_mixed_types_refused_before_launch(lib, entry, M):
    from mixq_tensorrt_llm_amd import _lib
    mixed = [BF16, HALF, HALF, HALF, HALF, HALF, HALF]          # bf16 A, fp16 fp_weight
    assert _fake_call(lib, mixed, M, entry=entry) == _lib.MIXQ_E_TYPE
    ok_in = [BF16, HALF, HALF, BF16, HALF, HALF, HALF]
    assert _fake_call(lib, ok_in, M, out_type=HALF, entry=entry) == _lib.MIXQ_E_TYPE   # fp16 output descriptor
    assert lib.mixq_error_string(_lib.MIXQ_E_TYPE).decode() == "descriptor types are not a supported combination"


@pytest.mark.parametrize("entry", ["tp", "tp_bias"])
def test_tp_entries_refuse_bf16(lib, entry):
    from mixq_tensorrt_llm_amd import _lib
    assert _fake_call(lib, [BF16, HALF, HALF, BF16, HALF, HALF, HALF], 4096, entry=entry) == _lib.MIXQ_E_TYPE


def test_headers_compile_with_a_host_that_negotiates_bf16(tmp_path):
    c = tmp_path / "t.c"
    c.write_text("""#include "mixq.h"
int probe(const mixq_handle* h, const mixq_tensor_desc* io) {
    int32_t types[7] = {MIXQ_TYPE_BF16, MIXQ_TYPE_HALF, MIXQ_TYPE_HALF, MIXQ_TYPE_BF16, MIXQ_TYPE_HALF, MIXQ_TYPE_HALF, MIXQ_TYPE_HALF};
    return mixq_get_output_data_type_for(h, 0, types, 7) == MIXQ_TYPE_BF16 && mixq_supports_format_combination(h, 0, io, 7, 1)
           && MIXQ_E_TYPE != MIXQ_OK;
}
""")
    cc = tmp_path / "t.cpp"
    cc.write_text("""#include "mixq_plugin.hpp"
int probe(const mixq_plugin::MixQPlugin& p) { int t[7] = {7, 1, 1, 7, 1, 1, 1}; return p.getOutputDataType(0, t, 7); }
""")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include"]
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(c), "-o", str(tmp_path / "c.o")] + inc, check=True,
                   capture_output=True, text=True)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-c", str(cc), "-o", str(tmp_path / "cc.o")] + inc,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_restatement_agrees_with_float64():
    """Rules 1-4 on random rows against an independent float64 computation (exact P inputs: the result is deterministic)."""
    rng = np.random.default_rng(7)
    M, N, K = 9, 48, 256
    A = (rng.standard_normal((M, K)) * 3).astype(np.float32)
    A[2] *= 1e20     # beyond fp16's range: bf16 keeps it
    A[3] = 0
    A_bits = R.bf16_rn(A)
    ind = np.sort(rng.choice(K, 16, replace=False)).astype(np.int32)
    A_bits[:, ind] = R.bf16_rn(rng.integers(-8, 9, (M, 16)).astype(np.float32) * 4)
    W = rng.integers(-127, 128, (N, K)).astype(np.int8)
    sW = (np.abs(rng.standard_normal(N)) * 1e-3 + 1e-4).astype(np.float16)
    fpW = R.bf16_rn(rng.integers(-8, 9, (N, 16)).astype(np.float32) * 0.25)
    out, qA, sA, fpA = R.prefill(A_bits, W, sW, fpW, ind)
    A64 = R.bf2f(A_bits).astype(np.float64)
    amax = np.abs(A64).max(axis=1)
    s64 = R.bf2f(R.bf16_rn((amax.astype(np.float32) / np.float32(127))))
    assert np.array_equal(R.bf2f(sA), s64)
    with np.errstate(invalid="ignore", divide="ignore"):
        q64 = np.clip(np.rint(A64 / s64[:, None].astype(np.float64)), -127, 127)
    q64 = np.nan_to_num(q64, nan=0.0)
    assert (np.abs(q64 - qA) <= 1).all() and (q64 == qA).mean() > 0.999   # (fp32 vs float64 quotient: a tie may break apart)
    P = R.bf2f(fpA).astype(np.float64) @ R.bf2f(fpW).astype(np.float64).T   # exact; rule 3 rounds it to bf16
    ref = qA.astype(np.float64) @ W.T.astype(np.float64) * (sW.astype(np.float64)[None, :] * s64[:, None]) + \
        R.bf2f(R.bf16_rn(P)).astype(np.float64)
    got = R.bf2f(out).astype(np.float64)
    assert (np.abs(got - ref) <= R.ulp_bf16(ref) * 0.5 * (1 + 2 ** -16) + 1e-300).all()
    assert np.isfinite(got[2]).all() and np.abs(got[2]).max() > 1e15
    assert (got[3] == R.bf2f(out[3])).all()
    # NaN handling: an all-NaN row has a NaN scale and zero quotients
    A_bits[4] = 0x7fc0
    q2, s2 = R.quant_rows(A_bits)
    assert np.isnan(R.bf2f(s2[4])) and (q2[4] == 0).all()


def test_pack_bf16_fp_weight_and_int8_refusal():
    from mixq_tensorrt_llm_amd import pack, parallel
    rng = np.random.default_rng(1)
    W = torch.from_numpy((rng.standard_normal((64, 256)) * 0.02).astype(np.float32)).to(torch.bfloat16)
    act = torch.from_numpy(np.abs(rng.standard_normal(256)).astype(np.float32))
    p = pack.pack_linear_weights(W, act, fp_dtype=torch.bfloat16)
    ind = p["fp_ind"].astype(np.int64)
    assert p["fp_weight"].dtype == np.uint16
    assert np.array_equal(p["fp_weight"], R.to_bits(W[:, torch.from_numpy(ind)]))
    p16 = pack.pack_linear_weights(W.to(torch.float16), act)
    for k in ("weight", "weights_scaling_factor", "qweight", "scales", "fp_ind"):
        assert np.array_equal(p[k], p16[k]), k
    with pytest.raises(ValueError):
        pack.pack_linear_weights(W, act, outlier_weights="int8", fp_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        parallel.shard_packed(p, 2, 0)


def test_checkpoint_round_trip_keeps_bf16_bits(tmp_path):
    from mixq_tensorrt_llm_amd import checkpoint, pack
    rng = np.random.default_rng(2)
    W = torch.from_numpy((rng.standard_normal((64, 256)) * 0.02).astype(np.float32)).to(torch.bfloat16)
    act = torch.from_numpy(np.abs(rng.standard_normal(256)).astype(np.float32))
    p = pack.pack_linear_weights(W, act, fp_dtype=torch.bfloat16)
    p["bias"] = R.bf16_rn(rng.standard_normal(64).astype(np.float32) * 1e6)
    checkpoint.save_checkpoint(str(tmp_path), {"l0": p})
    _, layers = checkpoint.load_checkpoint(str(tmp_path))
    assert layers["l0"]["fp_weight"].dtype == torch.bfloat16 and layers["l0"]["bias"].dtype == torch.bfloat16
    back = checkpoint.from_carriers(layers["l0"])
    for k in ("weight", "weights_scaling_factor", "fp_weight", "fp_ind", "qweight", "bias"):
        assert np.array_equal(np.asarray(back[k]), np.asarray(p[k])), k
