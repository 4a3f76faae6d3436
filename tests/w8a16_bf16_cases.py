"""Shapes, inputs, expected bits and call helpers of the bf16 weight-only GEMM tests (helper module, not a test file).

The contract (include/mixq.h, mixq_w8a16_gemm_forward_typed with MIXQ_TYPE_BF16):
    S[m,n]   = sum_k fp32(A[m,k]) * fp32(q[k,n] - 128)        fp32 sum in the kernel's own order
    Out[m,n] = bf16_rn(fp32(scale[n]) * S[m,n])               one fp32 multiply, one rounding
`q` below is the un-interleaved int8 matrix (the stored byte minus 128); the kernels read its interleaved uint8 image."""
import ctypes
import functools

import numpy as np

import bf16_restate as R
from mixq_tensorrt_llm_amd import _lib

HALF, BF16 = _lib.MIXQ_TYPE_HALF, _lib.MIXQ_TYPE_BF16

# N % 128, N % 256, N % 4 == 2, K % 128 == 64, one K stage, M across the 16- / 32-row tile and the 256-row pass boundaries
RAGGED = [(5, 2, 64), (7, 130, 192), (33, 258, 320), (64, 128, 4160), (65, 384, 128), (129, 640, 1088), (255, 96, 704),
          (257, 256, 256), (300, 1026, 1600), (700, 136, 448)]
SPLIT_K = [(128, 12288, 256), (512, 3584, 1088)]   # with scratch the plan splits K over workgroups

# mixq_debug_set_gemm_variant values (the `form` fixture of test_gpu_w8a16_gemm.py documents them)
AUTO, NARROW, KS_AUTO = 80, 81, 85
KS_KNOB = {1: 86, 2: 87, 4: 88, 8: 89}
RW_AUTO, RW_OFF, RW_ON = 845, 846, 847
SKINNY_AUTO, SKINNY_OFF = 850, 851
SKINNY_SHAPES = (852, 853, 854, 855)          # 32 columns x 8 / 16 waves, 64 columns x 8 / 16 waves
SKINNY_SHAPES_16 = (859, 8590)                # 16 columns x 8 / 16 waves, up to 16 tokens
DECODE_SKINNY, DECODE_GEMV, DECODE_AUTO = 856, 857, 858
WIDE_ROWS = {1: 32, 2: 64, 3: 128, 4: 256, 5: 64, 6: 128}
WIDE_RW = (1, 2, 5, 6)                         # configurations with a register-weight build


def wide_knob(cfg):
    return 830 + cfg


def wide_split_allowed(cfg, K, ks):
    """wo_wide_plan: a forced split is taken where every workgroup keeps 4 (tiles up to 64 rows) / 8 stages of 64 k."""
    if ks == 1:
        return True
    small = WIDE_ROWS[cfg] <= 64
    hi = min((K // 64) // (4 if small else 8), 16 if small else 8)
    return ks <= hi


def reset_forms(lib):
    for v in (843, RW_AUTO, AUTO, KS_AUTO):
        lib.mixq_debug_set_gemm_variant(v)


def interleave(q):
    out = np.empty(q.shape, np.uint8)
    _lib.check(_lib.load().mixq_preprocess_weights_int8(out.ctypes.data, np.ascontiguousarray(q).ctypes.data, q.shape[0], q.shape[1]),
               "preprocess")
    return out


def odd_scales(rng, N):
    """Random fp16 scales that are no powers of two (the lowest mantissa bit is set)."""
    sc = (rng.random(N) * 1e-3 + 1e-4).astype(np.float16)
    return (sc.view(np.uint16) | 1).view(np.float16)


@functools.lru_cache(maxsize=None)
def integer_case(M, N, K):
    """(A bits [M,K], q int8 [K,N], interleaved image, scale fp16 [N], expected bf16 bits [M,N]).  A = integers in [-4, 4] times a
    per-row power of two (2^100, 2^-100, 1), q any int8: every partial sum of the integer part is below 4 * 128 * 4160 < 2^24, so S is
    exact in fp32 in every order and the expected bits are a condition, not a tolerance."""
    assert K <= 4160
    rng = np.random.default_rng(1000003 * M + 1009 * N + K)
    Ai = rng.integers(-4, 5, size=(M, K)).astype(np.float64)
    q = rng.integers(-128, 128, size=(K, N), dtype=np.int8)
    sc = odd_scales(rng, N)
    e = np.array([100.0, -100.0, 0.0])[np.arange(M) % 3]
    A32 = (Ai * np.exp2(e)[:, None]).astype(np.float32)
    A_bits = R.bf16_rn(A32)
    assert np.array_equal(R.bf2f(A_bits), A32)                                # exact in bf16
    S = ((Ai @ q.astype(np.float64)) * np.exp2(e)[:, None]).astype(np.float32)  # exact: |integer sum| < 2^24, times a power of two
    with np.errstate(over="raise", invalid="raise"):
        want = R.bf16_rn(sc.astype(np.float32)[None, :] * S)
    assert np.isfinite(R.bf2f(want)).all()
    for a in (A_bits, q, sc, want):
        a.setflags(write=False)
    return A_bits, q, interleave(q), sc, want


@functools.lru_cache(maxsize=None)
def random_case(M, N, K):
    """(A bits, q, image, scale, float64 reference, float64 sum of magnitudes) for the bounded comparison."""
    rng = np.random.default_rng(7 * M + 13 * N + K)
    q = rng.integers(-128, 128, size=(K, N), dtype=np.int8)
    sc = odd_scales(rng, N)
    A_bits = R.bf16_rn(rng.standard_normal((M, K)).astype(np.float32))
    ref64, mag = R.decode64(A_bits, q, sc)
    return A_bits, q, interleave(q), sc, ref64, mag


def accumulation_bound(ref64, mag, K):
    """One bf16 rounding step of the result plus the fp32 accumulation bound with a factor of two (K * 2^-23 * sum |a w s|): the bound
    tests/test_gpu_bf16_operator.py applies to the M <= 4 kernels."""
    return R.ulp_bf16(ref64) + K * 2.0 ** -23 * mag


class Device:
    """One problem's operands on the GPU and calls of the typed entry on them."""

    def __init__(self, lib, torch, A_bits, qi, sc):
        self.lib, self.torch = lib, torch
        self.M, self.K = A_bits.shape
        self.N = sc.shape[0]
        dev = torch.device("cuda:0")
        self.a = R.from_bits(A_bits, dev)
        self.w = torch.from_numpy(qi).to(dev)
        self.s = torch.from_numpy(np.ascontiguousarray(sc)).to(dev)
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def size(self, typ=BF16, rows=None):
        return int(self.lib.mixq_w8a16_gemm_workspace_size_typed(self.M if rows is None else rows, self.N, self.K, typ))

    def call(self, scratch=True, rows=None, typ=BF16, a=None):
        """(output bits on the device [rows, N] as int16, reported name).  With scratch: a zero-filled workspace of the entry's own
        size; the call is repeated on it and must give the same bits and leave the hand-over words zero."""
        torch, lib = self.torch, self.lib
        M = self.M if rows is None else rows
        a = self.a if a is None else a
        out = torch.full((M, self.N), float("nan"), dtype=torch.bfloat16 if typ == BF16 else torch.float16, device=self.a.device)
        n = self.size(typ, M) if scratch else 0
        ws = torch.zeros(max(n, 16384), dtype=torch.uint8, device=self.a.device) if scratch else None
        args = lambda o: (a.data_ptr(), self.w.data_ptr(), self.s.data_ptr(), o.data_ptr(), M, self.N, self.K, typ,
                          ws.data_ptr() if scratch else None, n, self.st)
        assert lib.mixq_w8a16_gemm_forward_typed(*args(out)) == 0
        name = lib.mixq_debug_last_gemm_kernel().decode()
        if scratch:
            again = torch.full_like(out, float("nan"))
            assert lib.mixq_w8a16_gemm_forward_typed(*args(again)) == 0
            assert torch.equal(out.view(torch.int16), again.view(torch.int16)), f"{name}: a repeat on the same scratch differs"
            assert int(ws[:16384].view(torch.int32).abs().sum()) == 0, f"{name}: hand-over words not re-armed"
        return out.view(torch.int16), name
