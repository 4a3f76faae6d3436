"""Restatement of the SiLU and SiLU x up epilogues of the fused mixed GEMM (include/mixq.h ``mixq_gemm_mixed_act_typed``) in
numpy, on top of tests/bf16_restate.py and tests/bf16_norm_restate.py, with an fp16 twin.  Per element, T the call's type:

    v   = fmaf(acc, sW sA, P)              fp32; through float64 as bf16_restate.prefill does, P the outlier product rounded to T
    g   = T_rn(v / (1 + exp(-v)))          numpy float32
    Out = g                                SiLU
    Out = T_rn(fp32(g) * fp32(mul))        SiLU x up: one multiply of the ROUNDED g (the fp32 product of two T values is exact)

16-bit values travel as uint16 bit patterns; `bf` selects bf16 (True) or fp16 (False); roundings go through torch CPU.  No GPU, no
library (helper module, not a test file)."""
import numpy as np
import torch

import bf16_norm_restate as NR
import bf16_restate as R


def rn(x, bf):
    """fp32 -> bits of T, round to nearest even."""
    if bf:
        return R.bf16_rn(x)
    x32 = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    return torch.from_numpy(x32).to(torch.float16).view(torch.int16).numpy().view(np.uint16)


def tof(bits, bf):
    """bits of T -> fp32."""
    bits = np.asarray(bits, dtype=np.uint16)
    return R.bf2f(bits) if bf else bits.view(np.float16).astype(np.float32)


def quant_rows(A_bits, bf):
    """(q int8 [M, K], sA bits [M]) of finite rows: sA = T_rn(amax / 127), q = sat(rint(A / sA)) -- bf16_restate.quant_rows and its
    fp16 twin.  (The GEMM takes q and sA as given; this only makes inputs a quantiser could have written.)"""
    if bf:
        return R.quant_rows(A_bits)
    A = tof(A_bits, False)
    sA = rn(np.abs(A).max(axis=1).astype(np.float32) / np.float32(127.0), False)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.rint(A / tof(sA, False)[:, None]).astype(np.float32)
    return np.where(np.isnan(q), np.float32(0), np.clip(q, -127, 127)).astype(np.int8), sA


def outlier_product_bits(fpA_bits, fpW_bits, bf):
    """P rounded to T from a float64 sum (exact for the inputs the bit-exact tests choose)."""
    P = tof(fpA_bits, bf).astype(np.float64) @ tof(fpW_bits, bf).astype(np.float64).T
    with np.errstate(over="ignore"):
        return rn(P.astype(np.float32), bf)


def pre_activation(q, sA_bits, fpA_bits, W_i8, sW_f16, fpW_bits, bf):
    """v fp32 [M, N]: line 1.  acc the exact int8 sums, sW sA the exact fp32 product, one fp32 rounding of the fma."""
    acc = q.astype(np.float64) @ W_i8.astype(np.float64).T
    s = (np.asarray(sW_f16, np.float16).astype(np.float32)[None, :] * tof(sA_bits, bf)[:, None]).astype(np.float64)
    P = tof(outlier_product_bits(fpA_bits, fpW_bits, bf), bf) if fpA_bits is not None else np.float32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        return (acc * s + np.asarray(P, np.float64)).astype(np.float32)


def silu32(v):
    """v / (1 + exp(-v)) in float32 (exp(-v) = inf gives -0 or +0, exp(-v) = 0 gives v)."""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (v / (np.float32(1.0) + np.exp(-v, dtype=np.float32))).astype(np.float32)


def silu_bits(v, bf):
    """Line 2: g as bits of T."""
    with np.errstate(over="ignore"):
        return rn(silu32(v), bf)


def mul_bits(g_bits, m_bits, bf):
    """Line 4: one multiply of the rounded g by mul, in T (the fp32 product is exact, so this is T's correctly rounded product)."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return rn(tof(g_bits, bf) * tof(m_bits, bf), bf)


def torch_mul_bits(g_bits, m_bits, bf):
    """The same through torch's own multiply in T on the CPU."""
    dt = torch.bfloat16 if bf else torch.float16
    a = torch.from_numpy(np.ascontiguousarray(g_bits).view(np.int16)).view(dt)
    b = torch.from_numpy(np.ascontiguousarray(m_bits).view(np.int16)).view(dt)
    return (a * b).view(torch.int16).numpy().view(np.uint16)


def ordinal(bits):
    """Bits of T -> integers in value order (+0 and -0 both 0): |ordinal(a) - ordinal(b)| counts the representable steps between."""
    b = np.asarray(bits, np.uint16).astype(np.int32)
    mag = b & 0x7FFF
    return np.where(b & 0x8000, -mag, mag)


def is_nan(bits, bf):
    return (np.asarray(bits, np.uint16) & 0x7FFF) > (0x7F80 if bf else 0x7C00)


def ulp_steps(got_bits, want_bits):
    """Representable steps of T between two results (neither NaN)."""
    return np.abs(ordinal(got_bits) - ordinal(want_bits))


__all__ = ["NR", "R", "rn", "tof", "quant_rows", "outlier_product_bits", "pre_activation", "silu32", "silu_bits", "mul_bits",
           "torch_mul_bits", "ordinal", "is_nan", "ulp_steps"]
