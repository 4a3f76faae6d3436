"""Restatement of the bf16 norm producer (include/mixq.h ``mixq_rmsnorm_typed`` / ``mixq_rmsnorm_extract_quant_typed``, DESIGN.md §1
"bf16 producer") and of the bf16 launcher-level GEMM on a producer's output (``mixq_gemm_mixed_typed``), in numpy float64 on top of
tests/bf16_restate.py.  bf16 values travel as uint16 bit patterns.  No GPU, no library (helper module, not a test file)."""
import numpy as np

import bf16_restate as R


def add_bits(x_bits, r_bits):
    """h = bf16_rn(fp32(x) + fp32(residual)): the fp32 sum of two bf16 values rounded once (torch's bf16 add)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return R.bf16_rn(R.bf2f(x_bits) + R.bf2f(r_bits))


def rmsnorm64(h_bits, gamma_bits, eps):
    """The ideal normalised row in float64: (h / sqrt(sum h^2 / K + eps)) * gamma, before any rounding and before the outlier
    columns are taken out.  A NaN (or an inf) in a row makes the whole row NaN, as in the kernel (rstd is NaN or 0 x inf)."""
    h = R.bf2f(h_bits).astype(np.float64)
    g = R.bf2f(gamma_bits).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        rstd = 1.0 / np.sqrt((h * h).sum(axis=1) / h.shape[1] + np.float64(np.float32(eps)))
        return (h * rstd[:, None]) * g[None, :]


def extract_zero(out_bits, ind):
    """(outliers bits [M, len(ind)], out bits with those columns zeroed): outliers[m, j] = out[m, ind[j]] as a bit copy, 0 for an
    ind[j] outside [0, K)."""
    out_bits = np.asarray(out_bits, np.uint16)
    ind = np.asarray(ind, np.int64)
    ok = (ind >= 0) & (ind < out_bits.shape[1])
    outl = np.zeros((out_bits.shape[0], ind.size), np.uint16)
    outl[:, ok] = out_bits[:, ind[ok]]
    zeroed = out_bits.copy()
    zeroed[:, ind[ok]] = 0
    return outl, zeroed


def gemm_acc_scale(q, sA_bits, W_i8, sW_f16):
    """(exact int32 sums as float64, the exact fp32 product sW sA as float64)."""
    acc = q.astype(np.float64) @ W_i8.astype(np.float64).T
    s = (np.asarray(sW_f16, np.float16).astype(np.float32)[None, :] * R.bf2f(sA_bits)[:, None]).astype(np.float64)
    return acc, s


def gemm_given(q, sA_bits, fpA_bits, W_i8, sW_f16, fpW_bits, bias_bits=None):
    """Out bits [M, N] = bf16_rn(fmaf(acc, sW sA, P)) (+ one bf16 add of the bias) GIVEN the producer's q / sA / fpA: acc the exact
    int8 sums, P the outlier product rounded to bf16 from a float64 sum (exact for the inputs the bit-exact tests choose)."""
    acc, s = gemm_acc_scale(q, sA_bits, W_i8, sW_f16)
    with np.errstate(invalid="ignore", over="ignore"):
        P = R.bf2f(R.bf16_rn(R.outlier_product(fpA_bits, fpW_bits).astype(np.float32)))
        v = (acc * s + P.astype(np.float64)).astype(np.float32)     # fmaf: one fp32 rounding (innocuous via float64)
    out = R.bf16_rn(v)
    return out if bias_bits is None else R.bias_add(out, bias_bits)


def gemm_reference64(q, sA_bits, fpA_bits, W_i8, sW_f16, fpW_bits):
    """(float64 result with an exact outlier product, that product): for bf16_restate.prefill_bound on random outlier weights."""
    acc, s = gemm_acc_scale(q, sA_bits, W_i8, sW_f16)
    with np.errstate(invalid="ignore", over="ignore"):
        P = R.outlier_product(fpA_bits, fpW_bits)
        return acc * s + P, P
