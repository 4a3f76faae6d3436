"""Restatement of the bf16 P-flavour entries (include/mixq.h ``mixq_quant_extract_typed``, ``mixq_find_outliers_typed``,
``mixq_dequant_weight_columns_typed``, ``mixq_mixlinear_forward_typed``; DESIGN.md §1 "bf16 P-flavour") in numpy / torch CPU on top
of tests/bf16_restate.py.  bf16 values travel as uint16 bit patterns.  No GPU, no library (helper module, not a test file)."""
import numpy as np

import bf16_restate as R


def in_range(ind, K):
    ind = np.asarray(ind, np.int64)
    return (ind >= 0) & (ind < K)


def quant_rows_zeroed(A_bits, ind):
    """(q int8 [M, K], sA bits [M], fpA bits [M, len], A bits after the call): fpA is a bit copy of the ORIGINAL columns (+0 for an
    index outside [0, K), which zeroes nothing), the in-range columns become 0x0000, and rules 1-2 (bf16_restate.quant_rows) run on
    the zeroed row."""
    A_bits = np.asarray(A_bits, np.uint16)
    ind = np.asarray(ind, np.int64).reshape(-1)
    ok = in_range(ind, A_bits.shape[1])
    fpA = np.zeros((A_bits.shape[0], ind.size), np.uint16)
    fpA[:, ok] = A_bits[:, ind[ok]]
    z = A_bits.copy()
    z[:, ind[ok]] = 0
    q, sA = R.quant_rows(z)
    return q, sA, fpA, z


def find_outliers(A_bits, sigma):
    """Ascending int32 columns holding some |fp32(a)| > fp32(sigma); NaN compares false, +-inf true."""
    with np.errstate(invalid="ignore"):
        hit = np.abs(R.bf2f(np.asarray(A_bits, np.uint16))) > np.float32(sigma)
    return np.flatnonzero(hit.any(axis=0)).astype(np.int32)


def dequant_columns(q_w, sW_f16, ind):
    """bf16 bits [N, len] = bf16_rn(fp32(q_w[n, ind[j]]) * fp32(sW[n])) (an exact fp32 product, one rounding); a zero column for an
    index outside [0, K)."""
    q_w = np.asarray(q_w, np.int8)
    ind = np.asarray(ind, np.int64).reshape(-1)
    ok = in_range(ind, q_w.shape[1])
    out = np.zeros((q_w.shape[0], ind.size), np.uint16)
    s = np.asarray(sW_f16, np.float16).astype(np.float32).reshape(-1, 1)
    out[:, ok] = R.bf16_rn(q_w[:, ind[ok]].astype(np.float32) * s)
    return out


def forward(A_bits, ind, q_w, sW, wc_bits, bias_bits=None):
    """(Out bits [M, N], q, sA, fpA, zeroed A) of a bf16 forward with the outlier set ``ind`` (-1 = padding) and outlier weights
    ``wc_bits`` [N, len]: bf16_rn(fmaf(acc, sW sA, bf16_rn(sum fp32(fpA) fp32(wc)))) on the zeroed row's q / sA with the original
    outlier values, then one bf16 add of the bias -- bf16_restate.prefill's rules 3-4 (P from a float64 sum: exact for the inputs the
    bit-exact tests choose)."""
    q, sA, fpA, z = quant_rows_zeroed(A_bits, ind)
    acc = q.astype(np.float64) @ np.asarray(q_w, np.int8).astype(np.float64).T
    s = (np.asarray(sW, np.float16).astype(np.float32).reshape(1, -1) * R.bf2f(sA)[:, None]).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if fpA.shape[1]:
            P = R.bf2f(R.bf16_rn(R.outlier_product(fpA, wc_bits).astype(np.float32))).astype(np.float64)
        else:
            P = np.zeros_like(acc)
        out = R.bf16_rn((acc * s + P).astype(np.float32))
    if bias_bits is not None:
        out = R.bias_add(out, bias_bits)
    return out, q, sA, fpA, z


def forward_reference64(A_bits, ind, q_w, sW, wc_bits):
    """(float64 result with an exact outlier product, that product) for bf16_restate.prefill_bound on random data."""
    q, sA, fpA, _ = quant_rows_zeroed(A_bits, ind)
    acc = q.astype(np.float64) @ np.asarray(q_w, np.int8).astype(np.float64).T
    s = (np.asarray(sW, np.float16).astype(np.float32).reshape(1, -1) * R.bf2f(sA)[:, None]).astype(np.float64)
    P = R.outlier_product(fpA, wc_bits) if fpA.shape[1] else np.zeros_like(acc)
    with np.errstate(invalid="ignore", over="ignore"):
        return acc * s + P, P
