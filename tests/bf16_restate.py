"""Restatement of a bf16 call of mixq_enqueue (include/mixq.h) in numpy fp32 / float64 and torch CPU bf16 rounding.

bf16 values travel as their uint16 bit patterns (numpy has no bf16).  No GPU, no library: the tests compare the operator with this.
"""
import numpy as np
import torch

BF16_MAX = 3.3895313892515355e38


def bf16_rn(x):
    """fp32 (or float64 -> fp32 first) -> bf16 bits, round to nearest even (torch CPU)."""
    x32 = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    return torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def bf2f(bits):
    """bf16 bits -> fp32."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_bits(t):
    """bf16 torch tensor -> uint16 bits (numpy)."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(bits, device=None):
    """uint16 bits -> bf16 torch tensor."""
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)
    return t.to(device) if device is not None else t


def quant_rows(A_bits):
    """Rules 1-2: (qA int8 [M, K], sA bf16 bits [M]).  amax drops NaNs; an all-NaN row gets a NaN scale; the quotient is the IEEE
    fp32 one, rounded half to even and saturated to [-127, 127]; a NaN quotient gives 0."""
    A = bf2f(A_bits)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        absA = np.abs(A)
        all_nan = np.isnan(absA).all(axis=1)
        amax = np.where(all_nan, np.float32(np.nan), np.nanmax(np.where(np.isnan(absA), -np.inf, absA), axis=1)).astype(np.float32)
        sA = bf16_rn(amax / np.float32(127.0))
        q = np.rint(A / bf2f(sA)[:, None]).astype(np.float32)
        q = np.where(np.isnan(q), np.float32(0), np.clip(q, -127, 127))
    return q.astype(np.int8), sA


def outlier_product(fpA_bits, fpW_bits):
    """The outlier product in float64 (exact for the inputs the bit-exact tests choose)."""
    return bf2f(fpA_bits).astype(np.float64) @ bf2f(fpW_bits).astype(np.float64).T


def prefill(A_bits, W_i8, sW_f16, fpW_bits, ind, bias_bits=None):
    """Rules 1-4 for one prefill call: Out bf16 bits [M, N].  P is rounded from a float64 sum (exact for the bit-exact tests'
    inputs; for random data the bound of `prefill_bound` covers the order of the fp32 sum)."""
    qA, sA = quant_rows(A_bits)
    fpA = np.ascontiguousarray(A_bits[:, ind])
    acc = qA.astype(np.float64) @ W_i8.astype(np.float64).T                  # exact int32 sums
    P = bf2f(bf16_rn(outlier_product(fpA, fpW_bits).astype(np.float32)))
    s = (sW_f16.astype(np.float32)[None, :] * bf2f(sA)[:, None]).astype(np.float64)   # exact fp32 product
    with np.errstate(invalid="ignore", over="ignore"):
        v = (acc * s + P.astype(np.float64)).astype(np.float32)             # fmaf: one fp32 rounding (innocuous via float64)
    out = bf16_rn(v)
    if bias_bits is not None:
        out = bias_add(out, bias_bits)
    return out, qA, sA, fpA


def bias_add(out_bits, bias_bits):
    with np.errstate(over="ignore", invalid="ignore"):
        return bf16_rn(bf2f(out_bits) + bf2f(bias_bits)[None, :])


def ulp_bf16(x):
    """Spacing of bf16 at |x| (>= the subnormal spacing 2^-133)."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return np.exp2(e - 7)


def prefill_reference64(A_bits, W_i8, sW_f16, fpW_bits, ind):
    """(float64 result with an exact outlier product, that product) for the element-wise bound of random data."""
    qA, sA = quant_rows(A_bits)
    acc = qA.astype(np.float64) @ W_i8.astype(np.float64).T
    P = outlier_product(A_bits[:, ind], fpW_bits)
    s = (sW_f16.astype(np.float32)[None, :] * bf2f(sA)[:, None]).astype(np.float64)
    return acc * s + P, P


def prefill_bound(got_bits, ref64, P64):
    """One bf16 rounding step of the result plus one bf16 ulp of P (its order-dependent fp32 sum, rounded to bf16)."""
    got = bf2f(got_bits).astype(np.float64)
    err = np.abs(got - ref64)
    lim = ulp_bf16(ref64) + ulp_bf16(P64) + 1e-30
    return err, lim


def decode64(A_bits, q_un, scale_f16):
    """M <= 4: float64 sum_k A[m,k] (q[k,n] - 128 as stored, i.e. the un-interleaved int8 w) * scale[n]; also sum |A w s|."""
    A = bf2f(A_bits).astype(np.float64)
    w = q_un.astype(np.float64) * scale_f16.astype(np.float64)[None, :]
    return A @ w, np.abs(A) @ np.abs(w)
