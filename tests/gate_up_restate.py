"""Restatement of the merged gate / up projection (include/mixq.h ``mixq_gemm_mixed_gate_up_typed``) in numpy, on top of
tests/silu_restate.py.  The merged layer has 2N rows in blocks of 8: row r(n) = 16 (n // 8) + n % 8 holds gate row n, row r(n) + 8 up
row n.  Per element, T the call's type:

    v_g, v_u = silu_restate.pre_activation on the merged layer, columns r(n) and r(n) + 8        fp32
    g   = T_rn(v_g / (1 + expf(-v_g)))
    u   = T_rn(v_u)
    Out = T_rn(fp32(g) * fp32(u))

``expf``: float32 array -> float32 array, numpy's by default.  The library's is the device's libm expf; the two agree except in the last
place of a few arguments (silu_restate's SiLU tests bound that), so a test that asks for the library's bits passes the device's expf.
16-bit values travel as uint16 bit patterns.  No GPU, no library (helper module, not a test file)."""
import numpy as np

import silu_restate as S


def merged_row(n):
    """Merged row of gate row n (the up row is 8 further on), written as the header writes it."""
    return 16 * (n // 8) + (n % 8)


def merged_rows(N):
    return np.array([merged_row(n) for n in range(N)], dtype=np.int64)


def merge_rows(gate, up):
    """The merged array of two [N, ...] arrays, by an explicit loop over the rows."""
    N = gate.shape[0]
    out = np.empty((2 * N,) + gate.shape[1:], gate.dtype)
    for n in range(N):
        out[merged_row(n)] = gate[n]
        out[merged_row(n) + 8] = up[n]
    return out


def silu_bits(v, bf, expf=None):
    v = np.asarray(v, np.float32)
    if expf is None:
        return S.silu_bits(v, bf)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        e = np.asarray(expf(-v), np.float32)
        return S.rn((v / (np.float32(1.0) + e)).astype(np.float32), bf)


def gate_up_from_v(v, bf, expf=None):
    """Out bits [M, N] from the pre-activations v fp32 [M, 2N] of the merged layer."""
    r = merged_rows(v.shape[1] // 2)
    with np.errstate(over="ignore"):
        u = S.rn(np.ascontiguousarray(v[:, r + 8]), bf)
    return S.mul_bits(silu_bits(np.ascontiguousarray(v[:, r]), bf, expf), u, bf)


def gate_up_bits(q, sA_bits, fpA_bits, W2_i8, sW2_f16, fpW2_bits, bf, expf=None):
    """Out bits [M, N] of the merged call (fpA_bits / fpW2_bits None: no outlier columns)."""
    return gate_up_from_v(S.pre_activation(q, sA_bits, fpA_bits, W2_i8, sW2_f16, fpW2_bits, bf), bf, expf)


__all__ = ["S", "merged_row", "merged_rows", "merge_rows", "silu_bits", "gate_up_from_v", "gate_up_bits"]
