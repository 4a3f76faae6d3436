"""CPU: the exact-product cases of tests/pflavour_exact.py really have ONE answer.  For every case tests/test_gpu_pflavour_fp16.py and the
4-bit additions of tests/test_gpu_int4.py use, ``oracle.gemm_fp16`` (which sums the O columns in index order) gives identical bits
under three random permutations of the columns -- so, from the reference alone, bit equality with it is a fair demand of any kernel,
whatever its summation order.  The helper's own conditions (integers, the 2^24 bound, no fp16 overflow, from_linear's restatement) are
asserted while the cases are built."""
import numpy as np
import pytest

import pflavour_exact as X


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def assert_order_free(oracle, fpA, fpW, what):
    want = oracle.gemm_fp16(fpA, fpW)
    assert np.isfinite(want.astype(np.float32)).all(), what
    rng = np.random.default_rng(fpA.shape[1] + fpA.shape[0])
    for i in range(3):
        p = rng.permutation(fpA.shape[1])
        got = oracle.gemm_fp16(np.ascontiguousarray(fpA[:, p]), np.ascontiguousarray(fpW[:, p]))
        assert np.array_equal(bits(got), bits(want)), f"{what}: permutation {i} of the {p.size} columns changes the oracle's bits"
    return want


def test_the_bound_the_construction_rests_on():
    assert X.A_MAX * X.K_MAX * X.O_MAX < 2 ** 24 and max(X.LATTICE_O) <= X.O_MAX
    assert float(X.ABOVE_SIGMA) > X.SIGMA and float(X.ABOVE_SIGMA) - X.SIGMA == 2.0 ** -8


def test_an_ordinary_product_is_not_order_free(oracle):
    """The control: with ordinary random operands the same three permutations DO change bits (else the test above proves nothing)."""
    rng = np.random.default_rng(0)
    a = (rng.standard_normal((70, 264)) * 8).astype(np.float16)
    w = (rng.standard_normal((208, 264)) * 0.02).astype(np.float16)
    want = oracle.gemm_fp16(a, w)
    p = rng.permutation(264)
    assert not np.array_equal(bits(oracle.gemm_fp16(np.ascontiguousarray(a[:, p]), np.ascontiguousarray(w[:, p]))), bits(want))


@pytest.mark.parametrize("M,N", X.LATTICE_MN)
def test_lattice_operands_are_order_free(oracle, M, N):
    for O in X.LATTICE_O:
        fpA, fpW, _ = X.exact_operands(M, N, O)
        want = assert_order_free(oracle, fpA, fpW, f"gemm_fp16 {M}x{N}x{O}")
        if O == 0:
            assert (bits(want) == 0).all()
        else:
            assert (want != 0).any()


@pytest.mark.parametrize("M", X.LAYER_M)
@pytest.mark.parametrize("N,K", X.LAYER_SHAPES)
@pytest.mark.parametrize("name", X.SCENARIOS)
def test_scenario_products_are_order_free(oracle, name, N, K, M):
    sc = X.scenario(name, N, K, M)
    recs = X.walk(oracle, sc)
    for i, r in enumerate(recs):
        if r["ind"].size:
            assert_order_free(oracle, r["fpA"], r["fpW"], f"{name} {M}x{N}x{K} call {i}")
    widths = [r["ind"].size for r in recs]
    frozen = [not r["add_outliers"] for r in recs]
    if name == "grow8" or name == "three_d":
        assert widths == [3, 8, 8, 8] and frozen == [False, True, True, True]
    elif name == "odd3":
        assert widths == [3, 3] and frozen == [True, True]
    elif name == "width":
        assert widths == [250, 258, 258] and frozen == [False, True, True]
    elif name == "bias":
        assert widths == [5, 9, 9, 9] and frozen == [False, True, True, True]
    else:   # the element AT sigma adopts nothing, whatever the oracle decides about the steps above it
        assert widths[0] == 0 and all(w <= 2 for w in widths) and not any(frozen)


@pytest.mark.parametrize("N,K,FP", X.INT4_LAYERS)
def test_int4_static_columns_are_order_free(oracle, N, K, FP):
    L = X.layer4(N, K, FP, seed=N + FP)
    _, _, ind, wc = oracle.mixlinear4_from_linear(L["W"], L["scales"], FP)
    assert np.array_equal(ind, L["ind"]) and np.array_equal(bits(wc), bits(L["W"][:, ind]))
    for M in X.INT4_M:
        x = X.activations4(L, M, seed=M)
        assert_order_free(oracle, np.ascontiguousarray(x[:, ind]), np.ascontiguousarray(wc), f"4-bit {M}x{N}x{K}")
        assert np.abs(np.delete(x, ind, axis=1).astype(np.float32)).max() < X.SIGMA, "nothing outside the static set is above sigma"
