"""Layers and activations of the fp16 P-flavour whose outlier product does not depend on the summation order (helper module, not a
test file; numpy, and tests/silu_restate.py for the SiLU rule).

The only order-dependent quantity of ``MixLinear_GEMM.forward`` is the fp32 accumulation of the outlier product
``activation_outliers . weight_cache^T``.  Here every term of one output's sum is an integer times the SAME power of two:

  8-bit layers   W[n, :] = k[n, :] 2^-e[n], integer |k| <= 127 with at least one |k| = 127 per row, e[n] in 6 .. 9.  Then
                 ``from_linear`` gives scale_col[n] = fp16(127 2^-e / 127) = 2^-e, q_weight = k, and every dequantised
                 ``weight_cache`` column is k 2^-e again.
  4-bit layers   the ``fp_features_num`` static outlier columns have that form (``weight_cache`` is a raw copy of them); the other
                 columns are ordinary random fp16.
  activations    the designated hot columns hold integers in +-[7, 64] in EVERY row (above sigma = 6, exact in fp16); everything else is
                 N(0, 0.8^2) clipped inside +-5.5, so nothing else is ever detected.

A sum of at most O_MAX = 264 such terms is an integer of magnitude <= 64 127 264 < 2^24 times 2^-e: every partial sum in every order
is exact in fp32, the fp16 rounding of the total is the one answer, and ``oracle.gemm_fp16`` gives it.  Everything downstream of the
product (the int8 sums, the dequant FMA, the bias add) is already exact in the oracle, so bit equality is a fair demand.
``check_product`` asserts the conditions per case; tests/test_pflavour_exact.py shows the order independence from the oracle alone."""
import numpy as np

SIGMA = 6.0
O_MAX = 264                      # the widest outlier set any case holds (the dynamic set freezes beyond 256 columns)
A_MAX, K_MAX = 64, 127
E_RANGE = (6, 9)
assert A_MAX * K_MAX * O_MAX < 2 ** 24, "a sum of O_MAX integer terms must stay exact in fp32"

ABOVE_SIGMA = np.nextafter(np.float16(SIGMA), np.float16(7.0))     # 6.0039: one fp16 step above sigma

# ---- the cases of tests/test_gpu_pflavour_fp16.py (the CPU test walks the same lists) ----------------------------------------------
LATTICE_MN = [(1, 4), (31, 28), (32, 32), (33, 36), (70, 208), (65, 1028)]
LATTICE_O = [0, 1, 7, 8, 9, 15, 16, 24, 37, 128, 129, 136, 264]
LAYER_SHAPES = [(272, 1088), (1040, 2048)]                          # (N, K)
LAYER_M = [1, 4, 5, 17, 70, 130, 300]
SCENARIOS = ["grow8", "odd3", "width", "bias", "three_d", "threshold"]
INT4_LAYERS = [(768, 2048, 256), (1024, 4096, 128)]                 # (N, K, fp_features_num): the two layers of tests/test_gpu_int4.py
INT4_M = [16, 96, 200]


# ---- building blocks ----------------------------------------------------------------------------------------------------------------
def exact_columns(rng, N, O, full_scale=False):
    """(fp16 [N, O] = k 2^-e, k int8 [N, O], e int [N]).  ``full_scale``: every row holds a +-127 (a whole 8-bit weight row needs it)."""
    k = rng.integers(-K_MAX, K_MAX + 1, (N, O)).astype(np.int8)
    if full_scale:
        assert O > 0
        k[np.arange(N), rng.integers(0, O, N)] = rng.choice(np.array([-K_MAX, K_MAX], np.int8), N)
    e = rng.integers(E_RANGE[0], E_RANGE[1] + 1, N)
    w = np.ldexp(k.astype(np.float32), -e[:, None]).astype(np.float16)
    assert np.array_equal(np.ldexp(w.astype(np.float64), e[:, None]), k.astype(np.float64)), "k 2^-e is exact in fp16"
    return w, k, e


def hot_integers(rng, shape):
    """Integers in +-[7, 64] as fp16."""
    return (rng.integers(7, A_MAX + 1, shape) * rng.choice([-1, 1], shape)).astype(np.float16)


def activations(M, K, hot, seed):
    """fp16 [M, K]: N(0, 0.8^2) clipped inside +-5.5, the columns ``hot`` integers in +-[7, 64] in every row."""
    rng = np.random.default_rng(seed)
    x = np.clip(rng.standard_normal((M, K)) * 0.8, -5.49, 5.49).astype(np.float16)
    hot = np.asarray(hot, np.int64)
    if hot.size:
        x[:, hot] = hot_integers(rng, (M, hot.size))
    return x


def check_product(fpA, fpW, e, a_step=1.0):
    """The three conditions under which fp16(fpA . fpW^T) is unique: integer activations up to 64, weights k 2^-e[n] with integer
    |k| <= 127, at most O_MAX terms; and no fp16 overflow of the product.  ``a_step``: the activations are integers times this power
    of two (the threshold scenario's 6.0039 = 1537 2^-8 in a set of at most two columns)."""
    fpA, fpW = np.asarray(fpA), np.asarray(fpW)
    assert fpA.dtype == np.float16 and fpW.dtype == np.float16 and fpA.shape[1] == fpW.shape[1] <= O_MAX
    a = fpA.astype(np.float64) / a_step
    k = np.ldexp(fpW.astype(np.float64), np.asarray(e)[:, None])
    assert np.array_equal(a, np.rint(a)) and (np.abs(a) <= A_MAX / a_step).all(), "an extracted activation is not an integer up to 64"
    assert np.array_equal(k, np.rint(k)) and (np.abs(k) <= K_MAX).all(), "a weight column is not k 2^-e with |k| <= 127"
    assert A_MAX / a_step * K_MAX * fpA.shape[1] < 2 ** 24
    if fpA.size and fpW.size:
        assert (np.abs(a) @ np.abs(fpW.astype(np.float64)).T).max() < 65504.0, "the product could overflow fp16"


def exact_operands(M, N, O, seed=0):
    """(fpA fp16 [M, O], fpW fp16 [N, O], e) for ``mixq_gemm_fp16`` alone, checked."""
    rng = np.random.default_rng(1000003 * M + 1009 * N + O + seed)
    fpA = hot_integers(rng, (M, O))
    fpW, _, e = exact_columns(rng, N, O)
    check_product(fpA, fpW, e)
    return fpA, fpW, e


# ---- 8-bit layers -------------------------------------------------------------------------------------------------------------------
def layer8(N, K, seed, bias=False):
    """dict(W fp16 [N, K], k, e, bias): an 8-bit layer; ``from_linear``'s numpy restatement (linear.py:113-120) must give back k and
    2^-e."""
    rng = np.random.default_rng(seed)
    W, k, e = exact_columns(rng, N, K, full_scale=True)
    sc = (np.abs(W).max(axis=1) / np.float16(127)).astype(np.float16)
    assert np.array_equal(sc.astype(np.float64), np.ldexp(1.0, -e)), "scale_col is not 2^-e"
    assert np.array_equal(np.rint(W / sc[:, None]).astype(np.int8), k), "q_weight is not k"
    b = (rng.standard_normal(N) * 0.1).astype(np.float16) if bias else None
    return dict(W=W, k=k, e=e, scale_col=sc, bias=b)


def _hot_sets(rng, K, sizes):
    """Disjoint ascending column sets of the given sizes; the first holds column 0 and the last column K - 1."""
    cols = rng.permutation(np.arange(1, K - 1))[:sum(sizes)]
    out, at = [], 0
    for n in sizes:
        out.append(cols[at:at + n].copy())
        at += n
    out[0][0] = 0
    out[-1][-1] = K - 1
    return [np.sort(s) for s in out]


def scenario(name, N, K, M):
    """One walk through the state machine: dict(layer = layer8(..), stop = cache.stop, calls = [x fp16, ...], hot = [columns that hold
    integers in that call]).  Every call's hot columns include all columns adopted by earlier calls -- a held column is extracted
    whatever its magnitude, so it must hold integers too.

      grow8      3 columns, then 5 more (8), frozen by cache.stop = 2; two more calls on the static one-call route (O = 8: the fused GEMM)
      odd3       3 columns, frozen by cache.stop = 1; the static route with an odd set (the two-step order)
      width      cache.stop = 100: 250 columns, then 8 more -> 258 > 256 freezes the layer; one static call with O = 258
      bias       as grow8 with 5 + 4 = 9 columns and a bias
      three_d    as grow8 with a 3-D input
      threshold  cache.stop = 100, no hot column: one call whose only large element is sigma itself, one with it one fp16 step above,
                 one more with another such element (the columns these can adopt hold integers up to 5 elsewhere)"""
    assert name in SCENARIOS
    seed = SCENARIOS.index(name) * 7919 + N * 31 + K + M
    rng = np.random.default_rng(seed)
    L = layer8(N, K, seed + 1, bias=(name == "bias"))
    x = lambda hot, i: activations(M, K, hot, seed + 100 + i)  # noqa: E731
    if name in ("grow8", "three_d", "bias"):
        a, b = _hot_sets(rng, K, (5, 4) if name == "bias" else (3, 5))
        both = np.concatenate((a, b))
        stop, hot = 2, [a, both, both, both]
    elif name == "odd3":
        a, = _hot_sets(rng, K, (3,))
        stop, hot = 1, [a, a]
    elif name == "width":
        a, b = _hot_sets(rng, K, (250, 8))
        both = np.concatenate((a, b))
        stop, hot = 100, [a, both, both]
    else:
        stop, hot = 100, [np.zeros(0, np.int64)] * 3
    calls = [x(h, i) for i, h in enumerate(hot)]
    if name == "threshold":
        for c in calls:                                        # the columns a triggered detection adopts hold small integers elsewhere
            c[:, [0, K // 2]] = rng.integers(-5, 6, (M, 2)).astype(np.float16)
        calls[0][M // 2, K - 1] = np.float16(SIGMA)            # == sigma: nothing to find
        calls[1][M - 1, 0] = -ABOVE_SIGMA                      # one fp16 step above
        calls[2][0, K // 2] = ABOVE_SIGMA                      # and once more on the grown (or not) layer
    if name == "three_d":
        lead = (2, M // 2) if M % 2 == 0 else (1, M)
        calls = [c.reshape(lead + (K,)) for c in calls]
    return dict(name=name, layer=L, stop=stop, calls=calls, hot=hot)


def walk(oracle, sc):
    """The oracle's state machine over the scenario's calls -> one record per call: want (fp16 [M, N]), x_after, ind, weight_cache,
    add_outliers, cnt, and the outlier product's operands fpA = x[:, ind] / fpW = weight_cache (checked by ``check_product``)."""
    L = sc["layer"]
    st = oracle.MixLinearState(L["k"], L["scale_col"], sigma=SIGMA, stop=sc["stop"], bias=L["bias"])
    out = []
    for x in sc["calls"]:
        x2 = np.ascontiguousarray(x.reshape(-1, x.shape[-1])).copy()
        before = x2.copy()
        want = oracle.mixlinear_forward(st, x2)
        rec = dict(want=want, x_after=x2, ind=st.ind.copy(), weight_cache=None if st.weight_cache is None else st.weight_cache.copy(),
                   add_outliers=st.add_outliers, cnt=st.cnt)
        if st.ind.size:
            rec["fpA"], rec["fpW"] = np.ascontiguousarray(before[:, st.ind]), np.ascontiguousarray(st.weight_cache)
            check_product(rec["fpA"], rec["fpW"], L["e"], a_step=2.0 ** -8 if sc["name"] == "threshold" else 1.0)
        out.append(rec)
    return out


# ---- 4-bit layers -------------------------------------------------------------------------------------------------------------------
def layer4(N, K, FP, seed):
    """dict(W fp16 [N, K], scales fp32 [K], ind, e): ordinary random weights whose ``FP`` static outlier columns (the top activation
    scales, stable order as ``from_linear`` picks them) are k 2^-e."""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((N, K)) * 0.02).astype(np.float16)
    scales = np.abs(rng.standard_normal(K)).astype(np.float32)
    ind = np.argsort(scales, kind="stable")[-FP:].astype(np.int32)
    cols, _, e = exact_columns(rng, N, FP)
    W[:, ind] = cols
    return dict(W=W, scales=scales, ind=ind, e=e)


def activations4(L, M, seed):
    x = activations(M, L["W"].shape[1], L["ind"], seed)
    check_product(x[:, L["ind"]], L["W"][:, L["ind"]], L["e"])
    return x


# ---- the SiLU rule of tests/test_gpu_silu_epilogue.py, for the fp16 P-flavour's SiLU outputs ---------------------------------------
def assert_silu_rule(got, want, what=""):
    """fp16 ``got`` against ``want`` (a SiLU output of the oracle: ``expf`` there, the device's exponential here): no NaN that the oracle
    does not have, at most one fp16 step (``silu_restate.ulp_steps``) apart, fewer than 0.1 % of the elements differing.  Prints and
    returns (largest step count, differing fraction)."""
    import silu_restate as S
    g, w = np.ascontiguousarray(got).view(np.uint16), np.ascontiguousarray(want).view(np.uint16)
    assert g.shape == w.shape, what
    gn, wn = S.is_nan(g, False), S.is_nan(w, False)
    assert not (gn & ~wn).any(), f"{what}: {int((gn & ~wn).sum())} NaN (or unwritten) outputs where the oracle has a number"
    assert not (wn & ~gn).any(), f"{what}: {int((wn & ~gn).sum())} numbers where the oracle has NaN"
    steps = np.where(wn, 0, S.ulp_steps(g, w))
    frac = float(((g != w) & ~wn).mean())
    print(f"{what}: SiLU max steps {int(steps.max())}, fraction differing {frac:.2e}")
    assert steps.max() <= 1, f"{what}: {int((steps > 1).sum())} outputs more than one fp16 step from the oracle (max {int(steps.max())})"
    assert frac < 1e-3, f"{what}: {frac:.2e} of the outputs differ from the oracle"
    return int(steps.max()), frac


def side_slack(fpA, fpW):
    """Order slack of the fp16 side product for ``conftest.assert_elementwise``: conftest.SIDE_GAMMA is the project's constant for 128
    products; the standard fp32 accumulation bound grows linearly with the number of products, so wider sets scale it by O / 128."""
    from conftest import SIDE_GAMMA
    O = fpA.shape[1]
    return max(1.0, O / 128.0) * SIDE_GAMMA * (np.abs(fpA.astype(np.float32)) @ np.abs(fpW.astype(np.float32)).T).astype(np.float64)
