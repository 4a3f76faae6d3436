"""GPU (-m gpu): the bf16 form of the fused RMSNorm / extract / quantise producer (mixq_rmsnorm_typed, mixq_rmsnorm_extract_quant_typed;
csrc/norm_kernels.hip BF) and the typed launcher-level GEMM that consumes what it writes (mixq_gemm_mixed_typed), through ctypes and
through mixlib / mixlinear / plugin.

  * the normalised row against the float64 restatement (tests/bf16_norm_restate.py) within ONE bf16 ulp: half an ulp of the final
    rounding plus an fp32 evaluation error far below 2^-20 relative (a handful of fp32 roundings at 2^-24 each and the reduction of K
    squares) -- derived, not tuned;
  * scale and q as an exact function of the GPU's own `out` bits (bf16_restate.quant_rows, the rules of mixq_enqueue's bf16 quantiser);
  * the residual-add form bit for bit against a torch bf16 add followed by the non-add entry, in place and out of place;
  * the GEMM bit for bit against the restatement on the producer's own q / scale / outliers (outlier weights with one power of two
    per row: the outlier product is exact in any order), random outlier weights within bf16_restate.prefill_bound;
  * MIXQ_TYPE_HALF against the entries it delegates to; the Python chain; a captured HIP graph.

Every output is allocated at exactly its declared size between guards of bf16 NaNs (tests/guarded.py); a fragment-major image's
padding keeps what the buffer held (include/mixq.h)."""
import ctypes
import functools

import numpy as np
import pytest

import bf16_norm_restate as NR
import bf16_restate as R
import guarded
from test_gpu_producers import frag_image_bytes, norm_form, outlier_columns

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EPS = 1e-5
HALF, BF16 = 1, 7
NANFILL, QFILL = guarded.BF16_NAN, 0x5A
GUARD = 64 << 10               # a stray row of the longest K here (28672 x 2 bytes) stays inside

# (M, K, O, q_layout): item 1 of the issue
PRODUCER_SHAPES = [(3, 256, 16, 0), (37, 1024, 128, 0), (5, 4096, 128, 0), (9, 8192, 128, 0), (6, 11008, 128, 0), (4, 28672, 128, 0),
                   (32, 4096, 128, 1), (2048, 4096, 128, 0)]
SHAPE_IDS = [f"{m}x{k}" + ("-frag" if lay else "") for m, k, _, lay in PRODUCER_SHAPES]


def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    from mixq_tensorrt_llm_amd import _lib
    lib = _lib.load()
    lib.mixq_debug_reset()
    yield lib
    lib.mixq_debug_reset()


class Buf(guarded.Guarded):
    def __init__(self, nbytes, fill=NANFILL, init=None, guard=GUARD):
        super().__init__(nbytes, fill, None if init is None else np.array(init), guard=guard, offset=0, device=dev())   # (a writable copy)


def take(buf, dtype, shape, what):
    guarded.assert_intact(buf, what)
    return buf.body(dtype, shape)


def bf16_form(M, K, quant, frag=0, add=False):
    """The fp16 twin's name (test_gpu_producers.norm_form) with ",ADD=1" behind FRAG and " [bf16]" behind the name, in front of " nt"."""
    name = norm_form(M, K, quant, None, frag)
    nt = name.endswith(" nt")
    name = name[:-3] if nt else name
    if add:
        name = name.replace(">", ",ADD=1>")
    return name + " [bf16]" + (" nt" if nt else "")


def same16(a, b, nan_above=0x7F80):
    """16-bit patterns equal, any NaN equal to any NaN -> flat indices that differ."""
    ua, ub = np.asarray(a, np.uint16).reshape(-1), np.asarray(b, np.uint16).reshape(-1)
    na, nb = (ua & 0x7FFF) > nan_above, (ub & 0x7FFF) > nan_above
    return np.flatnonzero(~((ua == ub) | (na & nb)))


# ------------------------------------------------------------------------------------------------------------------ inputs ----
@functools.lru_cache(maxsize=None)
def producer_case(M, K, O, seed=0):
    """x, gamma (bf16 bits), ind, and the float64 reference of the normalised row -- computed once per shape and shared (read-only).
    Rows scaled by 0.1 .. 8, half of the outlier columns x 15, the last row all zero, and where M > 3 a row with a single NaN outside
    the outlier columns."""
    rng = np.random.default_rng(1000 * K + M + seed)
    ind = outlier_columns(K, O, seed=K + O)
    x = (rng.standard_normal((M, K)) * rng.uniform(0.1, 8.0, (M, 1))).astype(np.float32)
    x[:, ind[::2]] *= 15.0
    x[M - 1] = 0.0
    nan_row = None
    if M > 3:
        nan_row = 1
        x[nan_row, int(np.setdiff1d(np.arange(K), ind)[K // 3])] = np.nan
    x_bits = R.bf16_rn(x)
    g_bits = R.bf16_rn((1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32))
    ref = NR.rmsnorm64(x_bits, g_bits, EPS)
    for a in (x_bits, g_bits, ind, ref):
        a.setflags(write=False)
    return x_bits, g_bits, ind, ref, nan_row


def residual_case(M, K, seed=1):
    """x and residual spanning exponents; row 0 cancels to 0, row 1 overflows to +-inf."""
    rng = np.random.default_rng(77 * K + M + seed)
    x = (rng.standard_normal((M, K)) * np.exp2(rng.integers(-12, 13, (M, K)))).astype(np.float32)
    r = (rng.standard_normal((M, K)) * np.exp2(rng.integers(-12, 13, (M, K)))).astype(np.float32)
    x_bits, r_bits = R.bf16_rn(x), R.bf16_rn(r)
    r_bits[0] = x_bits[0] ^ 0x8000
    x_bits[1] = r_bits[1] = R.bf16_rn(np.where(rng.random(K) < 0.5, 3.0e38, -3.0e38).astype(np.float32))
    return x_bits, r_bits


# ----------------------------------------------------------------------------------------------------------------- running ----
def run_norm(lib, x_bits, g_bits, ind, quant, frag=0, typ=BF16, r_bits=None, h_in=None, entry=None):
    """One producer call on exact-size guarded buffers.  r_bits: with the residual add; h_in: None = h in a buffer of its own,
    "x" / "r" = in place.  entry: an fp16 entry to call instead of the typed one (a function of the argument tuples).
    -> dict of the bodies after the call (16-bit tensors as uint16 bits); every guard is checked."""
    M, K = x_bits.shape
    O = 0 if ind is None else ind.size
    add = r_bits is not None
    xg = Buf(x_bits.nbytes, init=x_bits)
    rg = Buf(r_bits.nbytes, init=r_bits) if add else None
    hg = {None: Buf(2 * M * K) if add else None, "x": xg, "r": rg}[h_in]
    g = torch.from_numpy(np.ascontiguousarray(g_bits).view(np.int16)).to(dev())
    out, outl, sc = Buf(2 * M * K), Buf(2 * M * O), Buf(2 * M)
    q = Buf(frag_image_bytes(M, K) if frag else M * K, QFILL)
    ip = torch.from_numpy(np.ascontiguousarray(ind)).to(dev()) if O else None
    head = (M, K, xg.ptr, rg.ptr if add else None, hg.ptr if add else None, g.data_ptr(), out.ptr, ctypes.c_float(EPS))
    tail = (ip.data_ptr() if O else None, O, outl.ptr if O else None, q.ptr, sc.ptr)
    if entry is not None:
        rc = entry(head, tail, frag)
    elif quant:
        rc = lib.mixq_rmsnorm_extract_quant_typed(*head, *tail, frag, typ, stream())
    else:
        rc = lib.mixq_rmsnorm_typed(*head, typ, stream())
    form = lib.mixq_debug_last_producer_kernel().decode()
    torch.cuda.synchronize()
    w = f"norm {M}x{K} quant={quant} O={O} frag={frag} add={add} h={h_in or 'own'}"
    res = dict(rc=rc, form=form, x=take(xg, np.uint16, (M, K), w + " x"), out=take(out, np.uint16, (M, K), w + " out"),
               outl=take(outl, np.uint16, (M, O), w + " outliers"), q=take(q, np.int8, None, w + " q"),
               scale=take(sc, np.uint16, None, w + " scale"), q_dev=q)
    if add:
        res.update(r=take(rg, np.uint16, (M, K), w + " residual"), h=take(hg, np.uint16, (M, K), w + " h"))
    return res


def row_major_q(got, M, K, frag):
    if not frag:
        return got["q"].reshape(M, K)
    from mixq_tensorrt_llm_amd import mixlib
    return mixlib.qa_to_row_major(got["q_dev"].body_bytes().view(torch.int8), M, K).cpu().numpy()


def assert_within_one_ulp(out_bits, ref64, what):
    got = R.bf2f(out_bits).astype(np.float64)
    nan_ref = np.isnan(ref64)
    assert np.array_equal(np.isnan(got), nan_ref), f"{what}: NaNs are not where the restatement has them"
    err = np.abs(np.where(nan_ref, 0.0, got) - np.where(nan_ref, 0.0, ref64))
    lim = R.ulp_bf16(np.where(nan_ref, 0.0, ref64))
    bad = err > lim
    print(f"{what}: max error {float((err / lim).max()):.3f} bf16 ulp")
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond one bf16 ulp, first {np.argwhere(bad)[0].tolist()}: {float(err[bad][0]):.3e} > {float(lim[bad][0]):.3e}"


def check_quantised(got, M, K, O, ind, frag, what):
    """(b) and (c): the outlier columns are zero; scale and q are bf16_restate.quant_rows of the GPU's own out bits."""
    assert (got["out"][:, ind] == 0).all(), what + ": an outlier column of out is not zero"
    q_ref, s_ref = R.quant_rows(got["out"])
    bad = same16(got["scale"], s_ref)
    assert bad.size == 0, f"{what}: scale differs from the restatement at rows {bad[:6].tolist()}"
    q = row_major_q(got, M, K, frag)
    assert np.array_equal(q, q_ref), f"{what}: {int((q != q_ref).sum())} int8 values differ from the restatement"
    return q


# --------------------------------------------------------------------------------------------------------------- 1. producer ----
@pytest.mark.parametrize("M,K,O,frag", PRODUCER_SHAPES, ids=SHAPE_IDS)
def test_bf16_producer(lib, M, K, O, frag):
    x_bits, g_bits, ind, ref, nan_row = producer_case(M, K, O)
    what = f"bf16 producer {M}x{K} O={O} frag={frag}"
    got = run_norm(lib, x_bits, g_bits, ind, 8, frag)
    assert got["rc"] == 0, what
    assert got["form"] == bf16_form(M, K, 8, frag), f"{what}: the launch took {got['form']!r}"
    assert np.array_equal(got["x"], x_bits), what + ": x was modified"
    full = got["out"].copy()
    full[:, ind] = got["outl"]                                    # (a) on the row with the outliers put back
    assert_within_one_ulp(full, ref, what)
    check_quantised(got, M, K, O, ind, frag, what)
    q = row_major_q(got, M, K, frag)
    assert got["scale"][M - 1] == 0 and (q[M - 1] == 0).all() and (got["out"][M - 1] & 0x7FFF == 0).all(), what + ": the zero row"
    if nan_row is not None:
        assert ((got["out"][nan_row] & 0x7FFF) > 0x7F80).sum() == K - O and ((got["outl"][nan_row] & 0x7FFF) > 0x7F80).all(), what
        # amax runs over the ZEROED row with NaNs dropped: the O zeroed outlier columns are the row's only numbers, so the scale is 0
        # here (what quant_rows makes of these out bits, checked above); the all-NaN row's NaN scale: test_bf16_all_nan_row below
        assert got["scale"][nan_row] == 0 and (q[nan_row] == 0).all(), what + ": the NaN row"


@pytest.mark.parametrize("M,K", [(37, 1024), (5, 4096), (4, 28672)])
def test_bf16_all_nan_row_gets_a_nan_scale(lib, M, K):
    """No outlier columns: the row with a single NaN normalises to an all-NaN row, whose scale is NaN and whose q is 0."""
    x_bits, g_bits, _, ref, nan_row = producer_case(M, K, 0)
    what = f"bf16 producer {M}x{K} O=0"
    got = run_norm(lib, x_bits, g_bits, None, 8)
    assert got["rc"] == 0 and got["form"] == bf16_form(M, K, 8), f"{what}: {got['rc']} {got['form']!r}"
    assert_within_one_ulp(got["out"], ref, what)
    q = check_quantised(got, M, K, 0, np.zeros(0, np.int64), 0, what)
    assert ((got["out"][nan_row] & 0x7FFF) > 0x7F80).all(), what + ": the NaN row's out"
    assert (got["scale"][nan_row] & 0x7FFF) > 0x7F80 and (q[nan_row] == 0).all(), what + ": the NaN row"


# ----------------------------------------------------------------------------------------------------------- 2. residual add ----
@pytest.mark.parametrize("M,K,O,frag", PRODUCER_SHAPES, ids=SHAPE_IDS)
def test_bf16_residual_add_equals_torch_add_then_plain_entry(lib, M, K, O, frag):
    x_bits, r_bits = residual_case(M, K)
    _, g_bits, ind, _, _ = producer_case(M, K, O)
    h_ref = R.to_bits(R.from_bits(x_bits, dev()) + R.from_bits(r_bits, dev()))          # torch's bf16 add
    assert same16(h_ref, NR.add_bits(x_bits, r_bits)).size == 0
    assert (h_ref[0] & 0x7FFF == 0).all() and (h_ref[1] & 0x7FFF == 0x7F80).all()      # the cancelling row, the overflowing row
    ref = run_norm(lib, h_ref, g_bits, ind, 8, frag)
    assert ref["rc"] == 0 and ref["form"] == bf16_form(M, K, 8, frag)
    for h_in in (None, "x", "r"):
        what = f"bf16 add + producer {M}x{K} frag={frag} h={h_in or 'own'}"
        got = run_norm(lib, x_bits, g_bits, ind, 8, frag, r_bits=r_bits, h_in=h_in)
        assert got["rc"] == 0 and got["form"] == bf16_form(M, K, 8, frag, add=True), f"{what}: {got['rc']} {got['form']!r}"
        for name, a, b in (("h", got["h"], h_ref), ("out", got["out"], ref["out"]), ("outliers", got["outl"], ref["outl"]),
                           ("scale", got["scale"], ref["scale"])):
            bad = same16(a, b)
            assert bad.size == 0, f"{what}: {bad.size} elements of {name} differ from add-then-norm, first {bad[:6].tolist()}"
        assert np.array_equal(got["q"], ref["q"]), f"{what}: q differs from add-then-norm"     # (the whole image: same pre-fill)
        if h_in != "x":
            assert np.array_equal(got["x"], x_bits), what + ": x was modified"
        if h_in != "r":
            assert np.array_equal(got["r"], r_bits), what + ": residual was modified"


# -------------------------------------------------------------------------------------------------------------- 3. plain norm ----
@pytest.mark.parametrize("M,K", [(5, 512), (33, 4096), (7, 11008)])
@pytest.mark.parametrize("add", [False, True], ids=["plain", "add"])
def test_bf16_plain_norm(lib, M, K, add):
    x_bits, g_bits, _, ref, _ = producer_case(M, K, 0)
    r_bits = None
    if add:
        rng = np.random.default_rng(M + K)
        r_bits = R.bf16_rn((rng.standard_normal((M, K)) * 2.0).astype(np.float32))
        ref = NR.rmsnorm64(NR.add_bits(x_bits, r_bits), g_bits, EPS)
    what = f"bf16 norm {M}x{K} add={add}"
    got = run_norm(lib, x_bits, g_bits, None, 0, r_bits=r_bits)
    assert got["rc"] == 0 and got["form"] == bf16_form(M, K, 0, 0, add), f"{what}: {got['rc']} {got['form']!r}"
    if add:
        assert same16(got["h"], NR.add_bits(x_bits, r_bits)).size == 0, what + ": h"
    assert_within_one_ulp(got["out"], ref, what)
    assert (got["q"].view(np.uint8) == QFILL).all() and ((got["scale"] & 0x7FFF) > 0x7F80).all(), what + ": q / scale were written"


# ------------------------------------------------------------------------------------------------------------------ 4. GEMM ----
GEMM_N, GEMM_O = 512, 128
GEMM_CASES = [(5, 1024), (40, 2048), (160, 1024), (300, 1024)]


@functools.lru_cache(maxsize=None)
def gemm_weights(N, K, O, exact):
    """W int8, sW fp16, fpW (bf16 bits; exact: one +-2^e per row, so the outlier product is one term in any order), bias (bf16 bits)."""
    rng = np.random.default_rng(N + K + O + exact)
    W = rng.integers(-127, 128, (N, K)).astype(np.int8)
    sW = rng.uniform(0.001, 0.02, N).astype(np.float16)
    if exact:
        fpW = np.zeros((N, O), np.float32)
        fpW[np.arange(N), rng.integers(0, O, N)] = np.exp2(rng.integers(-6, 3, N)) * rng.choice([-1.0, 1.0], N)
    else:
        fpW = (rng.standard_normal((N, O)) * 0.05).astype(np.float32)
    return W, sW, R.bf16_rn(fpW), R.bf16_rn(rng.standard_normal(N).astype(np.float32))


def upload(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a.view(np.int16) if a.dtype == np.float16 else a).to(dev())


def run_gemm(lib, prod, W, sW, fpW, bias, M, N, K, O, layout, typ=BF16, entry=None):
    """mixq_gemm_mixed_typed (or `entry`, an fp16 entry) on a producer's q image / scale / outliers -> (rc, Out bits, kernel name)."""
    qd = prod["q_dev"]
    ts = [upload(a) for a in (prod["scale"], sW, prod["outl"], fpW, W)]
    sa, sw, fpa, fpw, w = (t.data_ptr() for t in ts)
    b = upload(bias) if bias is not None else None
    out = Buf(2 * M * N, guard=guarded.out_guard(N, 2))
    if entry is not None:
        rc = entry(qd.ptr, w, sa, sw, fpa, fpw, b.data_ptr() if b is not None else None, out.ptr)
    else:
        rc = lib.mixq_gemm_mixed_typed(qd.ptr, w, sa, sw, fpa, fpw, b.data_ptr() if b is not None else None, out.ptr, M, N, K, O, layout, typ,
                                       None, 0, stream())
    name = lib.mixq_debug_last_gemm_kernel().decode()
    torch.cuda.synchronize()
    return rc, take(out, np.uint16, (M, N), f"gemm {M}x{N}x{K} layout={layout} bias={bias is not None}"), name


@pytest.mark.parametrize("M,K", GEMM_CASES, ids=[f"M{m}-K{k}" for m, k in GEMM_CASES])
def test_bf16_gemm_on_the_producers_output(lib, M, K):
    N, O = GEMM_N, GEMM_O
    x_bits, g_bits, ind, _, _ = producer_case(M, K, O)
    layout = int(lib.mixq_qa_layout(M, N, K))
    if (M, K) == (40, 2048):
        assert layout == 1, "40 x 512 x 2048 is in the fragment-major image's domain"
    prod = run_norm(lib, x_bits, g_bits, ind, 8, layout)
    assert prod["rc"] == 0
    q = check_quantised(prod, M, K, O, ind, layout, f"producer {M}x{K}")
    W, sW, fpW, bias = gemm_weights(N, K, O, True)
    for b in (None, bias):
        what = f"bf16 gemm {M}x{N}x{K} layout={layout} bias={b is not None}"
        rc, got, name = run_gemm(lib, prod, W, sW, fpW, b, M, N, K, O, layout)
        assert rc == 0 and name.endswith(" [bf16]"), f"{what}: rc {rc}, kernel {name!r}"
        if M == 5:
            assert "skinny" in name, name
        want = NR.gemm_given(q, prod["scale"], prod["outl"], W, sW, fpW, b)
        bad = same16(got, want)
        assert bad.size == 0, f"{what} ({name}): {bad.size} of {got.size} elements differ from the restatement, first {bad[:6].tolist()}"
    # random outlier weights: one bf16 step of the result plus one ulp of P (the bound of the bf16 operator tests)
    W, sW, fpW, _ = gemm_weights(N, K, O, False)
    rc, got, name = run_gemm(lib, prod, W, sW, fpW, None, M, N, K, O, layout)
    assert rc == 0 and name.endswith(" [bf16]")
    ref64, P64 = NR.gemm_reference64(q, prod["scale"], prod["outl"], W, sW, fpW)
    nan = np.isnan(ref64)
    assert np.array_equal((got & 0x7FFF) > 0x7F80, nan)
    err, lim = R.prefill_bound(np.where(nan, 0, got), np.where(nan, 0.0, ref64), np.where(nan, 0.0, P64))
    print(f"bf16 gemm {M}x{N}x{K} random fpW: max error / bound {float((err / lim).max()):.3f}")
    assert (err <= lim).all(), f"{int((err > lim).sum())} elements outside the bound"


# ------------------------------------------------------------------------------------------------------- 5. MIXQ_TYPE_HALF ----
def test_half_type_is_the_existing_entry(lib):
    M, K, O, N = 37, 1024, 128, GEMM_N
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((M, K)) * 3).astype(np.float16)
    x[:, ::9] *= 12
    r = (rng.standard_normal((M, K)) * 5).astype(np.float16)
    g = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float16)
    xb, rb, gb = (a.view(np.uint16) for a in (x, r, g))
    ind = outlier_columns(K, O, seed=2)
    st = stream()
    old = {(0, False): lambda h, t, f: lib.mixq_rmsnorm(*h[:3], *h[5:], st),
           (0, True): lambda h, t, f: lib.mixq_add_rmsnorm(*h, st),
           (8, False): lambda h, t, f: lib.mixq_rmsnorm_extract_quant_layout(*h[:3], *h[5:], *t, f, st),
           (8, True): lambda h, t, f: lib.mixq_add_rmsnorm_extract_quant_layout(*h, *t, f, st)}
    for (quant, add), entry in old.items():
        kw = dict(r_bits=rb if add else None)
        got = run_norm(lib, xb, gb, ind if quant else None, quant, typ=HALF, **kw)
        want = run_norm(lib, xb, gb, ind if quant else None, quant, entry=entry, **kw)
        assert got["rc"] == 0 and want["rc"] == 0 and got["form"] == want["form"] and "[bf16]" not in got["form"], (quant, add, got["form"])
        for name in ("out", "outl", "scale", "q") + (("h",) if add else ()):
            assert np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), f"type HALF, quant {quant} add {add}: {name} differs"
    # the GEMM at 160 rows, on the fp16 producer's output
    M = 160
    x = (rng.standard_normal((M, K)) * 3).astype(np.float16)
    x[:, ind[::2]] *= 12
    prod = run_norm(lib, x.view(np.uint16), gb, ind, 8, typ=HALF)
    W, sW, fpW_bf, bias_bf = gemm_weights(N, K, O, False)
    fpW = R.bf2f(fpW_bf).astype(np.float16)
    bias = R.bf2f(bias_bf).astype(np.float16)
    for b, entry in ((None, lambda qa, w, sa, sw, fa, fw, bb, o: lib.mixq_gemm_mixed_layout(qa, w, sa, sw, fa, fw, o, M, N, K, O, 0, None, 0, st)),
                     (bias, lambda qa, w, sa, sw, fa, fw, bb, o: lib.mixq_gemm_mixed_bias(qa, w, sa, sw, fa, fw, bb, o, M, N, K, O, None, 0, st))):
        rc1, got, k1 = run_gemm(lib, prod, W, sW, fpW, b, M, N, K, O, 0, typ=HALF)
        rc2, want, k2 = run_gemm(lib, prod, W, sW, fpW, b, M, N, K, O, 0, entry=entry)
        assert rc1 == 0 and rc2 == 0 and k1 == k2 and "[bf16]" not in k1, (rc1, rc2, k1, k2)
        assert np.array_equal(got, want), f"type HALF gemm, bias={b is not None}: differs from the existing entry"
        assert np.isfinite(got.view(np.float16).astype(np.float32)).all()


# ----------------------------------------------------------------------------------------------------------- 6. Python chain ----
def build_chain(N, K, seed):
    from mixq_tensorrt_llm_amd import mixlinear, pack, plugin
    rng = np.random.default_rng(seed)
    act = np.abs(rng.standard_normal(K)).astype(np.float32)
    Wt = torch.from_numpy((rng.standard_normal((N, K)) * 0.02).astype(np.float32)).to(torch.bfloat16)
    p = pack.pack_linear_weights(Wt, torch.from_numpy(act), fp_dtype=torch.bfloat16)
    _, _, fpW, bias = gemm_weights(N, K, 128, True)
    p["fp_weight"], p["bias"] = fpW.copy(), bias.copy()           # (one power of two per row: an exact outlier product)
    layer = plugin.MixQLinear(K, N, bias=True, dtype=torch.bfloat16, device=dev()).load(p)
    cache = mixlinear.MixLibCache(inputdim=256, device=dev(), dtype=torch.bfloat16)
    gamma = R.from_bits(R.bf16_rn((1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)), dev())
    norm = mixlinear.FasterTransformerRMSNorm(gamma, EPS, cache, dtype=torch.bfloat16)
    norm.next_layer = layer
    return p, layer, cache, norm


def chain_inputs(M, K, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((M, K), generator=g).to(torch.bfloat16).to(dev())
    res = (4.0 * torch.randn((M, K), generator=g)).to(torch.bfloat16).to(dev())
    return x, res


def chain_restatement(p, cache, M, K, lay):
    from mixq_tensorrt_llm_amd import mixlib
    q = cache.q_xcache if not lay else mixlib.qa_to_row_major(cache.q_xcache, M, K)
    return NR.gemm_given(q.cpu().numpy().reshape(M, K), R.to_bits(cache.x_scale.reshape(-1)[:M]), R.to_bits(cache.activation_outliers),
                         p["weight"], p["weights_scaling_factor"], p["fp_weight"], p["bias"])


@pytest.mark.parametrize("M", [16, 160])
def test_python_chain_norm_then_forward_quantised(lib, M):
    N, K = 512, 1024
    p, layer, cache, norm = build_chain(N, K, seed=M)
    x, res = chain_inputs(M, K, seed=M + 1)
    h_want = res + x
    n, h = norm.forward_residual(x, res)
    assert ",ADD=1> [bf16]" in lib.mixq_debug_last_producer_kernel().decode()
    y = layer.forward_quantised(cache.q_xcache, cache.x_scale, cache.activation_outliers, cache.q_layout)
    torch.cuda.synchronize()
    assert lib.mixq_debug_last_gemm_kernel().decode().endswith(" [bf16]")
    assert h.data_ptr() == res.data_ptr() and torch.equal(res.view(torch.int16), h_want.view(torch.int16)), "residual holds h"
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (M, N) and n.dtype == torch.bfloat16
    assert cache.activation_outliers.dtype == torch.bfloat16 and cache.q_layout == lib.mixq_qa_layout(M, N, K)
    q_ref, s_ref = R.quant_rows(R.to_bits(n))
    assert same16(R.to_bits(cache.x_scale.reshape(-1)[:M]), s_ref).size == 0
    want = chain_restatement(p, cache, M, K, cache.q_layout)
    bad = same16(R.to_bits(y), want)
    assert bad.size == 0, f"chain M={M}: {bad.size} of {want.size} outputs differ from the restatement"
    assert torch.isfinite(y.float()).all()


# ---------------------------------------------------------------------------------------------------------- 7. HIP graph ----
def test_bf16_chain_in_a_captured_graph(lib):
    M, N, K = 16, 512, 1024
    p, layer, cache, norm = build_chain(N, K, seed=3)
    x, res0 = chain_inputs(M, K, seed=4)
    res = res0.clone()

    def step():
        res.copy_(res0)
        n, h = norm.forward_residual(x, res)
        return n, layer.forward_quantised(cache.q_xcache, cache.x_scale, cache.activation_outliers, cache.q_layout)

    n_e, y_e = step()                                              # eager warm-up: also the bits to reproduce
    torch.cuda.synchronize()
    n_bits, y_bits, h_bits = R.to_bits(n_e), R.to_bits(y_e), R.to_bits(res)
    assert same16(y_bits, chain_restatement(p, cache, M, K, cache.q_layout)).size == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        n_g, y_g = step()
    for _ in range(2):
        n_g.zero_()
        y_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(R.to_bits(n_g), n_bits) and np.array_equal(R.to_bits(y_g), y_bits) and np.array_equal(R.to_bits(res), h_bits)
