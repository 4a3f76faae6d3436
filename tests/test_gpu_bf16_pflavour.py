"""GPU (-m gpu): bf16 through the P-flavour -- the zeroing quantiser on bf16 rows (mixq_quant_extract_typed), dynamic outlier
detection and the weight columns in bf16 (mixq_find_outliers_typed, mixq_dequant_weight_columns_typed), the two-launch forward
(mixq_mixlinear_forward_typed), and mixlinear.MixLinear_GEMM / MixLlamaMLP with dtype=torch.bfloat16.

Everything is compared bit for bit with tests/bf16_pflavour_restate.py (numpy / torch CPU on top of tests/bf16_restate.py); random
outlier weights stay within bf16_restate.prefill_bound, the bound of the bf16 operator tests.  The C-ABI cases run in buffers of
exactly the declared sizes between guards (tests/guarded.py: 64 KiB for inputs, out_guard for outputs) that are compared after the
call.  Out-of-range indices are only -1 and K."""
import ctypes
import functools

import numpy as np
import pytest

import bf16_pflavour_restate as PR
import bf16_restate as R
import guarded
from test_gpu_producers import frag_image_bytes, qe_form

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HALF, BF16 = 1, 7
OK, SHAPE, ALIGN = 0, 2, 3
NANFILL, QFILL = guarded.BF16_NAN, 0x5A


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
    def __init__(self, nbytes, fill=NANFILL, init=None, guard=guarded.IN_GUARD):
        super().__init__(nbytes, fill, None if init is None else np.array(init), guard=guard, offset=0, device=dev())   # (a writable copy)


def take(buf, dtype, shape, what):
    guarded.assert_intact(buf, what)
    return buf.body(dtype, shape)


def upload(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype in (np.uint16, np.float16) else a).to(dev())


def same16(a, b, nan_above=0x7F80):
    """16-bit patterns equal, any NaN equal to any NaN -> flat indices that differ."""
    ua, ub = np.asarray(a, np.uint16).reshape(-1), np.asarray(b, np.uint16).reshape(-1)
    na, nb = (ua & 0x7FFF) > nan_above, (ub & 0x7FFF) > nan_above
    return np.flatnonzero(~((ua == ub) | (na & nb)))


def bf16_qe_form(M, K, zero, frag=0):
    """The fp16 entry's form name for the same (M, K, layout) + " [bf16]", " nt" behind it."""
    name = qe_form(M, K, zero, None, frag)
    nt = name.endswith(" nt")
    return (name[:-3] if nt else name) + " [bf16]" + (" nt" if nt else "")


# ------------------------------------------------------------------------------------------------- 1. the zeroing quantiser ----
def outlier_set(K, n, seed):
    """0, K - 1, a duplicate and (from 5 entries on) one -1; from 8 entries on also K; the rest random (duplicates allowed)."""
    if n == 0:
        return np.zeros(0, np.int32)
    rng = np.random.default_rng(seed)
    ind = rng.integers(0, K, n).astype(np.int32)
    ind[:5] = [0, K - 1, 7, 7, -1]
    if n >= 8:
        ind[6] = K
    return ind


def special_rows(M, K, ind, seed):
    """bf16 rows (bits).  Row 0: small values everywhere, the only large ones in the outlier columns (zeroing changes amax: a
    T-flavour kernel fails here), with -0.0 and a subnormal; row 1 all NaN; row 2 all zero; row 3 +-inf; row 4 up to bf16 max."""
    rng = np.random.default_rng(seed)
    A = R.bf16_rn((rng.standard_normal((M, K)) * 3).astype(np.float32))
    real = ind[(ind >= 0) & (ind < K)]
    A[0] = R.bf16_rn(rng.uniform(-0.5, 0.5, K).astype(np.float32))
    A[0, real] = R.bf16_rn((1000.0 + np.arange(real.size)).astype(np.float32))
    A[0, 2], A[0, 3] = 0x8000, 0x0001
    if M > 2:
        A[1] = 0xFFC1
        A[2] = 0
    if M > 4:
        A[3, 5], A[3, 9] = 0x7F80, 0xFF80
        A[4] = R.bf16_rn(rng.uniform(-1, 1, K).astype(np.float32) * 3e38)
        A[4, 6] = 0x7F7F
    return A


def run_qe(lib, A_bits, ind, zero, frag=0, typ=BF16):
    """mixq_quant_extract_typed on exact-size guarded buffers -> dict of the bodies after the call; every guard is checked."""
    M, K = A_bits.shape
    O = ind.size
    a = Buf(A_bits.nbytes, init=A_bits, guard=guarded.out_guard(K, 2))
    q = Buf(frag_image_bytes(M, K) if frag else M * K, QFILL, guard=guarded.out_guard(K, 1))
    s = Buf(2 * M, guard=guarded.out_guard(1, 2))
    f = Buf(2 * M * O, guard=guarded.out_guard(O, 2))
    ip = upload(ind) if O else None
    rc = lib.mixq_quant_extract_typed(M, K, a.ptr, q.ptr, s.ptr, f.ptr if O else None, ip.data_ptr() if O else None, O, int(zero), frag, typ,
                                      stream())
    form = lib.mixq_debug_last_producer_kernel().decode()
    torch.cuda.synchronize()
    w = f"quant_extract_typed {M}x{K} O={O} zero={zero} frag={frag}"
    if frag:
        from mixq_tensorrt_llm_amd import mixlib
        guarded.assert_intact(q, w + " q")
        qb = mixlib.qa_to_row_major(q.body_bytes().view(torch.int8), M, K).cpu().numpy()
    else:
        qb = take(q, np.int8, (M, K), w + " q")
    return dict(rc=rc, form=form, A=take(a, np.uint16, (M, K), w + " A"), q=qb, sA=take(s, np.uint16, None, w + " sA"),
                fpA=take(f, np.uint16, (M, O), w + " fpA"))


def compose_zero_then_quant(lib, A_bits, ind, frag=0):
    """mixq_extract_outliers_set_zero on the in-range indices (a bit copy: it serves bf16 rows unchanged), then the bf16 quantiser
    with len = 0 on the zeroed rows."""
    M, K = A_bits.shape
    real = np.ascontiguousarray(ind[(ind >= 0) & (ind < K)])
    a = Buf(A_bits.nbytes, init=A_bits, guard=guarded.out_guard(K, 2))
    if real.size:
        f = Buf(2 * M * real.size, guard=guarded.out_guard(real.size, 2))
        ip = upload(real)
        assert lib.mixq_extract_outliers_set_zero(M, K, a.ptr, f.ptr, ip.data_ptr(), real.size, stream()) == OK
        torch.cuda.synchronize()
        guarded.assert_intact(f, "set_zero fpA")
    zeroed = take(a, np.uint16, (M, K), "set_zero A")
    got = run_qe(lib, zeroed, np.zeros(0, np.int32), 0, frag)
    assert got["rc"] == OK
    return got


def check_zeroing_case(lib, A_bits, ind, frag=0):
    M, K = A_bits.shape
    what = f"bf16 zeroing quantiser {M}x{K} len={ind.size} frag={frag}"
    q, sA, fpA, z = PR.quant_rows_zeroed(A_bits, ind)
    got = run_qe(lib, A_bits, ind, 1, frag)
    assert got["rc"] == OK, what
    assert got["form"] == bf16_qe_form(M, K, True, frag), f"{what}: the launch took {got['form']!r}"
    assert np.array_equal(got["A"], z), f"{what}: A after the call (zeroed columns 0x0000, every other element unchanged)"
    assert np.array_equal(got["fpA"], fpA), f"{what}: fpA is not a bit copy of the original columns"
    assert same16(got["sA"], sA).size == 0, f"{what}: sA rows {same16(got['sA'], sA)[:6].tolist()}"
    assert np.array_equal(got["q"], q), f"{what}: {int((got['q'] != q).sum())} int8 values differ from the restatement"
    comp = compose_zero_then_quant(lib, A_bits, ind, frag)
    assert np.array_equal(comp["q"], got["q"]) and np.array_equal(comp["sA"], got["sA"]) and np.array_equal(comp["A"], got["A"]), \
        what + ": differs from set_zero + quantiser(len = 0)"
    return got


@pytest.mark.parametrize("K", [72, 1032, 2048, 4096, 8200, 16392, 32776])
@pytest.mark.parametrize("M", [1, 3, 5, 70])
def test_zeroing_quantiser_bit_exact(lib, M, K):
    for n in (0, 5, 128):
        ind = outlier_set(K, n, seed=K + n)
        A_bits = special_rows(M, K, ind, seed=M * 100003 + K + n)
        got = check_zeroing_case(lib, A_bits, ind)
        if n:
            real = ind[(ind >= 0) & (ind < K)]
            assert (got["A"][:, real] == 0).all()
            # the row whose only large values sit in the outlier columns: the scale comes from the small ones
            assert R.bf2f(got["sA"][0]) < 0.01 and R.bf2f(R.quant_rows(A_bits)[1][0]) > 1.0
        if M > 2 and n == 0:
            assert (got["sA"][1] & 0x7FFF) > 0x7F80 and (got["q"][1] == 0).all(), "the all-NaN row: NaN scale, q = 0"
        elif M > 2:   # its zeroed columns are the row's only numbers: amax = 0
            assert got["sA"][1] == 0 and (got["q"][1] == 0).all() and ((got["fpA"][1, ind >= 0][ind[ind >= 0] < K] & 0x7FFF) > 0x7F80).all()
        if M > 2:
            assert got["sA"][2] == 0 and (got["q"][2] == 0).all(), "the all-zero row"
        # zero_outliers = 0 in bf16: the quantiser a bf16 mixq_enqueue runs; A is untouched
        t = run_qe(lib, A_bits, ind, 0)
        q_t, s_t = R.quant_rows(A_bits)
        what = f"bf16 quantiser {M}x{K} len={n} zero=0"
        assert t["rc"] == OK and t["form"] == bf16_qe_form(M, K, False), f"{what}: {t['rc']} {t['form']!r}"
        assert np.array_equal(t["A"], A_bits), what + ": A was modified"
        assert np.array_equal(t["q"], q_t) and same16(t["sA"], s_t).size == 0, what
        assert np.array_equal(t["fpA"], PR.quant_rows_zeroed(A_bits, ind)[2]), what + ": fpA"


@pytest.mark.parametrize("M,K", [(5, 2048), (33, 8192)])
def test_zeroing_quantiser_fragment_major(lib, M, K):
    assert lib.mixq_qa_layout(M, 4096, K) == 1, "the fragment-major image's domain for N = 4096"
    ind = outlier_set(K, 128, seed=M)
    got = check_zeroing_case(lib, special_rows(M, K, ind, seed=K + M), ind, frag=1)
    assert "FRAG=1> [bf16]" in got["form"]


def test_zeroing_quantiser_non_temporal(lib):
    M, K = 2048, 4096                                              # the smallest image written with non-temporal stores
    ind = outlier_set(K, 128, seed=1)
    got = check_zeroing_case(lib, special_rows(M, K, ind, seed=2), ind)
    assert got["form"].endswith(" [bf16] nt"), got["form"]


# --------------------------------------------------------------------------------------------------------- 2. find_outliers ----
def outlier_rows(M, K, sigma, seed):
    """Rows within +-5 with, in distinct columns: the largest bf16 value that is not above sigma (sigma itself where bf16 holds it:
    not flagged), the next bf16 above it, its negative, a NaN, +-inf."""
    rng = np.random.default_rng(seed)
    A = R.bf16_rn(rng.uniform(-5, 5, (M, K)).astype(np.float32))
    at = int(R.bf16_rn(np.float32(sigma)).reshape(-1)[0])
    if R.bf2f(np.uint16(at)) > np.float32(sigma):
        at -= 1                                                   # (round-to-nearest went up)
    assert R.bf2f(np.uint16(at)) <= np.float32(sigma) < R.bf2f(np.uint16(at + 1))
    specials = [at, at + 1, (at + 1) | 0x8000, 0x7FC0, 0x7F80, 0xFF80]
    cols = [0, 1, 2, 3, 4, 5] if K == 8 else [0, K - 1, 9, 33, K // 2, K - 8]
    for i, (c, v) in enumerate(zip(cols, specials)):
        A[(i * 5) % M if i % 2 else M - 1 - (i % M), c] = v
    want = [c for c, v in zip(cols, specials) if v not in (at, 0x7FC0)]
    return A, sorted(want)


def run_find(lib, A_bits, sigma, capacity):
    M, K = A_bits.shape
    a = Buf(A_bits.nbytes, init=A_bits)
    ws = torch.empty(int(lib.mixq_find_outliers_workspace_size(K)), dtype=torch.uint8, device=dev())
    ind = Buf(4 * capacity, QFILL)
    cnt = Buf(4, QFILL)
    rc = lib.mixq_find_outliers_typed(a.ptr, M, K, ctypes.c_float(sigma), ws.data_ptr(), ind.ptr if capacity else None, cnt.ptr, capacity,
                                      BF16, stream())
    torch.cuda.synchronize()
    w = f"find_outliers {M}x{K} sigma={sigma} capacity={capacity}"
    assert rc == OK, w
    assert np.array_equal(take(a, np.uint16, (M, K), w + " A"), A_bits)
    return int(take(cnt, np.int32, None, w + " count")[0]), take(ind, np.int32, None, w + " ind")


@pytest.mark.parametrize("sigma", [6.0, 6.01])
@pytest.mark.parametrize("K", [8, 72, 4096, 8200])
@pytest.mark.parametrize("M", [1, 7, 300])
def test_find_outliers_bf16(lib, M, K, sigma):
    A_bits, planted = outlier_rows(M, K, sigma, seed=M + K)
    want = PR.find_outliers(A_bits, sigma)
    assert want.tolist() == planted
    count, ind = run_find(lib, A_bits, sigma, K)
    assert count == want.size and np.array_equal(ind[:count], want), (count, ind[:count].tolist(), want.tolist())
    assert (ind[count:].view(np.uint8) == QFILL).all(), "indices past the count were written"


def test_find_outliers_bf16_capacity_below_the_count(lib):
    A_bits, planted = outlier_rows(7, 4096, 6.0, seed=3)
    cap = len(planted) - 2
    count, ind = run_find(lib, A_bits, 6.0, cap)
    assert count == len(planted) and ind.tolist() == planted[:cap]


# ------------------------------------------------------------------------------------------------- 3. dequant_weight_columns ----
@pytest.mark.parametrize("K", [64, 4096])
@pytest.mark.parametrize("N", [1, 16, 272])
def test_dequant_weight_columns_bf16(lib, N, K):
    rng = np.random.default_rng(N + K)
    W = rng.integers(-128, 128, (N, K)).astype(np.int8)
    sW = rng.uniform(0.0005, 0.03, N).astype(np.float16)
    sW[0] = np.float16(6e-8)                                       # a subnormal scale
    if N > 2:
        sW[2] = np.float16(60000.0)
    w_d, s_d = upload(W), upload(sW)
    for n in (1, 8, 13, 128):
        ind = rng.integers(0, K, n).astype(np.int32)
        if n == 1:
            ind[0] = K - 1 if K == 64 else K
        else:
            ind[:4] = [0, -1, K - 1, K]
        out = Buf(2 * N * n, guard=guarded.out_guard(n, 2))
        i_d = upload(ind)
        rc = lib.mixq_dequant_weight_columns_typed(w_d.data_ptr(), s_d.data_ptr(), i_d.data_ptr(), n, out.ptr, N, K, BF16, stream())
        torch.cuda.synchronize()
        what = f"dequant_weight_columns {N}x{K} len={n}"
        got = take(out, np.uint16, (N, n), what)
        want = PR.dequant_columns(W, sW, ind)
        assert rc == OK and np.array_equal(got, want), f"{what}: {int((got != want).sum())} elements differ"
        assert (got[:, (ind < 0) | (ind >= K)] == 0).all()


# ---------------------------------------------------------------------------------------------- 4. mixq_mixlinear_forward_typed ----
FORWARD_CASES = [(5, 272, 2048, 128, 0), (33, 64, 128, 8, 0), (70, 272, 2048, 0, 0), (130, 16, 256, 24, 2), (300, 272, 1152, 128, 0)]


@functools.lru_cache(maxsize=None)
def forward_case(M, N, K, O, pads, exact):
    """x (bf16 bits; the outlier columns x 15), ind (the last `pads` entries -1), W int8, sW fp16, weight_cache (bf16 bits; exact: one
    +-2^e per row, so the outlier product is one term in any order; zero columns under the padding)."""
    rng = np.random.default_rng(M + N + K + O + exact)
    ind = np.full(O, -1, np.int32)
    ind[:O - pads] = rng.choice(K, O - pads, replace=False)
    if O - pads >= 2:
        ind[0], ind[1] = 0, K - 1
        ind[2:O - pads] = rng.choice(np.arange(1, K - 1), O - pads - 2, replace=False)
    x = (rng.standard_normal((M, K)) * 3).astype(np.float32)
    x[:, ind[:O - pads]] *= 15.0
    W = rng.integers(-127, 128, (N, K)).astype(np.int8)
    sW = rng.uniform(0.001, 0.02, N).astype(np.float16)
    wc = np.zeros((N, O), np.float32)
    if O and exact:
        wc[np.arange(N), rng.integers(0, O - pads, N)] = np.exp2(rng.integers(-6, 3, N)) * rng.choice([-1.0, 1.0], N)
    elif O:
        wc[:, :O - pads] = rng.standard_normal((N, O - pads)) * 0.05
    out = (R.bf16_rn(x), ind, W, sW, R.bf16_rn(wc))
    for a in out:
        a.setflags(write=False)
    return out


def run_forward(lib, x_bits, ind, W, sW, wc_bits, layout, typ=BF16, named=False, O_arg=None, out_offset=0):
    M, K = x_bits.shape
    N, O = W.shape[0], ind.size
    xg = Buf(x_bits.nbytes, init=x_bits, guard=guarded.out_guard(K, 2))
    q = Buf(frag_image_bytes(M, K) if layout else M * K, QFILL, guard=guarded.out_guard(K, 1))
    s, f = Buf(2 * M, guard=guarded.out_guard(1, 2)), Buf(2 * M * O, guard=guarded.out_guard(max(O, 1), 2))
    out = Buf(2 * M * N + out_offset, guard=guarded.out_guard(N, 2))
    ts = [upload(a) for a in (W, sW)] + [upload(ind) if O else None, upload(wc_bits) if O else None]
    w_d, s_d, i_d, c_d = (t.data_ptr() if t is not None else None for t in ts)
    head = (M, N, K, O if O_arg is None else O_arg, xg.ptr, i_d, w_d, s_d, c_d, s.ptr, q.ptr, f.ptr if O else None, out.ptr + out_offset, layout)
    if named:
        rc = lib.mixq_mixlinear_forward(*head, None, 0, stream())
    else:
        rc = lib.mixq_mixlinear_forward_typed(*head, typ, None, 0, stream())
    prod, kern = lib.mixq_debug_last_producer_kernel().decode(), lib.mixq_debug_last_gemm_kernel().decode()
    torch.cuda.synchronize()
    w = f"mixlinear_forward {M}x{N}x{K} O={O} layout={layout}"
    if layout:
        from mixq_tensorrt_llm_amd import mixlib
        guarded.assert_intact(q, w + " q_x")
        qb = mixlib.qa_to_row_major(q.body_bytes().view(torch.int8), M, K).cpu().numpy()
    else:
        qb = take(q, np.int8, (M, K), w + " q_x")
    return dict(rc=rc, prod=prod, kern=kern, x=take(xg, np.uint16, (M, K), w + " x"), q=qb, sA=take(s, np.uint16, None, w + " x_scale"),
                fpA=take(f, np.uint16, (M, O), w + " outliers"), out=take(out, np.uint16, None, w + " out")[out_offset // 2:].reshape(M, N))


def three_calls(lib, x_bits, ind, W, sW, wc_bits, layout):
    """set-zero extract (in-range indices; the padding's outlier columns are zero), the bf16 quantiser, mixq_gemm_mixed_typed."""
    M, K = x_bits.shape
    N, O = W.shape[0], ind.size
    real = (ind >= 0) & (ind < K)
    xg = Buf(x_bits.nbytes, init=x_bits, guard=guarded.out_guard(K, 2))
    fpA = np.zeros((M, O), np.uint16)
    if real.any():
        fr = Buf(2 * M * int(real.sum()), guard=guarded.out_guard(O, 2))
        ip = upload(np.ascontiguousarray(ind[real]))
        assert lib.mixq_extract_outliers_set_zero(M, K, xg.ptr, fr.ptr, ip.data_ptr(), int(real.sum()), stream()) == OK
        torch.cuda.synchronize()
        fpA[:, real] = take(fr, np.uint16, (M, int(real.sum())), "set_zero outliers")
    q = Buf(frag_image_bytes(M, K) if layout else M * K, QFILL, guard=guarded.out_guard(K, 1))
    s = Buf(2 * M, guard=guarded.out_guard(1, 2))
    assert lib.mixq_quant_extract_typed(M, K, xg.ptr, q.ptr, s.ptr, None, None, 0, 0, layout, BF16, stream()) == OK
    out = Buf(2 * M * N, guard=guarded.out_guard(N, 2))
    ts = [upload(a) for a in (W, sW)] + [upload(fpA) if O else None, upload(wc_bits) if O else None]
    w_d, s_d, f_d, c_d = (t.data_ptr() if t is not None else None for t in ts)
    assert lib.mixq_gemm_mixed_typed(q.ptr, w_d, s.ptr, s_d, f_d, c_d, None, out.ptr, M, N, K, O, layout, BF16, None, 0, stream()) == OK
    kern = lib.mixq_debug_last_gemm_kernel().decode()
    torch.cuda.synchronize()
    for g in (xg, q, s):
        guarded.assert_intact(g, "three calls")
    return take(out, np.uint16, (M, N), "three calls out"), kern


@pytest.mark.parametrize("M,N,K,O,pads", FORWARD_CASES, ids=[f"{m}x{n}x{k}-O{o}" for m, n, k, o, _ in FORWARD_CASES])
def test_mixlinear_forward_bf16(lib, M, N, K, O, pads):
    layout = int(lib.mixq_qa_layout(M, N, K))
    x_bits, ind, W, sW, wc = forward_case(M, N, K, O, pads, True)
    what = f"bf16 mixlinear_forward {M}x{N}x{K} O={O} layout={layout}"
    got = run_forward(lib, x_bits, ind, W, sW, wc, layout)
    assert got["rc"] == OK, what
    assert got["prod"] == bf16_qe_form(M, K, True, layout) and got["kern"].endswith(" [bf16]"), f"{what}: {got['prod']!r}, {got['kern']!r}"
    want, q, sA, fpA, z = PR.forward(x_bits, ind, W, sW, wc)
    assert np.array_equal(got["x"], z) and np.array_equal(got["q"], q) and np.array_equal(got["fpA"], fpA), what + ": the producer's outputs"
    assert same16(got["sA"], sA).size == 0, what + ": x_scale"
    bad = same16(got["out"], want)
    assert bad.size == 0, f"{what} ({got['kern']}): {bad.size} of {want.size} outputs differ from the restatement, first {bad[:6].tolist()}"
    comp, kern = three_calls(lib, x_bits, ind, W, sW, wc, layout)
    assert kern == got["kern"] and np.array_equal(comp, got["out"]), what + ": differs from the three-call composition"
    # random outlier weights: one bf16 step of the result plus one ulp of P
    if O:
        x_bits, ind, W, sW, wc = forward_case(M, N, K, O, pads, False)
        got = run_forward(lib, x_bits, ind, W, sW, wc, layout)
        assert got["rc"] == OK
        ref64, P64 = PR.forward_reference64(x_bits, ind, W, sW, wc)
        err, lim = R.prefill_bound(got["out"], ref64, P64)
        print(f"{what} random outlier weights: max error / bound {float((err / lim).max()):.3f}")
        assert (err <= lim).all(), f"{what}: {int((err > lim).sum())} elements outside bf16_restate.prefill_bound"


def test_mixlinear_forward_half_type_is_the_named_entry(lib):
    M, N, K, O = 70, 272, 2048, 128
    x_bits, ind, W, sW, wc = forward_case(M, N, K, O, 0, False)
    x16 = R.bf2f(x_bits).astype(np.float16).view(np.uint16)
    wc16 = R.bf2f(wc).astype(np.float16).view(np.uint16)
    a = run_forward(lib, x16, ind, W, sW, wc16, 0, typ=HALF)
    b = run_forward(lib, x16, ind, W, sW, wc16, 0, named=True)
    assert a["rc"] == OK and b["rc"] == OK and a["prod"] == b["prod"] and a["kern"] == b["kern"] and "[bf16]" not in a["prod"] + a["kern"]
    for name in ("x", "q", "sA", "fpA", "out"):
        assert np.array_equal(a[name], b[name]), f"MIXQ_TYPE_HALF: {name} differs from mixq_mixlinear_forward"
    assert np.isfinite(a["out"].view(np.float16).astype(np.float32)).all()


def test_a_refused_bf16_forward_leaves_x_untouched(lib):
    M, N, K, O = 33, 64, 128, 8
    x_bits, ind, W, sW, wc = forward_case(M, N, K, O, 0, True)
    got = run_forward(lib, x_bits, np.r_[ind, ind[:4]].astype(np.int32), W, sW, np.zeros((N, 12), np.uint16), 0)     # O = 12
    assert got["rc"] == SHAPE and np.array_equal(got["x"], x_bits)
    assert (got["q"].view(np.uint8) == QFILL).all() and ((got["out"] & 0x7FFF) > 0x7F80).all(), "a refused call wrote something"
    got = run_forward(lib, x_bits, ind, W, sW, wc, 0, out_offset=8)                                                # a misaligned out
    assert got["rc"] == ALIGN and np.array_equal(got["x"], x_bits) and (got["q"].view(np.uint8) == QFILL).all()
    got = run_forward(lib, x_bits, ind, W, sW, wc, 1)                               # a fragment-major image outside its domain
    assert got["rc"] == SHAPE and np.array_equal(got["x"], x_bits)


# ------------------------------------------------------------------------------------------------------------ 5. Python layer ----
LN, LK, SIGMA = 64, 256, 6.0


def make_layer(seed, bias=True, n=LN, k=LK, pow2_scales=False):
    from mixq_tensorrt_llm_amd import mixlinear
    g = torch.Generator().manual_seed(seed)
    Wt = (torch.randn((n, k), generator=g) * 0.05).to(torch.bfloat16)
    b = torch.randn(n, generator=g).to(torch.bfloat16) if bias else None
    cache = mixlinear.MixLibCache(inputdim=64, sigma=SIGMA, device=dev(), dtype=torch.bfloat16)
    layer = mixlinear.MixLinear_GEMM.from_linear(Wt, b, bit=8, cache=cache, dev=dev(), dtype=torch.bfloat16)
    if pow2_scales:   # dequantised outlier weights q * 2^-7: products with small-integer activations add exactly in any order
        layer.scale_col.fill_(2.0 ** -7)
    assert layer.q_weight.dtype == torch.int8 and layer.scale_col.dtype == torch.float16 and layer.ind.numel() == 0
    return layer, cache


def layer_np(layer):
    return (layer.q_weight.cpu().numpy(), layer.scale_col.cpu().numpy().reshape(-1),
            None if layer.bias is None else R.to_bits(layer.bias))


def set_static(layer, ind, exact=True, seed=0):
    """A static padded outlier set: ind (-1 padded to a multiple of 8) and matching weight_cache columns (zero under the padding)."""
    rng = np.random.default_rng(seed)
    n = layer.out_features
    real = np.asarray(ind, np.int32)
    full = np.full((real.size + 7) // 8 * 8, -1, np.int32)
    full[:real.size] = real
    wc = np.zeros((n, full.size), np.float32)
    if exact:
        wc[np.arange(n), rng.integers(0, real.size, n)] = np.exp2(rng.integers(-6, 3, n)) * rng.choice([-1.0, 1.0], n)
    else:
        wc[:, :real.size] = rng.standard_normal((n, real.size)) * 0.05
    layer.ind = upload(full)
    layer.weight_cache = R.from_bits(R.bf16_rn(wc), dev())
    layer.add_outliers = False
    return full, R.bf16_rn(wc)


def acts(M, K, seed, big=()):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((M, K), generator=g) * 1.5).clamp(-4, 4)
    for r, c, v in big:
        x[r, c] = v
    return x.to(torch.bfloat16)


def test_layer_unfused_static_padded_set(lib):
    layer, cache = make_layer(1)
    ind, wc = set_static(layer, [3, 200, 255, 0, 17])
    x = acts(9, LK, 2, big=[(1, 200, 40.0), (4, 0, -33.0)])
    x_bits = R.to_bits(x)
    xd = x.to(dev())
    y = layer.forward(xd, cache, unfused=True)
    torch.cuda.synchronize()
    assert lib.mixq_debug_last_producer_kernel().decode() == bf16_qe_form(9, LK, True, cache.q_layout)
    qw, sW, bias = layer_np(layer)
    want, q, sA, fpA, z = PR.forward(x_bits, ind, qw, sW, wc, bias)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (9, LN)
    assert same16(R.to_bits(y), want).size == 0
    assert np.array_equal(R.to_bits(xd), z) and np.array_equal(R.to_bits(cache.activation_outliers), fpA)
    assert cache.activation_outliers.shape[1] == layer.ind.shape[0] == layer.weight_cache.shape[1] == 8


def test_layer_fused_route_behind_the_bf16_norm(lib):
    from mixq_tensorrt_llm_amd import mixlib, mixlinear
    layer, cache = make_layer(3)
    set_static(layer, [3, 200, 255, 0, 17], exact=False)
    gamma = (1 + 0.1 * torch.randn(LK, generator=torch.Generator().manual_seed(4))).to(torch.bfloat16).to(dev())
    norm = mixlinear.FasterTransformerRMSNorm(gamma, 1e-5, cache, dtype=torch.bfloat16)
    norm.next_layer = layer
    x = acts(9, LK, 5, big=[(1, 200, 40.0)]).to(dev())
    n = norm(x)
    y = layer(n, cache)
    want = mixlib.gemm_mixed(cache.q_xcache, layer.q_weight, cache.x_scale, layer.scale_col, cache.activation_outliers, layer.weight_cache,
                             9, LN, LK, bias=layer.bias, qa_layout=cache.q_layout)
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and np.array_equal(R.to_bits(y), R.to_bits(want))
    # and the GEMM itself (no bias) within the bound of the restatement on the normalised row with its outliers put back
    plain = mixlib.gemm_mixed(cache.q_xcache, layer.q_weight, cache.x_scale, layer.scale_col, cache.activation_outliers, layer.weight_cache,
                              9, LN, LK, qa_layout=cache.q_layout)
    torch.cuda.synchronize()
    qw, sW, _ = layer_np(layer)
    ind = layer.ind.cpu().numpy()
    n_full = R.to_bits(n).copy()
    real = ind[ind >= 0]
    assert (n_full[:, real] == 0).all()
    n_full[:, real] = R.to_bits(cache.activation_outliers)[:, :real.size]
    ref64, P64 = PR.forward_reference64(n_full, ind, qw, sW, R.to_bits(layer.weight_cache))
    err, lim = R.prefill_bound(R.to_bits(plain), ref64, P64)
    assert (err <= lim).all(), f"{int((err > lim).sum())} elements outside bf16_restate.prefill_bound"
    assert torch.isfinite(y.float()).all()


def test_layer_dynamic_step_adopts_a_new_column(lib):
    from mixq_tensorrt_llm_amd import mixlinear
    layer, cache = make_layer(6, pow2_scales=True)
    held = upload(np.array([5, -1, -1, -1, -1, -1, -1, -1], np.int32))
    layer.ind = held
    layer.weight_cache = mixlinear.dequant_weight_columns(layer.q_weight, layer.scale_col, held, dtype=torch.bfloat16)
    assert layer.add_outliers is True
    x = acts(9, LK, 7)
    g = torch.Generator().manual_seed(8)
    x[:, 5] = torch.randint(-64, 65, (9,), generator=g).to(torch.bfloat16)     # small integers: exact products, exact sums
    x[2, 100] = 50.0
    x[7, 100] = -24.0
    x_bits = R.to_bits(x)
    xd = x.to(dev())
    y = layer.forward(xd, cache, unfused=True)
    torch.cuda.synchronize()
    ind = layer.ind.cpu().numpy()
    assert ind.tolist() == [5, 100, -1, -1, -1, -1, -1, -1], ind.tolist()
    assert cache.new_ind.cpu().numpy().tolist() == [100] and cache.ind is layer.ind
    assert layer.weight_cache.shape == (LN, 8) and cache.activation_outliers.shape == (9, 8)
    qw, sW, bias = layer_np(layer)
    wc = PR.dequant_columns(qw, sW, ind)
    assert np.array_equal(R.to_bits(layer.weight_cache), wc)
    want, q, sA, fpA, z = PR.forward(x_bits, ind, qw, sW, wc, bias)
    assert np.array_equal(R.to_bits(xd), z), "the new column is zeroed in the inputs"
    assert np.array_equal(R.to_bits(cache.activation_outliers), fpA)
    assert np.array_equal(cache.q_xcache.cpu().numpy(), q) and cache.q_layout == 0, "the rows are re-quantised row-major"
    bad = same16(R.to_bits(y), want)
    assert bad.size == 0, f"{bad.size} outputs differ from the restatement with the grown set"
    assert layer.add_outliers is True and layer.cnt == 1
    # nothing above sigma is left: the next call adds nothing and reaches cache.stop
    y2 = layer.forward(x.to(dev()), cache, unfused=True)
    torch.cuda.synchronize()
    assert layer.ind.cpu().numpy().tolist() == ind.tolist() and layer.add_outliers is False
    assert same16(R.to_bits(y2), want).size == 0


def test_layer_with_128_real_columns_stops_detecting(lib):
    from mixq_tensorrt_llm_amd import mixlinear
    layer, cache = make_layer(9, bias=False)
    held = upload(np.arange(128, dtype=np.int32))
    layer.ind = held
    layer.weight_cache = mixlinear.dequant_weight_columns(layer.q_weight, layer.scale_col, held, dtype=torch.bfloat16)
    x = acts(9, LK, 10, big=[(3, 200, 50.0)])
    y = layer.forward(x.to(dev()), cache, unfused=True)
    torch.cuda.synchronize()
    assert layer.ind is held and layer.add_outliers is False and layer.weight_cache.shape == (LN, 128)
    qw, sW, bias = layer_np(layer)
    ref64, P64 = PR.forward_reference64(R.to_bits(x), np.arange(128), qw, sW, R.to_bits(layer.weight_cache))
    err, lim = R.prefill_bound(R.to_bits(y), ref64, P64)
    assert (err <= lim).all(), f"{int((err > lim).sum())} elements outside bf16_restate.prefill_bound"


def test_gate_projection_fused_silu_mul(lib):
    from mixq_tensorrt_llm_amd import mixlib
    up, cache = make_layer(11, bias=False)
    gate, _ = make_layer(12, bias=False)
    set_static(up, [3, 200, 255, 0, 17], exact=False)
    x = acts(9, LK, 13, big=[(1, 200, 40.0)]).to(dev())
    up_out = up.forward(x, cache, unfused=True)
    got = gate.forward_without_preconditionFusedSilu(x, cache, mul=up_out)
    assert lib.mixq_debug_last_gemm_kernel().decode().endswith(" [bf16]")
    assert gate.ind is up.ind
    wc = PR.dequant_columns(gate.q_weight.cpu().numpy(), gate.scale_col.cpu().numpy().reshape(-1), up.ind.cpu().numpy())
    assert np.array_equal(R.to_bits(gate.weight_cache), wc)
    want = mixlib.gemm_mixed(cache.q_xcache, gate.q_weight, cache.x_scale, gate.scale_col, cache.activation_outliers, gate.weight_cache,
                             9, LN, LK, qa_layout=cache.q_layout, act="silu", mul=up_out)
    torch.cuda.synchronize()
    assert got.dtype == torch.bfloat16 and np.array_equal(R.to_bits(got), R.to_bits(want))
    assert torch.isfinite(got.float()).all() and got.float().abs().max() > 0


def test_mlp_on_three_bf16_layers(lib):
    """MixLlamaMLP unchanged on three bf16 layers behind a bf16 norm, dynamic detection on.  Up and down: within
    bf16_restate.prefill_bound of the restatement on the layer's own input and final set; the gate projection: its pre-activation
    GEMM within the same bound, and the fused SiLU x up launch bit-identical to mixlib.gemm_mixed(act="silu", mul=) (whose rule
    tests/test_gpu_silu_epilogue.py pins)."""
    from mixq_tensorrt_llm_amd import mixlib, mixlinear
    H, I, M = 256, 64, 9
    up, cache = make_layer(21, bias=False, n=I, k=H)
    gate, _ = make_layer(22, bias=False, n=I, k=H)
    down, _ = make_layer(23, bias=False, n=H, k=I)
    down.cache = cache
    gamma = (1 + 0.1 * torch.randn(H, generator=torch.Generator().manual_seed(24))).to(torch.bfloat16).to(dev())
    norm = mixlinear.FasterTransformerRMSNorm(gamma, 1e-5, cache, dtype=torch.bfloat16)
    norm.next_layer = up
    mlp = mixlinear.MixLlamaMLP(gate, down, up, cache)
    x = acts(M, H, 25, big=[(1, 200, 60.0), (5, 31, -45.0)]).to(dev())
    n = norm(x)
    n0 = R.to_bits(n).copy()                                       # before the up projection zeroes its new columns
    assert (R.bf2f(n0) > SIGMA).any()
    y = mlp(n)
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (M, H) and torch.isfinite(y.float()).all()
    up_ind = up.ind.cpu().numpy()
    assert up_ind.size % 8 == 0 and {31, 200} <= set(up_ind.tolist()) and gate.ind is up.ind
    assert up.weight_cache.shape[1] == up_ind.size == gate.weight_cache.shape[1]

    def bound(got_bits, x_bits, layer):
        wc = R.to_bits(layer.weight_cache) if layer.ind.shape[0] else np.zeros((layer.out_features, 0), np.uint16)   # (no columns: no cache)
        ref64, P64 = PR.forward_reference64(x_bits, layer.ind.cpu().numpy(), layer.q_weight.cpu().numpy(),
                                            layer.scale_col.cpu().numpy().reshape(-1), wc)
        err, lim = R.prefill_bound(got_bits, ref64, P64)
        return float((err / lim).max())

    # replay the pieces on the final sets (static now: the same bits the MLP computed, since detection added nothing further)
    for layer in (up, gate, down):
        layer.add_outliers = False
    n2 = R.from_bits(n0, dev())
    up_out = up.forward(n2, cache, unfused=True)
    assert bound(R.to_bits(up_out), n0, up) <= 1.0
    gate_plain = mixlib.gemm_mixed(cache.q_xcache, gate.q_weight, cache.x_scale, gate.scale_col, cache.activation_outliers,
                                   gate.weight_cache, M, I, H, qa_layout=cache.q_layout)
    assert bound(R.to_bits(gate_plain), n0, gate) <= 1.0
    gate_out = gate.forward_without_preconditionFusedSilu(n2, cache, mul=up_out)
    want = mixlib.gemm_mixed(cache.q_xcache, gate.q_weight, cache.x_scale, gate.scale_col, cache.activation_outliers, gate.weight_cache,
                             M, I, H, qa_layout=cache.q_layout, act="silu", mul=up_out)
    assert np.array_equal(R.to_bits(gate_out), R.to_bits(want))
    g_bits = R.to_bits(gate_out).copy()
    y2 = down.forward(gate_out, None, True)
    torch.cuda.synchronize()
    assert bound(R.to_bits(y2), g_bits, down) <= 1.0
    assert np.array_equal(R.to_bits(y2), R.to_bits(y)), "the MLP's result is the composition of its three layers"


def test_static_route_in_a_captured_graph(lib):
    layer, cache = make_layer(31)
    ind, wc = set_static(layer, [3, 200, 255, 0, 17])
    x0 = acts(9, LK, 32, big=[(1, 200, 40.0)]).to(dev())
    x = x0.clone()

    def step():
        x.copy_(x0)                                                # (the forward zeroes the outlier columns of its input)
        return layer.forward(x, cache, unfused=True)

    y_e = step()                                                   # eager warm-up: also the bits to reproduce
    torch.cuda.synchronize()
    y_bits = R.to_bits(y_e)
    qw, sW, bias = layer_np(layer)
    assert same16(y_bits, PR.forward(R.to_bits(x0), ind, qw, sW, wc, bias)[0]).size == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g = step()
    for _ in range(2):
        y_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(R.to_bits(y_g), y_bits)
