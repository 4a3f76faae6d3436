"""The activation producers -- the int8 quantiser + outlier gather (csrc/quant_kernels.hip), the fused RMSNorm producer
(csrc/norm_kernels.hip), the 4-bit quantiser (csrc/int4_kernels.hip) and Int8quantize -- BIT-EXACT against the oracle in
every form their launchers can pick: block-per-row 256 x {2, 4}, wavefront-per-row 64 x {2, 4, 8, 16} (four rows per block),
256 x {8, 16}, the two-pass long form, each with and without the outlier zeroing (P / T flavour), the fragment-major qA image
(FRAG), and the non-temporal stores of 8 Mi-element images.

A producer that is off by one int8 step on a few elements still passes every end-to-end tolerance, so each case here compares
qA / sA / fpA (and the mutated A) bit for bit, in guarded buffers whose bytes around the output must stay untouched, and asserts
which form the launch took (mixq_debug_last_producer_kernel); the last GPU test asserts that the whole list of forms was reached.
The forms are forced with the quantisers' block-per-row knob (mixq_debug_set_gemm_variant 1301 + n: 64 << n rows; 1300: the
measured rules), reset around every case.

The permutation into the fragment-major image is written here from its description in include/mixq.h, not from
mixlib.qa_to_row_major; a CPU test checks that the two are inverses."""
import ctypes

import numpy as np
import pytest

import guarded
from conftest import make_layer

torch = pytest.importorskip("torch")

MIXQ_E_SHAPE = 2
GUARD = 256                  # bytes of pattern in front of and behind every output buffer
QFILL, HFILL = 0x5A, 0xA5    # guard / pre-fill bytes: int8 outputs, fp16 outputs (0xA5A5: a normal negative fp16)
KNOB_BLOCK_ROWS_64 = 1301    # block-per-row up to 64 rows: 65.. rows take the wavefront forms wherever K <= 8192
NT_ELEMS = 8 << 20           # images of at least this many elements are written with non-temporal stores

REACHED = set()              # producer forms the GPU tests below have run (and checked)


# ---------------------------------------------------------------------------------------------- fragment-major layout ----
def frag_offsets(M, K):
    """Byte offset of element (row r, column k) of a row-major [M, K] int8 matrix in the fragment-major image (include/mixq.h,
    MIXQ_QA_FRAGMENT_MAJOR): for 16-row tile t and 64-byte k-step s, the 1-KiB block t * ceil(K / 64) + s holds at lane * 16 the
    16 bytes (row t * 16 + lane % 16, k = s * 64 + (lane / 16) * 16 ...)."""
    steps = (K + 63) // 64
    r = np.arange(M, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    lane = r % 16 + 16 * ((k % 64) // 16)
    return ((r // 16) * steps + k // 64) * 1024 + lane * 16 + k % 16


def frag_image_bytes(M, K):
    """Whole 16-row tiles x whole 64-byte k-steps."""
    return ((M + 15) // 16) * ((K + 63) // 64) * 1024


def frag_permute(q, fill):
    """Row-major int8 [M, K] -> the fragment-major image; the padding (rows M.. of the last tile, k = K.. of the last k-step) holds
    ``fill``."""
    M, K = q.shape
    img = np.full(frag_image_bytes(M, K), np.int8(np.uint8(fill).view(np.int8)), np.int8)
    img[frag_offsets(M, K)] = q
    return img


FRAG_M = [5, 16, 17, 33, 64]
FRAG_K = [1088, 1040, 4144, 8208, 16368]     # K % 64 = 0, 16, 48, 16, 48; 256 x 2, 256 x 2, 256 x 4, 256 x 8, 256 x 8


def test_frag_permutation_inverts_qa_to_row_major():
    """CPU: the forward permutation above and mixlib.qa_to_row_major are inverses, for every shape the image tests use."""
    from mixq_tensorrt_llm_amd import mixlib
    rng = np.random.default_rng(0)
    for M in FRAG_M:
        for K in FRAG_K:
            q = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
            off = frag_offsets(M, K)
            assert np.unique(off).size == M * K and off.max() < frag_image_bytes(M, K)
            img = frag_permute(q, QFILL)
            back = mixlib.qa_to_row_major(torch.from_numpy(img), M, K).numpy()
            assert np.array_equal(back, q), (M, K)
            # and the other way round: the permutation of what qa_to_row_major reads is the image, on every non-padding byte
            noise = rng.integers(-128, 128, size=frag_image_bytes(M, K), dtype=np.int8)
            rm = mixlib.qa_to_row_major(torch.from_numpy(noise), M, K).numpy()
            assert np.array_equal(frag_permute(rm, QFILL)[off], noise[off]), (M, K)


# ------------------------------------------------------------------------------------------------------------ helpers ----
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded(guarded.Guarded):
    """A device buffer of ``nbytes`` with GUARD bytes of ``fill`` in front and behind (and, unless ``init`` is given, ``fill``
    inside).  ``ptr`` is 256-byte aligned like the allocation.  (tests/guarded.py: the buffer every GPU test file shares.)"""

    def __init__(self, nbytes, fill, init=None):
        super().__init__(nbytes, fill, init, guard=GUARD, offset=0, device=dev())


def take(lib, guarded, dtype, shape, what):
    body, ok = guarded.get(dtype, shape)
    assert ok, f"{what}: a write outside the buffer (guard bytes changed)"
    return body


def last_form(lib):
    return lib.mixq_debug_last_producer_kernel().decode()


def note_form(lib, want, what):
    got = last_form(lib)
    assert got == want, f"{what}: the launch took {got!r}, expected {want!r}"
    REACHED.add(got)


def qe_form(M, K, zero, block_rows=None, frag=0):
    """The form launch_quant_extract picks (block_rows: the knob's threshold, None = the measured rules)."""
    nvec = K // 8
    thr = block_rows if block_rows is not None else (2048 if nvec <= 512 else 1 << 40)
    t = None
    if (M <= thr or frag) and nvec > 128:
        t = (256, 2) if nvec <= 512 else (256, 4) if nvec <= 1024 else None
    if t is None:
        t = next(((a, b) for a, b in [(64, 2), (64, 4), (64, 8), (64, 16), (256, 8), (256, 16)] if nvec <= a * b), None)
    if t is None:
        return f"quant_extract_long_kernel<ZERO={int(zero)}>"
    nt = " nt" if frag == 0 and M * K >= NT_ELEMS else ""
    return f"quant_extract_kernel<TPR={t[0]},MAXV={t[1]},ZERO={int(zero)},FRAG={frag}>{nt}"


def norm_form(M, K, quant, block_rows=None, frag=0):
    """The form launch_rmsnorm_quant picks (its block-per-row rule has no row limit unless the knob sets one)."""
    nvec = K // 8
    thr = block_rows if block_rows is not None else 1 << 40
    t = None
    if (M <= thr or frag) and nvec > 128:
        t = (256, 2) if nvec <= 512 else (256, 4) if nvec <= 1024 else None
    if t is None:
        t = next((a, b) for a, b in [(64, 2), (64, 4), (64, 8), (64, 16), (256, 8), (256, 16)] if nvec <= a * b)
    nt = " nt" if quant == 8 and frag == 0 and M * K >= NT_ELEMS else ""
    return f"rmsnorm_quant_kernel<TPR={t[0]},MAXV={t[1]},QUANT={quant},FRAG={frag}>{nt}"


@pytest.fixture(scope="module")
def lib():
    from mixq_tensorrt_llm_amd import _lib
    lib = _lib.load()
    assert lib.mixq_debug_knobs_enabled() == 1, "the form knobs need MIXQ_DEBUG_KNOBS=1 (tests/conftest.py)"
    lib.mixq_debug_reset()
    yield lib
    lib.mixq_debug_reset()


@pytest.fixture()
def knob(lib):
    """Set one quantiser knob for the case; every knob back to its default afterwards, pass or fail."""
    def set_(v):
        if v is not None:
            lib.mixq_debug_set_gemm_variant(v)
    yield set_
    lib.mixq_debug_reset()


def activations(M, K, seed):
    """fp16 rows with one special row each up front: zero, a NaN in the last column, all NaN, +-inf, 65504 in the last vector,
    a subnormal maximum, the maximum in the last / the first column.  One row: the last-column maximum."""
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((M, K)) * np.exp(rng.uniform(-4, 4, (M, 1)))).astype(np.float16)
    specials = []

    def last_max(r):
        r[K - 1] = np.float16(1000.0)

    def first_max(r):
        r[0] = np.float16(-3000.0)

    def zero(r):
        r[:] = 0

    def nan_last(r):
        r[K - 1] = np.nan

    def all_nan(r):
        r[:] = np.nan

    def infs(r):
        r[K // 2] = np.inf
        r[0] = -np.inf

    def big(r):
        r[max(K - 5, 0)] = np.float16(65504.0)

    def subnormal(r):
        r[:] = (rng.uniform(-1, 1, K) * 2.0 ** -15).astype(np.float16)   # |x| < 2^-14: every value subnormal

    specials = [last_max] if M == 1 else [zero, nan_last, all_nan, infs, big, subnormal, last_max, first_max]
    for i, f in enumerate(specials[:M]):
        f(A[i])
    return A


def outlier_columns(K, O, seed):
    """O distinct columns including column 0, K - 1, columns of the row's last 16-byte vector and one on a 64-vector
    boundary, the rest random."""
    O = min(O, K)
    rng = np.random.default_rng(seed)
    want = [K - 1, 0, K - 8, K - 3, min(64 * 8 - 1, K - 2), min(64 * 8, K - 4), K - 2, 1]
    cols = []
    for c in want:
        if 0 <= c < K and c not in cols and len(cols) < O:
            cols.append(c)
    rest = np.setdiff1d(np.arange(K), cols)
    cols += rng.choice(rest, O - len(cols), replace=False).tolist()
    return np.array(cols, np.int32)


def run_quant_extract(lib, A, ind, zero, frag=0):
    """mixq_quant_extract(_layout) on guarded buffers -> (A after, qA body, sA, fpA, qA image guard ok).  frag: qA is the
    fragment-major image, pre-filled with QFILL."""
    M, K = A.shape
    O = ind.size
    a = Guarded(A.nbytes, HFILL, A)
    qbytes = frag_image_bytes(M, K) if frag else M * K
    q = Guarded(qbytes, QFILL)
    s = Guarded(2 * M, HFILL)
    f = Guarded(2 * M * O, HFILL)
    i_d = torch.from_numpy(ind).to(dev()) if O else None
    ip = i_d.data_ptr() if O else None
    if frag:
        rc = lib.mixq_quant_extract_layout(M, K, a.ptr, q.ptr, s.ptr, f.ptr if O else None, ip, O, int(zero), 1, stream())
    else:
        rc = lib.mixq_quant_extract(M, K, a.ptr, q.ptr, s.ptr, f.ptr if O else None, ip, O, int(zero), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    what = f"quant_extract {M}x{K} O={O} zero={zero} frag={frag}"
    return (take(lib, a, np.float16, (M, K), what + " A"), take(lib, q, np.int8, None, what + " qA"),
            take(lib, s, np.float16, None, what + " sA"), take(lib, f, np.float16, (M, O), what + " fpA"))


def check_flavours(oracle, lib, A, ind, form_of, what):
    """T flavour (A untouched) and P flavour (outlier columns zeroed in A first) through the C ABI, bit-exact, in the expected
    form.  Returns the oracle's P-flavour result for further checks."""
    M, K = A.shape
    # T: gather + quantise, A untouched, the outliers count toward amax
    a_t, q_t, s_t, f_t = run_quant_extract(lib, A, ind, zero=False)
    note_form(lib, form_of(False), what + " T")
    qo, so = oracle.quant_rows(A)
    assert np.array_equal(bits(a_t), bits(A)), f"{what} T: A was modified"
    assert np.array_equal(bits(s_t), bits(so)), f"{what} T: sA differs in rows {np.flatnonzero(bits(s_t) != bits(so))[:8]}"
    bad = np.argwhere(q_t.reshape(M, K) != qo)
    assert bad.size == 0, f"{what} T: {len(bad)} qA bytes differ, first (row, k) {bad[:4].tolist()}"
    assert np.array_equal(bits(f_t), bits(A[:, ind])), f"{what} T: fpA differs"
    # P: the outlier columns are zeroed in A, then leave amax / quantisation
    a_p, q_p, s_p, f_p = run_quant_extract(lib, A, ind, zero=True)
    note_form(lib, form_of(True), what + " P")
    Az = A.copy()
    fz = oracle.extract_outliers(Az, ind, set_zero=True)
    qz, sz = oracle.quant_rows(Az)
    assert np.array_equal(bits(a_p), bits(Az)), f"{what} P: A not mutated exactly as the oracle mutates it"
    assert np.array_equal(bits(s_p), bits(sz)), f"{what} P: sA differs in rows {np.flatnonzero(bits(s_p) != bits(sz))[:8]}"
    bad = np.argwhere(q_p.reshape(M, K) != qz)
    assert bad.size == 0, f"{what} P: {len(bad)} qA bytes differ, first (row, k) {bad[:4].tolist()}"
    assert np.array_equal(bits(f_p), bits(fz)), f"{what} P: fpA differs"
    return Az, qz, sz, fz


def check_mixlib_flavours(oracle, lib, A, ind, block_rows, what):
    """The same through mixlib: FindRowScale (T), FindRowScaleFusedExtracOutliers (P), ExtractOutliersAndSetToZeros +
    FindRowScale (P, unfused)."""
    from mixq_tensorrt_llm_amd import mixlib
    M, K = A.shape
    O = ind.size
    qo, so = oracle.quant_rows(A)
    Az = A.copy()
    fz = oracle.extract_outliers(Az, ind, set_zero=True)
    qz, sz = oracle.quant_rows(Az)
    x = torch.from_numpy(A).to(dev())
    s = torch.empty(M, dtype=torch.float16, device=dev())
    q = mixlib.FindRowScale(x, s, M, K, 8)
    note_form(lib, qe_form(M, K, False, block_rows), what + " FindRowScale")
    assert np.array_equal(q.cpu().numpy(), qo) and np.array_equal(bits(s.cpu().numpy()), bits(so)), what + " FindRowScale"
    assert np.array_equal(bits(x.cpu().numpy()), bits(A)), what + " FindRowScale modified A"
    i_d = torch.from_numpy(ind).to(dev())
    x2 = torch.from_numpy(A).to(dev())
    s2 = torch.empty(M, dtype=torch.float16, device=dev())
    q2, f2 = mixlib.FindRowScaleFusedExtracOutliers(x2, s2, i_d, O, M, K)
    note_form(lib, qe_form(M, K, True, block_rows), what + " FindRowScaleFusedExtracOutliers")
    assert np.array_equal(q2.cpu().numpy(), qz) and np.array_equal(bits(s2.cpu().numpy()), bits(sz)), what + " fused P"
    assert np.array_equal(bits(f2.cpu().numpy()), bits(fz)) and np.array_equal(bits(x2.cpu().numpy()), bits(Az)), what + " fused P"
    x3 = torch.from_numpy(A).to(dev())
    f3 = mixlib.ExtractOutliersAndSetToZeros(i_d, x3)
    note_form(lib, "extract_kernel<ZERO=1>", what + " ExtractOutliersAndSetToZeros")
    s3 = torch.empty(M, dtype=torch.float16, device=dev())
    q3 = mixlib.FindRowScale(x3, s3, M, K, 8)
    assert np.array_equal(q3.cpu().numpy(), qz) and np.array_equal(bits(s3.cpu().numpy()), bits(sz)), what + " unfused P"
    assert np.array_equal(bits(f3.cpu().numpy()), bits(fz)) and np.array_equal(bits(x3.cpu().numpy()), bits(Az)), what + " unfused P"


# --------------------------------------------------------------------- 1. int8 quantise + extract: every form, both flavours
# K just below / above each form's nvec boundary (nvec = K / 8: 64 x 2 | 256 x 2 or 64 x 4 | 64 x 8 | 256 x 4 or 64 x 16 | 256 x 8 |
# 256 x 16 | long), rows taking ONE partial vector, and nvec % 64 odd (1016: 127, 2856: 357)
QE_K = [8, 24, 1016, 1024, 1032, 2048, 2056, 2856, 4096, 4104, 8192, 8200, 16384, 16392, 32768, 32776]
# (rows, knob): 1 row and 67 rows (67 % 4 = 3: a partial block of the wavefront forms) with block-per-row up to 64 rows; 6 rows
# under the measured rules
QE_ROWS = [(1, KNOB_BLOCK_ROWS_64), (67, KNOB_BLOCK_ROWS_64), (6, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,knob_v", QE_ROWS, ids=lambda v: str(v))
@pytest.mark.parametrize("K", QE_K)
def test_quant_extract_every_form_bit_exact(oracle, lib, knob, K, M, knob_v):
    knob(knob_v)
    block_rows = 64 if knob_v == KNOB_BLOCK_ROWS_64 else None
    A = activations(M, K, seed=K * 131 + M)
    for O in (0, 1, 8, 128):
        ind = outlier_columns(K, O, seed=K + O)
        what = f"{M}x{K} O={ind.size} knob={knob_v}"
        check_flavours(oracle, lib, A, ind, lambda z: qe_form(M, K, z, block_rows), what)
    check_mixlib_flavours(oracle, lib, A, outlier_columns(K, 128, seed=K), block_rows, f"{M}x{K} knob={knob_v}")


# many rows under the measured rules: just below / at the 8 Mi-element non-temporal mark (block-per-row up to 2048 rows at K = 4096),
# one row past the block-per-row limit, the widest wavefront form and the 256 x 16 form at prefill sizes
QE_LARGE = [(2047, 4096), (2048, 4096), (2049, 4096), (8192, 1024), (257, 32768)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,K", QE_LARGE)
def test_quant_extract_large_and_non_temporal(oracle, lib, knob, M, K):
    knob(None)
    A = activations(M, K, seed=M + K)
    ind = outlier_columns(K, 128, seed=K)
    check_flavours(oracle, lib, A, ind, lambda z: qe_form(M, K, z), f"{M}x{K}")


# --------------------------------------------------------------------------- 2. fused RMSNorm producer: every form x quant 0 / 8 / 4
NORM_K = [8, 1024, 1032, 2048, 2056, 2856, 4096, 4104, 8192, 8200, 16384, 16392, 32768]
EPS = 1e-5


def norm_inputs(M, K, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((M, K)) * np.exp(rng.uniform(-3, 3, (M, 1)))).astype(np.float16)
    if M > 2:
        x[0] = 0                                # rstd = 1 / sqrt(eps)
        x[1, K - 1] = np.float16(30000.0)       # one dominant element, in the row's last vector
    gamma = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float16)
    return x, gamma


def assert_normalised(out_np, o_ref, what):
    """(1) the normalised row within one fp16 ulp of the ideal one (the sum of squares is reduced in another order)."""
    denom = np.maximum(np.abs(o_ref.astype(np.float64)), 1e-3)
    err = (np.abs(out_np.astype(np.float64) - o_ref.astype(np.float64)) / denom).max()
    assert err < 1.1e-3, f"{what}: normalised row off by {err:.3e} relative"


def run_norm(lib, x, gamma, ind, quant, frag=0):
    """mixq_rmsnorm / mixq_rmsnorm_extract_quant(4 / _layout) on guarded buffers -> (rc, out, outl, q, scale)."""
    M, K = x.shape
    O = 0 if ind is None else ind.size
    xd = torch.from_numpy(x).to(dev())
    g = torch.from_numpy(gamma).to(dev())
    out = Guarded(2 * M * K, HFILL)
    outl = Guarded(2 * M * O, HFILL)
    qbytes = M * K // 2 if quant == 4 else (frag_image_bytes(M, K) if frag else M * K)
    q = Guarded(qbytes, QFILL)
    sc = Guarded(2 * M, HFILL)
    ip = torch.from_numpy(ind).to(dev()) if O else None
    args = (M, K, xd.data_ptr(), g.data_ptr(), out.ptr, ctypes.c_float(EPS))
    if quant == 0:
        rc = lib.mixq_rmsnorm(*args, stream())
    elif quant == 4:
        rc = lib.mixq_rmsnorm_extract_quant4(*args, ip.data_ptr() if O else None, O, outl.ptr if O else None, q.ptr, sc.ptr,
                                             stream())
    else:
        rc = lib.mixq_rmsnorm_extract_quant_layout(*args, ip.data_ptr() if O else None, O, outl.ptr if O else None, q.ptr,
                                                   sc.ptr, frag, stream())
    torch.cuda.synchronize()
    what = f"rmsnorm {M}x{K} quant={quant} O={O} frag={frag}"
    return (rc, take(lib, out, np.float16, (M, K), what + " out"), take(lib, outl, np.float16, (M, O), what + " outliers"),
            take(lib, q, np.uint8 if quant == 4 else np.int8, None, what + " q"), take(lib, sc, np.float16, None, what + " scale"))


def check_norm(oracle, lib, x, gamma, block_rows, what):
    """quant 0, then 8 (O = 128 and 1) and 4 (O = 8 and 0) on the same rows, each in its expected form."""
    M, K = x.shape
    rc, plain, _, _, _ = run_norm(lib, x, gamma, None, 0)
    assert rc == 0
    note_form(lib, norm_form(M, K, 0, block_rows), what + " quant 0")
    assert_normalised(plain, oracle.rmsnorm_extract_quant(x, gamma, EPS), what + " quant 0")
    for quant, Os in ((8, (128, 1)), (4, (8, 0))):
        for O in Os:
            ind = outlier_columns(K, O, seed=K + O)
            w = f"{what} quant {quant} O={ind.size}"
            rc, out, outl, q, sc = run_norm(lib, x, gamma, ind, quant)
            assert rc == 0, (w, rc)
            note_form(lib, norm_form(M, K, quant, block_rows), w)
            o_ref, outl_ref, _, _ = oracle.rmsnorm_extract_quant(x, gamma, EPS, ind)
            assert_normalised(out, o_ref, w)
            assert np.all(out[:, ind] == 0), w + ": outlier columns not zeroed"
            assert O == 0 or (np.abs(outl.astype(np.float64) - outl_ref.astype(np.float64))
                              / np.maximum(np.abs(outl_ref.astype(np.float64)), 1e-3)).max() < 1.1e-3, w + ": outliers"
            # the same form without quantisation normalises with the same arithmetic: the row before zeroing, bit for bit
            want_out = plain.copy()
            want_out[:, ind] = 0
            assert np.array_equal(bits(out), bits(want_out)), w + ": normalised row differs from mixq_rmsnorm's"
            assert np.array_equal(bits(outl), bits(plain[:, ind])), w + ": outliers differ from mixq_rmsnorm's row"
            # (2) given the GPU's normalised row, scale and quantised rows are bit-exact
            if quant == 8:
                qz, sz = oracle.quant_rows(out)
                assert np.array_equal(bits(sc), bits(sz)), w + ": scale"
                bad = np.argwhere(q.reshape(M, K) != qz)
                assert bad.size == 0, f"{w}: {len(bad)} int8 bytes differ, first {bad[:4].tolist()}"
            else:
                qz, sz = oracle.quant4_rows(out)
                assert np.array_equal(bits(sc), bits(sz)), w + ": scale"
                bad = np.argwhere(q.reshape(M, K // 2) != qz)
                assert bad.size == 0, f"{w}: {len(bad)} packed int4 bytes differ, first {bad[:4].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("M,knob_v", QE_ROWS, ids=lambda v: str(v))
@pytest.mark.parametrize("K", NORM_K)
def test_rmsnorm_producer_every_form(oracle, lib, knob, K, M, knob_v):
    knob(knob_v)
    x, gamma = norm_inputs(M, K, seed=K * 7 + M)
    check_norm(oracle, lib, x, gamma, 64 if knob_v == KNOB_BLOCK_ROWS_64 else None, f"{M}x{K} knob={knob_v}")


@pytest.mark.gpu
def test_rmsnorm_producer_non_temporal(oracle, lib, knob):
    """An 8 Mi-element image under the measured rules: 256 x 2 with non-temporal int8 stores."""
    knob(None)
    x, gamma = norm_inputs(2048, 4096, seed=5)
    check_norm(oracle, lib, x, gamma, None, "2048x4096")


@pytest.mark.gpu
def test_rmsnorm_producer_rejects_rows_over_32768(lib):
    """K = 32776 is refused with MIXQ_E_SHAPE before anything is launched: every output keeps its bytes."""
    K, M = 32776, 3
    x, gamma = norm_inputs(M, K, seed=1)
    ind = outlier_columns(K, 8, seed=2)
    for quant, frag in ((0, 0), (8, 0), (4, 0), (8, 1)):
        rc, out, outl, q, sc = run_norm(lib, x, gamma, None if quant == 0 else ind, quant, frag)
        assert rc == MIXQ_E_SHAPE, (quant, frag, rc)
        assert np.all(out.view(np.uint8) == HFILL) and np.all(outl.view(np.uint8) == HFILL), (quant, frag)
        assert np.all(q.view(np.uint8) == QFILL) and np.all(sc.view(np.uint8) == HFILL), (quant, frag)


# ----------------------------------------------------------------------------------------- 3. fragment-major images, directly
@pytest.mark.gpu
@pytest.mark.parametrize("K", FRAG_K)
@pytest.mark.parametrize("M", FRAG_M)
def test_quant_extract_fragment_image(oracle, lib, knob, M, K):
    """The image of mixq_quant_extract_layout byte for byte against permute(oracle q), both flavours: the padding of a partial
    16-row tile / 64-byte k-step keeps the buffer's bytes (include/mixq.h); sA / fpA / A as in row-major."""
    knob(None)
    A = activations(M, K, seed=M * K)
    ind = outlier_columns(K, 128, seed=K)
    assert lib.mixq_qa_bytes(M, K, 1) == frag_image_bytes(M, K) and lib.mixq_qa_bytes(M, K, 0) == M * K
    for zero in (False, True):
        a, img, s, f = run_quant_extract(lib, A, ind, zero, frag=1)
        what = f"{M}x{K} zero={zero}"
        note_form(lib, qe_form(M, K, zero, frag=1), what)
        Az = A.copy()
        fo = oracle.extract_outliers(Az, ind, set_zero=zero)
        qo, so = oracle.quant_rows(Az)
        want = frag_permute(qo, QFILL)
        bad = np.flatnonzero(img != want)
        assert bad.size == 0, f"{what}: {bad.size} image bytes differ, first offsets {bad[:6].tolist()}"
        assert np.array_equal(bits(s), bits(so)) and np.array_equal(bits(f), bits(fo)) and np.array_equal(bits(a), bits(Az)), what


@pytest.mark.gpu
@pytest.mark.parametrize("K", FRAG_K)
@pytest.mark.parametrize("M", FRAG_M)
def test_rmsnorm_fragment_image(oracle, lib, knob, M, K):
    """mixq_rmsnorm_extract_quant_layout's image against permute(oracle q of the GPU's normalised row), padding untouched."""
    knob(None)
    x, gamma = norm_inputs(M, K, seed=M + K)
    ind = outlier_columns(K, 128, seed=K)
    rc, out, outl, img, sc = run_norm(lib, x, gamma, ind, 8, frag=1)
    assert rc == 0, rc
    what = f"{M}x{K}"
    note_form(lib, norm_form(M, K, 8, frag=1), what)
    o_ref, _, _, _ = oracle.rmsnorm_extract_quant(x, gamma, EPS, ind)
    assert_normalised(out, o_ref, what)
    qz, sz = oracle.quant_rows(out)
    assert np.array_equal(bits(sc), bits(sz)), what
    bad = np.flatnonzero(img != frag_permute(qz, QFILL))
    assert bad.size == 0, f"{what}: {bad.size} image bytes differ, first offsets {bad[:6].tolist()}"
    # and the row-major producer of the same rows gives the same bits
    rc, out_r, outl_r, q_r, sc_r = run_norm(lib, x, gamma, ind, 8)
    assert rc == 0 and np.array_equal(q_r.reshape(M, K), qz) and np.array_equal(bits(out_r), bits(out))
    assert np.array_equal(bits(outl_r), bits(outl)) and np.array_equal(bits(sc_r), bits(sc))


@pytest.mark.gpu
@pytest.mark.parametrize("M,K", [(65, 4096), (5, 1024), (5, 16392), (64, 16400), (3, 8)])
def test_fragment_layout_rejects_unsupported_shapes(lib, M, K):
    """Outside quant_frag_layout_supported (1..64 rows, 1024 < K <= 16384) both producers refuse the image: MIXQ_E_SHAPE,
    nothing written."""
    A = activations(M, K, seed=3)
    ind = outlier_columns(K, 8, seed=4)
    a = Guarded(A.nbytes, HFILL, A)
    q = Guarded(frag_image_bytes(M, K), QFILL)
    s = Guarded(2 * M, HFILL)
    f = Guarded(2 * M * ind.size, HFILL)
    i_d = torch.from_numpy(ind).to(dev())
    for zero in (0, 1):
        rc = lib.mixq_quant_extract_layout(M, K, a.ptr, q.ptr, s.ptr, f.ptr, i_d.data_ptr(), ind.size, zero, 1, stream())
        assert rc == MIXQ_E_SHAPE, (M, K, zero, rc)
    torch.cuda.synchronize()
    assert np.array_equal(bits(a.get(np.float16, (M, K))[0]), bits(A))
    assert np.all(q.get(np.uint8)[0] == QFILL) and np.all(s.get(np.uint8)[0] == HFILL) and np.all(f.get(np.uint8)[0] == HFILL)
    if K <= 32768:
        x, gamma = norm_inputs(M, K, seed=6)
        rc, out, outl, img, sc = run_norm(lib, x, gamma, ind, 8, frag=1)
        assert rc == MIXQ_E_SHAPE, (M, K, rc)
        assert np.all(img.view(np.uint8) == QFILL) and np.all(out.view(np.uint8) == HFILL)


# (rows, N, K): decode batches mixq_enqueue serves with the fragment-major qA (skinny GEMM), K % 64 in {16, 48, 0}
ENQ_CASES = [(5, 1024, 1040), (17, 1024, 4144), (31, 1024, 1088)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", ENQ_CASES)
def test_enqueue_ignores_stale_image_padding(oracle, lib, knob, M, N, K):
    """mixq_enqueue writes qA into the caller's workspace: with the workspace poisoned, the stale bytes in a partial tile /
    k-step of the image must not reach the output -- the same bits as on a zeroed workspace, and within the operator's bound."""
    from conftest import assert_prefill_parity
    from mixq_tensorrt_llm_amd import plugin
    knob(None)
    A, W, act = make_layer(M, N, K, seed=K)
    # the layer's tensors straight from the oracle's packing steps (the EETQ qweight, read by 1..4-row calls only, is a placeholder:
    # its preprocessing wants K % 64 == 0)
    sW = oracle.weight_scales(W)
    ind = oracle.select_outliers(act, 128)
    p = dict(weight=oracle.quantize_weight(W, sW, ind), weights_scaling_factor=sW, fp_weight=np.ascontiguousarray(W[:, ind]),
             fp_ind=ind.astype(np.int32))

    def carrier(a, shape):
        return torch.from_numpy(np.ascontiguousarray(a)).view(torch.float16).reshape(shape).to(dev())

    plug = plugin.MixQPlugin.create(M, N, K)
    sw = carrier(sW, (N,))
    ins = [torch.from_numpy(A).to(dev()), carrier(p["weight"], (N, K // 2)), sw, carrier(p["fp_weight"], (N, 128)),
           carrier(p["fp_ind"], (256,)), torch.zeros((K, N // 2), dtype=torch.float16, device=dev()), sw]
    nbytes = plug.workspace_size(M, N, K)
    outs = []
    for fill in (HFILL, 0):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev())
        outs.append(plug.enqueue(ins, workspace=ws).cpu().numpy())
        note_form(lib, qe_form(M, K, False, frag=1), f"enqueue {M}x{N}x{K}")
    assert np.array_equal(bits(outs[0]), bits(outs[1])), f"{M}x{N}x{K}: output depends on stale workspace bytes"
    assert_prefill_parity(oracle, outs[1], A, p, f"enqueue {M}x{N}x{K}")


# ------------------------------------------------------------------------- 4. Int8quantize / FindRowScale(bit = 4) across K
SCALE_K = [8, 1016, 1024, 1032, 2056, 4104, 8200, 16392, 32776]


@pytest.mark.gpu
@pytest.mark.parametrize("K", SCALE_K)
def test_int8_quantize_with_scale_bit_exact(oracle, lib, K):
    """Int8quantize (cult.cu:1732-1771) with caller scales: normal, 0, -0, subnormal, +inf, NaN, and the rows' own scales."""
    M = 13
    A = activations(M, K, seed=K)
    _, own = oracle.quant_rows(A)
    s = own.copy()
    s[:6] = np.float16([0.0, -0.0, 6e-8, np.inf, np.nan, 1e-3])
    src = torch.from_numpy(A).to(dev())
    sd = torch.from_numpy(s).to(dev())
    q = Guarded(M * K, QFILL)
    assert lib.mixq_int8_quantize_with_scale(M, K, src.data_ptr(), sd.data_ptr(), q.ptr, stream()) == 0
    torch.cuda.synchronize()
    note_form(lib, "quant_with_scale_kernel", f"{M}x{K}")
    got = take(lib, q, np.int8, (M, K), f"Int8quantize {M}x{K}")
    want = oracle.quant_with_scale(A, s)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{M}x{K}: {len(bad)} bytes differ, first {bad[:4].tolist()}"
    assert np.array_equal(bits(src.cpu().numpy()), bits(A))
    from mixq_tensorrt_llm_amd import mixlib
    assert np.array_equal(mixlib.Int8quantize(src, sd).cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K", [(1, 8), (3, 24), (7, 1032), (13, 2056), (6, 4104), (67, 8200), (5, 16392), (2, 32768)])
def test_find_row_scale_4bit_across_k(oracle, lib, M, K):
    """FindRowScale(bit = 4): packed int4 rows + amax / 7 scales, up to K = 32768, odd numbers of 16-byte vectors, ragged rows."""
    from mixq_tensorrt_llm_amd import mixlib
    A = activations(M, K, seed=K + 4)
    x = torch.from_numpy(A).to(dev())
    s = Guarded(2 * M, HFILL)
    q = Guarded(M * K // 2, QFILL)
    assert lib.mixq_int4quant(M, K, x.data_ptr(), q.ptr, s.ptr, stream()) == 0
    torch.cuda.synchronize()
    note_form(lib, "quant4_rows_kernel", f"{M}x{K}")
    qo, so = oracle.quant4_rows(A)
    got_s = take(lib, s, np.float16, None, "int4 scale")
    got_q = take(lib, q, np.uint8, (M, K // 2), "int4 rows")
    assert np.array_equal(bits(got_s), bits(so))
    bad = np.argwhere(got_q != qo)
    assert bad.size == 0, f"{M}x{K}: {len(bad)} packed bytes differ, first {bad[:4].tolist()}"
    sc = torch.empty(M, dtype=torch.float16, device=dev())
    assert np.array_equal(mixlib.FindRowScale(x, sc, M, K, 4).cpu().numpy(), qo)
    assert np.array_equal(bits(sc.cpu().numpy()), bits(so)) and np.array_equal(bits(x.cpu().numpy()), bits(A))


# ------------------------------------------------------------------------------------------------ 5. every form was reached
def required_forms():
    need = set()
    for z in (0, 1):
        for t, v in [(64, 2), (64, 4), (64, 8), (64, 16), (256, 2), (256, 4), (256, 8), (256, 16)]:
            need.add(f"quant_extract_kernel<TPR={t},MAXV={v},ZERO={z},FRAG=0>")
        for t, v in [(256, 2), (256, 4), (256, 8)]:
            need.add(f"quant_extract_kernel<TPR={t},MAXV={v},ZERO={z},FRAG=1>")
        for t, v in [(256, 2), (64, 8), (64, 2), (256, 16)]:
            need.add(f"quant_extract_kernel<TPR={t},MAXV={v},ZERO={z},FRAG=0> nt")
        need.add(f"quant_extract_long_kernel<ZERO={z}>")
    for quant in (0, 8, 4):
        for t, v in [(64, 2), (64, 4), (64, 8), (64, 16), (256, 2), (256, 4), (256, 8), (256, 16)]:
            need.add(f"rmsnorm_quant_kernel<TPR={t},MAXV={v},QUANT={quant},FRAG=0>")
    for t, v in [(256, 2), (256, 4), (256, 8)]:
        need.add(f"rmsnorm_quant_kernel<TPR={t},MAXV={v},QUANT=8,FRAG=1>")
    need.add("rmsnorm_quant_kernel<TPR=256,MAXV=2,QUANT=8,FRAG=0> nt")
    need |= {"extract_kernel<ZERO=1>", "quant_with_scale_kernel", "quant4_rows_kernel"}
    return need


@pytest.mark.gpu
def test_every_producer_form_was_reached():
    """Runs last in this file: the cases above between them took every form of every producer launcher."""
    need = required_forms()
    missing = sorted(need - REACHED)
    assert not missing, f"producer forms not reached ({len(missing)}): {missing}\nreached: {sorted(REACHED)}"
    print(f"\n{len(REACHED)} producer forms reached:\n  " + "\n  ".join(sorted(REACHED)))
