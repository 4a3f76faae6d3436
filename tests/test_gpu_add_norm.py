"""The residual-add forms of the fused RMSNorm producer (mixq_add_rmsnorm, mixq_add_rmsnorm_extract_quant_layout,
mixq_add_rmsnorm_extract_quant4; csrc/norm_kernels.hip ADD) against the UNFUSED SEQUENCE ON THE SAME LIBRARY: h_ref = x + residual
as a host fp16 add (correctly rounded, like the kernel's), then the existing entry on h_ref.  The existing entries are pinned to
the oracle by test_gpu_norm.py / test_gpu_producers.py; the add forms take the same form and grid for the same (M, K, quant,
layout) and continue on the rounded h, so h, out, outliers, scale and q must be equal BY BIT PATTERN -- no tolerance anywhere.
The one licence: any NaN equals any NaN (a hardware add and a host add may pick different payloads).

Every buffer the entry touches -- x and residual too -- is allocated at exactly its declared size between guard bytes."""
import ctypes

import numpy as np
import pytest

import test_gpu_producers as P
from test_gpu_producers import EPS, HFILL, KNOB_BLOCK_ROWS_64, NORM_K, QE_ROWS, QFILL, Guarded, bits, dev, stream, take

torch = pytest.importorskip("torch")

ADD_MARK = ",ADD=1>"         # include/mixq.h: the add forms report the plain form's name with ",ADD=1" behind FRAG


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


def add_form(M, K, quant, block_rows=None, frag=0):
    return P.norm_form(M, K, quant, block_rows, frag).replace(">", ADD_MARK)


# -------------------------------------------------------------------------------------------------------------- inputs ----
def add_inputs(M, K, seed):
    """x, residual, gamma.  Rows in general position (per-row magnitudes over e^+-3, the two operands of different size so that
    most sums round), and up front as many of these rows as M holds, the three that test the ADD itself first:
      rounding   x ~ N(0, 1), r ~ 8 N(0, 1): nearly every sum needs its rounding
      cancel     r = -x: h is exactly 0 (rstd = 1 / sqrt(eps), scale 0)
      overflow   x = r = 40000: the sum overflows to +inf
    then the producers' own special rows (test_gpu_producers.activations): a zero row, a NaN in the last column, +-inf, 65504 in
    the row's last vector, an all-NaN row, a subnormal row."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((M, K)) * np.exp(rng.uniform(-3, 3, (M, 1)))).astype(np.float16)
    r = (rng.standard_normal((M, K)) * np.exp(rng.uniform(-3, 3, (M, 1)))).astype(np.float16)

    def rounding(i):
        x[i] = rng.standard_normal(K).astype(np.float16)
        r[i] = (8.0 * rng.standard_normal(K)).astype(np.float16)

    def cancel(i):
        r[i] = -x[i]

    def overflow(i):
        x[i] = r[i] = np.float16(40000.0)

    def zero(i):
        x[i] = r[i] = 0

    def nan_last(i):
        x[i, K - 1] = np.nan

    def infs(i):
        x[i, K // 2] = np.inf
        r[i, 0] = -np.inf

    def big(i):
        x[i, max(K - 5, 0)] = np.float16(65504.0)
        r[i, max(K - 5, 0)] = 0

    def all_nan(i):
        r[i] = np.nan

    def subnormal(i):
        x[i] = (rng.uniform(-1, 1, K) * 2.0 ** -15).astype(np.float16)
        r[i] = (rng.uniform(-1, 1, K) * 2.0 ** -15).astype(np.float16)

    for i, f in enumerate([rounding, cancel, overflow, nan_last, infs, big, zero, all_nan, subnormal][:M]):
        f(i)
    gamma = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float16)
    return x, r, gamma


def host_add(x, r):
    """fp16 + fp16 on the host: numpy adds in fp32 and rounds once to nearest-even -- the correctly rounded fp16 sum."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (x + r).astype(np.float16)


def columns(K, seed):
    """128 outlier columns where K >= 128, else K / 2."""
    return P.outlier_columns(K, 128 if K >= 128 else K // 2, seed)


# -------------------------------------------------------------------------------------------------------------- running ----
def run_add(lib, x, r, gamma, ind, quant, frag=0, h_in=None):
    """The add entry of ``quant`` on exact-size guarded buffers.  h_in: None = a buffer of its own, "x" / "r" = in place.
    -> dict(rc, h, out, outl, q, scale, x, r): the bodies after the call; every guard is checked."""
    M, K = x.shape
    O = 0 if ind is None else ind.size
    xg, rg = Guarded(x.nbytes, HFILL, x), Guarded(r.nbytes, HFILL, r)
    hg = {None: Guarded(2 * M * K, HFILL), "x": xg, "r": rg}[h_in]
    g = torch.from_numpy(gamma).to(dev())
    out, outl, sc = Guarded(2 * M * K, HFILL), Guarded(2 * M * O, HFILL), Guarded(2 * M, HFILL)
    q = Guarded(M * K // 2 if quant == 4 else (P.frag_image_bytes(M, K) if frag else M * K), QFILL)
    ip = torch.from_numpy(ind).to(dev()) if O else None
    args = (M, K, xg.ptr, rg.ptr, hg.ptr, g.data_ptr(), out.ptr, ctypes.c_float(EPS))
    tail = (ip.data_ptr() if O else None, O, outl.ptr if O else None, q.ptr, sc.ptr)
    if quant == 0:
        rc = lib.mixq_add_rmsnorm(*args, stream())
    elif quant == 4:
        rc = lib.mixq_add_rmsnorm_extract_quant4(*args, *tail, stream())
    else:
        rc = lib.mixq_add_rmsnorm_extract_quant_layout(*args, *tail, frag, stream())
    form = P.last_form(lib)
    torch.cuda.synchronize()
    w = f"add_rmsnorm {M}x{K} quant={quant} O={O} frag={frag} h={h_in or 'own'}"
    return dict(rc=rc, form=form, x=take(lib, xg, np.float16, (M, K), w + " x"), r=take(lib, rg, np.float16, (M, K), w + " residual"),
                h=take(lib, hg, np.float16, (M, K), w + " h"), out=take(lib, out, np.float16, (M, K), w + " out"),
                outl=take(lib, outl, np.float16, (M, O), w + " outliers"),
                q=take(lib, q, np.uint8 if quant == 4 else np.int8, None, w + " q"), scale=take(lib, sc, np.float16, None, w + " scale"))


def same16(a, b):
    """fp16 arrays equal by bit pattern, any NaN equal to any NaN.  -> indices that differ."""
    ua, ub = bits(a).reshape(-1), bits(b).reshape(-1)
    nan_a, nan_b = (ua & 0x7FFF) > 0x7C00, (ub & 0x7FFF) > 0x7C00
    return np.flatnonzero(~((ua == ub) | (nan_a & nan_b)))


def assert_same(got, h_ref, ref, what):
    """got: run_add's dict; ref: run_norm's (rc, out, outl, q, scale) on h_ref."""
    rc, out, outl, q, scale = ref
    assert got["rc"] == 0 and rc == 0, (what, got["rc"], rc)
    for name, a, b in (("h", got["h"], h_ref), ("out", got["out"], out), ("outliers", got["outl"], outl), ("scale", got["scale"], scale)):
        bad = same16(a, b)
        assert bad.size == 0, f"{what}: {bad.size} elements of {name} differ from the unfused sequence, first flat indices {bad[:6].tolist()}"
    bad = np.flatnonzero(got["q"].reshape(-1) != q.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} bytes of q differ from the unfused sequence, first offsets {bad[:6].tolist()}"


def check_against_unfused(lib, x, r, gamma, ind, quant, block_rows, what, frag=0, h_in=None):
    M, K = x.shape
    h_ref = host_add(x, r)
    got = run_add(lib, x, r, gamma, ind, quant, frag, h_in)
    assert got["form"] == add_form(M, K, quant, block_rows, frag), f"{what}: the launch took {got['form']!r}"
    ref = P.run_norm(lib, h_ref, gamma, ind, quant, frag)
    assert P.last_form(lib) == P.norm_form(M, K, quant, block_rows, frag), what   # (the sequence it is compared with took the plain form)
    assert_same(got, h_ref, ref, what)
    if h_in != "x":
        assert np.array_equal(bits(got["x"]), bits(x)), what + ": x was modified"
    if h_in != "r":
        assert np.array_equal(bits(got["r"]), bits(r)), what + ": residual was modified"
    return got


# ------------------------------------------------------------------------------------------- 1. every form x quant 0 / 8 / 4
@pytest.mark.gpu
@pytest.mark.parametrize("M,knob_v", QE_ROWS, ids=lambda v: str(v))
@pytest.mark.parametrize("K", NORM_K)
def test_add_norm_every_form_equals_the_unfused_sequence(lib, knob, K, M, knob_v):
    knob(knob_v)
    block_rows = 64 if knob_v == KNOB_BLOCK_ROWS_64 else None
    x, r, gamma = add_inputs(M, K, seed=K * 11 + M)
    ind = columns(K, seed=K)
    for quant in (0, 8, 4):
        check_against_unfused(lib, x, r, gamma, None if quant == 0 else ind, quant, block_rows, f"{M}x{K} knob={knob_v} quant {quant}")


# ------------------------------------------------------------------------------------------------ 2. fragment-major images
@pytest.mark.gpu
@pytest.mark.parametrize("K", [2048, 2856, 8192, 16384])
@pytest.mark.parametrize("M", [1, 16, 37, 64])
def test_add_norm_fragment_image_equals_the_unfused_image(lib, knob, M, K):
    """Both images start from the same byte (QFILL): the padding of a partial 16-row tile / 64-byte k-step keeps whatever the
    buffer held, so the WHOLE image is compared byte for byte."""
    knob(None)
    x, r, gamma = add_inputs(M, K, seed=M * 3 + K)
    got = check_against_unfused(lib, x, r, gamma, columns(K, seed=K + 1), 8, None, f"{M}x{K} fragment-major", frag=1)
    assert got["q"].size == P.frag_image_bytes(M, K)


# ---------------------------------------------------------------------------------------------- 3. in place / out of place
@pytest.mark.gpu
@pytest.mark.parametrize("M,K", [(37, 4096), (6, 11008)])
def test_add_norm_in_place_and_out_of_place(lib, knob, M, K):
    """h_out == residual (the residual-stream update), h_out == x, and a buffer of its own: the same bits, all equal to the
    unfused sequence; with its own buffer x and residual keep their bytes (checked in check_against_unfused)."""
    knob(None)
    x, r, gamma = add_inputs(M, K, seed=M + K)
    ind = columns(K, seed=K + 2)
    runs = {h_in: check_against_unfused(lib, x, r, gamma, ind, 8, None, f"{M}x{K} h_out={h_in or 'own'}", h_in=h_in)
            for h_in in ("r", "x", None)}
    h_ref = host_add(x, r)
    assert same16(runs["r"]["r"], h_ref).size == 0 and np.array_equal(bits(runs["r"]["x"]), bits(x))
    assert same16(runs["x"]["x"], h_ref).size == 0 and np.array_equal(bits(runs["x"]["r"]), bits(r))
    for name in ("h", "out", "outl", "scale", "q"):
        for h_in in ("r", "x"):
            assert np.array_equal(runs[h_in][name].view(np.uint8), runs[None][name].view(np.uint8)), (name, h_in)


# ------------------------------------------------------------------------------------------------------ 4. buffer contract
@pytest.mark.gpu
@pytest.mark.parametrize("M,K,knob_v", [(5, 1024, None), (3, 2856, None), (67, 4096, KNOB_BLOCK_ROWS_64)])
def test_add_norm_buffer_contract(lib, knob, M, K, knob_v):
    """h, out, outliers, q, scale -- and x, residual -- at exactly their declared sizes between guards (run_add checks every
    guard): 5 x 1024 has a partial block of the four-rows-per-block form, 3 x 2856 a ragged last round of vectors, 67 x 4096 with
    the knob a partial block of the wavefront-per-row form.  Rows past M and vectors past K / 8 load and store nothing."""
    knob(knob_v)
    block_rows = 64 if knob_v == KNOB_BLOCK_ROWS_64 else None
    x, r, gamma = add_inputs(M, K, seed=M * K)
    ind = columns(K, seed=K + 3)
    for quant in (0, 8, 4):
        for h_in in (None, "r"):
            check_against_unfused(lib, x, r, gamma, None if quant == 0 else ind, quant, block_rows,
                                  f"{M}x{K} quant {quant} h_out={h_in or 'own'}", h_in=h_in)
    if M <= 64 and 1024 < K <= 16384:      # the fragment-major image exists for this shape (include/mixq.h)
        check_against_unfused(lib, x, r, gamma, ind, 8, None, f"{M}x{K} fragment-major", frag=1)


# ------------------------------------------------------------------------------------------------- 5. through the Python layer
def build_block(K, F, bit, seed):
    """norm -> MixLlamaMLP(gate, down, up) with a static set of 128 outlier columns, as a P-flavour decoder block wires them."""
    from mixq_tensorrt_llm_amd import mixlinear
    d = dev()
    g = torch.Generator(device="cpu").manual_seed(seed)
    W_up, W_gate = ((torch.randn((F, K), generator=g) * 0.02).to(torch.float16).to(d) for _ in range(2))
    W_down = (torch.randn((K, F), generator=g) * 0.02).to(torch.float16).to(d)
    scales = torch.rand(K, generator=g).to(d)
    gamma = (torch.rand(K, generator=g) + 0.5).to(torch.float16).to(d)
    cache = mixlinear.MixLibCache(inputdim=256, bit=bit, device=d)
    mk = lambda W: mixlinear.MixLinear_GEMM.from_linear(W, None, bit=bit, cache=cache, dev=d, layer_scales=scales,   # noqa: E731
                                                        fp_features_num=128)
    up, gate = mk(W_up), mk(W_gate)
    down = mixlinear.MixLinear_GEMM.from_linear(W_down, None, bit=8, cache=cache, dev=d, layer_scales=torch.rand(F, generator=g).to(d),
                                                fp_features_num=128)
    up.add_outliers = gate.add_outliers = down.add_outliers = False
    norm = mixlinear.FasterTransformerRMSNorm(gamma, 1e-6, cache)
    norm.next_layer = up
    return cache, norm, mixlinear.MixLlamaMLP(gate, down, up, cache)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,F,bit", [(160, 1024, 512, 8), (8, 1024, 512, 8), (8, 2048, 1024, 8), (160, 1024, 512, 4)])
def test_forward_residual_equals_add_then_forward(lib, knob, M, K, F, bit):
    """FasterTransformerRMSNorm.forward_residual(x, residual) -> MLP == `residual += x; forward(residual)` -> MLP, bit for bit
    on the MLP output; the returned h is the torch sum, in residual's storage.  8 x 2048 -> 1024 is a decode batch in the
    fragment-major image's domain (8 x 1024 is not: K must exceed 1024)."""
    from mixq_tensorrt_llm_amd import mixlib
    knob(None)
    cache, norm, mlp = build_block(K, F, bit, seed=M + K + bit)
    g = torch.Generator(device="cpu").manual_seed(M * K)
    x = torch.randn((M, K), generator=g).to(torch.float16).to(dev())
    res = (4.0 * torch.randn((M, K), generator=g)).to(torch.float16).to(dev())
    # the unfused block
    r1 = res.clone()
    r1 += x
    out1 = norm(r1)
    lay1 = getattr(cache, "q_layout", 0)    # the producer's choice: read before the MLP, whose down projection overwrites it
    y1 = mlp(out1).clone()
    # the fused one
    r2 = res.clone()
    out2, h2 = norm.forward_residual(x.clone(), r2)
    assert ADD_MARK in P.last_form(lib), P.last_form(lib)
    assert h2.data_ptr() == r2.data_ptr(), "h is written into residual's storage"
    assert getattr(cache, "q_layout", 0) == lay1
    y2 = mlp(out2)
    torch.cuda.synchronize()
    if bit == 8:
        assert lay1 == mixlib.qa_layout(M, F, K)
        if (M, K) == (8, 2048):
            assert lay1 == mixlib.QA_FRAGMENT_MAJOR, "this shape is in the fragment-major image's domain"
    assert torch.equal(h2, r1), "h differs from the torch sum"
    assert torch.equal(y2.view(torch.int16), y1.view(torch.int16)), "MLP output differs from add + forward"
    assert torch.isfinite(y1.float()).all()


@pytest.mark.gpu
def test_python_wrapper_defaults_to_the_residual_in_place(lib):
    from mixq_tensorrt_llm_amd import mixlib
    d = dev()
    g = torch.Generator(device="cpu").manual_seed(3)
    x, r = (torch.randn((5, 1032), generator=g).to(torch.float16).to(d) for _ in range(2))
    gamma = torch.ones(1032, dtype=torch.float16, device=d)
    want_h = r + x
    want_out = torch.empty_like(x)
    mixlib.layernorm_forward_cuda(want_h, gamma, want_out, 1e-6)
    out = torch.empty_like(x)
    h = mixlib.add_layernorm_forward_cuda(x, r, gamma, out, 1e-6)      # h_out=None: in place into the residual
    assert h.data_ptr() == r.data_ptr() and torch.equal(r, want_h) and torch.equal(out.view(torch.int16), want_out.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------ 6. large image
@pytest.mark.gpu
def test_add_norm_non_temporal_image(lib, knob):
    """2048 x 4096: an 8 Mi-element int8 image, written with non-temporal stores (the " nt" form)."""
    knob(None)
    M, K = 2048, 4096
    x, r, gamma = add_inputs(M, K, seed=9)
    got = check_against_unfused(lib, x, r, gamma, columns(K, seed=K + 4), 8, None, f"{M}x{K}")
    assert got["form"].endswith(ADD_MARK + " nt"), got["form"]
