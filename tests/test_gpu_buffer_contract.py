"""GPU (-m gpu): WHERE the GEMM families read and write -- the buffer contract of include/mixq.h.

Every other GPU test hands the library roomy, 256-byte-aligned torch allocations, whose slack (the caching allocator rounds every
request up) swallows a store a few rows past [M, N], an exchange slot past the declared scratch or a workspace carve that runs over
mixq_workspace_size.  Here every buffer of a call is a tests/guarded.py buffer: exactly the declared size, at the MINIMUM alignment
the entry accepts (``ptr % 256 == 16`` wherever the entry asks for 16 bytes; the element's natural alignment where the kernel loads
element by element: scale_row, the fpA_intB scale; ``ptr % 128 == 8`` for the plugin workspace), between two guards of pattern bytes
that are compared byte for byte after the call.  Per family (forced onto a small ragged shape: M one more and one less than a multiple
of its tile height, N = 16 x odd, K = 16 x odd where the family takes a partial last slice; and once on a shape its rule picks):

 1. output guard: D pre-filled with a pattern, every element written, the bits of the same call on ordinary buffers;
 2. workspace / scratch of exactly the declared size (hand-over words zero again afterwards);
 3. every input in its own guarded buffer, the guards filled twice (fp16 NaN / 1.0, int8 0x7f / 0x80, fp_ind 0 / K - 1): identical
    output bits, inputs unchanged;
 4. aliasing: y == D for int8FusedDequantize / Silu / SiluMul, out == y for dequantizationSilu;
 5. accumulators past 2^24 (blocks of +-127 / -128 that give every row, column and K range of a tile its own sum; the addend is
    minus the fp16-rounded product, so that the LOW bits of every sum reach the fp16 output) and scale vectors with 0, -0, a
    subnormal, 65504 and NaN: EPI_INT32 equals the exact integer product, EPI_DEQUANT (+ addend, + bias) oracle.dequant_epilogue, bit
    for bit; the SiLU epilogues keep the bound of test_gpu_parity.test_fused_dequant_epilogue (<= 1 fp16 ulp in < 0.1 % of elements).

Each case asserts the family it took (mixq_debug_last_gemm_kernel, the scratch size of the expected split, mixq_describe_plan for the
automatic shapes); the last test asserts that the whole list was reached.  Knobs are reset around every case.

Guard sizes are conditions, not measurements (tests/guarded.py): an [M, N] output gets max(64 KiB, 256 rows x N x element size) on
both sides (the tallest tile is 256 rows), scratch and workspaces 1 MiB (four 256-KiB slots), inputs 64 KiB."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

import guarded as G
from guarded import Guarded, assert_intact

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OUT_PAT, SCR_PAT, WS_PAT = 0xA5, 0xC3, 0x3C   # guard bytes of outputs / scratch / workspaces; outputs are pre-filled with OUT_PAT too
WORDS = 16384                                  # hand-over words at the start of every exchange scratch (csrc/mixq_launch.h)
O = 128                                        # outlier columns of the operator
MIN16 = 16                                     # ptr % 256 of a pointer the entry checks for 16 bytes
REACHED = set()


# ------------------------------------------------------------------------------------------------------------ plumbing ----
@pytest.fixture(scope="module")
def lib():
    from mixq_tensorrt_llm_amd import _lib
    lib = _lib.load()
    assert lib.mixq_debug_knobs_enabled() == 1, "the form knobs need MIXQ_DEBUG_KNOBS=1 (tests/conftest.py)"
    lib.mixq_debug_reset()
    yield lib
    lib.mixq_debug_reset()
    _OUTS.clear(), _SCRATCH.clear(), _RIGS.clear()
    torch.cuda.empty_cache()


@pytest.fixture()
def knobs(lib):
    """Set the case's knobs; every knob back to its default afterwards, pass or fail."""
    lib.mixq_debug_reset()

    def set_(values):
        for v in values:
            lib.mixq_debug_set_gemm_variant(v)
    yield set_
    lib.mixq_debug_reset()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def vp(x):
    return None if x is None else ctypes.c_void_p(int(x))


def last_kernel(lib):
    return lib.mixq_debug_last_gemm_kernel().decode()


def roomy(nbytes, N, esize=2):
    """An ORDINARY output buffer for the reference run: nbytes pre-filled with 0x7e at the front of a larger allocation (a guard's worth
    of slack behind it, so that a stray store of the code under test cannot leave the memory this test owns there either)."""
    return torch.full((nbytes + G.out_guard(N, esize),), 0x7E, dtype=torch.uint8, device="cuda:0")[:nbytes]


FILLS = {"f16": (G.F16_NAN, G.F16_ONE), "bf16": (G.BF16_NAN, G.BF16_ONE), "i8": (G.I8_MAX, G.I8_MIN)}


class Rig:
    """The inputs of one call, each in its own guarded buffer of exact size; ``specs``: name -> (array, kind, ptr % 256), kind a key
    of FILLS or a pair of guard patterns."""

    def __init__(self, specs):
        self.np, self.g, self.orig, self.plain, self.fills = {}, {}, {}, {}, {}
        for name, (arr, kind, off) in specs.items():
            arr = np.ascontiguousarray(arr)
            self.fills[name] = FILLS[kind] if isinstance(kind, str) else kind
            self.np[name] = arr
            self.g[name] = Guarded(arr.nbytes, self.fills[name][0], init=arr, guard=G.IN_GUARD, offset=off)
            self.orig[name] = self.g[name].body_bytes().clone()
            self.plain[name] = self.orig[name].clone()             # the same bytes in an ordinary allocation

    def set_fill(self, which):
        for name, g in self.g.items():
            g.set_guards(self.fills[name][which])

    def ptr(self, name):
        return self.g[name].ptr

    def pptr(self, name):
        return self.plain[name].data_ptr()

    def restore(self, name):
        self.g[name].body_bytes().copy_(self.orig[name])
        self.plain[name].copy_(self.orig[name])

    def check(self, what, changed=()):
        """Guards intact, and every input (but those in ``changed``) still holds its bytes."""
        for name, g in self.g.items():
            assert_intact(g, f"{what}: input {name}")
            if name not in changed:
                assert torch.equal(g.body_bytes(), self.orig[name]), f"{what}: input {name} was modified"


_OUTS, _SCRATCH, _RIGS = {}, {}, {}


def fresh_out(nbytes, guard, offset=MIN16, init=None):
    """A guarded output of exactly nbytes, pre-filled with OUT_PAT (or ``init``, device bytes: the aliasing cases)."""
    key = (nbytes, guard, offset)
    g = _OUTS.get(key)
    if g is None:
        g = _OUTS[key] = Guarded(nbytes, OUT_PAT, guard=guard, offset=offset)
    if init is None:
        g.body_bytes().fill_(OUT_PAT)
    else:
        g.body_bytes().copy_(init)
    return g


def fresh_scratch(nbytes):
    """Exchange scratch of exactly nbytes, zero-filled, at 16-byte alignment; None where the form needs none."""
    if nbytes == 0:
        return None
    g = _SCRATCH.get(nbytes)
    if g is None:
        g = _SCRATCH[nbytes] = Guarded(nbytes, SCR_PAT, guard=G.SCRATCH_GUARD, offset=MIN16)
    g.body_bytes().zero_()
    return g


def check_out(g, ref_bits, what):
    damage = g.guard_damage()
    if damage is not None:
        _OUTS.pop((g.n, g.guard, g.offset), None)
        raise AssertionError(f"{what}: a store outside the output -- {damage}")
    if not torch.equal(g.body_bytes(), ref_bits):
        diff = torch.nonzero(g.body_bytes() != ref_bits).reshape(-1)
        unwritten = int((g.body_bytes()[diff] == OUT_PAT).sum())
        raise AssertionError(f"{what}: {diff.numel()} output bytes differ from the call on ordinary buffers, first at byte {int(diff[0])}, "
                             f"last at {int(diff[-1])} ({unwritten} of them equal the pre-fill byte)")


def check_scratch(g, what):
    if g is None:
        return
    damage = g.guard_damage()
    if damage is not None:
        _SCRATCH.pop(g.n, None)
        raise AssertionError(f"{what}: a store outside the scratch of {g.n} bytes -- {damage}")
    assert int(g.body_bytes()[:WORDS].to(torch.int32).sum()) == 0, f"{what}: hand-over words left non-zero"


# --------------------------------------------------------------------------------------------- the int8 GEMM families ----
Fam = namedtuple("Fam", "name knobs bm N K expect scratch int32 mult", defaults=(1,))
# scratch: None = the form takes no exchange scratch | (tile rows, tile columns, parts) of the split the knobs force: the declared size
# must be the hand-over words + one int32 tile per part and tile.  int32: mixq_gemm_s8s8s32 (EPI_INT32) reaches the family too.
# mult: the forced cases have mult x bm +- 1 rows.

TWO_BARRIER_BM = [32, 128, 256, 64, 128, 128, 256, 64, 64, 64, 64, 64, 128, 64, 128, 32, 64, 64, 32, 128, 64, 64, 32, 64]  # csrc/gemm_kernels.hip launch_epi
N_RAGGED, K_RAGGED = 272, 1040          # 16 x 17, 16 x 65: no tile width divides N, the last 128-byte K slice holds 16 bytes
FAMILIES = [
    Fam("skinny-pieces", (), 16, N_RAGGED, K_RAGGED, "gemm_skinny_kernel", None, True),       # row-major weight in 64-byte pieces
    Fam("skinny-runs", (), 16, N_RAGGED, 1280, "gemm_skinny_kernel", None, True),             # ... in 256-byte runs (K % 256 == 0)
]
FAMILIES += [Fam(f"two-barrier-cfg{i}", (10 + i,), bm, N_RAGGED, K_RAGGED, "two-barrier", None, True) for i, bm in enumerate(TWO_BARRIER_BM)]
# small tiles, K split over 2 / 4 / 8 / 16 workgroups (knob 62 / 64 / 68 / 66; 8 slices per part at least); 1 = no other schedule
FAMILIES += [Fam(f"xsplit-{xs}", (1, 66 if xs == 16 else 60 + xs), 32, N_RAGGED, 1024 * xs + 16, "two-barrier", (32, 64, xs), False)
             for xs in (2, 4, 8, 16)]
FAMILIES += [Fam("xsplit-2-64x64", (1, 62), 64, 2064, 2064, "two-barrier", (64, 64, 2), False, 2)]   # (two tile rows: 32-row tiles would be more than 128)
# the deep form: 4 waves (1241 + xs), 8 waves (+ 10), 8 waves and 5 stages (+ 20); 4 slices per part at least
FAMILIES += [Fam(f"deep-{xs}", (1241 + xs,), 128, N_RAGGED, 4112, "w8a8o16_kernel<DEEP>", (128, 128, xs), False) for xs in (1, 2, 4, 8)]
FAMILIES += [Fam(f"deep-8wave-{xs}", (1251 + xs,), 128, N_RAGGED, 4112, "w8a8o16_kernel<DEEP>", (128, 128, xs), False) for xs in (1, 2, 4, 8)]
FAMILIES += [Fam(f"deep-5stage-{xs}", (1261 + xs,), 128, N_RAGGED, 4112, "w8a8o16_kernel<DEEP>", (128, 128, xs), False) for xs in (1, 4)]
# the mid kernel (1271 + xs; whole 128-byte slices only: K = 33 slices): N = 304 = 16 x 19 makes four 96-wide but three 128-wide
# tile columns, so the rule takes 96-wide tiles and knob 1431 the 128-wide ones; 1412 / 1411: the rotated K walk on / off
FAMILIES += [Fam(f"mid-{bn}-{'split' if xs > 1 else 'unsplit'}-{'rot' if rot == 1412 else 'norot'}", (1271 + xs, rot, 1431 if bn == 128 else 1430),
                 128, 304, 4224, "mid_kernel<DEEP>", (128, bn, xs), False)
             for bn in (128, 96) for xs in (1, 2) for rot in (1412, 1411)]
FAMILIES += [Fam(f"mid-{bn}-split{xs}", (1271 + xs, 1431 if bn == 128 else 1430), 128, 304, 4224, "mid_kernel<DEEP>", (128, bn, xs), False)
             for bn in (128, 96) for xs in (4, 8)]
FAMILIES += [
    Fam("pp128", (5,), 128, N_RAGGED, K_RAGGED, "pp128_kernel", None, True),
    Fam("pp256", (2,), 256, N_RAGGED, K_RAGGED, "pp_kernel (256x256", None, True),
]
FAMILIES += [Fam(f"pp256-split-{s}", (1241, 70 + s), 256, N_RAGGED, 4112, "pp_kernel<SPLITK>", (256, 256, s), False) for s in (2, 4, 8)]
FAM = {f.name: f for f in FAMILIES}
FORCED = [(f.name, f.bm * f.mult + d) for f in FAMILIES for d in (1, -1)]


def declared_scratch(f, M, N):
    """Bytes mixq_gemm_scratch_size must declare for the split the family's knobs force."""
    if f.scratch is None or f.scratch[2] == 1:
        return 0
    bm, bn, parts = f.scratch
    tm = (M + bm - 1) // bm
    if f.expect.startswith(("w8a8o16_kernel<DEEP>", "mid_kernel")):   # room for 128- or 96-wide parked tiles, whichever is more
        per = max(tm * ((N + 127) // 128) * 128 * 128 * 4, tm * ((N + 95) // 96) * 128 * 96 * 4)
        return WORDS + per * parts
    return WORDS + tm * ((N + bn - 1) // bn) * parts * bm * bn * 4


def special_bias(N, seed):
    rng = np.random.default_rng(seed)
    b = (rng.standard_normal(N) * 0.5).astype(np.float16)
    sub = np.float16(2.0 ** -24)
    b[:8] = np.array([0.0, -0.0, 65504.0, -65504.0, sub, -sub, np.float16(3e-5), 1.0], np.float16)
    return b


def gemm_rig(M, N, K):
    """Random operands of every launcher-level int8 GEMM entry (cached per shape)."""
    key = ("gemm", M, N, K)
    if key not in _RIGS:
        rng = np.random.default_rng(M * 7 + N * 3 + K)
        specs = {
            "qA": (rng.integers(-127, 128, (M, K), dtype=np.int8), "i8", MIN16),
            "W": (rng.integers(-127, 128, (N, K), dtype=np.int8), "i8", MIN16),
            "sA": ((rng.random(M) * 0.05 + 0.01).astype(np.float16), "f16", 2),      # loaded element by element in every family: no check in the entry
            "sW": ((rng.random(N) * 4e-4 + 1e-4).astype(np.float16), "f16", MIN16),
            "fpA": (rng.standard_normal((M, O)).astype(np.float16), "f16", MIN16),
            "fpW": ((rng.standard_normal((N, O)) * 0.02).astype(np.float16), "f16", MIN16),
            "y": ((rng.standard_normal((M, N)) * 0.5).astype(np.float16), "f16", MIN16),
            "mul": (rng.standard_normal((M, N)).astype(np.float16), "f16", MIN16),
            "bias": (special_bias(N, M + K), "f16", MIN16),
        }
        _RIGS[key] = Rig(specs)
    return _RIGS[key]


ENTRIES = ("mixed", "mixed_bias", "dq", "dq_y", "dq_silu", "dq_silu_mul", "int32")
USES = {"mixed": ("qA", "W", "sA", "sW", "fpA", "fpW"), "mixed_bias": ("qA", "W", "sA", "sW", "fpA", "fpW", "bias"),
        "dq": ("qA", "W", "sA", "sW"), "dq_y": ("qA", "W", "sA", "sW", "y"), "dq_silu": ("qA", "W", "sA", "sW", "y"),
        "dq_silu_mul": ("qA", "W", "sA", "sW", "y", "mul"), "int32": ("qA", "W")}


def call_entry(lib, entry, P, out, M, N, K, scr, scr_bytes, n_out=O):
    """One launcher-level call; P: name -> pointer of every input, out / scr pointers."""
    a = lambda n: vp(P[n])  # noqa: E731
    st = stream()
    if entry == "mixed":
        return lib.mixq_gemm_mixed_scratch(a("qA"), a("W"), a("sA"), a("sW"), a("fpA"), a("fpW"), vp(out), M, N, K, n_out, vp(scr), scr_bytes, st)
    if entry == "mixed_bias":
        return lib.mixq_gemm_mixed_bias(a("qA"), a("W"), a("sA"), a("sW"), a("fpA"), a("fpW"), a("bias"), vp(out), M, N, K, n_out, vp(scr), scr_bytes, st)
    if entry == "dq":
        return lib.mixq_int8_fused_dequantize(a("qA"), a("W"), a("sA"), a("sW"), None, vp(out), M, N, K, vp(scr), st)
    if entry == "dq_y":
        return lib.mixq_int8_fused_dequantize(a("qA"), a("W"), a("sA"), a("sW"), a("y"), vp(out), M, N, K, vp(scr), st)
    if entry == "dq_silu":
        return lib.mixq_int8_fused_dequantize_silu(a("qA"), a("W"), a("sA"), a("sW"), a("y"), vp(out), M, N, K, vp(scr), st)
    if entry == "dq_silu_mul":
        return lib.mixq_int8_fused_dequantize_silu_mul(a("qA"), a("W"), a("sA"), a("sW"), a("y"), a("mul"), vp(out), M, N, K, vp(scr), st)
    assert entry == "int32"
    return lib.mixq_gemm_s8s8s32(a("qA"), a("W"), vp(out), M, N, K, st)


def plain_run(lib, f, entry, rig, M, N, K, n_scr):
    """The call on ordinary (roomy, 256-byte-aligned) buffers -> output bytes on the device."""
    esize = 4 if entry == "int32" else 2
    out = roomy(M * N * esize, N, esize)
    scr = torch.zeros(n_scr + (1 << 20), dtype=torch.uint8, device="cuda:0") if n_scr else None
    P = {n: rig.pptr(n) for n in USES[entry]}
    rc = call_entry(lib, entry, P, out.data_ptr(), M, N, K, scr.data_ptr() if n_scr else None, n_scr)
    assert rc == 0, f"{f.name} {entry} on ordinary buffers: mixq error {rc}"
    torch.cuda.synchronize()
    assert f.expect in last_kernel(lib), f"{f.name} {entry}: the launch took {last_kernel(lib)!r}"
    return out


def guarded_run(lib, f, entry, rig, M, N, K, n_scr, ref, what, alias=False):
    """The same call with every buffer guarded, at exact size and minimum alignment, once per guard fill."""
    esize = 4 if entry == "int32" else 2
    for which in (0, 1):
        rig.set_fill(which)
        out = fresh_out(M * N * esize, G.out_guard(N, esize), init=rig.orig["y"] if alias else None)
        scr = fresh_scratch(n_scr)
        P = {n: rig.ptr(n) for n in USES[entry]}
        if alias:
            P["y"] = out.ptr
        rc = call_entry(lib, entry, P, out.ptr, M, N, K, scr.ptr if scr else None, n_scr)
        assert rc == 0, f"{what} fill {which}: mixq error {rc}"
        torch.cuda.synchronize()
        assert f.expect in last_kernel(lib), f"{what}: the launch took {last_kernel(lib)!r}"
        check_out(out, ref, f"{what} (guard fill {which})")
        check_scratch(scr, f"{what} (guard fill {which})")
        rig.check(f"{what} (guard fill {which})")


@pytest.mark.parametrize("name,M", FORCED, ids=[f"{n}-M{m}" for n, m in FORCED])
def test_forced_family_in_guarded_buffers(lib, knobs, name, M):
    """Checks 1-4 on the launcher-level entries, the family forced onto a small ragged shape."""
    f = FAM[name]
    N, K = f.N, f.K
    rig = gemm_rig(M, N, K)
    knobs(f.knobs)
    n_scr = int(lib.mixq_gemm_scratch_size(M, N, K))
    assert n_scr == declared_scratch(f, M, N), f"{name}: mixq_gemm_scratch_size({M}, {N}, {K}) = {n_scr}, the forced split needs {declared_scratch(f, M, N)}"
    for entry in ENTRIES:
        if entry == "int32" and not f.int32:
            continue
        ref = plain_run(lib, f, entry, rig, M, N, K, n_scr)
        guarded_run(lib, f, entry, rig, M, N, K, n_scr, ref, f"{name} {entry} {M}x{N}x{K}")
        if entry in ("dq_y", "dq_silu", "dq_silu_mul"):       # y may alias D (include/mixq.h)
            guarded_run(lib, f, entry, rig, M, N, K, n_scr, ref, f"{name} {entry} y == D {M}x{N}x{K}", alias=True)
    REACHED.add(name)


# ---------------------------------------------------------------------------- accumulator extremes, special scales ----
def extreme_operands(M, N, K, seed):
    """int8 operands in 16 K ranges (of any length: the sums keep their low bits) of constant +-127 / -128 / 126 per row (column): every row, column and K range carries its own
    sum, most |sums| pass 2^24.  Rows 0 / 1 and columns 0 / 1 are all -128 / 127 (the int32 extremes of the shape)."""
    rng = np.random.default_rng(seed)
    R = 16
    cuts = np.unique(np.concatenate([[0, K], rng.choice(np.arange(1, K), R - 1, replace=False)]))
    lens = np.diff(cuts)
    base = rng.choice([-1, 1], R)

    def table(rows):
        sign = base[None, :] * np.where(rng.random((rows, R)) < 0.125, -1, 1)
        pos = rng.choice(np.array([127, 127, 126], np.int64), (rows, R))
        neg = rng.choice(np.array([-128, -128, -127], np.int64), (rows, R))
        t = np.where(sign > 0, pos, neg)
        t[0], t[1] = -128, 127
        return np.repeat(t, lens, axis=1).astype(np.int8)
    A, B = table(M), table(N)
    assert K * 128 * 128 < 2 ** 31
    acc = (A.astype(np.float64) @ B.astype(np.float64).T).astype(np.int64)      # exact: every partial sum is below 2^53
    assert np.abs(acc).max() < 2 ** 31
    assert acc[0, 0] == 128 * 128 * K and acc[0, 1] == -128 * 127 * K and acc[1, 1] == 127 * 127 * K
    return A, B, acc


SUB = np.float16(3 * 2.0 ** -24)


def special_scales(M, N, silu):
    """sA = 2^-4, sW = 2^-10 (their product is exact), with 0, -0, a subnormal -- and, unless silu, 65504 and NaN -- on rows / columns 2.."""
    sA = np.full(M, 2.0 ** -4, np.float16)
    sW = np.full(N, 2.0 ** -10, np.float16)
    sp = [0.0, -0.0, SUB] + ([] if silu else [65504.0, np.nan])
    sA[2:2 + len(sp)] = np.array(sp, np.float16)
    sW[2:2 + len(sp)] = np.array(sp, np.float16)
    sW[8] = np.float16(2.0 ** -14)
    return sA, sW


def check_oracle_masks(want, acc, sA, sW, y, what):
    """CPU, before anything runs on the GPU: the oracle is NaN exactly on the NaN rows / columns, infinite exactly where the exact
    value overflows fp16 (and no value sits near that threshold), finite everywhere else."""
    nan = np.isnan(sA.astype(np.float64))[:, None] | np.isnan(sW.astype(np.float64))[None, :]
    assert np.array_equal(np.isnan(want), nan), f"{what}: oracle NaN mask"
    with np.errstate(invalid="ignore", over="ignore"):
        v = acc.astype(np.float64) * (sA.astype(np.float64)[:, None] * sW.astype(np.float64)[None, :]) + (0 if y is None else y.astype(np.float64))
    mag = np.where(nan, 0, np.abs(v))
    assert not ((mag > 65000) & (mag < 66000)).any(), f"{what}: a value next to the fp16 overflow threshold"
    assert np.array_equal(np.isinf(want), mag >= 66000), f"{what}: oracle inf mask"
    return nan


EXTREME_K = {"skinny-pieces": 28672 + 16, "two-barrier-cfg7": 28672, "two-barrier-cfg23": 28672 + 16, "xsplit-16": 28672 + 16, "deep-8": 28672 + 16,
             "deep-8wave-8": 28672 + 16, "mid-128-split8": 28672, "mid-96-split8": 28672, "pp128": 28672 + 16, "pp256": 28672 + 16,
             "pp256-split-8": 28672 + 16}


def extreme_k(f):
    """K of the family's extremes case: 28672 (+ 16 where a partial last slice is accepted) for one form of every kind, else the
    forced shape's K, raised to 4112 where that is too short for sums past 2^24."""
    return EXTREME_K.get(f.name, f.K if f.K >= 2064 else 4112 if f.name != "skinny-runs" else 4096)


def bits16(a):
    return np.ascontiguousarray(a).view(np.uint16)


def same_bits_or_both_nan(got, want, nan, what):
    g, w = bits16(got), bits16(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN where the oracle has none, or none where it has one"
    bad = (g != w) & ~nan
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outputs differ from the oracle, first at {i}: got {got[i]!r} (0x{g[i]:04x}) "
                             f"want {want[i]!r} (0x{w[i]:04x}); rows {sorted(set(np.argwhere(bad)[:, 0].tolist()))[:8]} "
                             f"columns {sorted(set(np.argwhere(bad)[:, 1].tolist()))[:8]}")


@pytest.mark.parametrize("name", [f.name for f in FAMILIES])
def test_accumulator_extremes_and_special_scales(oracle, lib, knobs, name):
    """Check 5, one case per family and split factor (M = its tile height + 1)."""
    f = FAM[name]
    M, N, K = f.bm * f.mult + 1, f.N, extreme_k(f)
    A, B, acc = extreme_operands(M, N, K, seed=M + N + K)
    big = np.abs(acc) > 2 ** 24
    inexact = acc != acc.astype(np.float32).astype(np.int64)
    assert big.mean() > 0.5 and inexact.mean() > 0.2, (big.mean(), inexact.mean())
    acc32 = acc.astype(np.int32)
    sA, sW = special_scales(M, N, silu=False)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (-(acc.astype(np.float64) * 2.0 ** -14)).astype(np.float16)     # minus the rounded product: fma(acc, 2^-14, y) is the rounding residual
    assert np.isfinite(y).all()
    bias = special_bias(N, K)
    bias[2:4] = np.float16([1000.0, -1000.0])
    want_y = oracle.dequant_epilogue(acc32, sA, sW, y)
    want_0 = oracle.dequant_epilogue(acc32, sA, sW, None)
    nan = check_oracle_masks(want_y, acc, sA, sW, y, name + " + y")
    assert np.array_equal(check_oracle_masks(want_0, acc, sA, sW, None, name), nan)
    plain = ~nan & np.isfinite(want_y)
    assert np.unique(bits16(want_y)[plain]).size > 200, "the residuals must carry the low bits of the sums"
    with np.errstate(invalid="ignore", over="ignore"):
        want_b = (want_0 + bias[None, :]).astype(np.float16)                 # one fp16 add of the rounded value (plugin.py:158-160)
    sA_s, sW_s = special_scales(M, N, silu=True)
    want_s = oracle.dequant_epilogue(acc32, sA_s, sW_s, y, silu=True)
    assert np.isfinite(want_s).all()

    rig = Rig({"qA": (A, "i8", MIN16), "W": (B, "i8", MIN16), "sA": (sA, "f16", 2), "sW": (sW, "f16", MIN16), "y": (y, "f16", MIN16),
               "bias": (bias, "f16", MIN16), "fpA": (np.zeros(8, np.float16), "f16", MIN16), "fpW": (np.zeros(8, np.float16), "f16", MIN16)})
    rig_s = Rig({"sA": (sA_s, "f16", 2), "sW": (sW_s, "f16", MIN16)})
    knobs(f.knobs)
    n_scr = declared_scratch(f, M, N)      # (a family without a K split over workgroups is offered no scratch: with it, long K would take one)
    assert n_scr == 0 or n_scr == int(lib.mixq_gemm_scratch_size(M, N, K)), (name, n_scr, int(lib.mixq_gemm_scratch_size(M, N, K)))

    def run(entry, scales=rig, n_out=0):
        esize = 4 if entry == "int32" else 2
        out = fresh_out(M * N * esize, G.out_guard(N, esize))
        scr = fresh_scratch(n_scr)
        P = {n: rig.ptr(n) for n in USES[entry]}
        P["sA"], P["sW"] = scales.ptr("sA"), scales.ptr("sW")
        rc = call_entry(lib, entry, P, out.ptr, M, N, K, scr.ptr if scr else None, n_scr, n_out=n_out)
        assert rc == 0, f"{name} {entry}: mixq error {rc}"
        torch.cuda.synchronize()
        assert f.expect in last_kernel(lib), f"{name} {entry}: the launch took {last_kernel(lib)!r}"
        assert_intact(out, f"{name} {entry} extremes: output")
        check_scratch(scr, f"{name} {entry} extremes")
        return out.body(np.int32 if entry == "int32" else np.float16, (M, N))

    what = f"{name} {M}x{N}x{K}"
    if f.int32:
        got = run("int32")
        bad = got != acc32
        assert not bad.any(), f"{what} EPI_INT32: {int(bad.sum())} sums differ from the exact product, first at {tuple(np.argwhere(bad)[0])}"
    same_bits_or_both_nan(run("dq_y"), want_y, nan, what + " EPI_DEQUANT + addend")
    same_bits_or_both_nan(run("dq"), want_0, nan, what + " EPI_DEQUANT")
    same_bits_or_both_nan(run("mixed", n_out=0), want_0, nan, what + " mixq_gemm_mixed_scratch without outliers")
    same_bits_or_both_nan(run("mixed_bias", n_out=0), want_b, np.isnan(want_b), what + " EPI_DEQUANT_BIAS")
    got_s = run("dq_silu", scales=rig_s)
    assert np.isfinite(got_s).all(), what + " SiLU: not finite"
    gb, wb = bits16(got_s).astype(np.int32), bits16(want_s).astype(np.int32)
    assert np.abs(gb - wb).max() <= 1, f"{what} SiLU: more than one fp16 ulp from the oracle ({np.abs(gb - wb).max()})"
    assert (gb != wb).mean() < 1e-3, f"{what} SiLU: {(gb != wb).mean():.2e} of the outputs differ from the oracle"
    rig.check(what + " extremes")
    rig_s.check(what + " extremes (SiLU scales)")
    REACHED.add("extremes:" + name)


# ------------------------------------------------------------------------------------ mixq_enqueue: the whole operator ----
_LAYERS = {}


def layer_np(N, K, rows):
    """A packed MixQ layer [N, K] with `rows` activations as numpy arrays (cached)."""
    from conftest import make_layer
    from mixq_tensorrt_llm_amd import pack
    key = (N, K)
    if key not in _LAYERS or _LAYERS[key][0].shape[0] < rows:
        A, W, act = make_layer(rows, N, K, seed=N + K)
        _LAYERS[key] = (A, pack.pack_linear_weights(torch.from_numpy(W), torch.from_numpy(act)))
    return _LAYERS[key]


def enqueue_rig(N, K, M, bf16=False):
    """The seven inputs of mixq_enqueue (+ a bias) for M rows, each guarded at the alignment the entry accepts: 16 bytes for A, weight,
    weights_scaling_factor, fp_weight, qweight and the bias; fp_ind (int32, gathered element by element) and scaling_factors (read by
    the M <= 4 forms only, element by element) at their natural alignment.  The fp_ind guards hold valid column indices."""
    key = ("enq", N, K, M, bf16)
    if key in _RIGS:
        return _RIGS[key]
    if K % 64 == 0:
        A_all, p = layer_np(N, K, max(M, 64))
        A = A_all[:M]
    else:   # (the interleaved qweight of the M <= 4 forms needs K % 64 == 0; calls of more rows only want a pointer there)
        assert M > 4
        rng = np.random.default_rng(N + K + M)
        ind = rng.choice(K, O, replace=False).astype(np.int32)
        A = rng.standard_normal((M, K)).astype(np.float32)
        A[:, ind] *= 20.0
        A = A.astype(np.float16)
        p = {"weight": rng.integers(-127, 128, (N, K), dtype=np.int8), "weights_scaling_factor": (rng.random(N) * 4e-4 + 1e-4).astype(np.float16),
             "fp_weight": (rng.standard_normal((N, O)) * 0.02).astype(np.float16), "fp_ind": ind, "qweight": np.zeros((K, N), np.uint8)}
    act = "bf16" if bf16 else "f16"

    def tobf(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).view(torch.int16).numpy()
    ind = np.ascontiguousarray(p["fp_ind"]).astype(np.int32)
    specs = {
        "A": (tobf(A) if bf16 else A, act, MIN16),
        "weight": (p["weight"], "i8", MIN16),
        "wsf": (p["weights_scaling_factor"], "f16", MIN16),
        "fp_weight": (tobf(p["fp_weight"]) if bf16 else p["fp_weight"], act, MIN16),
        "fp_ind": (ind, (G.i32_pattern(0), G.i32_pattern(K - 1)), 4),
        "qweight": (p["qweight"], (b"\x7f", b"\x80"), MIN16),
        "sf": (p["weights_scaling_factor"], "f16", 2),
        "bias": (tobf(special_bias(N, M)) if bf16 else special_bias(N, M), act, MIN16),
    }
    rig = Rig(specs)
    if len(_RIGS) > 40:
        for k in [k for k in _RIGS if k[0] == "enq"][:8]:
            del _RIGS[k]
    _RIGS[key] = rig
    return rig


ENQ_NAMES = ("A", "weight", "wsf", "fp_weight", "fp_ind", "qweight", "sf")


def enqueue_call(lib, h, ptr_of, out_ptr, ws_ptr, M, N, K, bf16, bias_ptr):
    from mixq_tensorrt_llm_amd._lib import MIXQ_TYPE_BF16, MIXQ_TYPE_HALF, TensorDesc
    t_act = MIXQ_TYPE_BF16 if bf16 else MIXQ_TYPE_HALF
    shapes = [(M, K), (N, K // 2), (N,), (N, O), (2 * O,), (K, N // 2), (N,)]
    in_desc = (TensorDesc * 7)(*[TensorDesc.make(s, t_act if i in (0, 3) else MIXQ_TYPE_HALF) for i, s in enumerate(shapes)])
    out_desc = TensorDesc.make((M, N), t_act)
    ins = (ctypes.c_void_p * 7)(*[ptr_of(n) for n in ENQ_NAMES])
    outs = (ctypes.c_void_p * 1)(out_ptr)
    if bias_ptr is not None:
        return lib.mixq_enqueue_bias(h, in_desc, ctypes.byref(out_desc), ins, outs, vp(bias_ptr), vp(ws_ptr), stream())
    return lib.mixq_enqueue(h, in_desc, ctypes.byref(out_desc), ins, outs, vp(ws_ptr), stream())


def enqueue_contract(lib, N, K, M, what, expect=None, bf16=False, out_offset=MIN16, max_m=None):
    """Checks 1-3 through mixq_enqueue / mixq_enqueue_bias: guarded inputs, guarded output, a guarded workspace of exactly
    mixq_workspace_size bytes at an odd base, pre-filled with 0xff -- against ordinary buffers and a roomy zeroed workspace."""
    rig = enqueue_rig(N, K, M, bf16)
    h = ctypes.c_void_p(lib.mixq_create(M, N, K))
    try:
        kernels = []
        for with_bias in (False, True):
            bias_plain = rig.pptr("bias") if with_bias else None
            n_ws = int(lib.mixq_workspace_size(h, M, N, K))
            ref = roomy(M * N * 2, N)
            ws = torch.zeros(n_ws + (4 << 20), dtype=torch.uint8, device="cuda:0")
            rc = enqueue_call(lib, h, rig.pptr, ref.data_ptr(), ws.data_ptr(), M, N, K, bf16, bias_plain)
            assert rc == 0, f"{what}: mixq error {rc} on ordinary buffers"
            torch.cuda.synchronize()
            kern = last_kernel(lib) if M > 4 else "w8a16"
            kernels.append(kern)
            if expect is not None and M > 4:
                assert expect in kern, f"{what}: the launch took {kern!r}"
            sizes = [n_ws] + ([int(lib.mixq_workspace_size(h, max_m, N, K))] if max_m and not with_bias else [])
            for which, nbytes in enumerate(sizes + sizes[:1]):      # (second fill: the exact size again)
                rig.set_fill(which % 2)
                out = fresh_out(M * N * 2, G.out_guard(N, 2), offset=out_offset)
                wsg = Guarded(nbytes, WS_PAT, guard=G.SCRATCH_GUARD, offset=8)       # ptr % 128 == 8: the base may be anything
                wsg.body_bytes().fill_(0xFF)
                rc = enqueue_call(lib, h, rig.ptr, out.ptr, wsg.ptr, M, N, K, bf16, rig.ptr("bias") if with_bias else None)
                assert rc == 0, f"{what}: mixq error {rc}"
                torch.cuda.synchronize()
                tag = f"{what}{' + bias' if with_bias else ''} (workspace {nbytes} bytes, guard fill {which % 2})"
                if M > 4:
                    assert last_kernel(lib) == kern, f"{tag}: {last_kernel(lib)!r} in guarded buffers, {kern!r} in ordinary ones"
                check_out(out, ref, tag)
                assert_intact(wsg, tag + ": workspace")
                rig.check(tag)
                del wsg
        assert kernels[0] == kernels[1], f"{what}: {kernels[0]!r} without the bias, {kernels[1]!r} with it"
        return kernels[0]
    finally:
        lib.mixq_destroy(h)


ENQ_FORCED = [(f.name, f.bm * f.mult + 1) for f in FAMILIES if not f.name.startswith("skinny")]


@pytest.mark.parametrize("name,M", ENQ_FORCED, ids=[f"{n}-M{m}" for n, m in ENQ_FORCED])
@pytest.mark.parametrize("act", ["fp16", "bf16"])
def test_enqueue_forced_family_in_guarded_buffers(lib, knobs, name, M, act):
    f = FAM[name]
    knobs(f.knobs + ((890,) if M <= 64 else ()))      # (up to 64 rows: row-major qA, so that the forced tiles are what runs)
    enqueue_contract(lib, f.N, f.K, M, f"enqueue {act} {name} {M}x{f.N}x{f.K}", expect=f.expect, bf16=act == "bf16", max_m=4 * M)
    REACHED.add(f"enqueue-{act}:{name}")


def plan_of(lib, M, N, K, image=False):
    buf = ctypes.create_string_buffer(256)
    assert lib.mixq_describe_plan(M, N, K, 1 if image else 0, buf, 256) == 0
    return buf.value.decode()


# (N, K, M, weight image, knobs, family): shapes the selection rule takes to each family by itself (docs/SELECTION_TABLE.md rows; 1421: the
# round-5 deep build where the rule now takes the mid kernel)
AUTO = [(4608, 3584, 17, False, (), "skinny-route"), (4608, 3584, 40, True, (), "skinny-image"), (4608, 3584, 64, False, (), "two-barrier"),
        (4608, 3584, 160, False, (), "two-barrier"), (4096, 11008, 80, False, (), "xsplit"), (4096, 11008, 160, False, (1421,), "deep"),
        (4608, 3584, 512, False, (), "mid-96"), (4608, 3584, 768, False, (), "mid-128"), (4096, 11008, 256, False, (), "mid-128"),
        (4608, 3584, 1024, False, (), "pp128"), (4608, 3584, 2048, False, (), "pp256"), (11008, 4096, 2048, False, (), "pp256-split")]


@pytest.mark.parametrize("N,K,M,image,knob,fam", AUTO, ids=[f"{c[5]}-{c[2]}x{c[0]}x{c[1]}" for c in AUTO])
def test_enqueue_automatic_family_in_guarded_buffers(lib, knobs, N, K, M, image, knob, fam):
    from test_gpu_bias_epilogue import family
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the selection tables are fitted on 256 CUs")
    knobs(knob)
    img = None
    if image:
        # the registered image lives in a guarded buffer of exactly mixq_weight_image_bytes, registered under the guarded weight's pointer
        rig = enqueue_rig(N, K, M)
        nb = int(lib.mixq_weight_image_bytes(N, K))
        assert nb == N * K
        img = Guarded(nb, 0x6B, guard=G.IN_GUARD, offset=MIN16)
        plain_img = torch.empty(nb, dtype=torch.uint8, device="cuda:0")       # (the ordinary-buffer run streams an image as well)
        for weight, image_ptr in ((rig.ptr("weight"), img.ptr), (rig.pptr("weight"), plain_img.data_ptr())):
            assert lib.mixq_weight_image_register(vp(weight), N, K, vp(image_ptr), stream()) == 0
            assert lib.mixq_weight_image_verify(vp(weight), stream()) == 0
        assert_intact(img, "weight image registration")
        assert torch.equal(img.body_bytes(), plain_img), "the image built in the guarded buffer differs from the ordinary one"
        image_bytes = img.body_bytes().clone()
    try:
        kern = enqueue_contract(lib, N, K, M, f"enqueue {fam} {M}x{N}x{K}", max_m=2 * M + 96)
        got = family(kern, plan_of(lib, M, N, K, image), M)
        assert got == fam, f"{M}x{N}x{K}: took {got!r} ({kern!r}; plan {plan_of(lib, M, N, K, image)!r})"
        if image:
            assert_intact(img, "weight image after the calls")
            assert torch.equal(img.body_bytes(), image_bytes), "the registered weight image was modified"
    finally:
        if image:
            lib.mixq_weight_image_unregister(vp(rig.ptr("weight")))
            lib.mixq_weight_image_unregister(vp(rig.pptr("weight")))
    REACHED.add("auto:" + fam)


@pytest.mark.parametrize("form,knob,off", [("gemv", 857, 2), ("skinny", 856, 8)])
@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_enqueue_decode_rows_in_guarded_buffers(lib, knobs, form, knob, off, M):
    """M <= 4 on qweight: the GEMV stores element by element (output at its natural alignment, ptr % 16 == 2); the fpA_intB skinny
    form stores four fp16 at once (N % 4 == 0: 8 bytes, what the entry asks for)."""
    N, K = 4608, 3584
    knobs((knob,))
    enqueue_contract(lib, N, K, M, f"enqueue {form} {M}x{N}x{K}", out_offset=off)
    REACHED.add(f"w8a16-{form}")


# ----------------------------------------------------------------------------- dequantization[_silu]: out may alias y ----
@pytest.mark.parametrize("M,N", [(45, 96), (130, 50), (1, 7), (300, 1030)])
def test_dequantization_in_place(oracle, lib, M, N):
    """mixq_dequantization adds into `out`; mixq_dequantization_silu takes y and may write over it (out == y).  Both kernels work
    element by element, so every buffer sits at its element's natural alignment (int32: 4 bytes, fp16: 2)."""
    rng = np.random.default_rng(M + N)
    x = rng.integers(-2 ** 20, 2 ** 20, (M, N)).astype(np.int32)
    sR = (rng.random(M) * 0.05 + 1e-3).astype(np.float16)
    sC = (rng.random(N) * 1e-3 + 1e-5).astype(np.float16)
    y = rng.standard_normal((M, N)).astype(np.float16)
    rig = Rig({"x": (x, (G.i32_pattern(2 ** 31 - 1), G.i32_pattern(-2 ** 31)), 4), "sR": (sR, "f16", 2), "sC": (sC, "f16", 2), "y": (y, "f16", 2)})
    want = oracle.dequantization(x, sR, sC, y)
    guard = G.out_guard(N, 2)
    outs = []
    for which in (0, 1):
        rig.set_fill(which)
        out = fresh_out(M * N * 2, guard, offset=2, init=rig.orig["y"])
        assert lib.mixq_dequantization(vp(out.ptr), vp(rig.ptr("x")), vp(rig.ptr("sR")), vp(rig.ptr("sC")), M, N, stream()) == 0
        torch.cuda.synchronize()
        assert_intact(out, "mixq_dequantization: output")
        rig.check("mixq_dequantization")
        assert np.array_equal(bits16(out.body(np.float16, (M, N))), bits16(want)), "mixq_dequantization differs from the oracle"
        # the SiLU twin: separate buffers, then out == y
        sep = fresh_out(M * N * 2, guard, offset=2)
        assert lib.mixq_dequantization_silu(vp(sep.ptr), vp(rig.ptr("x")), vp(rig.ptr("sR")), vp(rig.ptr("sC")), vp(rig.ptr("y")), M, N, stream()) == 0
        torch.cuda.synchronize()
        assert_intact(sep, "mixq_dequantization_silu: output")
        rig.check("mixq_dequantization_silu")
        ref = sep.body_bytes().clone()
        assert not bool((sep.body(np.uint16) == 0xA5A5).all())
        al = fresh_out(M * N * 2, guard, offset=2, init=rig.orig["y"])
        assert lib.mixq_dequantization_silu(vp(al.ptr), vp(rig.ptr("x")), vp(rig.ptr("sR")), vp(rig.ptr("sC")), vp(al.ptr), M, N, stream()) == 0
        torch.cuda.synchronize()
        check_out(al, ref, "mixq_dequantization_silu out == y")
        outs.append(ref)
    assert torch.equal(outs[0], outs[1])
    got = outs[0].cpu().numpy().view(np.float16).reshape(M, N)
    ws = oracle.dequantization_silu(x, sR, sC, y)
    gb, wb = bits16(got).astype(np.int32), bits16(ws).astype(np.int32)
    assert np.abs(gb - wb).max() <= 1 and (gb != wb).mean() < 1e-3
    REACHED.add("dequantization")


# --------------------------------------------------------------------------- the quantisers' qA at 8-byte alignment ----
@pytest.mark.parametrize("M,K", [(7, 1040), (70, 4104), (3, 8)])
def test_quantiser_output_at_eight_byte_alignment(lib, M, K):
    """mixq_int8quant / mixq_quant_extract / mixq_int8_quantize_with_scale store qA eight bytes at a time (rows are K % 8 == 0 bytes
    long) and ask for no more than that: qA at ptr % 16 == 8, the scales and the gathered outliers (element stores) at their fp16
    alignment, the outlier indices at their int32 alignment."""
    rng = np.random.default_rng(M + K)
    n_out = min(O, K)
    ind = rng.choice(K, n_out, replace=False).astype(np.int32)
    A = (rng.standard_normal((M, K)) * 3).astype(np.float16)
    rig = Rig({"A": (A, "f16", MIN16), "ind": (ind, (G.i32_pattern(0), G.i32_pattern(K - 1)), 4)})
    st = stream()
    q0, s0, f0 = roomy(M * K, K, 1), roomy(2 * M, 1), roomy(2 * M * n_out, n_out)
    assert lib.mixq_quant_extract(M, K, vp(rig.pptr("A")), vp(q0.data_ptr()), vp(s0.data_ptr()), vp(f0.data_ptr()), vp(rig.pptr("ind")), n_out, 0, st) == 0
    torch.cuda.synchronize()
    for which in (0, 1):
        rig.set_fill(which)
        q = fresh_out(M * K, G.out_guard(K, 1), offset=8)
        sa = fresh_out(2 * M, 64 << 10, offset=2)
        fp = fresh_out(2 * M * n_out, G.out_guard(n_out, 2), offset=2)
        assert lib.mixq_quant_extract(M, K, vp(rig.ptr("A")), vp(q.ptr), vp(sa.ptr), vp(fp.ptr), vp(rig.ptr("ind")), n_out, 0, st) == 0
        torch.cuda.synchronize()
        what = f"mixq_quant_extract {M}x{K} (guard fill {which})"
        check_out(q, q0, what + " qA"), check_out(sa, s0, what + " sA"), check_out(fp, f0, what + " fpA")
        rig.check(what)
        q = fresh_out(M * K, G.out_guard(K, 1), offset=8)
        sa = fresh_out(2 * M, 64 << 10, offset=2)
        assert lib.mixq_int8quant(M, K, vp(rig.ptr("A")), vp(q.ptr), vp(sa.ptr), st) == 0
        torch.cuda.synchronize()
        check_out(q, q0, f"mixq_int8quant {M}x{K} qA"), check_out(sa, s0, f"mixq_int8quant {M}x{K} scale")
        q2 = fresh_out(M * K, G.out_guard(K, 1), offset=8)
        assert lib.mixq_int8_quantize_with_scale(M, K, vp(rig.ptr("A")), vp(sa.ptr), vp(q2.ptr), st) == 0
        torch.cuda.synchronize()
        assert_intact(q2, f"mixq_int8_quantize_with_scale {M}x{K}")
        rig.check(what + " (quantisers)")
    REACHED.add("quantiser-qA")


# ------------------------------------------------------------------- the fragment-major qA image at its declared size ----
@pytest.mark.parametrize("K", [1040, 1280])          # a partial last 64-byte k-step / whole steps (weight in 64-byte pieces / 256-byte runs)
@pytest.mark.parametrize("M", [5, 17, 33, 63, 64])   # partial and whole 16-row tiles
def test_fragment_major_image_at_its_declared_size(lib, knobs, M, K):
    """5..64 rows: the quantiser writes the skinny GEMM's fragment-major image into a buffer of exactly mixq_qa_bytes(M, K, layout)
    and the GEMM reads it from there.  The image's padding (rows M.. of the last tile, k = K.. of the last k-step) keeps the
    pre-fill -- 0x7f in one run, 0x80 in the other -- and must not reach the output."""
    N = N_RAGGED
    assert lib.mixq_qa_layout(M, N, K) == 1, "the shape must take the fragment-major image"
    nq = int(lib.mixq_qa_bytes(M, K, 1))
    assert nq == (M + 15) // 16 * 16 * ((K + 63) // 64 * 64)
    rng = np.random.default_rng(M + K)
    ind = rng.choice(K, O, replace=False).astype(np.int32)
    A = rng.standard_normal((M, K)).astype(np.float32)
    A[:, ind] *= 20.0
    rig = Rig({"A": (A.astype(np.float16), "f16", MIN16), "ind": (ind, (G.i32_pattern(0), G.i32_pattern(K - 1)), 4),
               "W": (rng.integers(-127, 128, (N, K), dtype=np.int8), "i8", MIN16),
               "sW": ((rng.random(N) * 4e-4 + 1e-4).astype(np.float16), "f16", MIN16),
               "fpW": ((rng.standard_normal((N, O)) * 0.02).astype(np.float16), "f16", MIN16),
               "y": ((rng.standard_normal((M, N)) * 0.5).astype(np.float16), "f16", MIN16)})
    st = stream()

    def flow(ptr, qa, sa, fpa, out, out2):
        rc = lib.mixq_quant_extract_layout(M, K, vp(ptr("A")), vp(qa), vp(sa), vp(fpa), vp(ptr("ind")), O, 0, 1, st)
        assert rc == 0, rc
        rc = lib.mixq_gemm_mixed_layout(vp(qa), vp(ptr("W")), vp(sa), vp(ptr("sW")), vp(fpa), vp(ptr("fpW")), vp(out), M, N, K, O, 1, None, 0, st)
        assert rc == 0, rc
        assert "gemm_skinny_kernel" in last_kernel(lib), last_kernel(lib)
        rc = lib.mixq_int8_fused_dequantize_layout(vp(qa), vp(ptr("W")), vp(sa), vp(ptr("sW")), vp(ptr("y")), None, vp(out2), M, N, K, 0, 1, None, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert "gemm_skinny_kernel" in last_kernel(lib), last_kernel(lib)

    z = lambda n: torch.zeros(n + 4096, dtype=torch.uint8, device="cuda:0")  # noqa: E731
    ref1, ref2 = roomy(M * N * 2, N), roomy(M * N * 2, N)
    pq, ps, pf = z(nq), z(2 * M), z(2 * M * O)
    flow(rig.pptr, pq.data_ptr(), ps.data_ptr(), pf.data_ptr(), ref1.data_ptr(), ref2.data_ptr())
    for which, pad in enumerate((0x7F, 0x80)):
        rig.set_fill(which)
        qa = Guarded(nq, pad, guard=G.IN_GUARD, offset=MIN16)
        sa = Guarded(2 * M, G.F16_NAN if which == 0 else G.F16_ONE, guard=G.IN_GUARD, offset=2)
        fpa = Guarded(2 * M * O, G.F16_NAN if which == 0 else G.F16_ONE, guard=G.IN_GUARD, offset=MIN16)
        out, out2 = fresh_out(M * N * 2, G.out_guard(N, 2)), fresh_out(M * N * 2, G.out_guard(N, 2), offset=MIN16 + 32)
        flow(rig.ptr, qa.ptr, sa.ptr, fpa.ptr, out.ptr, out2.ptr)
        what = f"fragment-major image {M}x{N}x{K} (padding 0x{pad:02x})"
        for g, name in ((qa, "qA image"), (sa, "sA"), (fpa, "fpA")):
            assert_intact(g, f"{what}: {name}")
        assert int((qa.body(np.uint8) == pad).sum()) >= nq - M * K, f"{what}: the quantiser wrote the image's padding"
        check_out(out, ref1, what + " mixq_gemm_mixed_layout")
        check_out(out2, ref2, what + " mixq_int8_fused_dequantize_layout")
        rig.check(what)
    REACHED.add("skinny-frag")


# ----------------------------------------------------------------------------- the weight-only (fpA_intB) GEMM forms ----
WoForm = namedtuple("WoForm", "name knobs rows K expect")
WO_ROWS = {831: 32, 832: 64, 833: 128, 834: 256, 835: 64, 836: 128}     # tile heights of the wide form's configurations
WO_FORMS = [WoForm("wo-narrow", (81,), 256, 1088, "w8a16 narrow")]
WO_FORMS += [WoForm(f"wo-wide-{c}-ks{k}", (c, k), WO_ROWS[c], 1088 if k <= 86 else 4160,
                    f"w8a16 wide cfg{c - 830}" + ("|K split" if k >= 87 else "")) for c in WO_ROWS for k in (85, 86, 87, 88, 89)]
WO_FORMS += [WoForm(f"wo-wide-{c}-{'registers' if rw == 847 else 'lds'}", (c, 86, rw), WO_ROWS[c], 1088,
                    f"w8a16 wide cfg{c - 830}" + ("| registers" if rw == 847 else "|!registers")) for c in (831, 832, 835, 836) for rw in (846, 847)]
WO_FORMS += [WoForm(f"wo-two-pass-{t}", (842, 843 if t == 256 else 844), t, 1088, f"w8a16 two-pass|{t}-row") for t in (256, 128)]
WO_FORMS += [WoForm(f"wo-skinny-{k}", (k,), 16, 1088, "w8a16 skinny") for k in (852, 853, 854, 855)]
WO = {f.name: f for f in WO_FORMS}
WO_CASES = [(f.name, f.rows + d, n) for f in WO_FORMS for d, n in ((1, 272), (-1, 274))]   # N % 4 == 0 / N % 4 == 2


def wo_rig(M, N, K):
    key = ("wo", M, N, K)
    if key not in _RIGS:
        from mixq_tensorrt_llm_amd import _lib
        rng = np.random.default_rng(M + 3 * N + K)
        q = rng.integers(-128, 128, size=(K, N), dtype=np.int8)
        qi = np.empty(q.shape, np.uint8)
        _lib.check(_lib.load().mixq_preprocess_weights_int8(qi.ctypes.data, q.ctypes.data, K, N), "preprocess")
        _RIGS[key] = Rig({"A": (rng.standard_normal((M, K)).astype(np.float16), "f16", MIN16), "W": (qi, (b"\x7f", b"\x80"), MIN16),
                          "scale": ((rng.random(N) * 1e-3 + 1e-4).astype(np.float16), "f16", 2)})   # (read element by element in every form)
    return _RIGS[key]


def wo_expect(expect, kern, what):
    for part in expect.split("|"):
        if part.startswith("!"):
            assert part[1:] not in kern, f"{what}: the launch took {kern!r}"
        else:
            assert part in kern, f"{what}: the launch took {kern!r}"


def wo_contract(lib, rig, M, N, K, n_ws, out_off, expect, what, ref=None):
    """mixq_w8a16_gemm_forward_ws in guarded buffers against the same call on ordinary ones (or ``ref``): the output at ``out_off``."""
    st = stream()
    if ref is None:
        ref = roomy(M * N * 2, N)
        ws = torch.zeros(n_ws + 4096, dtype=torch.uint8, device="cuda:0")
        rc = lib.mixq_w8a16_gemm_forward_ws(vp(rig.pptr("A")), vp(rig.pptr("W")), vp(rig.pptr("scale")), vp(ref.data_ptr()), M, N, K,
                                            vp(ws.data_ptr()) if n_ws else None, n_ws, st)
        assert rc == 0, f"{what}: mixq error {rc} on ordinary buffers"
        torch.cuda.synchronize()
        wo_expect(expect, last_kernel(lib), what)
    for which in (0, 1):
        rig.set_fill(which)
        out = fresh_out(M * N * 2, G.out_guard(N, 2), offset=out_off)
        scr = fresh_scratch(n_ws)
        rc = lib.mixq_w8a16_gemm_forward_ws(vp(rig.ptr("A")), vp(rig.ptr("W")), vp(rig.ptr("scale")), vp(out.ptr), M, N, K,
                                            vp(scr.ptr) if scr else None, n_ws, st)
        assert rc == 0, f"{what}: mixq error {rc}"
        torch.cuda.synchronize()
        wo_expect(expect, last_kernel(lib), what)
        check_out(out, ref, f"{what} (guard fill {which})")
        check_scratch(scr, f"{what} (guard fill {which})")
        rig.check(f"{what} (guard fill {which})")
    return ref


@pytest.mark.parametrize("name,M,N", WO_CASES, ids=[f"{n}-M{m}-N{c}" for n, m, c in WO_CASES])
def test_weight_only_form_in_guarded_buffers(lib, knobs, name, M, N):
    """Every fpA_intB form: activations and weight at 16 bytes, the scale at its natural alignment, the output at what its stores need
    (8 bytes where N % 4 == 0: four fp16 per store; 4 bytes where N % 4 == 2; 16 for the two-pass form, whose second pass stores
    16-byte pieces), the workspace at exactly mixq_w8a16_gemm_workspace_size."""
    f = WO[name]
    K = f.K
    rig = wo_rig(M, N, K)
    knobs(f.knobs)
    n_ws = int(lib.mixq_w8a16_gemm_workspace_size(M, N, K))
    two_pass = "two-pass" in name
    if two_pass and N % 8:   # rows of the output are not 16-byte aligned: the forced form does not apply, a fused form runs
        wo_contract(lib, rig, M, N, K, n_ws, 4, "w8a16|!two-pass", f"{name} {M}x{N}x{K} (N % 8 != 0)")
        return
    if two_pass:
        assert n_ws >= WORDS + 2 * N * K
    off = MIN16 if two_pass else 8 if N % 4 == 0 else 4
    wo_contract(lib, rig, M, N, K, n_ws, off, f.expect, f"{name} {M}x{N}x{K}")
    if two_pass:   # an output that is 8- but not 16-byte aligned keeps the fused forms (same scratch offered): the bits of the call with the two-pass form off
        knobs((841,))
        ref = roomy(M * N * 2, N)
        ws = torch.zeros(n_ws, dtype=torch.uint8, device="cuda:0")
        assert lib.mixq_w8a16_gemm_forward_ws(vp(rig.pptr("A")), vp(rig.pptr("W")), vp(rig.pptr("scale")), vp(ref.data_ptr()), M, N, K,
                                              vp(ws.data_ptr()), n_ws, stream()) == 0
        torch.cuda.synchronize()
        knobs(f.knobs)
        wo_contract(lib, rig, M, N, K, n_ws, 8, "w8a16|!two-pass", f"{name} {M}x{N}x{K}, output 8-byte aligned", ref=ref)
    REACHED.add(name)


WO_AUTO = [(48, 12288, 256, "skinny"), (64, 10240, 192, "narrow"), (200, 4096, 512, "wide"), (700, 3584, 704, "wide"), (1300, 8704, 128, "two-pass")]


@pytest.mark.parametrize("M,N,K,form", WO_AUTO)
def test_weight_only_automatic_plan_in_guarded_buffers(lib, knobs, M, N, K, form):
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the plan is fitted on 256 CUs")
    rig = wo_rig(M, N, K)
    n_ws = int(lib.mixq_w8a16_gemm_workspace_size(M, N, K))
    wo_contract(lib, rig, M, N, K, n_ws, MIN16 if form == "two-pass" else 8, "w8a16 " + form, f"fpA_intB automatic {M}x{N}x{K}")
    REACHED.add("wo-auto:" + form)


@pytest.mark.parametrize("knob,form,off", [(857, "GEMV", 2), (856, "skinny", 8)])
@pytest.mark.parametrize("M", [1, 4])
def test_weight_only_decode_rows_in_guarded_buffers(lib, knobs, knob, form, off, M):
    """mixq_w8a16_gemm_forward at 1..4 tokens: the GEMV stores element by element (output at ptr % 16 == 2), the skinny form 8 bytes."""
    N, K = 272, 1088
    rig = wo_rig(M, N, K)
    knobs((knob,))
    wo_contract(lib, rig, M, N, K, 0, off, "w8a16 " + form, f"fpA_intB {form} {M}x{N}x{K}")
    REACHED.add("wo-decode:" + form)


# -------------------------------------------------------------------------------------------- the packed-int4 stream ----
def s4_rig(M, N, kp):
    key = ("s4", M, N, kp)
    if key not in _RIGS:
        rng = np.random.default_rng(M + N + kp)
        _RIGS[key] = Rig({"A": (rng.integers(0, 256, (M, kp), dtype=np.uint8), (b"\x7f", b"\x80"), MIN16),
                          "B": (rng.integers(0, 256, (N, kp), dtype=np.uint8), (b"\x7f", b"\x80"), MIN16),
                          "sA": ((rng.random(M) * 0.05 + 0.01).astype(np.float16), "f16", 2),
                          "sW": ((rng.random(N) * 4e-3 + 1e-3).astype(np.float16), "f16", MIN16),
                          "y": ((rng.standard_normal((M, N)) * 0.5).astype(np.float16), "f16", MIN16),
                          "x": (rng.standard_normal((M, 2 * kp)).astype(np.float16), "f16", MIN16)})
    return _RIGS[key]


S4_CASES = [("rule", 872, 17, 272, 528), ("rule", 872, 15, 272, 528), ("pieces", 873, 17, 272, 528), ("pieces", 873, 63, 272, 528),
            ("runs", 874, 17, 272, 528), ("runs", 874, 15, 272, 528), ("runs", 874, 65 - 1, 272, 528), ("rule", 872, 8, 12288, 2048)]


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("route,knob,M,N,kp", S4_CASES)
def test_int4_stream_in_guarded_buffers(lib, knobs, route, knob, M, N, kp, silu):
    """mixq_int4_fused_dequantize[_silu] on decode batches: one launch on the PACKED weight, no workspace (declared size 0)."""
    rig = s4_rig(M, N, kp)
    knobs((knob,))
    assert lib.mixq_int4_fused_workspace_size(M, N, kp) == 0
    fn = lib.mixq_int4_fused_dequantize_silu if silu else lib.mixq_int4_fused_dequantize
    st = stream()
    ref = roomy(M * N * 2, N)
    assert fn(vp(rig.pptr("A")), vp(rig.pptr("B")), vp(rig.pptr("sA")), vp(rig.pptr("sW")), vp(rig.pptr("y")), vp(ref.data_ptr()), M, N, kp, None, st) == 0
    torch.cuda.synchronize()
    for which in (0, 1):
        rig.set_fill(which)
        out = fresh_out(M * N * 2, G.out_guard(N, 2))
        assert fn(vp(rig.ptr("A")), vp(rig.ptr("B")), vp(rig.ptr("sA")), vp(rig.ptr("sW")), vp(rig.ptr("y")), vp(out.ptr), M, N, kp, None, st) == 0
        torch.cuda.synchronize()
        assert "gemm_skinny_s4_kernel (packed" in last_kernel(lib), last_kernel(lib)
        what = f"int4 stream {route} {M}x{N}x{2 * kp} silu={silu} (guard fill {which})"
        check_out(out, ref, what)
        rig.check(what)
    REACHED.add("int4-stream-" + route)


@pytest.mark.parametrize("M,knob", [(1, 875), (15, 877), (16, 877)])
def test_int4_quantiser_inside_form_in_guarded_buffers(lib, knobs, M, knob):
    """mixq_int4_linear_forward, the rows quantised inside the weight-streaming launch (one row by rule; knob 877: up to 16): x_scale is
    WRITTEN -- a guarded output at its natural alignment --, q_packed and the workspace are not touched (NULL)."""
    N, kp = 272, 528
    rig = s4_rig(M, N, kp)
    knobs((knob,))
    st = stream()
    ref = roomy(M * N * 2, N)
    ref_s = torch.full((2 * M + 64,), 0x7E, dtype=torch.uint8, device="cuda:0")
    args = lambda x, B, xs, sW, y, D: (vp(x), vp(B), vp(xs), None, vp(sW), vp(y), vp(D), M, N, kp, 0, None, st)  # noqa: E731
    assert lib.mixq_int4_linear_forward(*args(rig.pptr("x"), rig.pptr("B"), ref_s.data_ptr(), rig.pptr("sW"), rig.pptr("y"), ref.data_ptr())) == 0
    torch.cuda.synchronize()
    assert "gemm_skinny_s4_kernel<QF>" in last_kernel(lib), last_kernel(lib)
    for which in (0, 1):
        rig.set_fill(which)
        out = fresh_out(M * N * 2, G.out_guard(N, 2))
        xs = fresh_out(2 * M, 64 << 10, offset=2)
        assert lib.mixq_int4_linear_forward(*args(rig.ptr("x"), rig.ptr("B"), xs.ptr, rig.ptr("sW"), rig.ptr("y"), out.ptr)) == 0
        torch.cuda.synchronize()
        assert "gemm_skinny_s4_kernel<QF>" in last_kernel(lib), last_kernel(lib)
        what = f"int4 quantiser-inside form {M}x{N}x{2 * kp} (guard fill {which})"
        check_out(out, ref, what)
        check_out(xs, ref_s[:2 * M], what + " x_scale")
        rig.check(what)
    REACHED.add("int4-quantiser-inside")


def test_int4_unpack_route_workspace_at_its_declared_size(lib, knobs):
    """More than 64 rows: both operands are widened into `workspace`, exactly mixq_int4_fused_workspace_size bytes at 16 bytes."""
    M, N, kp = 65, 272, 528
    rig = s4_rig(M, N, kp)
    n_ws = int(lib.mixq_int4_fused_workspace_size(M, N, kp))
    assert n_ws == (2 * M * kp + 15) // 16 * 16 + (2 * N * kp + 15) // 16 * 16
    st = stream()
    ref = roomy(M * N * 2, N)
    ws = torch.zeros(n_ws + 4096, dtype=torch.uint8, device="cuda:0")
    call = lambda p, D, w: lib.mixq_int4_fused_dequantize(vp(p("A")), vp(p("B")), vp(p("sA")), vp(p("sW")), vp(p("y")), vp(D), M, N, kp, vp(w), st)  # noqa: E731
    assert call(rig.pptr, ref.data_ptr(), ws.data_ptr()) == 0
    torch.cuda.synchronize()
    for which in (0, 1):
        rig.set_fill(which)
        out = fresh_out(M * N * 2, G.out_guard(N, 2))
        wsg = Guarded(n_ws, WS_PAT, guard=G.SCRATCH_GUARD, offset=MIN16)
        wsg.body_bytes().fill_(0xFF)
        assert call(rig.ptr, out.ptr, wsg.ptr) == 0
        torch.cuda.synchronize()
        what = f"int4 unpack route {M}x{N}x{2 * kp} (guard fill {which})"
        check_out(out, ref, what)
        assert_intact(wsg, what + ": workspace")
        rig.check(what)
    REACHED.add("int4-unpack")


# ---------------------------------------------------------------------------------------------------------- coverage ----
def required():
    need = {f.name for f in FAMILIES} | {"extremes:" + f.name for f in FAMILIES}
    need |= {f"enqueue-{a}:{n}" for n, _ in ENQ_FORCED for a in ("fp16", "bf16")}
    need |= {"auto:" + c[5] for c in AUTO} | {"w8a16-gemv", "w8a16-skinny", "dequantization"}
    need |= {f.name for f in WO_FORMS} | {"wo-auto:" + c[3] for c in WO_AUTO} | {"wo-decode:GEMV", "wo-decode:skinny", "skinny-frag", "quantiser-qA"}
    need |= {"int4-stream-rule", "int4-stream-pieces", "int4-stream-runs", "int4-quantiser-inside", "int4-unpack"}
    return need


def test_every_family_was_reached():
    """Runs last: every family of the list above went through its guarded cases in this session (a skipped case covers nothing)."""
    missing = sorted(required() - REACHED)
    assert not missing, f"{len(missing)} families not reached: {missing}"
