"""GPU (-m gpu): every output element of every plan the selection ladder takes BY ITSELF (csrc/gemm_plan.hip plan_gemm).

tests/golden/plan_cells.json (tools/plan_cells.py, host only) holds the cheapest (M, N, K, registered weight image) of every plan text
mixq_describe_plan can print on a fixed lattice, plus cells named by hand for plan attributes the text does not show (the mid kernel's
rotated K walk, the non-temporal weight loads of the skinny run route and of the tile kernels, the M <= 4 launch on qweight).  Here each
cell goes through mixq_enqueue exactly as an integrator calls it -- every knob at its default, a workspace of exactly
mixq_workspace_size(h, M, N, K) bytes in a tests/guarded.py buffer at ptr % 128 == 8, an output of exactly M x N elements in a guarded
buffer pre-filled with NaN, the weight image registered for the image cells -- and per cell:

 a. the plan is the pinned one (mixq_describe_plan's text, mixq_debug_last_gemm_kernel()'s family; 256-CU parts only -- the numeric
    checks below run on whatever plan another part takes);
 b. every element against a restatement of the operator: qA / sA / fpA from the oracle's quantiser, the int32 sums from ONE float64
    matmul of the int8 operands on the device (exact: |sum| <= 127^2 K < 2^53 in any order; cross-checked against oracle.gemm_s8s8s32 on
    16 rows), P16 from oracle.gemm_fp16, the result from oracle.dequant_epilogue; conftest.assert_elementwise with prefill_slack, and the
    1e-3-of-maximum bound (conftest.assert_prefill_parity's two bounds).  The M <= 4 cells: oracle.w8a16_gemv with w8a16_slack;
 c. the bits of the same call with the GEMM forced to the two-barrier kernel, K not split over workgroups (knobs 1 + 70: the baseline
    of the "gives the bits of the one-workgroup form" tests).  No family needed the relaxation to (b)'s bound.  (M <= 4: no int8 GEMM
    runs, nothing to force);
 d. the guards of workspace and output are intact and no NaN is left in the output;
 e. a second call on the same handle and the same, uncleared workspace with other activations gives the bits of that input's own
    first call; and all cells of one family enqueued back to back on one stream without synchronising, on ONE workspace sized for the
    largest, each give their own solo bits.

One cell per family also runs as a bf16 call (tests/bf16_restate.py, prefill_bound) and through mixq_enqueue_bias
(assert_prefill_parity(bias=...)); the three hidden-attribute cells equal the same call with the attribute switched off (knobs 1411,
887, 1291)."""
import ctypes
import json
import os
import time

import numpy as np
import pytest

import bf16_restate as R
import guarded as G
from conftest import GOLDEN, assert_elementwise, assert_prefill_parity, make_layer, prefill_slack, ulp16, w8a16_slack
from guarded import Guarded, assert_intact

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

O = 128
WS_PAT, WS_FILL = 0x3C, 0xFF          # workspace guards / the workspace's own pre-fill (an engine's workspace holds anything)
OUT_PAT = 0xA5                        # output guards (the body is pre-filled with NaN)
WS_OFFSET, OUT_OFFSET = 8, 16         # ptr % 256: the workspace base may be anything (8), the output is checked for 16 bytes
BASELINE_KNOBS = (1, 70)              # the two-barrier kernel for every M > 4, no K split over workgroups
ATTRIBUTE_OFF = {"mid-rotated-walk": 1411, "skinny-runs-nontemporal": 887, "tiles-nontemporal": 1291}

_PINNED = json.load(open(os.path.join(GOLDEN, "plan_cells.json")))
CELLS = [dict(c, id=f"{c['M']}x{c['N']}x{c['K']}{'-image' if c['image'] else ''}") for c in _PINNED["cells"]]
CELLS += [dict(c, id=c["name"]) for c in _PINNED["named"]]
CELL = {c["id"]: c for c in CELLS}


def family_of(plan):
    """The kernel family of a plan text (the seven of plan_gemm + the M <= 4 launch)."""
    if plan.startswith("w8a16"):
        return "w8a16"
    said = plan.split(", then ")[1]
    for prefix, fam in (("skinny", "skinny"), ("deep", "mid" if "copy-only waves" in said else "deep"), ("ping-pong 128x256", "pp128"),
                        ("ping-pong 256x256 tiles,", "pp256-split"), ("ping-pong 256x256 tiles:", "pp256-split"),
                        ("ping-pong 256x256 tiles", "pp256"), ("two-barrier", "two-barrier")):
        if said.startswith(prefix):
            return fam
    raise AssertionError(f"unknown plan text {plan!r}")


FAMILIES = sorted({family_of(c["plan"]) for c in CELLS})
FIRST_OF_FAMILY = {}
for _c in CELLS:
    FIRST_OF_FAMILY.setdefault(family_of(_c["plan"]), _c["id"])      # (cells are sorted by cost: the cheapest of each family)
TIMES = {}


# ------------------------------------------------------------------------------------------------------------ plumbing ----
@pytest.fixture(scope="module")
def lib():
    from mixq_tensorrt_llm_amd import _lib
    lib = _lib.load()
    assert lib.mixq_debug_knobs_enabled() == 1, "the form knobs need MIXQ_DEBUG_KNOBS=1 (tests/conftest.py)"
    lib.mixq_debug_reset()
    yield lib
    lib.mixq_debug_reset()
    _LAYERS.clear(), _SOLO.clear()
    torch.cuda.empty_cache()
    if TIMES:
        slow = sorted(TIMES.items(), key=lambda kv: -kv[1])[:3]
        print("\nslowest plan cells: " + ", ".join(f"{k} {v:.1f} s" for k, v in slow))


@pytest.fixture()
def knobs(lib):
    """Knobs at their defaults before and after, pass or fail; the returned function sets some in between."""
    lib.mixq_debug_reset()

    def set_(values):
        lib.mixq_debug_reset()
        for v in values:
            lib.mixq_debug_set_gemm_variant(v)
    yield set_
    lib.mixq_debug_reset()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync():
    """Wait for the device; a HIP error here is a fault of the device, after which nothing more is started on it: the run ends."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported an error, no further test is started: {e}", returncode=3)


def vp(x):
    return None if x is None else ctypes.c_void_p(int(x))


def on_cu256():
    return torch.cuda.get_device_properties(0).multi_processor_count == 256


def described(lib, c):
    buf = ctypes.create_string_buffer(320)
    assert lib.mixq_describe_plan(c["M"], c["N"], c["K"], c["image"], buf, 320) == 0
    return buf.value.decode()


_LAYERS, _SOLO = {}, {}
_ROWS = {}
for _c in CELLS:
    _ROWS[(_c["N"], _c["K"])] = max(_ROWS.get((_c["N"], _c["K"]), 0), _c["M"])


class Layer:
    """One packed layer [N, K] on the host and on the device, with activations for the tallest cell that uses it."""

    def __init__(self, oracle, N, K):
        A, W, act = make_layer(_ROWS[(N, K)] + 1, N, K, seed=N + K)
        self.A, self.p = A, oracle.pack_linear_weights(W, act)
        p = self.p
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
        self.ind = np.ascontiguousarray(p["fp_ind"]).astype(np.int32)
        self.d = {"weight": dev(p["weight"]), "wsf": dev(p["weights_scaling_factor"]), "fp_weight": dev(p["fp_weight"]),
                  "fp_weight_bf16": R.from_bits(R.bf16_rn(p["fp_weight"].astype(np.float32)), "cuda:0"), "fp_ind": dev(self.ind),
                  "qweight": dev(p["qweight"])}
        self.image = self.image_weight = None

    def acts(self, M, other=False):
        """The cell's activations, rows 0 .. M - 1; other: rows M .. 1 (another row at every place but, for even M, the middle one)."""
        return (self.A[1:M + 1][::-1] if other else self.A[:M]).copy()

    def weight_ptr(self, lib, image):
        """The int8 weight of a call; the image cells take a copy of their own (the registry goes by the weight's pointer) with its
        image buffer of exactly mixq_weight_image_bytes."""
        if not image:
            return self.d["weight"].data_ptr()
        if self.image_weight is None:
            N, K = self.d["weight"].shape
            self.image_weight = self.d["weight"].clone()
            self.image = Guarded(int(lib.mixq_weight_image_bytes(N, K)), 0x6B, guard=G.IN_GUARD, offset=16)
        return self.image_weight.data_ptr()

    def register(self, lib):
        N, K = self.d["weight"].shape
        w = self.weight_ptr(lib, 1)
        assert lib.mixq_weight_image_register(vp(w), N, K, vp(self.image.ptr), stream()) == 0
        assert lib.mixq_weight_image_verify(vp(w), stream()) == 0
        assert_intact(self.image, "weight image registration")
        return w


def layer_of(oracle, N, K):
    if (N, K) not in _LAYERS:
        if sum(L.d["weight"].numel() for L in _LAYERS.values()) > (1 << 30):     # (keep the resident weights below ~1 GiB + their float64 twins)
            _LAYERS.clear()
        _LAYERS[(N, K)] = Layer(oracle, N, K)
    return _LAYERS[(N, K)]


def enqueue(lib, h, L, A_d, out_ptr, ws_ptr, M, N, K, bf16=False, bias_ptr=None, image=0):
    from mixq_tensorrt_llm_amd._lib import MIXQ_TYPE_BF16, MIXQ_TYPE_HALF, TensorDesc
    t_act = MIXQ_TYPE_BF16 if bf16 else MIXQ_TYPE_HALF
    shapes = [(M, K), (N, K // 2), (N,), (N, O), (2 * O,), (K, N // 2), (N,)]
    in_desc = (TensorDesc * 7)(*[TensorDesc.make(s, t_act if i in (0, 3) else MIXQ_TYPE_HALF) for i, s in enumerate(shapes)])
    out_desc = TensorDesc.make((M, N), t_act)
    d = L.d
    ins = (ctypes.c_void_p * 7)(A_d.data_ptr(), L.weight_ptr(lib, image), d["wsf"].data_ptr(), d["fp_weight_bf16" if bf16 else "fp_weight"].data_ptr(),
                                d["fp_ind"].data_ptr(), d["qweight"].data_ptr(), d["wsf"].data_ptr())
    outs = (ctypes.c_void_p * 1)(out_ptr)
    if bias_ptr is not None:
        return lib.mixq_enqueue_bias(h, in_desc, ctypes.byref(out_desc), ins, outs, vp(bias_ptr), vp(ws_ptr), stream())
    return lib.mixq_enqueue(h, in_desc, ctypes.byref(out_desc), ins, outs, vp(ws_ptr), stream())


class Call:
    """One cell's call in guarded buffers: the handle, the registered image, the workspace of exactly mixq_workspace_size bytes and an
    output of exactly M x N elements pre-filled with NaN."""

    def __init__(self, lib, L, c, bf16=False):
        self.lib, self.L, self.c, self.bf16 = lib, L, c, bf16
        M, N, K = c["M"], c["N"], c["K"]
        self.h = ctypes.c_void_p(lib.mixq_create(M, N, K))
        self.n_ws = int(lib.mixq_workspace_size(self.h, M, N, K))
        self.ws = Guarded(self.n_ws, WS_PAT, guard=G.SCRATCH_GUARD, offset=WS_OFFSET)
        self.ws.body_bytes().fill_(WS_FILL)
        self.nan = 0x7FC0 if bf16 else 0x7E00
        self.out = Guarded(M * N * 2, OUT_PAT, init=torch.full((M * N,), self.nan, dtype=torch.int16, device="cuda:0"),
                           guard=G.out_guard(N, 2), offset=OUT_OFFSET)
        self.registered = L.register(lib) if c["image"] else None

    def run(self, A_d, what, bias_ptr=None):
        """One enqueue on the output pre-filled with NaN again -> the output's bytes (a device copy); checks (d)."""
        c = self.c
        self.out.body_bytes().view(torch.int16).fill_(self.nan)
        rc = enqueue(self.lib, self.h, self.L, A_d, self.out.ptr, self.ws.ptr, c["M"], c["N"], c["K"], self.bf16, bias_ptr, c["image"])
        assert rc == 0, f"{what}: mixq error {rc}"
        sync()
        assert_intact(self.out, f"{what}: output")
        assert_intact(self.ws, f"{what}: workspace of {self.n_ws} bytes")
        got = self.out.body_bytes().clone()
        dt = torch.bfloat16 if self.bf16 else torch.float16
        left = int(torch.isnan(got.view(dt)).sum())
        assert left == 0, f"{what}: {left} of {c['M'] * c['N']} outputs are NaN (not written, or wrong)"
        return got

    def close(self):
        if self.registered:
            self.lib.mixq_weight_image_unregister(vp(self.registered))
            self.registered = None
            assert_intact(self.L.image, "weight image after the calls")
        if self.h:
            self.lib.mixq_destroy(self.h)
            self.h = None


def dev_acts(A):
    return torch.from_numpy(A).to("cuda:0")


def restated(oracle, L, A):
    """(want fp16 [M, N], slack) of the operator on A: host quantiser, exact device int32 sums, host side product and epilogue."""
    p = L.p
    M = A.shape[0]
    qA, sA = oracle.quant_rows(A)
    fpA = oracle.extract_outliers(A, L.ind)
    acc64 = torch.from_numpy(qA).to("cuda:0").double() @ L.d["weight"].double().T
    assert float(acc64.abs().max()) < 2.0 ** 31
    acc = acc64.to(torch.int32).cpu().numpy()
    del acc64
    rows = np.unique(np.concatenate([[0, M - 1], np.random.default_rng(M).integers(0, M, 14)]))
    assert np.array_equal(acc[rows], oracle.gemm_s8s8s32(qA[rows], p["weight"])), "the device's float64 sums differ from oracle.gemm_s8s8s32"
    P16 = oracle.gemm_fp16(fpA, p["fp_weight"])
    want = oracle.dequant_epilogue(acc, sA, p["weights_scaling_factor"], P16)
    return want, prefill_slack({"P": P16}, A, p)


def unprocessed_qweight(lib, L):
    K, N = L.p["qweight"].shape
    q_un = np.empty((K, N), np.int8)
    lib.mixq_unprocess_weights_int8(q_un.ctypes.data, L.p["qweight"].ctypes.data, K, N)
    return q_un


def solo(lib, oracle, c):
    """The cell's automatic call on its own (cached: output bytes on the device)."""
    if c["id"] not in _SOLO:
        L = layer_of(oracle, c["N"], c["K"])
        call = Call(lib, L, c)
        try:
            _SOLO[c["id"]] = call.run(dev_acts(L.acts(c["M"])), f"{c['id']} solo")
        finally:
            call.close()
    return _SOLO[c["id"]]


def baseline(lib, knobs, L, c, A_d, extra=()):
    """The same call under other knobs, in ordinary buffers with a workspace sized under those knobs -> output bytes."""
    M, N, K = c["M"], c["N"], c["K"]
    knobs(extra)
    h = ctypes.c_void_p(lib.mixq_create(M, N, K))
    try:
        ws = torch.zeros(int(lib.mixq_workspace_size(h, M, N, K)) + 256, dtype=torch.uint8, device="cuda:0")
        out = torch.zeros(M * N * 2 + G.out_guard(N, 2), dtype=torch.uint8, device="cuda:0")[:M * N * 2]
        assert enqueue(lib, h, L, A_d, out.data_ptr(), ws.data_ptr(), M, N, K) == 0
        sync()
        kern = lib.mixq_debug_last_gemm_kernel()
    finally:
        lib.mixq_destroy(h)
        knobs(())
    return out, kern


# ------------------------------------------------------------------------------------------------------------ the cells ----
@pytest.mark.parametrize("cid", [c["id"] for c in CELLS])
def test_plan_cell(oracle, lib, knobs, cid):
    from test_gpu_selection import FAMILY
    t0 = time.perf_counter()
    c = CELL[cid]
    M, N, K = c["M"], c["N"], c["K"]
    assert M * N * K <= _PINNED["lattice"]["max_MNK"]
    L = layer_of(oracle, N, K)
    A, A2 = L.acts(M), L.acts(M, other=True)
    call = Call(lib, L, c)
    try:
        got_d = call.run(dev_acts(A), cid)
        launched = lib.mixq_debug_last_gemm_kernel()
        # a. the pinned plan
        if on_cu256():
            said = described(lib, c)
            assert said == c["plan"], f"{cid}: pinned {c['plan']!r}, the library says {said!r}"
            if M > 4:
                want_kernel = next(k for p_, k in FAMILY if said.split(", then ")[1].startswith(p_))
                assert want_kernel in launched, (cid, said, launched)
            else:
                assert b"w8a16" in launched, (cid, launched)
        # b. every element against the restatement
        got = got_d.cpu().numpy().view(np.float16).reshape(M, N)
        if M > 4:
            want, slack = restated(oracle, L, A)
        else:
            q_un = unprocessed_qweight(lib, L)
            want = oracle.w8a16_gemv(A, q_un, L.p["weights_scaling_factor"])
            slack = w8a16_slack(A, q_un, L.p["weights_scaling_factor"])
        rel = np.abs(got.astype(np.float64) - want.astype(np.float64)).max() / max(np.abs(want.astype(np.float64)).max(), 1e-30)
        print(f"{cid}: {launched.decode()}; max-normalised error {rel:.3e}")
        assert rel < 1e-3, f"{cid}: max-normalised error {rel:.3e}"
        assert_elementwise(got, want, slack, f"{cid} ({launched.decode()})")
        _SOLO[cid] = got_d
        # e. the same handle and workspace again, uncleared, on other activations == those activations on a workspace in its first state
        second = call.run(dev_acts(A2), f"{cid} second call")
        assert not torch.equal(second, got_d)
        call.ws.body_bytes().fill_(WS_FILL)
        first = call.run(dev_acts(A2), f"{cid} other activations, first call")
        assert torch.equal(second, first), f"{cid}: a second call on the uncleared workspace differs from that input's first call"
    finally:
        call.close()
    if M > 4:
        # c. the bits of the two-barrier kernel, K not split over workgroups
        base, kern = baseline(lib, knobs, L, c, dev_acts(A), BASELINE_KNOBS)
        assert b"two-barrier" in kern, kern
        assert torch.equal(got_d, base), (f"{cid}: {int((got_d != base).sum())} output bytes differ from the two-barrier kernel's "
                                          f"({launched.decode()})")
        if cid in ATTRIBUTE_OFF:   # the attribute the plan text does not show, switched off: the same family, the same bits
            off, kern = baseline(lib, knobs, L, c, dev_acts(A), (ATTRIBUTE_OFF[cid],))
            assert kern == launched, (kern, launched)
            assert torch.equal(got_d, off), f"{cid}: differs from the same plan with knob {ATTRIBUTE_OFF[cid]}"
    TIMES[cid] = time.perf_counter() - t0


@pytest.mark.parametrize("fam", FAMILIES)
def test_one_family_back_to_back_on_one_workspace(oracle, lib, knobs, fam):
    """(e) All cells of one family on one stream, no synchronisation in between, one workspace sized for the largest of them."""
    cells = [c for c in CELLS if family_of(c["plan"]) == fam]
    solos = [solo(lib, oracle, c) for c in cells]
    layers = [layer_of(oracle, c["N"], c["K"]) for c in cells]
    acts = [dev_acts(L.acts(c["M"])) for L, c in zip(layers, cells)]
    handles = [ctypes.c_void_p(lib.mixq_create(c["M"], c["N"], c["K"])) for c in cells]
    images = []
    try:
        n_ws = max(int(lib.mixq_workspace_size(h, c["M"], c["N"], c["K"])) for h, c in zip(handles, cells))
        ws = Guarded(n_ws, WS_PAT, guard=G.SCRATCH_GUARD, offset=WS_OFFSET)
        ws.body_bytes().fill_(WS_FILL)
        outs = [Guarded(c["M"] * c["N"] * 2, OUT_PAT, init=torch.full((c["M"] * c["N"],), 0x7E00, dtype=torch.int16, device="cuda:0"),
                        guard=G.out_guard(c["N"], 2), offset=OUT_OFFSET) for c in cells]
        for L, c in zip(layers, cells):
            if c["image"]:
                images.append(L.register(lib))
        sync()
        for h, L, c, A_d, out in zip(handles, layers, cells, acts, outs):
            assert enqueue(lib, h, L, A_d, out.ptr, ws.ptr, c["M"], c["N"], c["K"], image=c["image"]) == 0
        sync()
        assert_intact(ws, f"{fam}: shared workspace of {n_ws} bytes")
        for c, L, out, want in zip(cells, layers, outs, solos):
            assert_intact(out, f"{fam} {c['id']}: output")
            assert torch.equal(out.body_bytes(), want), f"{fam}: {c['id']} back to back differs from its solo call"
    finally:
        for w in images:
            lib.mixq_weight_image_unregister(vp(w))
        for h in handles:
            lib.mixq_destroy(h)


@pytest.mark.parametrize("fam", FAMILIES)
def test_bf16_twin_and_bias_form_of_one_cell_per_family(oracle, lib, knobs, fam):
    c = CELL[FIRST_OF_FAMILY[fam]]
    M, N, K = c["M"], c["N"], c["K"]
    L = layer_of(oracle, N, K)
    p, A = L.p, L.acts(M)
    # the bias form, fp16
    bias = (np.random.default_rng(N + M).standard_normal(N) * 0.5).astype(np.float16)
    bias[:6] = np.array([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 3e-5, 1.0], np.float16)
    bias_d = torch.from_numpy(bias).to("cuda:0")
    call = Call(lib, L, c)
    try:
        got = call.run(dev_acts(A), f"{c['id']} + bias", bias_ptr=bias_d.data_ptr()).cpu().numpy().view(np.float16).reshape(M, N)
        kern = lib.mixq_debug_last_gemm_kernel()
    finally:
        call.close()
    if M > 4:
        assert_prefill_parity(oracle, got, A, p, f"{c['id']} + bias ({kern.decode()})", bias=bias)
    else:
        q_un = unprocessed_qweight(lib, L)
        want = oracle.w8a16_gemv(A, q_un, p["weights_scaling_factor"])
        slack = w8a16_slack(A, q_un, p["weights_scaling_factor"]) + ulp16(want)
        with np.errstate(over="ignore"):
            want = (want + bias[None, :]).astype(np.float16)
        assert_elementwise(got, want, slack, f"{c['id']} + bias")
    # the bf16 twin
    A_bits = R.bf16_rn(A.astype(np.float32))
    fpw_bits = R.bf16_rn(p["fp_weight"].astype(np.float32))
    call = Call(lib, L, c, bf16=True)
    try:
        got = R.to_bits(call.run(R.from_bits(A_bits, "cuda:0"), f"{c['id']} bf16").view(torch.bfloat16).reshape(M, N))
        kern16 = lib.mixq_debug_last_gemm_kernel()
    finally:
        call.close()
    if M > 4:
        assert kern16 == kern + b" [bf16]", (kern, kern16)
        ref, P = R.prefill_reference64(A_bits, p["weight"], p["weights_scaling_factor"], fpw_bits, L.ind.astype(np.int64))
        err, lim = R.prefill_bound(got, ref, P)
    else:
        ref, mag = R.decode64(A_bits, unprocessed_qweight(lib, L), p["weights_scaling_factor"])
        err = np.abs(R.bf2f(got).astype(np.float64) - ref)
        lim = R.ulp_bf16(ref) + K * 2.0 ** -23 * mag     # one bf16 rounding + an fp32 accumulation bound (tests/test_gpu_bf16_operator.py)
    assert (err <= lim).all(), (c["id"], float((err / lim).max()))


def test_every_family_was_pinned():
    """The pinned cells reach the seven int8 GEMM families and the M <= 4 launch (so the per-family tests above cover each)."""
    assert FAMILIES == sorted(["skinny", "two-barrier", "deep", "mid", "pp128", "pp256", "pp256-split", "w8a16"]), FAMILIES
