"""CPU: the return code of every argument-checking entry of the C ABI, over a grid of refused (or empty) calls, against a recorded table.

The entries of csrc/mixq_api.hip check their arguments by class -- BADARG, SHAPE, ALIGN, with entry-specific extras -- and the order of
the classes is part of the ABI.  tests/golden/abi_refusals.json holds one digit (the return code) per call of the grid below, recorded
with tools/record_abi_refusals.py from a build whose codes are the accepted ones; this module replays the grid against the tree's library.

Only calls that are answered before anything reaches the device are in the grid: a call stays only if `bad` (a sufficient condition
for a refusal, stated per family below) holds or a count is zero, and the recorder aborts on MIXQ_E_HIP and on MIXQ_OK with every
count positive.  Dummy 16-byte aligned integers stand in for pointers, so on a machine WITH a device a wrongly accepted call would launch
on them: the module skips itself there.  The table is a check for the CPU run."""
import ctypes
import itertools
import json
import os

import pytest

from conftest import ROOT

from mixq_tensorrt_llm_amd import _lib

FIXTURE = os.path.join(ROOT, "tests", "golden", "abi_refusals.json")
OK, E_HIP = 0, 4
HALF, BF16 = _lib.MIXQ_TYPE_HALF, _lib.MIXQ_TYPE_BF16
ROW, FRAG = 0, 1
EPS = 1e-5

_NAMES = ("x r h g out ind outl q sc A qA sA fpA W sW fpW bias mul Out scratch mask cnt qw sc_col wcache x_scale C ws "
          "in0 in1 in2 in3 in4 in5 in6 out0").split()
ADDR = {n: 0x100000 + 0x1000 * i for i, n in enumerate(_NAMES)}          # distinct 16-byte aligned "pointers"

SIZES_M = [-1, 0, 4, 16, 64, 65]
SIZES_K = [0, 12, 64, 1024, 2048, 4096, 32776]
LAYOUTS = [-1, 0, 1, 2]
COUNTS = [-1, 0, 8, 136]
TYPES = [0, HALF, 2, BF16, 8, -1]


def ptr(name):
    return [0, ADDR[name] + 2, ADDR[name] + 4, ADDR[name] + 8]


def frag_ok(M, K):
    return 0 < M <= 64 and K % 8 == 0 and 1024 < K <= 16384


def null(kw, *names):
    return any(kw[n] == 0 for n in names)


def off(kw, a, *names):
    return any(kw[n] % a for n in names if n in kw)


class Entry:
    """One exported entry: `args` names its parameters in order (a float is passed as it stands, None is the null stream), `bases` are
    valid calls, `axes` the values each parameter takes in turn and in pairs, `bad` the refusals this grid relies on, `counts` the sizes
    whose zero makes the call empty."""

    def __init__(self, name, args, bases, axes, bad, counts=("M",), empties=True):
        self.name, self.args, self.bases, self.axes, self.bad, self.counts, self.empties = name, args, bases, axes, bad, counts, empties

    def empty(self, kw):
        return any(kw[c] == 0 for c in self.counts)

    def grid(self):
        out = []
        for base in self.bases:
            axes = {a: v for a, v in self.axes.items() if a in base}
            cands = [dict(base)] + [dict(base, **{a: v}) for a in axes for v in axes[a]]
            for a, b in itertools.combinations(axes, 2):
                cands += [dict(base, **{a: va, b: vb}) for va in axes[a] for vb in axes[b]]
            out += [kw for kw in cands if (self.bad(kw) or self.empty(kw)) and (self.empties or not self.empty(kw))]
        return out

    def call(self, lib, kw):
        return getattr(lib, self.name)(*[kw[a] if isinstance(a, str) else a for a in self.args])


# ------------------------------------------------------------------------------------------ norm producer ---
def norm_entry(name, args, quant, add, layout=False, typed=False):
    base = dict(M=4, K=4096, x=ADDR["x"], g=ADDR["g"], out=ADDR["out"])
    axes = dict(M=SIZES_M, K=SIZES_K, x=ptr("x"), g=ptr("g"), out=ptr("out"))
    if quant:
        base.update(ind=ADDR["ind"], len=8, outl=ADDR["outl"], q=ADDR["q"], sc=ADDR["sc"])
        axes.update(ind=ptr("ind"), len=COUNTS, outl=ptr("outl"), q=ptr("q"), sc=ptr("sc"))
    bases = [base]
    if add:
        axes.update(r=ptr("r"), h=ptr("h") + [ADDR["out"], ADDR["x"]])
        with_add = dict(base, r=ADDR["r"], h=ADDR["h"])
        bases = [with_add, dict(base, r=0, h=0)] if typed else [with_add]
    if layout:
        axes.update(layout=LAYOUTS)
        bases = [dict(b, layout=lay, M=16) for b in bases for lay in (ROW, FRAG)]
    if typed:
        axes.update(type=TYPES)
        bases = [dict(b, type=t) for b in bases for t in (HALF, BF16)]

    def bad(kw):
        M, K, lay = kw["M"], kw["K"], kw.get("layout", ROW)
        need = ["x", "g", "out"] + (["q", "sc"] if quant else []) + (["r", "h"] if add and not typed else [])
        return (M < 0 or K <= 0 or K % 8 != 0 or K > 32768 or lay not in (ROW, FRAG) or kw.get("type", HALF) not in (HALF, BF16)
                or (M > 0 and null(kw, *need)) or (add and (kw["r"] == 0) != (kw["h"] == 0)) or (add and kw["h"] == kw["out"] != 0)
                or (quant and (kw["len"] < 0 or (kw["len"] > 0 and null(kw, "ind", "outl"))))
                or (lay == FRAG and M > 0 and not frag_ok(M, K)) or off(kw, 16, "x", "r", "h", "g", "out")
                or (quant and kw["q"] % (4 if quant == 4 else 16 if lay == FRAG else 8) != 0))

    return Entry(name, args, bases, axes, bad)


_N = ["M", "K", "x", "g", "out", EPS]
_NA = ["M", "K", "x", "r", "h", "g", "out", EPS]
_Q = ["ind", "len", "outl", "q", "sc"]
NORM = [
    norm_entry("mixq_rmsnorm", _N + [None], 0, False),
    norm_entry("mixq_rmsnorm_extract_quant", _N + _Q + [None], 8, False),
    norm_entry("mixq_rmsnorm_extract_quant4", _N + _Q + [None], 4, False),
    norm_entry("mixq_rmsnorm_extract_quant_layout", _N + _Q + ["layout", None], 8, False, layout=True),
    norm_entry("mixq_add_rmsnorm", _NA + [None], 0, True),
    norm_entry("mixq_add_rmsnorm_extract_quant_layout", _NA + _Q + ["layout", None], 8, True, layout=True),
    norm_entry("mixq_add_rmsnorm_extract_quant4", _NA + _Q + [None], 4, True),
    norm_entry("mixq_rmsnorm_typed", _NA + ["type", None], 0, True, typed=True),
    norm_entry("mixq_rmsnorm_extract_quant_typed", _NA + _Q + ["layout", "type", None], 8, True, layout=True, typed=True),
]


# ------------------------------------------------------------------------------------------ row quantiser ---
def quant_entry(name, args, outliers=True, layout=False, typed=False):
    base = dict(M=4, K=4096, A=ADDR["A"], qA=ADDR["qA"], sA=ADDR["sA"])
    axes = dict(M=SIZES_M, K=SIZES_K, A=ptr("A"), qA=ptr("qA"), sA=ptr("sA"))
    if outliers:
        base.update(fpA=ADDR["fpA"], ind=ADDR["ind"], len=8, zero=1)
        axes.update(fpA=ptr("fpA"), ind=ptr("ind"), len=COUNTS, zero=[0])
    bases = [base]
    if layout:
        axes.update(layout=LAYOUTS)
        bases = [dict(b, layout=lay, M=16) for b in bases for lay in (ROW, FRAG)]
    if typed:
        axes.update(type=TYPES)
        bases = [dict(b, type=t) for b in bases for t in (HALF, BF16)]

    def bad(kw):
        M, K, lay = kw["M"], kw["K"], kw.get("layout", ROW)
        return (M < 0 or K <= 0 or K % 8 != 0 or lay not in (ROW, FRAG) or kw.get("type", HALF) not in (HALF, BF16)
                or (M > 0 and null(kw, "A", "qA", "sA")) or (outliers and (kw["len"] < 0 or (kw["len"] > 0 and null(kw, "fpA", "ind"))))
                or (lay == FRAG and not frag_ok(M, K)) or kw["A"] % 16 != 0 or kw["qA"] % (16 if lay == FRAG else 8) != 0)

    return Entry(name, args, bases, axes, bad)


_QE = ["M", "K", "A", "qA", "sA", "fpA", "ind", "len", "zero"]
QUANT = [
    quant_entry("mixq_int8quant", ["M", "K", "A", "qA", "sA", None], outliers=False),
    quant_entry("mixq_quant_extract", _QE + [None]),
    quant_entry("mixq_quant_extract_layout", _QE + ["layout", None], layout=True),
    quant_entry("mixq_quant_extract_typed", _QE + ["layout", "type", None], layout=True, typed=True),
]


# -------------------------------------------------------------------- outlier finder, column dequantiser ---
def finder_entry(name, typed):
    # (empty calls are left out: the empty path clears the mask through the dummy pointer)
    base = dict(A=ADDR["A"], M=4, K=4096, mask=ADDR["mask"], ind=ADDR["ind"], cnt=ADDR["cnt"], cap=8)
    axes = dict(A=ptr("A"), M=[-1, 0, 65], K=SIZES_K, mask=[0], ind=[0], cnt=[0], cap=COUNTS)
    bases = [dict(base, type=t) for t in (HALF, BF16)] if typed else [base]
    if typed:
        axes.update(type=TYPES)

    def bad(kw):
        return (kw["M"] < 0 or kw["K"] <= 0 or kw["cap"] < 0 or null(kw, "mask", "cnt") or (kw["cap"] > 0 and kw["ind"] == 0)
                or (kw["M"] > 0 and kw["A"] == 0) or kw["K"] % 8 != 0 or (kw["M"] > 0 and kw["A"] % 16 != 0)
                or kw.get("type", HALF) not in (HALF, BF16))

    return Entry(name, ["A", "M", "K", 3.0, "mask", "ind", "cnt", "cap"] + (["type"] if typed else []) + [None], bases, axes, bad, empties=False)


def columns_entry(name, typed):
    base = dict(qw=ADDR["qw"], sc_col=ADDR["sc_col"], ind=ADDR["ind"], len=8, out=ADDR["out"], N=32, K=4096)
    axes = dict(qw=ptr("qw"), sc_col=ptr("sc_col"), ind=ptr("ind"), len=COUNTS, out=ptr("out"), N=[-1, 0, 40], K=SIZES_K)
    bases = [dict(base, type=t) for t in (HALF, BF16)] if typed else [base]
    if typed:
        axes.update(type=TYPES)

    def bad(kw):
        return (kw["N"] < 0 or kw["K"] <= 0 or kw["len"] < 0 or (kw["N"] > 0 and kw["len"] > 0 and null(kw, "qw", "sc_col", "ind", "out"))
                or kw.get("type", HALF) not in (HALF, BF16))

    return Entry(name, ["qw", "sc_col", "ind", "len", "out", "N", "K"] + (["type"] if typed else []) + [None], bases, axes, bad, counts=("N", "len"))


OUTLIER = [finder_entry("mixq_find_outliers", False), finder_entry("mixq_find_outliers_typed", True),
           columns_entry("mixq_dequant_weight_columns", False), columns_entry("mixq_dequant_weight_columns_typed", True)]

# --------------------------------------------------------------------------------------------- mixed GEMM ---
SILU, SILU_MUL = 1, 3
_G = ["qA", "W", "sA", "sW", "fpA", "fpW"]
_MNKO = ["M", "N", "K", "O"]
_S = ["scratch", "bytes", None]


def mixed_entry(name, args, bias=None, layout=False, typed=False, act=False):
    """bias: None (the entry takes none) | "required" | "optional"."""
    base = dict(qA=ADDR["qA"], W=ADDR["W"], sA=ADDR["sA"], sW=ADDR["sW"], fpA=ADDR["fpA"], fpW=ADDR["fpW"], Out=ADDR["Out"], M=16, N=32, K=64,
                O=8, scratch=0, bytes=0)
    axes = dict(qA=ptr("qA"), W=ptr("W"), sA=ptr("sA"), sW=ptr("sW"), fpA=ptr("fpA"), fpW=ptr("fpW"), Out=ptr("Out"), M=[-1, 0, 5, 65],
                N=[-1, 0, 24, 4096], K=SIZES_K, O=COUNTS + [4], scratch=[ADDR["scratch"]], bytes=[1 << 30])
    bases = [base]
    if bias:
        axes.update(bias=ptr("bias"))
        bases = [dict(base, bias=ADDR["bias"])] + ([dict(base, bias=0)] if bias == "optional" else [])
    if act:
        axes.update(epi=[-1, 0, SILU, 2, SILU_MUL, 4], mul=ptr("mul") + [ADDR["Out"]])
        bases = [dict(b, epi=e, mul=ADDR["mul"] if e == SILU_MUL else 0) for b in bases for e in (0, SILU, SILU_MUL)]
    if layout:
        axes.update(layout=LAYOUTS)
        bases = [dict(b, layout=lay) for b in bases for lay in (ROW, FRAG)]
    if typed:
        axes.update(type=TYPES)
        bases = [dict(b, type=t) for b in bases for t in (HALF, BF16)]

    def bad(kw):
        M, N, K, O, lay, typ = kw["M"], kw["N"], kw["K"], kw["O"], kw.get("layout", ROW), kw.get("type", HALF)
        one_pass = bool(kw.get("bias")) or typ == BF16 or kw.get("epi", 0) != 0 or lay == FRAG   # (no room for the two-step order)
        return (M < 0 or N < 0 or K <= 0 or O < 0 or lay not in (ROW, FRAG) or typ not in (HALF, BF16)
                or (M > 0 and N > 0 and (null(kw, "qA", "W", "sA", "sW", "Out") or (O > 0 and null(kw, "fpA", "fpW"))))
                or K % 16 != 0 or N % 16 != 0 or O % 8 != 0 or off(kw, 16, "qA", "W", "Out", "sW") or (O > 0 and off(kw, 16, "fpA", "fpW"))
                or (bias == "required" and kw["bias"] == 0) or off(kw, 16, "bias", "mul") or (O > 128 and one_pass)
                or (act and (kw["epi"] not in (0, SILU, SILU_MUL) or (kw["epi"] == SILU_MUL) != (kw["mul"] != 0) or kw["mul"] == kw["Out"] != 0)))

    return Entry(name, args, bases, axes, bad, counts=("M", "N"))


MIXED = [
    mixed_entry("mixq_gemm_mixed", _G + ["Out"] + _MNKO + [None]),
    mixed_entry("mixq_gemm_mixed_scratch", _G + ["Out"] + _MNKO + _S),
    mixed_entry("mixq_gemm_mixed_bias", _G + ["bias", "Out"] + _MNKO + _S, bias="required"),
    mixed_entry("mixq_gemm_mixed_layout", _G + ["Out"] + _MNKO + ["layout"] + _S, layout=True),
    mixed_entry("mixq_gemm_mixed_typed", _G + ["bias", "Out"] + _MNKO + ["layout", "type"] + _S, bias="optional", layout=True, typed=True),
    mixed_entry("mixq_gemm_mixed_act_typed", _G + ["mul", "Out"] + _MNKO + ["epi", "layout", "type"] + _S, layout=True, typed=True, act=True),
]


# ------------------------------------------------------------------- the other users of the GemmParams ---
def plain_gemm_entry(name, args, scales=True, fused=False):
    base = dict(A=ADDR["A"], W=ADDR["W"], Out=ADDR["Out"], M=16, N=32, K=64)
    axes = dict(A=ptr("A"), W=ptr("W"), Out=ptr("Out"), M=[-1, 0, 65], N=[-1, 0, 24], K=SIZES_K)
    if scales:
        base.update(sA=ADDR["sA"], sW=ADDR["sW"], y=0, ws=0)
        axes.update(sA=ptr("sA"), sW=ptr("sW"), y=ptr("fpA"), ws=ptr("ws"))
    bases = [base]
    if fused:
        axes.update(epi=[-1, 0, SILU, 2, SILU_MUL, 4], mul=ptr("mul"), layout=LAYOUTS)
        bases = [dict(base, epi=e, mul=ADDR["mul"] if e == SILU_MUL else 0, layout=ROW) for e in (0, SILU, SILU_MUL)]

    def bad(kw):
        M, N, K = kw["M"], kw["N"], kw["K"]
        return (M < 0 or N < 0 or K <= 0 or (M > 0 and N > 0 and (null(kw, "A", "W", "Out") or (scales and null(kw, "sA", "sW"))))
                or K % 16 != 0 or N % 16 != 0 or off(kw, 16, "A", "W", "Out", "y") or (scales and kw["sW"] % 16 != 0)
                or (fused and (kw["epi"] not in (0, SILU, SILU_MUL) or kw["layout"] not in (ROW, FRAG)
                               or (kw["epi"] == SILU_MUL and (kw["mul"] == 0 or kw["mul"] % 16 != 0)))))

    return Entry(name, args, bases, axes, bad, counts=("M", "N"))


PLAIN = [
    plain_gemm_entry("mixq_gemm_s8s8s32", ["A", "W", "Out", "M", "N", "K", None], scales=False),
    plain_gemm_entry("mixq_int8_fused_dequantize", ["A", "W", "sA", "sW", "y", "Out", "M", "N", "K", "ws", None]),
    plain_gemm_entry("mixq_int8_fused_dequantize_layout", ["A", "W", "sA", "sW", "y", "mul", "Out", "M", "N", "K", "epi", "layout", "ws", None],
                     fused=True),
]


# ------------------------------------------------------------------------------------------- MixLinear ---
def mixlinear_entry(name, typed):
    """The fp16 form launches its quantiser before the GEMM's checks run, so only what it refuses before that launch is in its grid;
    the bf16 form refuses everything first."""
    args = ["M", "N", "K", "O", "x", "ind", "qw", "sc_col", "wcache", "x_scale", "qA", "outl", "out", "layout"] + (["type"] if typed else []) + _S
    base = dict(M=16, N=32, K=4096, O=8, x=ADDR["x"], ind=ADDR["ind"], qw=ADDR["qw"], sc_col=ADDR["sc_col"], wcache=ADDR["wcache"],
                x_scale=ADDR["x_scale"], qA=ADDR["qA"], outl=ADDR["outl"], out=ADDR["out"], layout=ROW, scratch=0, bytes=0)
    axes = dict(M=[-1, 0, 4, 65], N=[-1, 0, 24], K=SIZES_K, O=COUNTS + [4], layout=LAYOUTS,
                **{p: ptr(p) for p in ("x", "ind", "qw", "sc_col", "wcache", "x_scale", "qA", "outl", "out")})
    bases = [dict(base, layout=lay) for lay in (ROW, FRAG)]
    if typed:
        axes.update(type=TYPES)
        bases = [dict(b, type=t) for b in bases for t in (HALF, BF16)]

    def bad(kw):
        M, N, K, O, lay, typ = kw["M"], kw["N"], kw["K"], kw["O"], kw["layout"], kw.get("type", HALF)
        first = (typ not in (HALF, BF16) or M < 0 or N < 0 or K <= 0 or O < 0 or lay not in (ROW, FRAG) or K % 8 != 0
                 or (M > 0 and N > 0 and (null(kw, "x", "qw", "sc_col", "x_scale", "qA", "out") or (O > 0 and null(kw, "ind", "wcache", "outl"))))
                 or (lay == FRAG and (O % 8 != 0 or O > 128 or M <= 4 or not frag_ok(M, K))) or kw["x"] % 16 != 0
                 or kw["qA"] % (16 if lay == FRAG else 8) != 0)
        if typ != BF16:
            return first
        return (first or O % 8 != 0 or O > 128 or K % 16 != 0 or N % 16 != 0 or off(kw, 16, "qA", "qw", "out", "sc_col")
                or (O > 0 and off(kw, 16, "outl", "wcache")))

    return Entry(name, args, bases, axes, bad, counts=("M", "N"))


MIXLINEAR = [mixlinear_entry("mixq_mixlinear_forward", False), mixlinear_entry("mixq_mixlinear_forward_typed", True)]


# --------------------------------------------------------------------------------------------- enqueue ---
class EnqueueEntry(Entry):
    """mixq_enqueue, _bias and _profiled: descriptor types and dims, a null input, a null workspace above four rows, K % 8, a misaligned A
    or bias.  Above four rows without a bias the GEMM's own checks run behind the quantiser's launch: they are not in the grid."""
    INPUTS = ["in0", "in1", "in2", "in3", "in4", "in5", "in6"]

    def __init__(self, name):
        self.name, self.counts, self.empties = name, ("M",), True
        self.has_bias = name == "mixq_enqueue_bias"
        base = dict(h=1, a_dims=(2, 8, 128), N=32, a_type=HALF, w_type=HALF, out_type=HALF, out0=ADDR["out0"], ws=ADDR["ws"],
                    **{i: ADDR[i] for i in self.INPUTS})
        self.axes = dict(h=[0], a_dims=[(-1, 128), (0, 128), (16, 0), (16, 12), (16, 136), (2, 136), (2, 72), (1 << 31, 128), (1 << 16, 1 << 16, 128),
                                        (), tuple([1] * 8 + [128])],
                         N=[0, -1, 24, 31, 1 << 31], a_type=[BF16, 0], w_type=[BF16, 0], out_type=[BF16, None], out0=[0, ADDR["out0"] + 2],
                         ws=[0], in0=ptr("in0"), in1=ptr("in1"), in2=ptr("in2"), in3=ptr("in3"), in4=[0], in5=ptr("in5"), in6=[0])
        if self.has_bias:
            base["bias"] = ADDR["bias"]
            self.axes["bias"] = ptr("bias")
        bases = [base, dict(base, a_dims=(2, 128))]
        self.bases = bases + [dict(b, a_type=BF16, w_type=BF16, out_type=BF16) for b in bases]

    @staticmethod
    def mnk(kw):
        d = kw["a_dims"]
        M = 1
        for v in d[:-1]:
            M *= v
        return M, kw["N"], (d[-1] if d else 0)

    def empty(self, kw):
        return 0 < len(kw["a_dims"]) <= 8 and self.mnk(kw)[0] == 0

    def bad(self, kw):
        (M, N, K), d, bias = self.mnk(kw), kw["a_dims"], kw.get("bias", 0)
        big = 1 << 31
        if (bias % 16 != 0 or kw["h"] == 0 or (kw["a_type"] == BF16 and (kw["w_type"] != BF16 or kw["out_type"] not in (BF16, None)))
                or not 0 < len(d) <= 8 or M < 0 or K <= 0 or N <= 0 or M >= big or K >= big or N >= big):
            return True
        if M == 0:
            return False
        if null(kw, "out0", *self.INPUTS):
            return True
        if M > 4:
            return (kw["ws"] == 0 or K % 8 != 0 or kw["in0"] % 16 != 0
                    or (bias != 0 and (K % 16 != 0 or N % 16 != 0 or off(kw, 16, "in1", "out0", "in2", "in3"))))
        return K % 64 != 0 or N % 2 != 0 or off(kw, 16, "in0", "in5")

    def call(self, lib, kw):
        d = kw["a_dims"]
        descs = (_lib.TensorDesc * 8)()
        descs[0] = _lib.TensorDesc.make(d[:8], kw["a_type"])
        descs[0].nbDims = len(d)
        descs[1] = _lib.TensorDesc.make((kw["N"], d[-1] if d else 0), _lib.MIXQ_TYPE_HALF)
        descs[3] = _lib.TensorDesc.make((kw["N"], 128), kw["w_type"])
        out_desc = None if kw["out_type"] is None else (_lib.TensorDesc * 1)(_lib.TensorDesc.make(d[:8], kw["out_type"]))
        inputs = (ctypes.c_void_p * 7)(*[kw[i] for i in self.INPUTS])
        outputs = (ctypes.c_void_p * 1)(kw["out0"])
        handle = self.handle(lib) if kw["h"] else None
        fn = getattr(lib, self.name)
        if self.has_bias:
            return fn(handle, descs, out_desc, inputs, outputs, kw["bias"], kw["ws"], None)
        if self.name == "mixq_enqueue_profiled":
            return fn(handle, descs, out_desc, inputs, outputs, kw["ws"], None, None, None)
        return fn(handle, descs, out_desc, inputs, outputs, kw["ws"], None)

    _handles = {}

    @classmethod
    def handle(cls, lib):
        if id(lib) not in cls._handles:
            cls._handles[id(lib)] = lib.mixq_create(0, 0, 0)
        return cls._handles[id(lib)]


ENQUEUE = [EnqueueEntry("mixq_enqueue"), EnqueueEntry("mixq_enqueue_bias"), EnqueueEntry("mixq_enqueue_profiled")]

ENTRIES = NORM + QUANT + OUTLIER + MIXED + PLAIN + MIXLINEAR + ENQUEUE


def codes(lib, entry, recording=False):
    """The grid's return codes as one digit per call.  recording: abort on a call that was not answered before the device."""
    out = []
    for kw in entry.grid():
        rc = entry.call(lib, kw)
        if recording and (rc == E_HIP or (rc == OK and not entry.empty(kw))):
            raise SystemExit(f"{entry.name}{kw}: answered {rc}: not a refusal before the device, and no empty call")
        assert 0 <= rc <= 9, (entry.name, kw, rc)
        out.append(str(rc))
    return "".join(out)


def _has_device():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


pytestmark = pytest.mark.skipif(_has_device(), reason="dummy pointers: a wrongly accepted call would launch on them")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def table():
    with open(FIXTURE) as f:
        return json.load(f)["entries"]


def test_the_table_covers_every_entry_of_the_grid(table):
    assert sorted(table) == sorted(e.name for e in ENTRIES)
    assert sum(len(v) for v in table.values()) > 40000


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e.name)
def test_return_codes_are_the_recorded_ones(lib, table, entry):
    want, grid = table[entry.name], entry.grid()
    assert len(want) == len(grid), "the grid changed: record the table again (tools/record_abi_refusals.py)"
    got = codes(lib, entry)
    wrong = [(kw, int(w), int(g)) for kw, w, g in zip(grid, want, got) if w != g]
    assert not wrong, f"{len(wrong)} of {len(grid)} calls changed their code; (call, recorded, now): {wrong[:5]}"


def test_the_one_kept_difference_between_siblings(lib):
    """An empty fragment-major call: the fp16 entry without the add refuses it (MIXQ_E_SHAPE), its add form and the bf16 form accept it.
    Kept as it is: a caller may depend on either."""
    by_name = {e.name: e for e in ENTRIES}
    kw = dict(M=0, K=4096, x=ADDR["x"], r=0, h=0, g=ADDR["g"], out=ADDR["out"], ind=ADDR["ind"], len=8, outl=ADDR["outl"], q=ADDR["q"],
              sc=ADDR["sc"], layout=FRAG, type=HALF)
    assert by_name["mixq_rmsnorm_extract_quant_layout"].call(lib, kw) == 2
    assert by_name["mixq_rmsnorm_extract_quant_typed"].call(lib, kw) == 2                      # (fp16 without the add: the same entry)
    assert by_name["mixq_rmsnorm_extract_quant_typed"].call(lib, dict(kw, type=BF16)) == OK
    assert by_name["mixq_add_rmsnorm_extract_quant_layout"].call(lib, dict(kw, r=ADDR["r"], h=ADDR["h"])) == OK
