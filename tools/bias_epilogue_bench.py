#!/usr/bin/env python3
"""The layer bias in the operator's epilogue against the separate add it replaces (a report, not a gate).

Per row count of the Qwen2-7B qkv projection (4608 x 3584, biased): device-event time per call of
    sep   = mixq_enqueue + torch's fp16 ``x + bias``   (what MixQLinear did before: two launches, a second pass over the output)
    fused = mixq_enqueue_bias                          (one launch chain, the add in the GEMM's epilogue)
alternating the two in one process, warm (one layer, cache-resident weights) and cold (the call walks through enough copies of
the layer's weights that none of them is in the Infinity Cache when it is used again).

--plain-only --lib PATH: time mixq_enqueue alone on the library at PATH (for a same-box A/B of the bias-free path against the
parent commit's library; only mixq_enqueue / mixq_workspace_size / mixq_create are bound, so an older ABI loads too).

usage: python tools/bias_epilogue_bench.py [--rows 1,4,32,...] [--iters 50] [--json out.json]
       python tools/bias_epilogue_bench.py --plain-only --lib path/to/libmixq_mi355x.so"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mixq_tensorrt_llm_amd._lib import TensorDesc  # noqa: E402

N, K = 4608, 3584
ROWS = [1, 4, 32, 64, 128, 256, 512, 65536]
COLD_BYTES = 400 << 20   # more weight bytes than the Infinity Cache holds (256 MiB) between two uses of one copy


def bind(path):
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lib.mixq_create.restype, lib.mixq_create.argtypes = vp, [ctypes.c_int32] * 3
    lib.mixq_workspace_size.restype, lib.mixq_workspace_size.argtypes = ctypes.c_size_t, [vp, i64, i64, i64]
    lib.mixq_enqueue.restype = ctypes.c_int
    lib.mixq_enqueue.argtypes = [vp, ctypes.POINTER(TensorDesc), ctypes.POINTER(TensorDesc), ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp]
    if hasattr(lib, "mixq_enqueue_bias"):
        lib.mixq_enqueue_bias.restype = ctypes.c_int
        lib.mixq_enqueue_bias.argtypes = [vp, ctypes.POINTER(TensorDesc), ctypes.POINTER(TensorDesc), ctypes.POINTER(vp),
                                          ctypes.POINTER(vp), vp, vp, vp]
    return lib


def layers(copies, dev):
    """`copies` independent sets of the layer's 7 operands (random int8 weight, scales, outliers, interleaved qweight)."""
    g = torch.Generator(device=dev).manual_seed(0)
    out = []
    for _ in range(copies):
        W = torch.randint(-127, 128, (N, K), dtype=torch.int8, device=dev, generator=g)
        sW = (torch.rand(N, device=dev, generator=g) * 4e-4 + 1e-4).half()
        fpW = (torch.randn((N, 128), device=dev, generator=g) * 0.02).half()
        ind = torch.randperm(K, device=dev, generator=g)[:128].to(torch.int32)
        qw = torch.randint(0, 256, (K, N), dtype=torch.uint8, device=dev, generator=g)
        ind_c = torch.zeros(256, dtype=torch.float16, device=dev)
        ind_c.view(torch.int32)[:128] = ind
        out.append([W.view(torch.float16), sW, fpW, ind_c, qw.view(torch.float16), sW])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(map(str, ROWS)))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--lib", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "mixq_tensorrt_llm_amd", "libmixq_mi355x.so"))
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = bind(a.lib)
    h = lib.mixq_create(0, 0, 0)
    cold_copies = max(2, COLD_BYTES // (2 * N * K) + 1)
    sets = layers(cold_copies, dev)
    bias = (torch.randn(N, device=dev) * 0.5).half()
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    results = []
    for M in [int(r) for r in a.rows.split(",")]:
        A = torch.randn((M, K), device=dev).half()
        out = torch.empty((M, N), dtype=torch.float16, device=dev)
        ws = torch.empty(max(int(lib.mixq_workspace_size(h, M, N, K)), 16), dtype=torch.uint8, device=dev)
        descs = (TensorDesc * 7)(*[TensorDesc.make(t.shape) for t in [A] + sets[0]])
        out_desc = TensorDesc.make(out.shape)
        outs = (ctypes.c_void_p * 1)(out.data_ptr())
        ptrs = [(ctypes.c_void_p * 7)(*[t.data_ptr() for t in [A] + s]) for s in sets]
        iters = a.iters if M < 65536 else max(6, a.iters // 8)

        def sep(i):
            rc = lib.mixq_enqueue(h, descs, ctypes.byref(out_desc), ptrs[i], outs, ctypes.c_void_p(ws.data_ptr()), st)
            assert rc == 0, rc
            if not a.plain_only:
                out.add_(bias)   # (in place: the same read + write of the output as `x + bias` without the allocation)

        def fused(i):
            rc = lib.mixq_enqueue_bias(h, descs, ctypes.byref(out_desc), ptrs[i], outs, ctypes.c_void_p(bias.data_ptr()),
                                       ctypes.c_void_p(ws.data_ptr()), st)
            assert rc == 0, rc

        forms = [("plain" if a.plain_only else "sep", sep)] + ([] if a.plain_only else [("fused", fused)])
        row = {"M": M}
        for mode in ("warm", "cold"):
            times = {name: [] for name, _ in forms}
            for it in range(iters + 3):
                for name, fn in forms:   # alternating in one process
                    idx = 0 if mode == "warm" else (it * len(forms) + [n for n, _ in forms].index(name)) % cold_copies
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn(idx)
                    e1.record()
                    e1.synchronize()
                    if it >= 3:
                        times[name].append(e0.elapsed_time(e1) * 1000.0)
            for name in times:
                v = sorted(times[name])
                row[f"{name}_{mode}_us"] = round(v[len(v) // 2], 2)
        if not a.plain_only:
            for mode in ("warm", "cold"):
                row[f"delta_{mode}_pct"] = round(100.0 * (row[f"fused_{mode}_us"] / row[f"sep_{mode}_us"] - 1.0), 1)
        print(json.dumps(row), flush=True)
        results.append(row)
        del A, out, ws
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"shape": [N, K], "lib": os.path.basename(os.path.dirname(os.path.dirname(os.path.abspath(a.lib)))),
                       "rows": results}, f, indent=1)


if __name__ == "__main__":
    main()
