#!/usr/bin/env python3
"""bf16 calls of mixq_enqueue against the fp16 call and the cast route (a report, not a gate).

Per BASELINE shape (Llama-2-7B qkv / o / gate-up / down, Qwen2-7B qkv) and row count, device-event time per call of
    fp16  = mixq_enqueue on fp16 A / fp_weight / output
    bf16  = mixq_enqueue on bf16 A / fp_weight / output (the bf16 call)
    cast  = bf16 A -> fp16, the fp16 call, fp16 Out -> bf16 (what a bf16 model had to do before)
alternating the three in one process, warm (one layer, cache-resident weights) and cold (the calls walk through enough copies of
the layer's weights that none of them is in the Infinity Cache when it is used again).

usage: python tools/bf16_enqueue_bench.py [--rows 1,4,32,...] [--iters 20] [--out profiles/bf16_enqueue_bench.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [("llama2-7b qkv", 12288, 4096), ("llama2-7b o", 4096, 4096), ("llama2-7b gate-up", 22016, 4096),
          ("llama2-7b down", 4096, 11008), ("qwen2-7b qkv", 4608, 3584)]
ROWS = [1, 4, 32, 256, 1024, 8192, 65536]
COLD_BYTES = 400 << 20   # more weight bytes than the Infinity Cache holds (256 MiB) between two uses of one copy


def layers_for(N, K, copies):
    from mixq_tensorrt_llm_amd import plugin
    rng = np.random.default_rng(N + K)
    out = []
    base = dict(
        weight=torch.from_numpy(rng.integers(-127, 128, (N, K), dtype=np.int8)).view(torch.float16).reshape(N, K // 2),
        sw=torch.from_numpy((np.abs(rng.standard_normal(N)) * 1e-3).astype(np.float16)),
        fpw=torch.from_numpy((rng.standard_normal((N, 128)) * 0.02).astype(np.float16)),
        ind=torch.from_numpy(np.sort(rng.choice(K, 128, replace=False)).astype(np.int32)).view(torch.float16),
        qweight=torch.from_numpy(rng.integers(0, 256, (K, N), dtype=np.uint8)).view(torch.float16).reshape(K, N // 2))
    for _ in range(copies):
        t = {k: v.cuda() for k, v in base.items()}
        t["fpw_bf"] = t["fpw"].to(torch.bfloat16)
        out.append(t)
    plug = plugin.MixQPlugin.create(1, N, K)
    return plug, out


def time_calls(fns, iters):
    """Alternate the callables, `iters` rounds; median device time per call of each (us)."""
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for _ in fns]
    for it in range(iters):
        for f, e in zip(fns, ev):
            e[it][0].record()
            f(it)
            e[it][1].record()
    torch.cuda.synchronize()
    return [float(np.median([a.elapsed_time(b) * 1e3 for a, b in e])) for e in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(map(str, ROWS)))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [int(r) for r in a.rows.split(",")]
    lines = ["# bf16 enqueue vs fp16 enqueue vs the cast route, median device time per call (us); ratios vs fp16",
             f"# {torch.cuda.get_device_name(0)}, {a.iters} alternating rounds per cell",
             f"{'shape':<18} {'rows':>6} {'mode':<5} {'fp16':>9} {'bf16':>9} {'cast':>9} {'bf16/fp16':>9} {'cast/bf16':>9}"]
    print("\n".join(lines), flush=True)
    for name, N, K in SHAPES:
        copies_cold = max(2, int(COLD_BYTES // (2 * N * K)) + 1)
        plug, ls = layers_for(N, K, copies_cold)
        for M in rows:
            x32 = torch.randn(M, K, device="cuda") * 2
            A16, Abf = x32.half(), x32.to(torch.bfloat16)
            o16 = torch.empty(M, N, dtype=torch.float16, device="cuda")
            obf = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
            ws = torch.empty(plug.workspace_size(M, N, K), dtype=torch.uint8, device="cuda")
            for mode in ("warm", "cold"):
                pick = (lambda it: ls[0]) if mode == "warm" else (lambda it: ls[it % len(ls)])

                def f16(it):
                    t = pick(it)
                    plug.enqueue([A16, t["weight"], t["sw"], t["fpw"], t["ind"], t["qweight"], t["sw"]], output=o16, workspace=ws)

                def fbf(it):
                    t = pick(it)
                    plug.enqueue([Abf, t["weight"], t["sw"], t["fpw_bf"], t["ind"], t["qweight"], t["sw"]], output=obf, workspace=ws)

                def fcast(it):
                    t = pick(it)
                    plug.enqueue([Abf.half(), t["weight"], t["sw"], t["fpw"], t["ind"], t["qweight"], t["sw"]], output=o16,
                                 workspace=ws)
                    obf.copy_(o16)

                for f in (f16, fbf, fcast):   # warm-up (first launches, workspace, lazily set kernel attributes)
                    f(0)
                iters = a.iters if M < 65536 else max(5, a.iters // 4)
                t16, tbf, tc = time_calls([f16, fbf, fcast], iters)
                line = f"{name:<18} {M:>6} {mode:<5} {t16:>9.1f} {tbf:>9.1f} {tc:>9.1f} {tbf / t16:>9.3f} {tc / tbf:>9.3f}"
                lines.append(line)
                print(line, flush=True)
            del x32, A16, Abf, o16, obf, ws
        del ls
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
