#!/usr/bin/env python3
"""The weight-only (W8A16) GEMM on bf16 rows next to the fp16 call of the same shape, ON THE SAME LIBRARY BUILD, in one process:

  (a) fp16   mixq_w8a16_gemm_forward_typed(MIXQ_TYPE_HALF)  = mixq_w8a16_gemm_forward_ws: the yardstick, its kernels are unchanged
  (b) bf16   mixq_w8a16_gemm_forward_typed(MIXQ_TYPE_BF16)  the same interleaved weight and fp16 scales

12288 x 4096 and 4096 x 11008 weights at 8 / 32 / 128 / 512 / 2048 tokens, each call with the scratch its own size query asks for.
A bf16 call takes the form of the fp16 call -- the table prints both names -- except at 2048 tokens, where fp16 dequantises the
weight once and runs the fp16 ping-pong GEMM (two-pass form) and bf16, which has no such form yet, runs the wide fused form: that
row is the case for a bf16 two-pass form.  Each leg is a batch of calls captured once into a HIP graph and replayed; the legs are
interleaved round by round after a warm-up.  The table gives the median of the rounds and the spread of the fp16 leg's own rounds
((max - min) / median) -- the yardstick for the ratio next to it.  No ratio is asserted: this is a probe, not a gate.
usage: python tools/bf16_w8a16_probe.py [--rounds 9] [--out profiles/bf16_w8a16_probe.txt]"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mixq_tensorrt_llm_amd import _lib  # noqa: E402

SHAPES = ((12288, 4096), (4096, 11008))     # (N, K)
ROWS = (8, 32, 128, 512, 2048)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    legs = ("fp16", "bf16")
    types = dict(fp16=_lib.MIXQ_TYPE_HALF, bf16=_lib.MIXQ_TYPE_BF16)
    lines = [f"bf16_w8a16_probe: {lib.mixq_version().decode()} on {torch.cuda.get_device_name(0)}; us per call, HIP-graph replay, median of "
             f"{a.rounds} interleaved rounds; spread = (max - min) / median of the fp16 leg's own rounds",
             f"{'N x K':>13} {'rows':>6} {'fp16 (a)':>10} {'bf16 (b)':>10} {'b / a':>7} {'spread a':>9}  form of (a) | form of (b)"]
    for s in lines:
        print(s, flush=True)
    g = torch.Generator(device=dev).manual_seed(0)
    for N, K in SHAPES:
        Wq = torch.randint(0, 256, (K, N), device=dev, generator=g, dtype=torch.uint8)
        sc = (torch.rand(N, device=dev, generator=g) * 1e-3 + 1e-4).to(torch.float16)
        for M in ROWS:
            iters = 100 if M <= 128 else 20
            x32 = torch.randn((M, K), device=dev, generator=g)
            bufs, fns, names = {}, {}, {}
            for leg in legs:
                dt = torch.float16 if leg == "fp16" else torch.bfloat16
                n = int(lib.mixq_w8a16_gemm_workspace_size_typed(M, N, K, types[leg]))
                bufs[leg] = dict(x=x32.to(dt), out=torch.empty((M, N), dtype=dt, device=dev),
                                 ws=torch.zeros(n, dtype=torch.uint8, device=dev) if n else None, n=n)

                def run(st, b=bufs[leg], typ=types[leg]):
                    rc = lib.mixq_w8a16_gemm_forward_typed(p(b["x"]), p(Wq), p(sc), p(b["out"]), M, N, K, typ, p(b["ws"]), b["n"], st)
                    assert rc == 0, rc
                fns[leg] = run
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            for leg in legs:
                fns[leg](st)
                names[leg] = lib.mixq_debug_last_gemm_kernel().decode()
            torch.cuda.synchronize()
            graphs = {}
            side = torch.cuda.Stream()
            for leg in legs:
                gr = torch.cuda.CUDAGraph()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    with torch.cuda.graph(gr, stream=side):
                        cst = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                        for _ in range(iters):
                            fns[leg](cst)
                graphs[leg] = gr

            def timed(run):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / iters * 1e3

            for gr in graphs.values():      # warm-up of every leg
                gr.replay()
            torch.cuda.synchronize()
            t = {n: [] for n in legs}
            for _ in range(a.rounds):
                for leg in legs:
                    t[leg].append(timed(graphs[leg].replay))
            med = {n: statistics.median(v) for n, v in t.items()}
            spread = (max(t["fp16"]) - min(t["fp16"])) / med["fp16"]
            s = (f"{f'{N} x {K}':>13} {M:>6} {med['fp16']:>10.2f} {med['bf16']:>10.2f} {med['bf16'] / med['fp16']:>7.3f} {spread:>9.3f}  "
                 f"{names['fp16']} | {names['bf16']}")
            lines.append(s)
            print(s, flush=True)
            del graphs, bufs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
