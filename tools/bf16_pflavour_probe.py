#!/usr/bin/env python3
"""The bf16 P-flavour forward (mixq_mixlinear_forward_typed, MIXQ_TYPE_BF16) and its zeroing quantiser alone
(mixq_quant_extract_typed, zero_outliers = 1) next to their fp16 twins (mixq_mixlinear_forward, mixq_quant_extract_layout), ON THE
SAME LIBRARY BUILD, in one process:

  (a) fp16   mixq_mixlinear_forward                                   two launches
  (b) bf16   mixq_mixlinear_forward_typed(MIXQ_TYPE_BF16)             two launches; moves the same bytes as (a)
  (c) fp16   mixq_quant_extract_layout(zero_outliers = 1)             the producer of (a) alone
  (d) bf16   mixq_quant_extract_typed(zero_outliers = 1, BF16)        the producer of (b) alone

4096 x 4096 weights, 128 outlier columns, row-major int8 rows unless mixq_qa_layout asks for the fragment-major image.  Each leg is
a batch of calls captured once into a HIP graph and replayed (the device-side chain without the host); the legs are interleaved
round by round after a warm-up.  The table gives the median of the rounds and, for the fp16 legs, the spread of their own rounds
((max - min) / median) -- the yardstick for the bf16 / fp16 ratios next to it.  No ratio is asserted: this is a probe, not a gate.
usage: python tools/bf16_pflavour_probe.py [--rounds 9] [--out profiles/bf16_pflavour_probe.txt]"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mixq_tensorrt_llm_amd import _lib  # noqa: E402

ROWS, N, K, O = (32, 256, 4096), 4096, 4096, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    legs = ("fp16 forward", "bf16 forward", "fp16 quantiser", "bf16 quantiser")
    lines = [f"bf16_pflavour_probe: {lib.mixq_version().decode()} on {torch.cuda.get_device_name(0)}; us per call, HIP-graph replay, median of "
             f"{a.rounds} interleaved rounds; {N} x {K} weights, {O} outlier columns; spread = (max - min) / median of the fp16 leg's own rounds",
             f"{'rows':>6} " + " ".join(f"{n:>15}" for n in legs) + f" {'b / a':>7} {'spread a':>9} {'d / c':>7} {'spread c':>9}  producer of (b) | GEMM of (b)"]
    for s in lines:
        print(s, flush=True)
    g = torch.Generator(device=dev).manual_seed(0)
    W = torch.randint(-127, 128, (N, K), device=dev, generator=g, dtype=torch.int8)
    sW = (torch.rand(N, device=dev, generator=g) * 0.01 + 0.001).to(torch.float16)
    wc32 = torch.randn((N, O), device=dev, generator=g) * 0.05
    ind = torch.randperm(K, device=dev, generator=g)[:O].to(torch.int32)
    for M in ROWS:
        iters = 200 if M <= 256 else 20
        lay = int(lib.mixq_qa_layout(M, N, K))
        need = int(lib.mixq_gemm_scratch_size(M, N, K))
        scr = torch.zeros(max(need, 16), dtype=torch.uint8, device=dev) if (need and not lay) else None
        x32 = torch.randn((M, K), device=dev, generator=g) * 2.0

        def buffers(dt):
            return dict(x=x32.to(dt), wc=wc32.to(dt), s=torch.empty(M, dtype=dt, device=dev), f=torch.empty((M, O), dtype=dt, device=dev),
                        q=torch.zeros(int(lib.mixq_qa_bytes(M, K, lay)), dtype=torch.int8, device=dev),
                        out=torch.empty((M, N), dtype=dt, device=dev))
        ba, bb = buffers(torch.float16), buffers(torch.bfloat16)

        def fwd(b, typ):
            def run(st):
                rc = lib.mixq_mixlinear_forward_typed(M, N, K, O, p(b["x"]), p(ind), p(W), p(sW), p(b["wc"]), p(b["s"]), p(b["q"]), p(b["f"]),
                                                      p(b["out"]), lay, typ, p(scr), scr.numel() if scr is not None else 0, st)
                assert rc == 0, rc
            return run

        def quant(b, typ):
            def run(st):
                rc = lib.mixq_quant_extract_typed(M, K, p(b["x"]), p(b["q"]), p(b["s"]), p(b["f"]), p(ind), O, 1, lay, typ, st)
                assert rc == 0, rc
            return run

        fns = dict(zip(legs, (fwd(ba, _lib.MIXQ_TYPE_HALF), fwd(bb, _lib.MIXQ_TYPE_BF16), quant(ba, _lib.MIXQ_TYPE_HALF),
                              quant(bb, _lib.MIXQ_TYPE_BF16))))
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for fn in fns.values():
            fn(st)
        fns[legs[1]](st)
        names = lib.mixq_debug_last_producer_kernel().decode() + " | " + lib.mixq_debug_last_gemm_kernel().decode()
        torch.cuda.synchronize()
        graphs = {}
        side = torch.cuda.Stream()
        for name, fn in fns.items():
            gr = torch.cuda.CUDAGraph()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.cuda.graph(gr, stream=side):
                    cst = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                    for _ in range(iters):
                        fn(cst)
            graphs[name] = gr

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
            for name in legs:
                t[name].append(timed(graphs[name].replay))
        med = {n: statistics.median(v) for n, v in t.items()}
        spread = {n: (max(v) - min(v)) / med[n] for n, v in t.items()}
        s = (f"{M:>6} " + " ".join(f"{med[n]:>15.2f}" for n in legs) +
             f" {med[legs[1]] / med[legs[0]]:>7.3f} {spread[legs[0]]:>9.3f} {med[legs[3]] / med[legs[2]]:>7.3f} {spread[legs[2]]:>9.3f}  {names}")
        lines.append(s)
        print(s, flush=True)
        del graphs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
