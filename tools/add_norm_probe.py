#!/usr/bin/env python3
"""Residual add fused into the RMSNorm / extract / quantise producer (mixq_add_rmsnorm_extract_quant_layout) against the unfused
sequence ON THE SAME LIBRARY BUILD, in one process: torch's in-place fp16 add into the residual + mixq_rmsnorm_extract_quant_layout
on it.  Both legs update the residual in place (h_out == residual), int8 rows, 128 outlier columns.

Two clocks per leg, device events around a batch of calls each:
  stream  the calls issued one by one from Python: what a caller of the C ABI sees, host launch cost included (the unfused leg
          makes two calls per norm, one of them through torch's dispatcher)
  graph   the same batch captured once into a HIP graph and replayed: the device-side chain without the host
The legs are interleaved round by round (A B A B ...) after a warm-up of both; the table holds the median round and the spread
(min .. max).  Before timing, both legs run once from the same residual and h / out / outliers / q / scale are compared byte for
byte.  usage: python tools/add_norm_probe.py [--rounds 9] [--out profiles/add_norm_probe.txt]"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mixq_tensorrt_llm_amd import _lib  # noqa: E402

# (rows, K, layout, calls per timed batch): decode batches, prefill chunks, and the fragment-major image of a decode batch
CASES = [(32, 4096, 0, 400), (256, 4096, 0, 400), (16384, 4096, 0, 40), (16384, 8192, 0, 20), (32, 4096, 1, 400)]
O, EPS = 128, 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    lines = [f"add_norm_probe: {lib.mixq_version().decode()} on {torch.cuda.get_device_name(0)}; us per norm (add included), "
             f"median of {a.rounds} interleaved rounds (min .. max); int8 rows, {O} outlier columns, residual updated in place",
             f"{'rows x K':>14} {'image':>9} {'clock':>7} {'add + norm (2 launches)':>30} {'fused (1 launch)':>30} {'fused / unfused':>16}  form"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    for s in lines:
        print(s, flush=True)
    g = torch.Generator(device=dev).manual_seed(0)
    for M, K, lay, iters in CASES:
        gamma = (torch.rand(K, device=dev, generator=g) + 0.5).to(torch.float16)
        ind = torch.randperm(K, device=dev, generator=g)[:O].to(torch.int32)
        # a small x on a unit residual: the residual stays finite over every call of the run (each call adds x once more)
        x = (torch.randn((M, K), device=dev, generator=g) * 2.0 ** -12).to(torch.float16)
        r0 = torch.randn((M, K), device=dev, generator=g).to(torch.float16)
        qbytes = int(lib.mixq_qa_bytes(M, K, lay))

        def buffers():
            return dict(r=r0.clone(), out=torch.empty_like(x), q=torch.zeros(qbytes, dtype=torch.int8, device=dev),
                        s=torch.empty(M, dtype=torch.float16, device=dev), f=torch.empty((M, O), dtype=torch.float16, device=dev))
        bu, bf = buffers(), buffers()

        def unfused(st):
            bu["r"].add_(x)
            rc = lib.mixq_rmsnorm_extract_quant_layout(M, K, p(bu["r"]), p(gamma), p(bu["out"]), EPS, p(ind), O, p(bu["f"]), p(bu["q"]),
                                                       p(bu["s"]), lay, st)
            assert rc == 0, rc

        def fused(st):
            rc = lib.mixq_add_rmsnorm_extract_quant_layout(M, K, p(x), p(bf["r"]), p(bf["r"]), p(gamma), p(bf["out"]), EPS, p(ind), O,
                                                           p(bf["f"]), p(bf["q"]), p(bf["s"]), lay, st)
            assert rc == 0, rc

        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        unfused(st)
        fused(st)
        form = lib.mixq_debug_last_producer_kernel().decode()
        torch.cuda.synchronize()
        for name in ("r", "out", "q", "s", "f"):
            assert torch.equal(bu[name].view(torch.uint8), bf[name].view(torch.uint8)), f"{M}x{K}: {name} differs between the legs"

        graphs = {}
        side = torch.cuda.Stream()
        for name, fn in (("unfused", unfused), ("fused", fused)):
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

        legs = {"stream": {"unfused": lambda: [unfused(st) for _ in range(iters)], "fused": lambda: [fused(st) for _ in range(iters)]},
                "graph": {"unfused": graphs["unfused"].replay, "fused": graphs["fused"].replay}}
        for clock, pair in legs.items():
            for run in pair.values():       # warm-up of both legs
                run()
            torch.cuda.synchronize()
            t = {"unfused": [], "fused": []}
            for _ in range(a.rounds):
                for name in ("unfused", "fused"):
                    bu["r"].copy_(r0)
                    bf["r"].copy_(r0)
                    torch.cuda.synchronize()
                    t[name].append(timed(pair[name]))
            cell = {n: f"{statistics.median(v):9.2f} ({min(v):8.2f} .. {max(v):8.2f})" for n, v in t.items()}
            ratio = statistics.median(t["fused"]) / statistics.median(t["unfused"])
            emit(f"{M:>7} x {K:<5} {'fragment' if lay else 'row-major':>9} {clock:>7} {cell['unfused']:>30} {cell['fused']:>30} {ratio:>16.3f}  {form}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
