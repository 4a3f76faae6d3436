#!/usr/bin/env python3
"""silu(gate(x)) * up(x) of a Llama MLP on a quantised activation, before and after the merged gate / up projection
(mixq_gemm_mixed_gate_up_typed), ON THE SAME LIBRARY BUILD, interleaved in one process, fp16 and bf16:

  A (status quo)  mixlib.gemm_mixed (up) + mixlib.gemm_mixed(act="silu", mul=up) (gate)    two launches, u [M, N] written and read back
  B               mixlib.gemm_gate_up on the merged layer (pack.merge_gate_up)             one launch

32 / 256 / 4096 rows on 11008 x 4096 (the merged GEMM is 22016 x 4096), 128 outlier columns, row-major int8 rows.  Each leg is timed
stream-issued (a batch of calls from Python between two events) and graph-replayed (the same batch captured once); legs alternate round by
round after a warm-up, the table shows the median of the rounds.  A is the yardstick, in the same process: a feature probe, not a speed
claim, and the Python default stays opt-in whatever it shows.
usage: python tools/gate_up_probe.py [--rounds 7] [--out profiles/gate_up_probe.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mixq_tensorrt_llm_amd import _lib, mixlib, pack  # noqa: E402

ROWS, N, K, O = (32, 256, 4096), 11008, 4096, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = [f"gate_up_probe: {lib.mixq_version().decode()} on {torch.cuda.get_device_name(0)}; us per silu(gate(x)) * up(x) on "
             f"{N} x {K}, {O} outlier columns; A = two launches (up, then gate with mul), B = mixq_gemm_mixed_gate_up_typed; median of {a.rounds} "
             f"interleaved rounds",
             f"{'type':>5} {'rows':>5} {'A stream':>10} {'B stream':>10} {'B / A':>7} {'A graph':>10} {'B graph':>10} {'B / A':>7}  kernel of B"]
    for s in lines:
        print(s, flush=True)
    g = torch.Generator(device=dev).manual_seed(0)
    Wg, Wu = (torch.randint(-127, 128, (N, K), device=dev, generator=g, dtype=torch.int8) for _ in range(2))
    sWg, sWu = ((torch.rand(N, device=dev, generator=g) * 1e-3 + 1e-4).half() for _ in range(2))
    ind = torch.arange(O, dtype=torch.int32)
    for dt in (torch.float16, torch.bfloat16):
        fpWg, fpWu = ((torch.randn((N, O), device=dev, generator=g) * 0.02).to(dt) for _ in range(2))
        m2 = pack.merge_gate_up(dict(weight=Wg, weights_scaling_factor=sWg, fp_weight=fpWg, fp_ind=ind),
                                dict(weight=Wu, weights_scaling_factor=sWu, fp_weight=fpWu, fp_ind=ind))
        W2, sW2, fpW2 = m2["weight"], m2["weights_scaling_factor"], m2["fp_weight"]
        for M in ROWS:
            iters = 100 if M <= 256 else 10
            q = torch.randint(-127, 128, (M, K), device=dev, generator=g, dtype=torch.int8)
            sA = (torch.rand(M, device=dev, generator=g) * 0.02 + 0.005).to(dt)
            fpA = (torch.randn((M, O), device=dev, generator=g) * 4).to(dt)
            u = torch.empty((M, N), dtype=dt, device=dev)
            out_a, out = torch.empty((M, N), dtype=dt, device=dev), torch.empty((M, N), dtype=dt, device=dev)

            def leg_a():
                mixlib.gemm_mixed(q, Wu, sA, sWu, fpA, fpWu, M, N, K, out=u)
                mixlib.gemm_mixed(q, Wg, sA, sWg, fpA, fpWg, M, N, K, out=out_a, act="silu", mul=u)

            def leg_b():
                mixlib.gemm_gate_up(q, W2, sA, sW2, fpA, fpW2, M, N, K, out=out)

            legs = dict(A=leg_a, B=leg_b)
            for fn in legs.values():
                fn()
            leg_b()
            kernel = lib.mixq_debug_last_gemm_kernel().decode()
            torch.cuda.synchronize()
            same = torch.equal(out.view(torch.int16), out_a.view(torch.int16))
            graphs, side = {}, torch.cuda.Stream()
            for name, fn in legs.items():
                gr = torch.cuda.CUDAGraph()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):
                        fn()                  # (the side stream's own exchange scratch exists before the capture)
                    torch.cuda.synchronize()
                    with torch.cuda.graph(gr, stream=side):
                        for _ in range(iters):
                            fn()
                graphs[name] = gr

            def timed(run):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / iters * 1e3

            def batch(fn):
                def run():
                    for _ in range(iters):
                        fn()
                return run

            runs = {("stream", n): batch(fn) for n, fn in legs.items()}
            runs.update({("graph", n): gr.replay for n, gr in graphs.items()})
            for r in runs.values():           # warm-up of every leg in both modes
                r()
            torch.cuda.synchronize()
            t = {k: [] for k in runs}
            for _ in range(a.rounds):
                for key, r in runs.items():   # A stream, B stream, A graph, B graph, round by round
                    t[key].append(timed(r))
            m = {k: statistics.median(v) for k, v in t.items()}
            s = (f"{'fp16' if dt == torch.float16 else 'bf16':>5} {M:>5} {m['stream', 'A']:>10.2f} {m['stream', 'B']:>10.2f} "
                 f"{m['stream', 'B'] / m['stream', 'A']:>7.3f} {m['graph', 'A']:>10.2f} {m['graph', 'B']:>10.2f} "
                 f"{m['graph', 'B'] / m['graph', 'A']:>7.3f}  {kernel}" + ("" if same else "  (A and B differ in bits: random outlier weights, another family's summation order)"))
            lines.append(s)
            print(s, flush=True)
            del graphs, runs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
