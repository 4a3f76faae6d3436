#!/usr/bin/env python3
"""The bf16 form of the fused residual add + RMSNorm / extract / quantise producer (mixq_rmsnorm_extract_quant_typed, MIXQ_TYPE_BF16)
next to its fp16 twin and to what a bf16 model paid before it, ON THE SAME LIBRARY BUILD, in one process:

  (a) fp16   mixq_add_rmsnorm_extract_quant_layout                      one launch
  (b) bf16   mixq_rmsnorm_extract_quant_typed(MIXQ_TYPE_BF16)           one launch; moves the same bytes as (a)
  (c) bf16 status quo: torch's in-place bf16 add into the residual, a torch RMSNorm, and the quantiser pass mixq_enqueue runs over
      the normalised row.  That quantiser has no entry of its own: the pass is timed as mixq_quant_extract on the same buffers
      (same form, grid and bytes as the bf16 quantiser; its values are not used).

All legs update the residual in place, int8 rows (row-major), 128 outlier columns.  Each leg is a batch of calls captured once into
a HIP graph and replayed (the device-side chain without the host); the legs are interleaved round by round after a warm-up, and the
whole measurement is made TWICE per run so that the table shows its own repeat spread (run 1 / run 2: median of the rounds).
usage: python tools/bf16_norm_probe.py [--rounds 7] [--out profiles/bf16_norm_probe.txt]"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mixq_tensorrt_llm_amd import _lib  # noqa: E402

ROWS, WIDTHS = (32, 256, 4096), (4096, 11008)
O, EPS = 128, 1e-6


def torch_rmsnorm(h, gamma):
    if hasattr(torch.nn.functional, "rms_norm"):
        return torch.nn.functional.rms_norm(h, (h.shape[-1],), gamma, EPS)
    hf = h.float()
    return (hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + EPS)).to(h.dtype) * gamma


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    legs = ("fp16 fused", "bf16 fused", "bf16 status quo")
    lines = [f"bf16_norm_probe: {lib.mixq_version().decode()} on {torch.cuda.get_device_name(0)}; us per add + norm + quantise, HIP-graph replay, "
             f"median of {a.rounds} interleaved rounds, measured twice (run 1 / run 2); int8 rows, {O} outlier columns, residual in place",
             f"{'rows x K':>14} " + " ".join(f"{n + ' (run 1 / run 2)':>30}" for n in legs) + f" {'b / a':>7} {'b / c':>7}  form of (b)"]
    for s in lines:
        print(s, flush=True)
    g = torch.Generator(device=dev).manual_seed(0)
    for K in WIDTHS:
        for M in ROWS:
            iters = 200 if M * K <= (1 << 21) else 20
            ind = torch.randperm(K, device=dev, generator=g)[:O].to(torch.int32)
            x32 = torch.randn((M, K), device=dev, generator=g) * 2.0 ** -12     # small: the residual stays finite over every call
            r32 = torch.randn((M, K), device=dev, generator=g)
            g32 = torch.rand(K, device=dev, generator=g) + 0.5

            def buffers(dt):
                return dict(x=x32.to(dt), r0=r32.to(dt), r=r32.to(dt), gamma=g32.to(dt), out=torch.empty((M, K), dtype=dt, device=dev),
                            q=torch.zeros((M, K), dtype=torch.int8, device=dev), s=torch.empty(M, dtype=dt, device=dev),
                            f=torch.empty((M, O), dtype=dt, device=dev))
            ba, bb, bc = buffers(torch.float16), buffers(torch.bfloat16), buffers(torch.bfloat16)

            def leg_a(st):
                rc = lib.mixq_add_rmsnorm_extract_quant_layout(M, K, p(ba["x"]), p(ba["r"]), p(ba["r"]), p(ba["gamma"]), p(ba["out"]), EPS,
                                                               p(ind), O, p(ba["f"]), p(ba["q"]), p(ba["s"]), 0, st)
                assert rc == 0, rc

            def leg_b(st):
                rc = lib.mixq_rmsnorm_extract_quant_typed(M, K, p(bb["x"]), p(bb["r"]), p(bb["r"]), p(bb["gamma"]), p(bb["out"]), EPS, p(ind), O,
                                                          p(bb["f"]), p(bb["q"]), p(bb["s"]), 0, _lib.MIXQ_TYPE_BF16, st)
                assert rc == 0, rc

            def leg_c(st):
                bc["r"].add_(bc["x"])
                n = torch_rmsnorm(bc["r"], bc["gamma"])
                rc = lib.mixq_quant_extract(M, K, p(n), p(bc["q"]), p(bc["s"]), p(bc["f"]), p(ind), O, 0, st)   # (timing stand-in, see above)
                assert rc == 0, rc

            fns = dict(zip(legs, (leg_a, leg_b, leg_c)))
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            for fn in fns.values():
                fn(st)
            leg_b(st)
            form = lib.mixq_debug_last_producer_kernel().decode()
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
            med = {n: [] for n in legs}
            for _ in range(2):              # the whole measurement twice: the table's own repeat spread
                t = {n: [] for n in legs}
                for _ in range(a.rounds):
                    for name in legs:
                        for b in (ba, bb, bc):
                            b["r"].copy_(b["r0"])
                        torch.cuda.synchronize()
                        t[name].append(timed(graphs[name].replay))
                for n in legs:
                    med[n].append(statistics.median(t[n]))
            cell = {n: f"{v[0]:9.2f} / {v[1]:9.2f}" for n, v in med.items()}
            mean = {n: (v[0] + v[1]) / 2 for n, v in med.items()}
            s = (f"{M:>7} x {K:<5} " + " ".join(f"{cell[n]:>30}" for n in legs) +
                 f" {mean[legs[1]] / mean[legs[0]]:>7.3f} {mean[legs[1]] / mean[legs[2]]:>7.3f}  {form}")
            lines.append(s)
            print(s, flush=True)
            del graphs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
