#!/usr/bin/env python3
"""bench.py -- prefill tokens/s of the MixQ W8A8O16 linear path, Llama-2-7B, on N x MI355X.

One "step" = one prefill pass of `--tokens` synthetic tokens (default 512 x 2048 = 1,048,576, BASELINE.json's quoted
config) through every MixQ'd linear of Llama-2-7B (attention.qkv 12288x4096, mlp.gate 11008x4096, mlp.proj 4096x11008;
32 layers = 96 operator calls per token chunk), executed in M-chunks of `--chunk` tokens (default 65536 = 32 sequences;
the work per token does not depend on the chunk).  Every call goes through the drop-in C ABI (`mixq_enqueue_profiled` == `mixq_enqueue` + two event
records around the GEMM launch).  Inputs (activations, packed weights) are resident in HBM before the timed region.

  python bench.py --gpus N --steps K --warmup W           (N>1: launched by torch.distributed.run, one rank per GPU)
  python bench.py ... --dump-outputs DIR                  (also writes the last timed step's outputs, see dump_last_step_outputs)
  python bench.py ... --full                              (also the informational measurements, after the headline one)

Multi-GPU: the path partitions over tokens with no data-path collective (each rank owns a full copy of the 4.6 GB of
packed weights and its own token stream) -> default "dp", weak scaling.  `--tp T` runs the north-star TP layout
instead (rows of W sharded T-ways, one RCCL all-gather of each fp16 output), strong scaling.

Prints ONE JSON line on rank 0: the contract fields, with `roofline` and `quantizer` objects derived from the events of the
timed steps.  A plain run does nothing else: set up, warm up, time the steps, dump if asked, print.  `--full` adds the
measurements that take runs of their own -- `small_m` / `config0`, `decode_step`, `int4`, `chunk_sweep`, `configs`,
`cpu_baseline` and, at N > 1, the tp = N leg -- each of which a `--no-*` option leaves out again; `--mid-m` adds `mid_m`.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

LLAMA2_7B = dict(name="Llama-2-7B", layers=32, linears=[("attention.qkv", 12288, 4096), ("mlp.gate", 11008, 4096),
                                                       ("mlp.proj", 4096, 11008)])
# BASELINE.json configs 4 and 5: the other two models, as the (N, K) of their MixQ linears on ONE GPU
QWEN2_7B = dict(name="Qwen2-7B-Instruct", layers=28, linears=[("attention.qkv", 4608, 3584), ("mlp.gate", 18944, 3584),
                                                            ("mlp.proj", 3584, 18944)])
LLAMA2_70B = dict(name="Llama-2-70B", layers=80, linears=[("attention.qkv", 10240, 8192), ("mlp.gate", 28672, 8192), ("mlp.proj", 8192, 28672)])
LLAMA2_70B_TP8 = dict(name="Llama-2-70B, one GPU's row shard at TP=8", layers=80,
                      linears=[("attention.qkv", 10240 // 8, 8192), ("mlp.gate", 28672 // 8, 8192), ("mlp.proj", 8192 // 8, 28672)])
NUM_OUTLIERS = 128
INT8_MFMA_PEAK_TOPS = 5033.0  # dense int8 MFMA: 256 CU x 4 SIMD x 2048 op/clk x 2.4 GHz = 2x the 2.5 PF bf16 dense peak
                              # (MI355X_MICROARCH.md:394 "I8 ... ~2x bf16 rate", 16x16x64 ceiling >= 3944 TOPS; cdna_hip_programming.md:286:
                              #  micro-benchmark ceiling 4404 TOPS for the 32x32x32 i8 form used here)


class Hip:
    """hipEvent_* straight from libamdhip64 (events are recorded inside the C ABI on torch's current stream)."""

    def __init__(self):
        self.lib = ctypes.CDLL("libamdhip64.so")
        self.lib.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        self.lib.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        self.lib.hipEventDestroy.argtypes = [ctypes.c_void_p]
        self.lib.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]

    def event(self):
        e = ctypes.c_void_p()
        assert self.lib.hipEventCreate(ctypes.byref(e)) == 0
        return e

    def record(self, ev, stream_ptr):
        rc = self.lib.hipEventRecord(ev, stream_ptr)
        assert rc == 0, f"hipEventRecord rc={rc}"

    def elapsed_ms(self, a, b):
        ms = ctypes.c_float()
        rc = self.lib.hipEventElapsedTime(ctypes.byref(ms), a, b)
        assert rc == 0, f"hipEventElapsedTime rc={rc}"
        return ms.value


class LineGuard:
    """Keeps the JSON line safe while a leg runs that may take the process down: a child process reads a copy of the line from a
    pipe and, if the pipe closes WITHOUT the disarm byte (this process died), writes it to `fd`.  The harness owns this -- the
    operator library installs no signal handlers -- and the dying process keeps its own exit status."""
    _CHILD = ("import os, sys\nfd = int(sys.argv[1])\ndata = sys.stdin.buffer.read()\n"
              "if not data.endswith(b'\\0'):\n    os.write(fd, data)\n")

    def __init__(self, fd, line: bytes):
        import subprocess
        self.p = subprocess.Popen([sys.executable, "-c", self._CHILD, str(fd)], stdin=subprocess.PIPE, pass_fds=[fd])
        self.p.stdin.write(line)
        self.p.stdin.flush()

    def disarm(self):
        if self.p is None:
            return
        try:
            self.p.stdin.write(b"\0")
            self.p.stdin.close()
            self.p.wait(timeout=30)
        except Exception:  # noqa: BLE001
            pass
        self.p = None


def synth_layer(N, K, dev, gen, n0=0, n1=None):
    """Random-init packed tensors of one MixQ linear, generated on device in the operator's own contract:
    int8 W ~ round(N(0, 32^2)) clipped (a gaussian weight row quantised with max|w|/127), outlier columns zero."""
    n1 = N if n1 is None else n1
    rows = n1 - n0
    W = torch.randn((rows, K), device=dev, generator=gen).mul_(32.0).round_().clamp_(-127, 127).to(torch.int8)
    ind = torch.randperm(K, device=dev, generator=gen)[:NUM_OUTLIERS].to(torch.int32)
    W[:, ind.long()] = 0
    sW = (torch.rand(rows, device=dev, generator=gen) * 4e-4 + 4e-4).to(torch.float16)
    fpw = (torch.randn((rows, NUM_OUTLIERS), device=dev, generator=gen) * 0.02).to(torch.float16)
    qweight = torch.zeros((K, rows), dtype=torch.uint8, device=dev)  # decode-path operand, untouched in prefill
    return dict(weight=W.view(torch.float16), weights_scaling_factor=sW, fp_weight=fpw,
                fp_ind=ind.view(torch.float16), qweight=qweight.view(torch.float16), ind_i32=ind)


def synth_activation(M, K, ind, dev, gen):
    A = torch.randn((M, K), device=dev, generator=gen)
    A[:, ind.long()] *= 20.0  # activation outliers in the fp_ind columns
    return A.to(torch.float16)


def graph_time_us(fn, dev, calls=100, reps=20):
    """Device-paced time per call: `calls` launches of fn(stream_ptr) captured into one HIP graph, replayed `reps` times."""
    gr = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        fn(ctypes.c_void_p(s.cuda_stream))      # (lazy initialisation happens outside the capture)
        s.synchronize()
        with torch.cuda.graph(gr, stream=s):
            stp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for _ in range(calls):
                fn(stp)
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        gr.replay()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1e3 / (reps * calls)


def small_m_points(lib, TensorDesc, dev, gen, st_ptr, iters=300):
    """Informational (never part of `value`): the HBM-bound end of the same operator, SURVEY §8d -- BASELINE config 0
    (one 4096 x 4096 MixQ linear, bs = 32) and decode steps (bs = 1 / 4: the W8A16 path on `qweight`, GEMV or MFMA skinny
    form) through mixq_enqueue, as weight bytes / time against the HBM peak.  Device-paced (HIP graph of 100 calls)."""
    out = {}
    layers = {}
    for name, M, N, K in (("config0_bs32_4096x4096", 32, 4096, 4096), ("decode_bs1_4096x4096", 1, 4096, 4096),
                          ("decode_bs1_qkv_12288x4096", 1, 12288, 4096), ("decode_bs4_qkv_12288x4096", 4, 12288, 4096),
                          ("decode_bs4_proj_4096x11008", 4, 4096, 11008)):
        if (N, K) not in layers:
            layers[(N, K)] = synth_layer(N, K, dev, gen)
        t = layers[(N, K)]
        A = synth_activation(M, K, t["ind_i32"], dev, gen)
        o = torch.empty((M, N), dtype=torch.float16, device=dev)
        ins = [A, t["weight"], t["weights_scaling_factor"], t["fp_weight"], t["fp_ind"], t["qweight"],
               t["weights_scaling_factor"]]
        in_desc = (TensorDesc * 7)(*[TensorDesc.make(x.shape) for x in ins])
        out_desc = TensorDesc.make(o.shape)
        in_ptrs = (ctypes.c_void_p * 7)(*[x.data_ptr() for x in ins])
        out_ptrs = (ctypes.c_void_p * 1)(o.data_ptr())
        h = ctypes.c_void_p(lib.mixq_create(M, N, K))
        ws = torch.empty(max(lib.mixq_workspace_size(h, M, N, K), 16), dtype=torch.uint8, device=dev)

        def run(st):
            rc = lib.mixq_enqueue(h, in_desc, ctypes.byref(out_desc), in_ptrs, out_ptrs, ctypes.c_void_p(ws.data_ptr()), st)
            assert rc == 0

        dt = graph_time_us(run, dev) * 1e-6
        out[name] = {"us_per_call": dt * 1e6, "weight_GBps": N * K / dt / 1e9, "hbm_frac": N * K / dt / 8e12,
                     "launches_per_call": 2 if M > 4 else 1, "timing": "HIP graph of 100 calls (device-paced)",
                     "cache": "warm: every call re-reads the SAME layer's weights, which the 256 MiB Infinity Cache then serves"
                              + (" -- except that M <= 4 calls on weights of 32 MiB and more stream them with non-temporal loads (no cache "
                                 "allocation: a model's decode step reads each layer once and can never find it resident; -4.6 % per decode "
                                 "step), so this loop no longer gains from re-reading one layer; the cold twin is what a decode step sees"
                                 if (M <= 4 and N * K >= (32 << 20)) else "")}
        # the same point with COLD weights, as in a model's decode step (every layer's weights come from HBM once per step):
        # the calls of the graph cycle through enough distinct copies of the streamed weight tensor to exceed the Infinity Cache
        try:
            widx = 1 if M > 4 else 5                      # `weight` (int8 [N, K]) feeds M > 4, `qweight` the decode path
            copies = (320 << 20) // (N * K) + 2
            alts = [ins[widx]] + [ins[widx].clone() for _ in range(copies - 1)]
            ptr_sets = []
            for wcopy in alts:
                v = [x.data_ptr() for x in ins]
                v[widx] = wcopy.data_ptr()
                ptr_sets.append((ctypes.c_void_p * 7)(*v))
            turn = [0]

            def run_cold(st):
                rc = lib.mixq_enqueue(h, in_desc, ctypes.byref(out_desc), ptr_sets[turn[0] % copies], out_ptrs,
                                      ctypes.c_void_p(ws.data_ptr()), st)
                turn[0] += 1
                assert rc == 0

            dc = graph_time_us(run_cold, dev) * 1e-6
            out[name]["cold"] = {"us_per_call": dc * 1e6, "weight_GBps": N * K / dc / 1e9, "hbm_frac": N * K / dc / 8e12,
                                 "weight_copies_cycled": copies,
                                 "what": f"{copies} distinct copies of the weight tensor ({copies * N * K >> 20} MiB > the "
                                         "Infinity Cache), one per call in turn: every call streams its weights from HBM"}
            if M > 4:   # the same two loops with a registered weight image per copy (mixq_weight_image_*: + N K bytes, same bits)
                imgs = [torch.empty(N * K, dtype=torch.int8, device=dev) for _ in alts]
                try:
                    st0 = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                    for wcopy, im in zip(alts, imgs):
                        assert lib.mixq_weight_image_register(ctypes.c_void_p(wcopy.data_ptr()), N, K, ctypes.c_void_p(im.data_ptr()), st0) == 0
                        # (an image is trusted after its FIRST USE check, which cannot run inside a stream capture: verify now, or the
                        #  captured calls on the copies that never ran eagerly would read `weight` itself)
                        assert lib.mixq_weight_image_verify(ctypes.c_void_p(wcopy.data_ptr()), st0) == 0
                    torch.cuda.synchronize(dev)
                    tw, tcold = graph_time_us(run, dev), graph_time_us(run_cold, dev)
                    out[name]["with_weight_image"] = {"us_per_call": tw, "cold_us_per_call": tcold, "hbm_frac": N * K / (tw * 1e-6) / 8e12,
                                                      "cold_hbm_frac": N * K / (tcold * 1e-6) / 8e12,
                                                      "what": "the layer's `weight` registered with mixq_weight_image_register: the "
                                                              "decode-batch GEMM streams a fragment-major copy (contiguous reads)"}
                finally:
                    for wcopy in alts:
                        lib.mixq_weight_image_unregister(ctypes.c_void_p(wcopy.data_ptr()))
                    del imgs
            del alts
        except Exception as e:  # noqa: BLE001
            out[name]["cold"] = {"error": repr(e)}
        lib.mixq_destroy(h)
    # BASELINE config 0 on the route the reference's PyTorch flavour really takes in decode (MixQ/src/mixquant/modules/fused/
    # norm.py:20-33 -> layernorm.cu:122-198, then linear.py's int8FusedDequantize): the RMSNorm in front of the linear -- a
    # launch the model runs anyway -- normalises, extracts the outliers and quantises in one pass, so the LINEAR is one launch
    # (the fused GEMM with its outlier side product).  Reported: the pair, the plain norm alone, and their difference = what the
    # linear adds to a model that has to run the norm in any case.
    try:
        M, N, K = 32, 4096, 4096
        t = layers[(N, K)]
        p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
        X = synth_activation(M, K, t["ind_i32"], dev, gen)
        gamma = torch.ones(K, dtype=torch.float16, device=dev)
        xn = torch.empty((M, K), dtype=torch.float16, device=dev)
        q = torch.empty((M, K), dtype=torch.int8, device=dev)
        sA = torch.empty(M, dtype=torch.float16, device=dev)
        outl = torch.empty((M, NUM_OUTLIERS), dtype=torch.float16, device=dev)
        o = torch.empty((M, N), dtype=torch.float16, device=dev)
        W8 = t["weight"].view(torch.int8)
        eps = ctypes.c_float(1e-6)

        lay = int(lib.mixq_qa_layout(M, N, K))     # the producer writes the image the GEMM reads fastest (fragment-major here)
        q = torch.empty(int(lib.mixq_qa_bytes(M, K, lay)), dtype=torch.int8, device=dev)

        def pair(st):
            assert lib.mixq_rmsnorm_extract_quant_layout(M, K, p(X), p(gamma), p(xn), eps, p(t["ind_i32"]), NUM_OUTLIERS,
                                                         p(outl), p(q), p(sA), lay, st) == 0
            assert lib.mixq_gemm_mixed_layout(p(q), p(W8), p(sA), p(t["weights_scaling_factor"]), p(outl), p(t["fp_weight"]),
                                              p(o), M, N, K, NUM_OUTLIERS, lay, None, 0, st) == 0

        def norm_only(st):
            assert lib.mixq_rmsnorm(M, K, p(X), p(gamma), p(xn), eps, st) == 0

        t_pair, t_norm = graph_time_us(pair, dev), graph_time_us(norm_only, dev)
        out["config0_norm_fused"] = {"us_per_call": t_pair - t_norm, "pair_us": t_pair, "plain_rmsnorm_us": t_norm,
                                     "weight_GBps": N * K / ((t_pair - t_norm) * 1e-6) / 1e9,
                                     "hbm_frac": N * K / ((t_pair - t_norm) * 1e-6) / 8e12, "launches_per_call": 1,
                                     "qa_layout": "fragment-major" if lay else "row-major",
                                     "what": "fused RMSNorm -> extract -> quant producer + fused GEMM, minus the plain "
                                             "RMSNorm the model runs anyway (the linear's marginal cost on the P-flavour "
                                             "decode route)"}
    except Exception as e:  # noqa: BLE001
        out["config0_norm_fused"] = {"error": repr(e)}
    return out


def decode_step_points(lib, TensorDesc, model, dev, gen, batches=(1, 4, 32, 64, 128, 256, 512)):
    """Informational (never part of `value`): ONE decode step's worth of the path -- all 96 MixQ linears of Llama-2-7B, each with
    ITS OWN weights (4.5 GB of int8 `weight` / `qweight`: cold by construction, no cache serves a layer twice), captured as one
    HIP graph of 96 mixq_enqueue calls, at batch 1 / 4 and at the batch sizes the reference publishes its tokens/s for
    (bs 32 / 64 / 128 / 256 / 512: MixQ/src/benchflops.py:311-315).  Each point: time per step, the GEMM kernel
    family the library chose per linear shape, and the fraction of the BINDING roofline -- algorithmic bytes (weights + fp16
    activations in + fp16 outputs) at 8 TB/s below the ridge, 2 bs N (K + 128) ops at the dense int8 MFMA peak above it.
    Linears only -- attention, norms and sampling are outside the path."""
    out = {}
    for bs in batches:
        calls, max_ws, wbytes, abytes, ops = [], 16, 0, 0, 0.0
        acts, outs = {}, {}
        for (t, ins) in model.keep:
            N, K = t["weight"].shape[0], ins[0].shape[1]
            if K not in acts:
                acts[K] = synth_activation(bs, K, t["ind_i32"], dev, gen)
            if N not in outs:
                outs[N] = torch.empty((bs, N), dtype=torch.float16, device=dev)
            v = [acts[K]] + list(ins[1:])
            in_desc = (TensorDesc * 7)(*[TensorDesc.make(x.shape) for x in v])
            out_desc = TensorDesc.make(outs[N].shape)
            in_ptrs = (ctypes.c_void_p * 7)(*[x.data_ptr() for x in v])
            out_ptrs = (ctypes.c_void_p * 1)(outs[N].data_ptr())
            h = ctypes.c_void_p(lib.mixq_create(bs, N, K))
            max_ws = max(max_ws, lib.mixq_workspace_size(h, bs, N, K))
            calls.append((h, in_desc, out_desc, in_ptrs, out_ptrs))
            wbytes += N * K
            abytes += 2 * bs * (K + N) + 2 * N * (1 + NUM_OUTLIERS)   # A in, Out, sW, fp_weight
            ops += 2.0 * bs * N * (K + (NUM_OUTLIERS if bs > 4 else 0))
        ws = torch.empty(max_ws, dtype=torch.uint8, device=dev)
        turn = [0]

        def run(st):
            h, in_desc, out_desc, in_ptrs, out_ptrs = calls[turn[0] % len(calls)]
            turn[0] += 1
            assert lib.mixq_enqueue(h, in_desc, ctypes.byref(out_desc), in_ptrs, out_ptrs, ctypes.c_void_p(ws.data_ptr()), st) == 0

        kernels = {}
        st0 = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for i in range(len(model.spec["linears"])):   # (one eager call per shape: which kernel family serves it)
            turn[0] = i
            run(st0)
            name = model.spec["linears"][i][0]
            kernels[name] = lib.mixq_debug_last_gemm_kernel().decode().split(" ")[0] if bs > 4 else "w8a16 (fpA_intB on qweight)"
        torch.cuda.synchronize(dev)
        turn[0] = -1   # (graph_time_us makes one call outside the capture: the captured 96 then start at linear 0)
        us = graph_time_us(run, dev, calls=len(calls), reps=10) * len(calls)
        t_hbm, t_mfma = (wbytes + abytes) / 8e12, ops / (INT8_MFMA_PEAK_TOPS * 1e12)
        out[f"bs{bs}"] = {"us_per_step": us, "linears": len(calls), "weight_GB": wbytes / 1e9, "weight_GBps": wbytes / us / 1e3,
                          "hbm_frac": wbytes / (us * 1e-6) / 8e12, "tokens_per_s_bound_by_these_linears": bs / (us * 1e-6),
                          "kernels": kernels,
                          "roofline": {"bound": "hbm" if t_hbm >= t_mfma else "mfma", "frac": max(t_hbm, t_mfma) / (us * 1e-6),
                                       "algorithmic_GB": (wbytes + abytes) / 1e9, "int8_TOP": ops / 1e12,
                                       "hbm_floor_us": t_hbm * 1e6, "mfma_floor_us": t_mfma * 1e6}}
        if 4 < bs <= 64:   # the same step with a weight image per layer (mixq_weight_image_*: + N K bytes per layer, same bits)
            try:
                imgs = []
                for (t, ins) in model.keep:
                    N, K = t["weight"].shape[0], ins[0].shape[1]
                    im = torch.empty(N * K, dtype=torch.int8, device=dev)
                    assert lib.mixq_weight_image_register(ctypes.c_void_p(t["weight"].data_ptr()), N, K, ctypes.c_void_p(im.data_ptr()), st0) == 0
                    assert lib.mixq_weight_image_verify(ctypes.c_void_p(t["weight"].data_ptr()), st0) == 0   # (before the capture: see small_m_points)
                    imgs.append(im)
                torch.cuda.synchronize(dev)
                turn[0] = -1
                us_i = graph_time_us(run, dev, calls=len(calls), reps=10) * len(calls)
                out[f"bs{bs}"]["with_weight_images"] = {
                    "us_per_step": us_i, "weight_GBps": wbytes / us_i / 1e3, "hbm_frac": wbytes / (us_i * 1e-6) / 8e12,
                    "roofline_frac": max(t_hbm, t_mfma) / (us_i * 1e-6),
                    "tokens_per_s_bound_by_these_linears": bs / (us_i * 1e-6), "extra_HBM_GB": wbytes / 1e9,
                    "what": "every layer's `weight` registered with mixq_weight_image_register (a fragment-major copy the decode-batch "
                            "GEMM streams with contiguous reads; the calls are the same mixq_enqueue calls, bit-identical outputs)"}
            except Exception as e:  # noqa: BLE001
                out[f"bs{bs}"]["with_weight_images"] = {"error": repr(e)}
            finally:
                for (t, ins) in model.keep:
                    lib.mixq_weight_image_unregister(ctypes.c_void_p(t["weight"].data_ptr()))
                imgs = None
        for c in calls:
            lib.mixq_destroy(c[0])
        del ws, acts, outs
    out["what"] = ("one decode step of the 96 MixQ linears of Llama-2-7B (qkv, gate, proj x 32 layers), every layer its own weights, "
                   "one HIP graph of 96 mixq_enqueue calls; M <= 4: the W8A16 path on qweight, M > 4: quantise + fused int8 GEMM; "
                   "bs 32..512 = the batch sizes of the reference's published tokens/s (benchflops.py:311-315)")
    return out


def int4_points(lib, model, dev, gen, decode_step, batches=(1, 32)):
    """Informational (never part of `value`): the 4-bit (W4A4) flavour of the same 96 linears in decode (MixLinear_GEMM bit = 4,
    MixQ/src/mixquant/modules/linear.py:121-143, cult.cu:2005-2060): every layer its own PACKED weights (2.25 GB), one HIP graph
    per step.  `gemm_only`: mixq_int4_fused_dequantize alone -- ONE launch per linear that streams the packed weight and widens
    it in registers (csrc/int4_gemm_kernels.hip); what a linear costs when the fused RMSNorm in front has already quantised the row
    (mixq_rmsnorm_extract_quant4, the P-flavour's decode route).  `two_launches`: mixq_int4quant + the GEMM.  Against the int8
    flavour's decode_step at the same batch (bs 1: the W8A16 GEMV on qweight; bs 32: quantise + int8 skinny GEMM).  `one_call` (one row):
    mixq_int4_linear_forward on the fp16 row -- ONE launch per linear, the row quantised inside the weight-streaming kernel."""
    out = {}
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    shapes = [(t["weight"].shape[0], ins[0].shape[1]) for (t, ins) in model.keep]
    ws4 = [torch.randint(0, 256, (N, K // 2), dtype=torch.uint8, device=dev, generator=gen) for (N, K) in shapes]
    sws = [t["weights_scaling_factor"] for (t, _) in model.keep]
    wbytes = sum(w.numel() for w in ws4)
    for bs in batches:
        acts = {K: torch.randn((bs, K), device=dev, generator=gen).to(torch.float16) for K in {k for _, k in shapes}}
        q4 = {K: torch.empty((bs, K // 2), dtype=torch.uint8, device=dev) for K in acts}
        sa = {K: torch.empty(bs, dtype=torch.float16, device=dev) for K in acts}
        outs = {N: torch.empty((bs, N), dtype=torch.float16, device=dev) for N in {n for n, _ in shapes}}
        st0 = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for K in acts:
            assert lib.mixq_int4quant(bs, K, p(acts[K]), p(q4[K]), p(sa[K]), st0) == 0
        turn = [0]

        def gemm_only(st):
            i = turn[0] % len(shapes)
            turn[0] += 1
            N, K = shapes[i]
            assert lib.mixq_int4_fused_dequantize(p(q4[K]), p(ws4[i]), p(sa[K]), p(sws[i]), None, p(outs[N]), bs, N, K // 2, None, st) == 0

        def two_launches(st):
            N, K = shapes[turn[0] % len(shapes)]
            assert lib.mixq_int4quant(bs, K, p(acts[K]), p(q4[K]), p(sa[K]), st) == 0
            gemm_only(st)

        def one_call(st):   # mixq_int4_linear_forward: ONE row is quantised INSIDE the weight-streaming launch (round 6; more rows = the two launches)
            i = turn[0] % len(shapes)
            turn[0] += 1
            N, K = shapes[i]
            assert lib.mixq_int4_linear_forward(p(acts[K]), p(ws4[i]), p(sa[K]), p(q4[K]), p(sws[i]), None, p(outs[N]), bs, N, K // 2, 0, None, st) == 0

        pt = {}
        for name, fn in (("gemm_only", gemm_only), ("two_launches", two_launches)) + ((("one_call", one_call),) if bs == 1 else ()):
            turn[0] = -1
            us = graph_time_us(fn, dev, calls=len(shapes), reps=10) * len(shapes)
            pt[name] = {"us_per_step": us, "weight_GBps": wbytes / us / 1e3, "hbm_frac": wbytes / (us * 1e-6) / 8e12}
        ref = (decode_step or {}).get(f"bs{bs}", {}).get("us_per_step")
        pt["int8_step_us"] = ref
        if ref:
            pt["speedup_vs_int8_step"] = {k: ref / pt[k]["us_per_step"] for k in ("gemm_only", "two_launches", "one_call") if k in pt}
        pt["kernel"] = lib.mixq_debug_last_gemm_kernel().decode()
        out[f"bs{bs}"] = pt
    out["weight_GB"] = wbytes / 1e9
    out["what"] = ("decode step of the 96 Llama-2-7B linears with 4-bit weights AND activations (W4A4, MixLinear_GEMM bit = 4): the packed "
                   "weight (N K / 2 bytes) is streamed once per call and widened to int8 in registers -- no unpack pass, no workspace")
    return out


def mid_m_points(lib, TensorDesc, dev, gen, st_ptr, iters=100):
    """Informational (never part of `value`): decode batches (32 / 128 / 512 rows) and a short prefill (1024 / 2048 tokens) of
    the same three linears, where the tiles no longer fill the chip and the library splits K over several workgroups per
    tile.  Whole operator (quantiser + GEMM) through mixq_enqueue."""
    out = {}
    for M in (32, 128, 512, 1024, 2048):   # 512 = the top of the batch range the reference publishes numbers for
        per = {}
        total = 0.0
        for name, N, K in LLAMA2_7B["linears"]:
            t = synth_layer(N, K, dev, gen)
            A = synth_activation(M, K, t["ind_i32"], dev, gen)
            o = torch.empty((M, N), dtype=torch.float16, device=dev)
            ins = [A, t["weight"], t["weights_scaling_factor"], t["fp_weight"], t["fp_ind"], t["qweight"],
                   t["weights_scaling_factor"]]
            in_desc = (TensorDesc * 7)(*[TensorDesc.make(x.shape) for x in ins])
            out_desc = TensorDesc.make(o.shape)
            in_ptrs = (ctypes.c_void_p * 7)(*[x.data_ptr() for x in ins])
            out_ptrs = (ctypes.c_void_p * 1)(o.data_ptr())
            h = ctypes.c_void_p(lib.mixq_create(M, N, K))
            ws = torch.empty(max(lib.mixq_workspace_size(h, M, N, K), 16), dtype=torch.uint8, device=dev)
            run = lambda: lib.mixq_enqueue(h, in_desc, ctypes.byref(out_desc), in_ptrs, out_ptrs,  # noqa: E731
                                           ctypes.c_void_p(ws.data_ptr()), st_ptr)
            for _ in range(10):
                assert run() == 0
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(iters):
                run()
            torch.cuda.synchronize(dev)
            dt = (time.perf_counter() - t0) / iters
            lib.mixq_destroy(h)
            total += dt
            per[name] = {"us_per_call": dt * 1e6, "TOPS": 2.0 * M * N * (K + NUM_OUTLIERS) / dt / 1e12,
                         "k_split": lib.mixq_gemm_scratch_size(M, N, K) > 0,
                         "kernel": lib.mixq_debug_last_gemm_kernel().decode()}
            del t, A, o, ws
        out[f"chunk_of_{M}_tokens"] = {"linears": per, "tokens_per_s": M / (total * LLAMA2_7B["layers"])}
    return out


def cpu_baseline(seconds_target=15.0):
    """The oracle (CPU restatement of the reference arithmetic, OpenMP) on a bounded sample: ONE Llama-2-7B layer
    (its three MixQ linears), M tokens chosen so the run takes ~seconds_target; tokens/s for the full model = M /
    (32 x t_layer), i.e. extrapolated linearly over the 32 identical layers."""
    import oracle
    oracle.build()
    rng = np.random.default_rng(0)
    shapes = [(n, k) for _, n, k in LLAMA2_7B["linears"]]
    layers = []
    for n, k in shapes:
        W = rng.integers(-127, 128, size=(n, k), dtype=np.int8)
        ind = rng.permutation(k)[:NUM_OUTLIERS].astype(np.int32)
        W[:, ind] = 0
        layers.append(dict(W=W, sW=(rng.random(n) * 4e-4 + 4e-4).astype(np.float16),
                           fpW=(rng.standard_normal((n, NUM_OUTLIERS)) * 0.02).astype(np.float16), ind=ind, k=k))

    def run(M):
        t0 = time.perf_counter()
        for L in layers:
            A = rng.standard_normal((M, L["k"])).astype(np.float16)
            oracle.linear_prefill(A, L["W"], L["sW"], L["fpW"], L["ind"])
        return time.perf_counter() - t0

    M, t = 64, 0.0
    for _ in range(4):  # grow the sample until it costs ~10-30 s of CPU work (small M under-uses the threads)
        t = run(M)
        if t >= 0.6 * seconds_target or M >= 16384:
            break
        M = int(min(16384, max(M * 2, M * seconds_target / max(t, 1e-3))))
        M -= M % 16
    tok_s = M / (t * LLAMA2_7B["layers"])
    # BASELINE configs[0] (mandatory): ONE 4096 x 4096 MixQ linear at bs = 32, the same call the `small_m`
    # object times on the GPU -- median of a few repetitions, microseconds per call
    W0 = rng.integers(-127, 128, size=(4096, 4096), dtype=np.int8)
    ind0 = rng.permutation(4096)[:NUM_OUTLIERS].astype(np.int32)
    W0[:, ind0] = 0
    sW0 = (rng.random(4096) * 4e-4 + 4e-4).astype(np.float16)
    fpW0 = (rng.standard_normal((4096, NUM_OUTLIERS)) * 0.02).astype(np.float16)
    A0 = rng.standard_normal((32, 4096)).astype(np.float16)
    reps = []
    for _ in range(7):
        t0 = time.perf_counter()
        oracle.linear_prefill(A0, W0, sW0, fpW0, ind0)
        reps.append(time.perf_counter() - t0)
    cfg0_us = sorted(reps)[len(reps) // 2] * 1e6
    return {"value": tok_s, "unit": "tokens/s", "cores": oracle.num_threads(), "kind": "port",
            "sample": f"oracle.linear_prefill on 1 of 32 Llama-2-7B layers (qkv+gate+proj), M={M} tokens, "
                      f"{t:.1f} s on {oracle.num_threads()} OpenMP threads; scaled x32 layers",
            "config0_bs32_4096x4096": {"us_per_call": cfg0_us, "tokens_per_s": 32 / (cfg0_us * 1e-6),
                                       "sample": "oracle.linear_prefill, one 4096x4096 MixQ linear, M=32, median of 7"}}


class Model:
    """Resident state of one rank: the packed weights of all 96 MixQ linears (or this rank's row shard of each),
    rotating activation chunks, output buffers, the plugin workspace, and prepared ctypes argument blocks."""

    def __init__(self, lib, TensorDesc, parallel, dev, gen, chunk, tp, tp_rank, acts=None, spec=None, nrot=8):
        self.lib, self.dev, self.chunk, self.tp = lib, dev, chunk, tp
        self.spec = spec = spec if spec is not None else LLAMA2_7B
        self.TensorDesc = TensorDesc
        self.calls, self.keep, self.outs, self.full = [], [], {}, {}
        self.acts = acts if acts is not None else {}
        max_ws = 0
        for layer in range(spec["layers"]):
            for name, N, K in spec["linears"]:
                n0, n1 = parallel.shard_bounds(N, tp, tp_rank) if tp > 1 else (0, N)
                t = synth_layer(N, K, dev, gen, n0, n1)
                if K not in self.acts:  # rotating chunks per K (>1 GB: never resident in the 256 MiB Infinity Cache)
                    self.acts[K] = [synth_activation(chunk, K, t["ind_i32"], dev, gen) for _ in range(nrot)]
                if (n1 - n0) not in self.outs:  # TP: two buffers per shape, so that the gather of call i overlaps GEMM i + 1
                    self.outs[n1 - n0] = [torch.empty((chunk, n1 - n0), dtype=torch.float16, device=dev)
                                          for _ in range(2 if tp > 1 else 1)]
                out = self.outs[n1 - n0][0]
                ins = [self.acts[K][0], t["weight"], t["weights_scaling_factor"], t["fp_weight"], t["fp_ind"],
                       t["qweight"], t["weights_scaling_factor"]]
                in_desc = (TensorDesc * 7)(*[TensorDesc.make(x.shape) for x in ins])
                out_desc = TensorDesc.make(out.shape)
                in_ptrs = [(ctypes.c_void_p * 7)(*([a.data_ptr()] + [x.data_ptr() for x in ins[1:]]))
                           for a in self.acts[K]]
                out_ptrs = [(ctypes.c_void_p * 1)(o.data_ptr()) for o in self.outs[n1 - n0]]
                h = lib.mixq_create(chunk, n1 - n0, K)
                max_ws = max(max_ws, lib.mixq_workspace_size(h, chunk, n1 - n0, K))
                self.calls.append((ctypes.c_void_p(h), in_desc, out_desc, in_ptrs, out_ptrs, n1 - n0, K,
                                   self.outs[n1 - n0], N))
                self.keep.append((t, ins))
        self.workspace = torch.empty(max_ws, dtype=torch.uint8, device=dev)
        self.ws_ptr = ctypes.c_void_p(self.workspace.data_ptr())
        self.gatherers = {}    # N -> parallel.PeerGather (tp > 1, peer-write transport)
        self.fused = {}        # (n_loc, K) -> True: the all-gather rides in the GEMM's store path (mixq_enqueue_tp)
        self.transport = None
        self.n_call = 0
        self.gather_done = [None, None]   # event of the last gather that READ output buffer 0 / 1

    def rechunked(self, chunk):
        """The same resident weights driven in M-chunks of `chunk` <= self.chunk tokens: activation and output buffers are row
        slices of this model's, the workspace is shared (mixq_workspace_size of the larger M covers every smaller one)."""
        assert self.tp == 1 and chunk <= self.chunk
        v = Model.__new__(Model)
        v.lib, v.dev, v.chunk, v.tp, v.spec, v.TensorDesc = self.lib, self.dev, chunk, 1, self.spec, self.TensorDesc
        v.acts, v.outs, v.full, v.keep = self.acts, self.outs, {}, self.keep
        v.workspace, v.ws_ptr = self.workspace, self.ws_ptr
        v.gatherers, v.fused, v.transport, v.n_call, v.gather_done = {}, {}, None, 0, [None, None]
        v.calls = []
        for (t, ins), old in zip(self.keep, self.calls):
            n_loc, K, outs, N = old[5], old[6], old[7], old[8]
            acts = [a[:chunk] for a in self.acts[K]]
            o = [x[:chunk] for x in outs]
            in_desc = (self.TensorDesc * 7)(*[self.TensorDesc.make(x.shape) for x in [acts[0]] + list(ins[1:])])
            out_desc = self.TensorDesc.make(o[0].shape)
            in_ptrs = [(ctypes.c_void_p * 7)(*([a.data_ptr()] + [x.data_ptr() for x in ins[1:]])) for a in acts]
            out_ptrs = [(ctypes.c_void_p * 1)(x.data_ptr()) for x in o]
            h = self.lib.mixq_create(chunk, n_loc, K)
            v.calls.append((ctypes.c_void_p(h), in_desc, out_desc, in_ptrs, out_ptrs, n_loc, K, o, N))
        return v

    def open_peer_transport(self, parallel, rank, group=None):
        """One-sided peer writes over xGMI for the output all-gather (csrc/tp_kernels.hip); falls back to RCCL -- on
        EVERY rank if any rank could not map its peers' buffers (the ranks must agree on the transport)."""
        err = None
        try:
            for N in sorted({c[8] for c in self.calls}):
                self.gatherers[N] = parallel.PeerGather(self.chunk, N, self.tp, rank, self.dev, group)
            # self-test before anything is timed (this transport has never seen a multi-GPU node): every rank pushes a
            # block that names it, and must find every peer's block in its place, without a wait timing out
            for N, g in self.gatherers.items():
                mine = torch.full((64, N // self.tp), float(rank + 1), dtype=torch.float16, device=self.dev)
                got = g.gather(mine)
                torch.cuda.synchronize(self.dev)
                want = torch.arange(1, self.tp + 1, dtype=torch.float16, device=self.dev).repeat_interleave(N // self.tp)
                if g.timed_out() or not torch.equal(got, want.expand(64, N)):
                    raise RuntimeError(f"peer-write self-test failed for N={N} (timed out: {g.timed_out()})")
            # second self-test: the all-gather FUSED into the GEMM's store path (mixq_enqueue_tp) must give the same tensor
            # as operator + push on the first call of every shape that supports it
            self.fused = {}
            for (h, in_desc, out_desc, in_ptrs_list, out_ptrs, n_loc, K, outs, N) in self.calls[:3]:
                if not self.lib.mixq_tp_fused_supported(self.chunk, n_loc, K):
                    continue
                g = self.gatherers[N]
                st = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
                rc = self.lib.mixq_enqueue(h, in_desc, ctypes.byref(out_desc), in_ptrs_list[0], out_ptrs[0], self.ws_ptr, st)
                assert rc == 0
                ref = g.gather(outs[0])
                got = g.enqueue_gather_raw(h, in_desc, in_ptrs_list[0], self.ws_ptr, self.chunk, K)
                torch.cuda.synchronize(self.dev)
                if g.timed_out() or not torch.equal(got, ref):
                    raise RuntimeError(f"fused peer-write self-test failed for N={N}, K={K}")
                self.fused[(n_loc, K)] = True
            if any((c[5], c[6]) not in self.fused for c in self.calls):
                self.fused = {}   # all or nothing: one PeerGather is never driven from two streams
        except Exception as e:  # noqa: BLE001
            err = repr(e)
        verdicts = [None] * self.tp
        dist.all_gather_object(verdicts, err, group=group)
        if all(v is None for v in verdicts):
            self.transport = "peer writes over xGMI, data lands in place: " + (
                "issued from the GEMM's own store path (mixq_enqueue_tp, per-M-chunk flags)" if self.fused
                else "mixq_tp_push_columns + flags")
        else:
            self.gatherers = {}
            self.fused = {}
            first = next(v for v in verdicts if v is not None)
            self.transport = f"rccl all_gather_into_tensor + column placement (peer transport unavailable: {first})"

    def close(self):
        for g in self.gatherers.values():
            g.close()
        self.gatherers = {}
        for c in self.calls:
            self.lib.mixq_destroy(c[0])
        self.calls, self.keep = [], []


DUMP_ROWS = 256   # rows sampled per output: 256 x (12288 + 11008 + 4096) float32 = 28 MB for Llama-2-7B (the cap is 64 MB)


def dump_last_step_outputs(model, chunk, out_dir):
    """The outputs the timed path returned in its last step, as float32 .npy: for every linear of the model, the output of its
    last call (the last layer, the last M-chunk) -- what is still resident when the step ends; at tp > 1 the gathered tensor.
    Rows: a fixed, seeded sample of DUMP_ROWS of the chunk (all of them when the chunk is smaller); the inputs come from the
    seeded generator, so the same arguments give the same inputs on every run."""
    rows = np.sort(np.random.default_rng(0).choice(chunk, size=min(DUMP_ROWS, chunk), replace=False))
    idx = torch.from_numpy(rows).to(model.dev)
    names = [name for name, _, _ in model.spec["linears"]]
    total = 0
    for name, call in zip(names, model.calls[-len(names):]):   # the calls of the last layer
        outs, N = call[7], call[8]
        out = model.full[N] if model.tp > 1 else outs[0]
        sample = out.index_select(0, idx).float().cpu().numpy()
        total += sample.nbytes
        assert total <= 64 << 20, "--dump-outputs: more than 64 MB"
        np.save(os.path.join(out_dir, f"{name}.npy"), sample)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30, help="timed steps (SURVEY 8d: >= 30; the median is reported too)")
    ap.add_argument("--warmup", type=int, default=10, help="untimed warm-up steps (SURVEY 8d: 10)")
    ap.add_argument("--tokens", type=int, default=512 * 2048, help="tokens per step per DP replica")
    ap.add_argument("--chunk", type=int, default=65536,
                    help="M of each operator call.  65536 tokens = 32 sequences: 256 tile rows, so that the 256x256 tiles "
                         "of all three shapes (48 / 43 / 16 tile columns) fill the 256 CUs in whole rounds")
    ap.add_argument("--tp", type=int, default=1,
                    help="rows-of-W sharding degree of the MAIN measurement (1 = pure DP, no collective).  Whatever this "
                         "is, a --full run on N > 1 GPUs also reports the north-star layout (tp = N) in the `tp` object")
    ap.add_argument("--full", action="store_true",
                    help="after the headline measurement, also run the informational ones (small_m, config0, decode_step, int4, "
                         "chunk_sweep, configs, cpu_baseline; the tp = N leg at N > 1); the --no-* options leave parts out")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-decode-step", action="store_true", help="skip the decode_step object (profiling runs: 3 graphs of 96 calls)")
    ap.add_argument("--no-small-m", action="store_true", help="skip the small_m object (counter passes: thousands of short launches)")
    ap.add_argument("--no-sweeps", action="store_true", help="skip the chunk_sweep and configs objects (profiling runs)")
    ap.add_argument("--mid-m", action="store_true",
                    help="add the informational 1024 / 2048-token prefill points (K split over workgroups) to the JSON line")
    ap.add_argument("--order", choices=["layer", "chunk"], default="layer",
                    help="layer: each linear sees all tokens before the next one (batched prefill); chunk: chunked prefill")
    ap.add_argument("--no-tp-leg", action="store_true", help="skip the tp = N measurement at N > 1")
    ap.add_argument("--no-tp-alternatives", action="store_true", help="tp = N leg: do not time the other transports (one step each)")
    ap.add_argument("--tp-steps", type=int, default=3, help="timed steps of the tp = N measurement")
    ap.add_argument("--no-config5", action="store_true", help="tp = N leg: skip BASELINE configs[4] (Llama-2-70B, rows of W sharded N ways + the all-gather)")
    ap.add_argument("--config5-layers", type=int, default=80, help="decoder layers of the Llama-2-70B leg (80 = the model; the one-GPU tests run 1)")
    ap.add_argument("--variant", type=int, default=0, help="GEMM schedule: 0 auto, 1 two-barrier, 2 ping-pong (A/B runs)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned as DIR/<linear>.npy (float32, a fixed "
                         "seeded sample of rows; rank 0) so that two builds can be compared output for output")
    args = ap.parse_args()
    if args.dump_outputs:   # fail before anything is measured, not after
        os.makedirs(args.dump_outputs, exist_ok=True)

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        # `python bench.py --gpus N ...` typed as is (the reference's multi-GPU scripts self-launch too,
        # mix_qwen_mpi.sh:17-27): re-run under torch.distributed.run, one rank per GPU; rank 0 of the child prints the
        # ONE JSON line on our stdout.
        import socket
        import subprocess
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    assert torch.cuda.is_available(), "bench.py needs a GPU (the MixQ operator has no CPU path)"
    # stdout carries exactly ONE line, the JSON record of rank 0: everything else any rank or library prints (RCCL / gloo
    # banners go through C stdio) is sent to stderr for the whole run; the record is written to the saved descriptor.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    def emit(record):
        os.write(json_fd, (json.dumps(record) + "\n").encode())
    # MIXQ_BENCH_SINGLE_GPU_RANKS=1: control-flow check of the N > 1 path on a ONE-GPU box -- every rank runs on GPU 0 and
    # the collectives (harness barrier / max over ranks AND the output all-gather) go through gloo; never used for
    # reported numbers.
    shared_gpu = os.environ.get("MIXQ_BENCH_SINGLE_GPU_RANKS") == "1" and world > 1
    if shared_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    red_dev = torch.device("cpu") if shared_gpu else dev
    backend = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        backend = "gloo" if shared_gpu else "nccl"
        if shared_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        assert dist.get_world_size() == world and dist.get_backend() == backend
    tp = args.tp
    assert world % tp == 0
    dp = world // tp
    tp_group = None
    if tp > 1:
        for g in range(dp):
            grp = dist.new_group(list(range(g * tp, (g + 1) * tp)))
            if rank // tp == g:
                tp_group = grp
    tp_rank = rank % tp

    if args.variant != 0:
        os.environ.setdefault("MIXQ_DEBUG_KNOBS", "1")
    from mixq_tensorrt_llm_amd import _lib, parallel
    from mixq_tensorrt_llm_amd._lib import TensorDesc
    lib = _lib.load()
    assert lib.initOpenAiTritonPlugins(None, b"tensorrt_llm")
    if args.variant != 0:   # (A/B runs only; the knob acts only where MIXQ_DEBUG_KNOBS=1 -- a default run never touches it)
        lib.mixq_debug_set_gemm_variant(args.variant)
    hip = Hip()

    chunk = min(args.chunk, args.tokens)
    assert args.tokens % chunk == 0
    n_chunks = args.tokens // chunk
    gen = torch.Generator(device=dev).manual_seed(1234 + rank)
    stream = torch.cuda.current_stream(dev)
    st_ptr = ctypes.c_void_p(stream.cuda_stream)
    comm_stream = torch.cuda.Stream(dev) if world > 1 else None

    def schedule(model, n_chunks):
        # "layer": batched-prefill order -- every linear consumes all bs x seq tokens (as M-chunks) before the next
        # linear runs, as an engine executing layer by layer over the whole batch does; its weights are fetched from
        # HBM once per step.  "chunk": each token chunk walks through all 96 linears (chunked-prefill serving order).
        if args.order == "layer":
            for call in model.calls:
                for c in range(n_chunks):
                    yield call, c
        else:
            for c in range(n_chunks):
                for call in model.calls:
                    yield call, c

    def one_step(model, group, events=None, n_chunks=n_chunks):
        ei = 0
        for (h, in_desc, out_desc, in_ptrs_list, out_ptrs, n_loc, K, outs, N), c in schedule(model, n_chunks):
            in_ptrs = in_ptrs_list[c % len(in_ptrs_list)]   # rotate the activation buffers of this K
            e0 = e1 = None
            if events is not None:
                e0, e1 = events[ei]
                ei += 1
            if model.tp > 1 and model.fused.get((n_loc, K)) and events is None:
                # operator + all-gather in ONE pass on the compute stream: the GEMM's epilogue writes this rank's column
                # block into every rank's buffer and publishes per-chunk flags; the stream then waits for the peers' flags
                model.full[N] = model.gatherers[N].enqueue_gather_raw(h, in_desc, in_ptrs, model.ws_ptr, model.chunk, K)
                continue
            par = model.n_call & 1 if model.tp > 1 else 0
            model.n_call += 1
            if model.tp > 1 and model.gather_done[par] is not None:
                stream.wait_event(model.gather_done[par])   # the gather that read this output buffer two calls ago
            rc = lib.mixq_enqueue_profiled(h, in_desc, ctypes.byref(out_desc), in_ptrs, out_ptrs[par], model.ws_ptr,
                                           st_ptr, e0, e1)
            if rc != 0:
                raise _lib.MixQError(rc, "mixq_enqueue")
            if model.tp > 1:
                # the ONE collective of the path: all-gather of the fp16 output columns on a side stream -- it overlaps
                # the next call's GEMM, which writes the other output buffer
                comm_stream.wait_stream(stream)
                with torch.cuda.stream(comm_stream):
                    if N in model.gatherers:
                        model.full[N] = model.gatherers[N].gather(outs[par])
                    else:
                        model.full[N] = parallel.all_gather_columns(outs[par], group, model.tp)
                    ev = torch.cuda.Event()
                    ev.record(comm_stream)
                model.gather_done[par] = ev
        if model.tp > 1:
            stream.wait_stream(comm_stream)

    def sync_all():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    def timed_run(model, group, steps, warmup, with_gemm_events, n_chunks=n_chunks):
        """W warm-up steps, then EXACTLY `steps` steps between barrier + synchronize brackets; max over ranks."""
        for _ in range(warmup):
            one_step(model, group, None, n_chunks)
        launches = n_chunks * len(model.calls)
        events = [[(hip.event(), hip.event()) for _ in range(launches)] for _ in range(steps)] if with_gemm_events else None
        marks = [hip.event() for _ in range(steps + 1)]   # per-step boundaries on the compute stream (median)
        sync_all()
        t0 = time.perf_counter()
        for s in range(steps):
            hip.record(marks[s], st_ptr)
            one_step(model, group, events[s] if events else None, n_chunks)
        hip.record(marks[steps], st_ptr)
        sync_all()
        elapsed = time.perf_counter() - t0
        if world > 1:
            tmax = torch.tensor([elapsed], dtype=torch.float64, device=red_dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            elapsed = float(tmax.item())
        per_step = sorted(hip.elapsed_ms(marks[s], marks[s + 1]) for s in range(steps))
        median = per_step[len(per_step) // 2] if steps % 2 else 0.5 * (per_step[steps // 2 - 1] + per_step[steps // 2])
        return elapsed, median, events, launches

    # ---- main measurement ------------------------------------------------------------------------------------
    model = Model(lib, TensorDesc, parallel, dev, gen, chunk, tp, tp_rank)
    if tp > 1:
        model.open_peer_transport(parallel, tp_rank, tp_group)
    elapsed, median_ms, events, launches_per_step = timed_run(model, tp_group, args.steps, args.warmup, True)
    if args.dump_outputs and rank == 0:   # before any later leg reuses the output buffers
        dump_last_step_outputs(model, chunk, args.dump_outputs)

    # ---- roofline of the dominant kernel (fused int8 GEMM), from the events recorded inside the timed region ----
    gemm_ms = 0.0
    for s in range(args.steps):
        for (e0, e1) in events[s]:
            gemm_ms += hip.elapsed_ms(e0, e1)
    n_launch = args.steps * launches_per_step
    avg_launch_s = gemm_ms / 1e3 / n_launch
    ops_per_launch = 0.0
    for c in model.calls:
        ops_per_launch += 2.0 * chunk * c[5] * c[6] + 2.0 * chunk * c[5] * NUM_OUTLIERS
    ops_per_launch /= len(model.calls)
    achieved_tops = ops_per_launch / avg_launch_s / 1e12
    kernel_name = lib.mixq_debug_last_gemm_kernel().decode()   # what launch_gemm selected for the last (chunk, N, K)

    tokens_total = args.tokens * dp * args.steps
    value = tokens_total / elapsed
    ms_per_step = elapsed / args.steps * 1e3
    int8_gop_per_token = sum(2.0 * n * k for _, n, k in LLAMA2_7B["linears"]) * LLAMA2_7B["layers"] / 1e9

    traffic, traffic_source = None, None
    try:  # PMC-derived HBM-side bytes per GEMM launch of exactly this mix: rocprofv3 --pmc passes of THIS command
        # (tools/pmc_bench.sh), committed under profiles/ -- counters cannot be read from inside the run
        t = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        if t.get("chunk") == chunk and tp == 1 and args.variant == 0:
            import hashlib
            h = hashlib.sha256()
            for rel in t.get("kernel_sources", []):
                h.update(open(os.path.join(ROOT, rel), "rb").read())
            if t.get("kernel_sources_sha256") == h.hexdigest():
                traffic = t["bytes_per_launch"]
                traffic_source = "profiles/pmc_traffic.json (" + t.get("collected", "rocprofv3 --pmc, see profiles/README.md") + ")"
            else:  # the kernel changed since the counters were collected: do not replay another kernel's bytes
                traffic_source = ("none: profiles/pmc_traffic.json was collected on other kernel sources (sha-256 mismatch); "
                                  "re-run tools/pmc_bench.sh + tools/pmc_traffic_update.py")
    except Exception:
        traffic = None
    res = None
    if rank == 0:
        res = {
            "metric": "prefill_tokens_per_sec", "value": value, "unit": "tokens/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "median_ms_per_step": median_ms, "value_at_median": args.tokens * dp / (median_ms / 1e3),
            "higher_is_better": True,
            "scaling": "weak" if tp == 1 else "strong", "vs_baseline": None, "dtype": "int8",
            "data": "synthetic",
            "config": {"workload": "Llama-2-7B W8A8O16 (int8_mix) prefill, bs=512 seq=2048: all 96 MixQ linears "
                                   "(qkv 12288x4096, gate 11008x4096, proj 4096x11008; 32 layers), 128 outlier cols",
                       "tokens_per_step_per_replica": args.tokens, "m_chunk": chunk,
                       "parallelism": f"dp{dp}" + (f"xtp{tp}" if tp > 1 else "") + (
                           " (`value` = independent DP replicas, weak scaling; the tp = N row-sharded layout is `tp_tokens_per_s`)"
                           if world > 1 and tp == 1 else ""),
                       "int8_gop_per_token": int8_gop_per_token},
            "gemm_tops_end_to_end": value * int8_gop_per_token / 1e3 / world,
            "roofline": {"bound": "mfma", "achieved": achieved_tops, "peak": INT8_MFMA_PEAK_TOPS, "unit": "TOP/s",
                         "frac": achieved_tops / INT8_MFMA_PEAK_TOPS, "traffic": traffic,
                         "traffic_source": traffic_source,
                         "kernel": kernel_name,
                         "avg_launch_ms": avg_launch_s * 1e3, "launches": n_launch,
                         "ops_per_launch": ops_per_launch,
                         "gemm_share_of_wall": gemm_ms / 1e3 / elapsed},
            # the other launch of every call (fused quantise + outlier extract, HBM-bound): algorithmic bytes of SURVEY §8d
            # row a4 over the wall time NOT spent in the GEMM (so launch gaps count against it)
            "quantizer": (lambda qb, qt: {"bound": "hbm", "achieved": qb / qt / 1e9, "peak": 8000.0, "unit": "GB/s",
                                          "frac": qb / qt / 8e12, "avg_launch_ms": qt * 1e3,
                                          "bytes_per_launch": qb, "timing": "step wall time minus GEMM event time"})(
                sum(chunk * (3 * k + 2 + 2 * NUM_OUTLIERS) for _, _, k in LLAMA2_7B["linears"]) / 3.0,
                max(elapsed - gemm_ms / 1e3, 1e-9) / n_launch),
        }
        try:  # informational small-M points (HBM-bound end of the operator); never part of `value`
            if args.full and not args.no_small_m:
                res["small_m"] = small_m_points(lib, TensorDesc, dev, gen, st_ptr)
        except Exception as e:  # noqa: BLE001
            res["small_m"] = {"error": repr(e)}
        try:  # BASELINE configs[0] in one place, both routes (VERDICT r4 #1c), with the algorithmic bytes each is priced against
            sm_ = res.get("small_m", {})
            c0, c0n = sm_.get("config0_bs32_4096x4096"), sm_.get("config0_norm_fused")
            if c0 and "us_per_call" in c0:
                M0, N0, K0 = 32, 4096, 4096
                alg = N0 * K0 + 2 * M0 * K0 + 2 * M0 * N0 + 2 * N0 * (1 + NUM_OUTLIERS)   # W + A in + Out + sW + fp_weight
                res["config0"] = {
                    "workload": "single 4096 x 4096 MixQ linear, bs = 32, int8_mix (BASELINE configs[0])", "algorithmic_bytes": alg,
                    "hbm_floor_us": alg / 8e12 * 1e6,
                    "t_flavour_two_launches": {"us_warm": c0["us_per_call"], "us_cold": (c0.get("cold") or {}).get("us_per_call"),
                                               "hbm_frac_warm": alg / (c0["us_per_call"] * 1e-6) / 8e12,
                                               "with_weight_image_us_warm": (c0.get("with_weight_image") or {}).get("us_per_call"),
                                               "with_weight_image_us_cold": (c0.get("with_weight_image") or {}).get("cold_us_per_call"),
                                               "what": "mixq_enqueue as the plugin runs it: quantise + extract (launch 1), fused GEMM (launch 2)"},
                    "p_flavour_norm_fused": None if not c0n or "us_per_call" not in c0n else {
                        "us_marginal": c0n["us_per_call"], "hbm_frac": alg / (c0n["us_per_call"] * 1e-6) / 8e12,
                        "what": "the RMSNorm in front quantises in its own pass (mixq_rmsnorm_extract_quant): the linear is ONE launch"},
                    "floor_of_two_launches": "two launches of trivial kernels of these grids cost 5.5 us here, + the quantiser's 2 us of work (row load -> "
                                             "amax -> stores on 32 of 256 CUs) 7.2, + a 16-MB weight stream that cannot start before the second launch: "
                                             "8-8.5 us (profiles/r03_concurrent_probe.txt, r03_small_m_timeline.txt); the one-launch builds measured 11.8-15.9 us",
                    "cpu_reference_us": None}
        except Exception as e:  # noqa: BLE001
            res["config0"] = {"error": repr(e)}
        if world == 1 and args.full and not args.no_decode_step:
            try:
                res["decode_step"] = decode_step_points(lib, TensorDesc, model, dev, gen)
            except Exception as e:  # noqa: BLE001
                res["decode_step"] = {"error": repr(e)}
        if world == 1 and args.full and not args.no_decode_step:
            try:
                res["int4"] = int4_points(lib, model, dev, gen, res.get("decode_step"))
            except Exception as e:  # noqa: BLE001
                res["int4"] = {"error": repr(e)}
        if args.mid_m:  # informational mid-M points (short prefill: tiles do not fill the chip); never part of `value`.
            # Opt-in: its launches of the ping-pong kernel would otherwise dilute that kernel's average in a
            # rocprofv3 --stats summary of this command, which has to agree with roofline.avg_launch_ms.
            try:
                res["mid_m"] = mid_m_points(lib, TensorDesc, dev, gen, st_ptr)
            except Exception as e:  # noqa: BLE001
                res["mid_m"] = {"error": repr(e)}
        if world == 1 and args.full and not args.no_sweeps:
            # ---- chunk_sweep + configs (VERDICT r3 #1c): the same path off the whole-round sweet spot of the headline chunk, and
            # on the other two BASELINE models.  Each point: whole model, every linear its own weights, GEMM events inside the
            # timed region (roofline-style frac of the int8 peak); never part of `value`.
            def measure(m, tokens, steps, warmup):
                nch = max(tokens // m.chunk, 1)
                names = {}
                for (h, in_desc, out_desc, in_ptrs_list, out_ptrs, n_loc, K, outs, N) in m.calls[:len(m.spec["linears"])]:
                    assert lib.mixq_enqueue(h, in_desc, ctypes.byref(out_desc), in_ptrs_list[0], out_ptrs[0], m.ws_ptr, st_ptr) == 0
                    names[f"{n_loc}x{K}"] = lib.mixq_debug_last_gemm_kernel().decode().split(" ")[0]
                el, med, ev, launches = timed_run(m, None, steps, warmup, True, nch)
                g_ms = sum(hip.elapsed_ms(e0, e1) for st_ in ev for (e0, e1) in st_)
                ops = sum(2.0 * m.chunk * c[5] * (c[6] + NUM_OUTLIERS) for c in m.calls) / len(m.calls)
                avg = g_ms / 1e3 / (steps * launches)
                gop_tok = sum(2.0 * n * k for _, n, k in m.spec["linears"]) * m.spec["layers"] / 1e9
                return {"tokens_per_s": nch * m.chunk * steps / el, "ms_per_step": el / steps * 1e3, "tokens_per_step": nch * m.chunk,
                        "m_chunk": m.chunk, "steps": steps, "warmup": warmup, "gemm_frac_of_int8_peak": ops / avg / 1e12 / INT8_MFMA_PEAK_TOPS,
                        "gemm_avg_launch_ms": avg * 1e3, "gemm_share_of_wall": g_ms / 1e3 / el, "int8_gop_per_token": gop_tok,
                        "gemm_tops_end_to_end": nch * m.chunk * steps / el * gop_tok / 1e3, "kernels": names}
            try:
                sweep = {}
                for c in (8192, 16384):
                    if c < chunk and args.tokens % c == 0:
                        v = model.rechunked(c)
                        sweep[f"chunk_{c}"] = measure(v, min(args.tokens, 262144), 3, 1)
                        for call in v.calls:
                            lib.mixq_destroy(call[0])
                sweep[f"chunk_{chunk}"] = {"tokens_per_s": value, "ms_per_step": ms_per_step, "m_chunk": chunk,
                                           "gemm_frac_of_int8_peak": achieved_tops / INT8_MFMA_PEAK_TOPS, "note": "the main measurement"}
                sweep["what"] = ("Llama-2-7B, the same resident weights, driven in M-chunks of 8192 / 16384 tokens (256K tokens per step, "
                                 "3 timed steps after 1): engines with max_num_tokens below 65536")
                res["chunk_sweep"] = sweep
            except Exception as e:  # noqa: BLE001
                res["chunk_sweep"] = {"error": repr(e)}
            try:
                cfgs = {}
                model.close()
                model.acts, model.outs, model.workspace = {}, {}, None
                torch.cuda.empty_cache()
                for key, spec in (("qwen2_7b", QWEN2_7B), ("llama2_70b_tp8_shard", LLAMA2_70B_TP8)):
                    m2 = Model(lib, TensorDesc, parallel, dev, gen, chunk, 1, 0, spec=spec, nrot=4)
                    pt = measure(m2, args.tokens, 2, 1)
                    pt["workload"] = (f"{spec['name']}: {spec['layers']} layers x " +
                                      ", ".join(f"{nm} {n}x{k}" for nm, n, k in spec["linears"]) + f", bs x seq = {args.tokens} tokens")
                    if key == "llama2_70b_tp8_shard":
                        pt["note"] = ("ONE GPU's share of BASELINE config 5 (rows of W sharded 8 ways): tokens/s of the shard's GEMMs; the "
                                      "all-gather of the fp16 outputs is the `tp` object's business and needs 8 GPUs")
                    else:
                        if chunk > 16384:
                            v2 = m2.rechunked(16384)
                            pt["chunk_16384"] = measure(v2, min(args.tokens, 262144), 2, 1)
                            for call in v2.calls:
                                lib.mixq_destroy(call[0])
                    cfgs[key] = pt
                    m2.close()
                    del m2
                    torch.cuda.empty_cache()
                res["configs"] = cfgs
            except Exception as e:  # noqa: BLE001
                res["configs"] = {"error": repr(e)}
        if world == 1 and args.full and not args.no_cpu_baseline:
            try:
                res["cpu_baseline"] = cpu_baseline()
                if isinstance(res.get("config0"), dict) and "error" not in res["config0"]:
                    res["config0"]["cpu_reference_us"] = res["cpu_baseline"].get("config0_bs32_4096x4096", {}).get("us_per_call")
            except Exception as e:  # the checker failing must not hide the measurement
                res["cpu_baseline"] = {"value": None, "unit": "tokens/s", "cores": 0, "kind": "port",
                                       "sample": f"failed: {e}"}
    # ---- the north-star layout as a first-class object: rows of W sharded over ALL N ranks (tp = N) + one all-gather of
    # every fp16 output, the whole model, timed between the same barrier + synchronize brackets.  At N = 1 it is the main
    # measurement itself; otherwise it is a leg of its own, run by --full.  A watchdog emits the main result and exits if the
    # collective never comes back.
    tp_obj = None
    if world == 1 or tp == world:
        tp_obj = {"tp": tp, "world_size": world, "value": value, "unit": "tokens/s", "ms_per_step": ms_per_step,
                  "steps": args.steps, "scaling": "strong", "collective": None if world == 1 else "all_gather",
                  "note": "identical to the main measurement" + (" (no collective at tp = 1)" if world == 1 else "")}
    elif args.full and not args.no_tp_leg:
        import threading

        partial = {}   # what the leg has measured so far (the watchdog emits it instead of nothing)
        guard = None

        def bail():
            if rank == 0:
                if guard is not None:
                    guard.disarm()
                if partial.get("tp"):
                    res["tp"] = dict(partial["tp"], watchdog="the comparison of transports did not finish in time")
                else:
                    res["tp"] = {"tp": world, "error": "watchdog: the tp = N measurement did not finish in 300 s"}
                emit(res)
            os._exit(0)

        wd = threading.Timer(300.0, bail)   # (a healthy leg takes well under a minute; a hung collective must not cost the line)
        wd.daemon = True
        wd.start()
        if rank == 0:   # ... and neither must a leg that takes the process down (a GPU memory fault ends in the runtime's abort()): a child
            # process holds a copy of the line and writes it if this process disappears; the process itself still dies with its signal
            # (non-zero status: the driver sees that the leg crashed)
            guard = LineGuard(json_fd, (json.dumps(dict(res, tp={
                "tp": world, "error": "the benchmark process died inside the tp = N leg (see its exit status)"})) + "\n").encode())
        try:
            acts = model.acts
            model.close()
            del model
            torch.cuda.empty_cache()
            assert dist.get_world_size() == world, "RCCL world size"
            tmodel = Model(lib, TensorDesc, parallel, dev, gen, chunk, world, rank, acts=acts)
            tmodel.open_peer_transport(parallel, rank)
            t_el, t_med, _, _ = timed_run(tmodel, None, args.tp_steps, 1, False)
            timed_out = any(g.timed_out() for g in tmodel.gatherers.values())
            recv = sum((world - 1) * args.tokens * (c[8] // world) * 2 for c in tmodel.calls)
            tp_obj = {"tp": world, "world_size": world, "backend": backend,
                      "value": args.tokens * args.tp_steps / t_el, "unit": "tokens/s",
                      "ms_per_step": t_el / args.tp_steps * 1e3, "median_ms_per_step": t_med, "steps": args.tp_steps,
                      "warmup": 1, "scaling": "strong",
                      "collective": "one all-gather of the fp16 output per linear per chunk" + (
                          ", written by the GEMM's own stores as its M chunks retire" if tmodel.fused
                          else ", on a side stream (overlaps the next GEMM)"), "transport": tmodel.transport, "peer_wait_timed_out": timed_out,
                      "allgather_recv_GB_per_gpu_per_step": recv / 1e9,
                      "tokens_per_step": args.tokens}
            if timed_out:  # a stale gather is not a measurement
                tp_obj = {"tp": world, "world_size": world, "transport": tmodel.transport,
                          "error": "a peer-write wait timed out: the gathered outputs of this leg are not valid"}
            partial["tp"] = tp_obj
            # The other transports of the same layout, one timed step each (first contact with a multi-GPU node should say
            # which one wins there; every rank takes the same branches: the transport was agreed on above).  Order: from the
            # transport just measured down to plain RCCL; a failure here costs only this comparison.
            if not timed_out and not args.no_tp_alternatives:
                wd.cancel()
                wd = threading.Timer(240.0, bail)
                wd.daemon = True
                wd.start()
                alts = {}
                try:
                    keep = dict(tmodel.gatherers)
                    if tmodel.fused:
                        tmodel.fused = {}
                        a_el, _, _, _ = timed_run(tmodel, None, 1, 1, False)
                        alts["peer writes by a push kernel after the GEMM (mixq_tp_push_columns + flags)"] = {"ms_per_step": a_el * 1e3}
                    if tmodel.gatherers:
                        if any(g.timed_out() for g in tmodel.gatherers.values()):
                            raise RuntimeError("a peer-write wait timed out")
                        tmodel.gatherers = {}
                        a_el, _, _, _ = timed_run(tmodel, None, 1, 1, False)
                        alts["rccl all_gather_into_tensor + column placement"] = {"ms_per_step": a_el * 1e3}
                        tmodel.gatherers = keep
                except Exception as e:  # noqa: BLE001
                    alts["error"] = repr(e)
                tp_obj["alternatives_one_step_each"] = alts
            # ---- BASELINE configs[4]: Llama-2-70B W8A8O16, rows of W sharded over the N GPUs of the node + ONE all-gather of the fp16
            # output per linear (reference: tensorrt_llm plugin.py:97,155-156), bs x seq = the same tokens, 2 timed steps.
            # The transport is opened -- and self-tested against the push-kernel transport, as the 7B leg above -- on the 70B shapes.
            if not args.no_config5 and "error" not in tp_obj:
                wd.cancel()
                wd = threading.Timer(900.0, bail)
                wd.daemon = True
                wd.start()
                c5 = None
                try:
                    tmodel.close()
                    del tmodel
                    torch.cuda.empty_cache()
                    spec5 = dict(LLAMA2_70B, layers=args.config5_layers)
                    m5 = Model(lib, TensorDesc, parallel, dev, gen, chunk, world, rank, spec=spec5, nrot=2)
                    m5.open_peer_transport(parallel, rank)
                    c_el, c_med, _, _ = timed_run(m5, None, 2, 1, False)
                    c_to = any(g.timed_out() for g in m5.gatherers.values())
                    recv5 = sum((world - 1) * args.tokens * (c[8] // world) * 2 for c in m5.calls)
                    gop5 = sum(2.0 * n * k for _, n, k in spec5["linears"]) * spec5["layers"] / 1e9
                    c5 = {"tp": world, "world_size": world, "value": args.tokens * 2 / c_el, "unit": "tokens/s", "ms_per_step": c_el / 2 * 1e3,
                          "median_ms_per_step": c_med, "steps": 2, "warmup": 1, "scaling": "strong", "layers": spec5["layers"],
                          "workload": (f"{spec5['name']}: {spec5['layers']} layers x " + ", ".join(f"{nm} {n}x{k}" for nm, n, k in spec5["linears"]) +
                                       f", rows of W sharded {world} ways, bs x seq = {args.tokens} tokens"),
                          "collective": "one all-gather of the fp16 output per linear per chunk", "transport": m5.transport,
                          "transport_self_tested": "every gatherer against a known pattern, the fused store path against operator + push (Model.open_peer_transport)",
                          "peer_wait_timed_out": c_to, "allgather_recv_GB_per_gpu_per_step": recv5 / 1e9, "int8_gop_per_token": gop5,
                          "int8_tops_all_gpus": args.tokens * 2 / c_el * gop5 / 1e3, "tokens_per_step": args.tokens}
                    if c_to:
                        c5 = {"tp": world, "transport": m5.transport, "error": "a peer-write wait timed out: the gathered outputs of this leg are not valid"}
                    m5.close()
                    del m5
                except Exception as e:  # noqa: BLE001 -- costs only this object
                    c5 = {"tp": world, "error": repr(e)}
                if rank == 0:
                    res.setdefault("configs", {})[f"llama2_70b_tp{world}"] = c5
        except Exception as e:  # noqa: BLE001 -- the main measurement must survive
            tp_obj = {"tp": world, "error": repr(e)}
        wd.cancel()
        if guard is not None:
            guard.disarm()
    if rank == 0 and tp_obj is not None:
        res["tp"] = tp_obj
    if rank == 0 and world > 1:
        # `value` is what config.parallelism says; the north-star layout (rows of W sharded over all N GPUs + one all-gather of
        # the fp16 output) is reported next to it at the top level, so that a scaling curve can be read for EITHER layout
        res["tp_tokens_per_s"] = (tp_obj or {}).get("value")
        res["value_layout"] = (f"{dp} data-parallel replica(s)" + (f" x tp{tp}" if tp > 1 else "") +
                               " -- no data-path collective at tp = 1; `tp_tokens_per_s` = the row-sharded layout (tp = N, "
                               "strong scaling: the same tokens, W sharded N ways, one all-gather per linear; null where "
                               "that leg did not run: --full runs it)")
    if rank == 0:
        emit(res)   # the line first: a teardown that hangs (a rank that died inside the tp = N leg) must not cost it
    if world > 1:
        import threading
        td = threading.Timer(60.0, lambda: os._exit(0))
        td.daemon = True
        td.start()
        try:
            dist.barrier()
            dist.destroy_process_group()
        except Exception:  # noqa: BLE001 -- nothing left to report
            pass
        td.cancel()


if __name__ == "__main__":
    main()
