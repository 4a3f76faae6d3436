// Fused W8A8O16 GEMM for gfx950 (MI355X):  Out = fp16( float(qA.W^T) * (sW[n]*sA[m]) + fp16(fpA.fpW^T) )
//
// Replaces (reference, CUDA):
//   kernel/i8gemm.cu:151-194 int8FusedDequantizeCUDA -> CUTLASS symmetric::GemmDequant
//       (kernel/symmetric/gemm/kernel/gemm_dequant.h:225-380 main loop,
//        kernel/symmetric/epilogue/thread/linear_combination_dequant.h:120-160 epilogue functor)
//   TsinghuaMixQPlugin.cpp:122-161 gemmfp16 (cuBLAS fp16 side GEMM over the 128 outlier columns)
//   TsinghuaMixQPlugin.cpp:36-77   gemm (cuBLAS s8 x s8 -> s32, the unfused route)
// in ONE launch: Out is written once and never re-read (the reference writes it, re-reads it as C and writes it again).
//
// CDNA4 mapping
//   * v_mfma_i32_32x32x32_i8, operands swapped: MFMA "A" = W rows (n), MFMA "B" = qA rows (m).  The 32x32 C/D layout
//     then gives every lane 4 consecutive n for one m per accumulator quad -> 8-byte fp16 stores, and the int32
//     accumulators are bit-exact by construction (integer adds commute).
//   * K is consumed in 128-byte slices per row.  Both operand tiles are staged global -> LDS with 16-byte
//     global_load_lds (no VGPR round trip).  The LDS image is lane-linear (hardware rule), so the bank-conflict
//     swizzle is applied to the per-lane SOURCE address and mirrored on the ds_read_b128 side:
//         16-B slot of row r = chunk ^ ((r >> 1) & 7)       (128-B rows: conflict-free for ds_read_b128's 16-lane groups)
//   * double-buffered LDS, one barrier per K slice: loads of slice t+1 are in flight while slice t is multiplied.
//   * The fp16 outlier side GEMM (O <= 128 columns) runs after the int8 main loop on v_mfma_f32_32x32x16_f16, tile by
//     tile, re-using the main loop's LDS; its fp32 sum is rounded to fp16 first (the reference materialises it in fp16
//     through a separate cuBLAS call) and enters the dequant FMA as the addend.
//   * 1-D grid, XCD-aware remap (block b runs on XCD b % 8): each XCD owns a contiguous run of tiles, walked in groups
//     of GROUP_M row-tiles so that co-resident workgroups share W / qA panels in that XCD's private L2.
#include "mixq_device.h"
#include "mixq_launch.h"
#include <atomic>
#include <cstdio>
#include <cstdlib>

namespace mixq {

constexpr int KSLICE = 128;  // bytes of K per LDS row (int8 elements)
constexpr int OSLICE = 256;  // bytes per LDS row in the outlier phase (128 fp16)
constexpr int GROUP_M = 4;

// KG > 1: in-workgroup split-K.  KG groups of WAVES_M x WAVES_N waves work on the same output tile, group g on the K
// slices g, g + KG, ... with its own LDS stages; the partial accumulators meet in LDS and group 0 runs the epilogue.
// (Small-N problems have too few tiles for the chip, and an LDS-DMA instruction costs the issuing wave 100-200 cycles:
// more waves per tile is what raises the operand stream, and no global scratch is needed.)
// PREO: the outlier operands of the epilogue get their own LDS region behind the stages and are copied there at kernel
// start, under the main loop, instead of after it (used by the one-workgroup-per-CU split-K configurations, where the
// extra (BM + BN) x 256 bytes of LDS cost no occupancy and the kernel is a chain of latencies).
// XSP: K is split over XS = p.xsplit WORKGROUPS per tile as well (consecutive blocks), for problems with so few tiles that most
// CUs would otherwise watch a few of them stream K.  Every workgroup parks its partial tile (BM x BN int32: 8-16 KiB)
// in p.splitk_ws with write-through stores and counts itself in; the one that arrives LAST adds the others' parked
// sums and runs the epilogue, the others are gone by then -- nobody ever waits, so there is nothing to dead-lock.
// Hand-over accesses are relaxed agent-scope atomics as in gemm_pp_kernels.hip (no fences); the counter of a tile lives
// in the first kSplitkWordsBytes of the scratch and is left zero.  Same int32 sums, same bits.
// ADMA (round 5): the slice copies are issued in ASM form (glds16_vaddr: not counted by the compiler's s_waitcnt insertion), so that
// NSTAGE - 1 slices really are in flight behind the explicit `s_waitcnt vmcnt(n)` of the loop -- with the builtin copies hipcc
// drains everything in front of every barrier and the loop runs ONE slice ahead whatever NSTAGE says (notebook R3.16: no effect
// where 2-5 workgroups share a CU and cover each other's round trips).  It is the regime with ONE workgroup per CU that needs it:
// mid-M problems (129..512 rows) whose 128 x 128 tiles, split over K, put exactly one workgroup on every CU -- there a slice's
// ~1 us L2 / HBM round trip, not its ~0.3 us of MFMA work, set the pace of the two-slice loop.
template <int BM, int BN, int WAVES_M, int WAVES_N, int EPI, int NSTAGE = 2, int KG = 1, bool PREO = false, bool XSP = false,
          bool ADMA = false>
__global__ __launch_bounds__(WAVES_M* WAVES_N* KG * 64) void gemm_w8a8o16_kernel(const GemmParams p)
{
    const int XS = XSP ? p.xsplit : 1; // workgroups per tile (2 / 4 / 8 / 16: index arithmetic only, so a run-time value)
    constexpr int NWAVES = WAVES_M * WAVES_N;
    constexpr int T = NWAVES * 64;      // threads of one K group
    constexpr int TT = T * KG;          // threads of the workgroup
    constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int X_BYTES = BN * KSLICE, Y_BYTES = BM * KSLICE;
    constexpr int STAGE_BYTES = X_BYTES + Y_BYTES;
    constexpr int XL = BN * 8 / T, YL = BM * 8 / T;       // 16-B loads per thread per K slice
    static_assert(BN * 8 % T == 0 && BM * 8 % T == 0, "tile rows must split evenly over the block");
    static_assert(WM % 32 == 0 && WN % 32 == 0, "wave tile must be a multiple of the 32x32 MFMA");
    static_assert((BM + BN) * OSLICE <= KG * NSTAGE * STAGE_BYTES, "outlier tiles must fit the main-loop LDS");
    static_assert((KG - 1) * NWAVES * TN * TM * 4096 <= KG * NSTAGE * STAGE_BYTES, "partial accumulators must fit");
    static_assert(BN * 16 % TT == 0 && BM * 16 % TT == 0, "outlier tile rows must split evenly over the block");
    static_assert(NSTAGE >= 2 && NSTAGE <= 8, "2..8 LDS stages");

    extern __shared__ __attribute__((aligned(16))) char smem_all[];

    const int tid_all = threadIdx.x;
    const int wave_all = __builtin_amdgcn_readfirstlane(tid_all >> 6);
    const int group = KG > 1 ? wave_all / NWAVES : 0;
    const int tid = KG > 1 ? tid_all - group * T : tid_all;   // thread inside its K group
    const int lane = tid & 63;
    const int wave = KG > 1 ? wave_all - group * NWAVES : wave_all;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    char* const smem = smem_all + group * (NSTAGE * STAGE_BYTES); // this group's stages

    // ---- block -> tile mapping (XCD-aware, grouped) ------------------------------------------------
    const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
    const int nwg = tiles_m * tiles_n;
    int t_lin;
    const int xrank = XSP ? (int)blockIdx.x % XS : 0; // which part of K this workgroup multiplies
    {
        const int bid = XSP ? (int)blockIdx.x / XS : (int)blockIdx.x, q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
        t_lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3); // bijective for any nwg
    }
    int tile_m, tile_n;
    {
        const int per_group = GROUP_M * tiles_n;
        const int g = t_lin / per_group, first_m = g * GROUP_M;
        const int gsz = min(tiles_m - first_m, GROUP_M);
        const int within = t_lin - g * per_group;
        tile_m = first_m + within % gsz;
        tile_n = within / gsz;
    }
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    // ---- per-thread global source offsets for the staging loads ------------------------------------
    // chunk index c = i*T + tid : LDS row = c/8, LDS slot = c%8 (linear image), source chunk = slot ^ ((row>>1)&7)
    const int64_t K = p.K;
    const char* xsrc[XL];
    const char* ysrc[YL];
    int xkoff, ykoff; // byte offset of this thread's source chunk inside the 128-B slice (same for every i)
    {
        const int slot = tid & 7;
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const int row = (i * T + tid) >> 3;
            const int grow = min(n0 + row, p.N - 1); // clamp: rows past N are loaded but never stored
            xsrc[i] = reinterpret_cast<const char*>(p.B) + (int64_t)grow * K + ((slot ^ ((row >> 1) & 7)) << 4);
        }
        xkoff = (slot ^ (((tid >> 3) >> 1) & 7)) << 4; // (row>>1)&7 does not depend on i (T/8 is a multiple of 16)
#pragma unroll
        for (int i = 0; i < YL; ++i) {
            const int row = (i * T + tid) >> 3;
            const int grow = min(m0 + row, p.M - 1);
            ysrc[i] = reinterpret_cast<const char*>(p.A) + (int64_t)grow * K + ((slot ^ ((row >> 1) & 7)) << 4);
        }
        ykoff = xkoff;
    }
    static_assert((T / 8) % 16 == 0, "row swizzle term must be i-invariant");

    const int nk_all = (p.K + KSLICE - 1) / KSLICE;
    const int kbeg = XSP ? nk_all * xrank / XS : 0;                 // this workgroup's slices: [kbeg, kbeg + nk)
    const int nk = (XSP ? nk_all * (xrank + 1) / XS : nk_all) - kbeg;
    const bool ktail = (p.K % KSLICE) != 0;

    // fpW / fpA tiles -> LDS (256-B rows, slot = chunk ^ (row & 15)); all threads of the workgroup take part
    const bool has_outliers = (EPI != EPI_INT32) && p.O > 0;
    char* const osmem = smem_all + (PREO ? KG * NSTAGE * STAGE_BYTES : 0);
    auto stage_outliers = [&]() __attribute__((always_inline)) {
        constexpr int OXL = BN * 16 / TT, OYL = BM * 16 / TT;
        const int obytes = p.O * 2; // valid bytes per row (O % 8 == 0)
        const int slot = tid_all & 15;
#pragma unroll
        for (int i = 0; i < OXL; ++i) {
            const int row = (i * TT + tid_all) >> 4;
            const int c = (slot ^ (row & 15)) << 4;
            const int grow = min(n0 + row, p.N - 1);
            const char* s2 = reinterpret_cast<const char*>(p.fpW) + (int64_t)grow * obytes + c;
            if (c >= obytes) s2 = static_cast<const char*>(p.zeros);
            glds16(s2, osmem + (i * TT + wave_all * 64) * 16);
        }
#pragma unroll
        for (int i = 0; i < OYL; ++i) {
            const int row = (i * TT + tid_all) >> 4;
            const int c = (slot ^ (row & 15)) << 4;
            const int grow = min(m0 + row, p.M - 1);
            const char* s2 = reinterpret_cast<const char*>(p.fpA) + (int64_t)grow * obytes + c;
            if (c >= obytes) s2 = static_cast<const char*>(p.zeros);
            glds16(s2, osmem + BN * OSLICE + (i * TT + wave_all * 64) * 16);
        }
    };
    if (PREO && has_outliers) stage_outliers(); // older than every slice copy: retired by the loop's first wait

    const unsigned lds_group0 = (unsigned)(size_t)(MIXQ_LDS_PTR(smem)); // LDS byte address of this group's stages (ADMA)
    const bool ntw = (p.flags & 2) != 0; // (launch_cfg: one tile row reads a weight of 32 MiB and more -- each of its lines exactly once)
    auto stage = [&](int buf, int kt) {
        char* xb = smem + buf * STAGE_BYTES;
        char* yb = xb + X_BYTES;
        const int64_t kbyte = (int64_t)(kbeg + kt) * KSLICE;
        const bool last_partial = ktail && (kbeg + kt == nk_all - 1);
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const char* s = xsrc[i] + kbyte;
            if (last_partial && (kbyte + xkoff >= K)) s = static_cast<const char*>(p.zeros);
            if (ADMA) {
                if (ntw) glds16_vaddr_nt(s, lds_group0 + buf * STAGE_BYTES + (i * T + wave * 64) * 16);
                else glds16_vaddr(s, lds_group0 + buf * STAGE_BYTES + (i * T + wave * 64) * 16);
            } else {
                if (ntw) glds16_nt(s, xb + (i * T + wave * 64) * 16);
                else glds16(s, xb + (i * T + wave * 64) * 16);
            }
        }
#pragma unroll
        for (int i = 0; i < YL; ++i) {
            const char* s = ysrc[i] + kbyte;
            if (last_partial && (kbyte + ykoff >= K)) s = static_cast<const char*>(p.zeros);
            if (ADMA) glds16_vaddr(s, lds_group0 + buf * STAGE_BYTES + X_BYTES + (i * T + wave * 64) * 16);
            else glds16(s, yb + (i * T + wave * 64) * 16);
        }
    };

    // ---- LDS read offsets for the MFMA fragments -----------------------------------------------------
    // lane l supplies row (l & 31) and the 16 K-bytes [(l >> 5) * 16, +16) of each 32-byte MFMA k-step.
    const int lr = lane & 31, lh = lane >> 5;
    const int sw = (lr >> 1) & 7;
    int koff[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) koff[ks] = ((ks * 2 + lh) ^ sw) << 4;
    const int xrow_off = (wn * WN + lr) * KSLICE;
    const int yrow_off = X_BYTES + (wm * WM + lr) * KSLICE;

    v16i acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;

    // ---- main loop -------------------------------------------------------------------------------------
    // NSTAGE LDS buffers, slices kt+1 .. kt+NSTAGE-1 in flight while slice kt is multiplied.  Small tiles are bound by
    // the HBM round trip of each slice, not by MFMA work: the deeper the prefetch, the more bytes in flight per CU.
    // (Round 3, read off the ISA: with the BUILTIN copies used here hipcc puts `s_waitcnt vmcnt(0)` in front of every
    //  __syncthreads() -- a pending LDS-DMA copy is a pending LDS write to the fence -- so in steady state only the slice issued
    //  one iteration ago is in flight; NSTAGE > 2 buys the first NSTAGE - 1 slices up front.  The asm-form copies
    //  (glds16_vaddr, explicit waits only) that really keep NSTAGE - 1 slices in flight measured +-1..3 % on 30 shapes from 48
    //  to 512 tokens (profiles/r03_tile_kernel_asm_dma_ab.txt): several workgroups per CU already cover the round trip.  Left
    //  as it was.)
    // (group g owns slices g, g + KG, ...: its it-th slice is kt = it * KG + g; every group runs the same number of
    //  iterations because the barrier is workgroup-wide)
#pragma unroll
    for (int s0 = 0; s0 < NSTAGE - 1; ++s0)
        if (s0 * KG + group < nk) stage(s0, s0 * KG + group);
    const int nit = (nk + KG - 1) / KG;
    const bool late_issue = ADMA && KG == 1 && NWAVES >= 8 && wave >= NWAVES / 2 && !(p.flags & 1);
    for (int it = 0; it < nit; ++it) {
        const int kt = it * KG + group;
        // copies complete in order: at most the (NSTAGE-2) younger slices may still be in flight once slice kt landed
        if (NSTAGE > 2 && (it + NSTAGE - 2) * KG + group < nk)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSTAGE - 2) * (XL + YL)) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads(); // slice kt has landed for every wave; everyone is done reading the previous slice's buffer
        // (all copies of slice it + NSTAGE - 1 at once, as early as possible: spreading them over the four k-steps -- which
        //  pays in the fpA_intB wide form -- measured +4..+8 % here on wide / long-K shapes, -3 % on 4096 x 4096: round 2)
        // ADMA with two waves per SIMD: the waves of the second half issue their copies AFTER their MFMAs, so that on every SIMD one
        // wave multiplies while the other sits in the 100..200-cycle issue stall of each LDS-DMA instruction (the poor man's ping-pong;
        // same counts per wave, so the vmcnt bookkeeping above is unchanged; the target buffer was last read one barrier ago)
        const bool do_stage = (it + NSTAGE - 1) * KG + group < nk;
        if (do_stage && !late_issue) stage((it + NSTAGE - 1) % NSTAGE, (it + NSTAGE - 1) * KG + group);
        if (KG > 1 && kt >= nk) continue; // (K groups past the end only keep the barrier count)
        const char* base = smem + (it % NSTAGE) * STAGE_BYTES;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            v4i xf[TN], yf[TM];
#pragma unroll
            for (int i = 0; i < TN; ++i)
                xf[i] = *reinterpret_cast<const v4i*>(base + xrow_off + i * 32 * KSLICE + koff[ks]);
#pragma unroll
            for (int j = 0; j < TM; ++j)
                yf[j] = *reinterpret_cast<const v4i*>(base + yrow_off + j * 32 * KSLICE + koff[ks]);
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(xf[i], yf[j], acc[i][j], 0, 0, 0);
        }
        if (do_stage && late_issue) {
            __builtin_amdgcn_sched_barrier(0); // (the copies stay behind the slice's MFMAs)
            stage((it + NSTAGE - 1) % NSTAGE, (it + NSTAGE - 1) * KG + group);
        }
    }

    // ---- (round 6) the scales the epilogue multiplies by are requested HERE, under the hand-overs and the outlier staging below: the store
    // loop used to load sA[m] and sW[n .. n + 3] right where it needed them -- a dependent L2 round trip in front of every tile's first store
    // (the mid-M kernel's timeline priced the same pattern at 1.3 us per tile, profiles/r06_mid_v1_timeline.txt).  Clamped: rows / columns past
    // the edge are never stored.
    float sa_pre[TM];
    uint2 sw_pre[TN][4], bias_pre[TN][4]; // (bias_pre: EPI_DEQUANT_BIAS only, requested with the weight scales)
    if (EPI != EPI_INT32) {
#pragma unroll
        for (int j = 0; j < TM; ++j) sa_pre[j] = o2f<epi_bf16(EPI)>(p.sA[min(m0 + wm * WM + j * 32 + lr, p.M - 1)]);
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int nb = min(n0 + wn * WN + i * 32 + 4 * lh + 8 * g, p.N - 4);
                sw_pre[i][g] = *reinterpret_cast<const uint2*>(p.sW + nb);
                if constexpr (epi_bias(EPI)) bias_pre[i][g] = *reinterpret_cast<const uint2*>(p.bias + nb);
            }
    }

    // ---- in-workgroup split-K: partial accumulators of groups 1.. -> LDS -> added by group 0 ----------
    if (KG > 1) {
        __syncthreads(); // main-loop LDS is dead
        if (group > 0) {
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j) {
                    char* r = smem_all + (((group - 1) * NWAVES + wave) * (TN * TM) + i * TM + j) * 4096 + lane * 16;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        *reinterpret_cast<v4i*>(r + q * 1024) =
                            v4i{acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                }
        }
        __syncthreads();
        if (group == 0) {
#pragma unroll
            for (int g2 = 1; g2 < KG; ++g2)
#pragma unroll
                for (int i = 0; i < TN; ++i)
#pragma unroll
                    for (int j = 0; j < TM; ++j) {
                        const char* r = smem_all + (((g2 - 1) * NWAVES + wave) * (TN * TM) + i * TM + j) * 4096 + lane * 16;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const v4i t4 = *reinterpret_cast<const v4i*>(r + q * 1024);
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[i][j][4 * q + e] += t4[e];
                        }
                    }
        }
    }

    // ---- K split over workgroups: park, count in, and only the last one to arrive goes on ----------------------------
    if (XSP) {
        // (the main-loop stages and the partial accumulators in LDS are dead by now: their first word carries the count;
        //  a static __shared__ variable would push the 64x64 form past the 160 KiB it already fills)
        volatile unsigned& arrived_s = *reinterpret_cast<volatile unsigned*>(smem_all);
        constexpr int TILE_DW = TN * TM * 16 * T; // dwords of one parked tile: [n tile][m tile][16][T threads of group 0]
        unsigned* const counter = static_cast<unsigned*>(p.splitk_ws) + t_lin;
        int* const slots = reinterpret_cast<int*>(static_cast<char*>(p.splitk_ws) + kSplitkWordsBytes) +
                           (size_t)t_lin * XS * TILE_DW;
        if (group == 0) {
            int* const mine = slots + (size_t)xrank * TILE_DW + tid;
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        __hip_atomic_store(mine + ((i * TM + j) * 16 + e) * T, acc[i][j][e], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // every write-through acknowledged
        }
        __syncthreads();
        if (tid_all == 0)
            arrived_s = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (arrived_s != (unsigned)(XS - 1)) return; // not the last one: done (the whole workgroup leaves)
        if (tid_all == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // re-armed
        if (group == 0) {
            for (int o = 1; o < XS; ++o) { // the other XS - 1 parts, in a rotation that depends on nothing but the rank
                const int* const theirs = slots + (size_t)((xrank + o) % XS) * TILE_DW + tid;
#pragma unroll
                for (int i = 0; i < TN; ++i)
#pragma unroll
                    for (int j = 0; j < TM; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e)
                            acc[i][j][e] += __hip_atomic_load(theirs + ((i * TM + j) * 16 + e) * T, __ATOMIC_RELAXED,
                                                              __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }

    // ---- outlier side GEMM operands (unless they were copied at kernel start) ----------------------------------------
    if (has_outliers && !PREO) {
        __syncthreads(); // main-loop LDS (and the partial accumulators) are dead
        stage_outliers();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if (has_outliers && PREO && KG == 1) __syncthreads(); // (KG > 1: the split-K hand-over above already synchronised)
    if (KG > 1 && group > 0) return; // (no barrier below this point)

    // ---- epilogue, one 32x32 tile at a time -----------------------------------------------------------
    const int osteps = has_outliers ? (p.O + 15) / 16 : 0;
#pragma unroll
    for (int i = 0; i < TN; ++i) {
#pragma unroll
        for (int j = 0; j < TM; ++j) {
            const int m = m0 + wm * WM + j * 32 + lr;
            const int nb0 = n0 + wn * WN + i * 32 + 4 * lh;
            if (EPI == EPI_INT32) {
                if (m < p.M) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int nb = nb0 + 8 * g;
                        if (nb < p.N) {
                            v4i o = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                            *reinterpret_cast<v4i*>(static_cast<int32_t*>(p.D) + (int64_t)m * p.N + nb) = o;
                        }
                    }
                }
                continue;
            }
            v16f P;
#pragma unroll
            for (int e = 0; e < 16; ++e) P[e] = 0.f;
            if (has_outliers) {
                const char* xo = osmem + (wn * WN + i * 32 + lr) * OSLICE;
                const char* yo = osmem + BN * OSLICE + (wm * WM + j * 32 + lr) * OSLICE;
                const int sw16 = lr & 15;
                for (int ks = 0; ks < osteps; ++ks) {
                    const int off = ((ks * 2 + lh) ^ sw16) << 4;
                    v8h xf = *reinterpret_cast<const v8h*>(xo + off);
                    v8h yf = *reinterpret_cast<const v8h*>(yo + off);
                    P = mfma32_o<epi_bf16(EPI)>(xf, yf, P);
                }
            }
            if constexpr (epi_gate_up(EPI)) { // merged gate / up: this lane's quads 2 gp and 2 gp + 1 are the gate and the up columns of output quad gp
                constexpr bool BF = epi_bf16(EPI);
                if (m < p.M) {
#pragma unroll
                    for (int gp = 0; gp < 2; ++gp) {
                        const int nb = nb0 + 16 * gp; // (GEMM column of the gate quad; N % 32 == 0: a 32-column block is inside or outside as a whole)
                        if (nb < p.N) {
                            const uint2 sg = sw_pre[i][2 * gp], su = sw_pre[i][2 * gp + 1];
                            const uint16_t sgh[4] = {(uint16_t)(sg.x & 0xffffu), (uint16_t)(sg.x >> 16), (uint16_t)(sg.y & 0xffffu), (uint16_t)(sg.y >> 16)};
                            const uint16_t suh[4] = {(uint16_t)(su.x & 0xffffu), (uint16_t)(su.x >> 16), (uint16_t)(su.y & 0xffffu), (uint16_t)(su.y >> 16)};
                            uint16_t oh[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float cg = has_outliers ? o2f<BF>(f2o_bits_of_f32_result<BF>(P[8 * gp + e])) : 0.f;
                                const float cu = has_outliers ? o2f<BF>(f2o_bits_of_f32_result<BF>(P[8 * gp + 4 + e])) : 0.f;
                                const float vg = __builtin_fmaf((float)acc[i][j][8 * gp + e], h2f(sgh[e]) * sa_pre[j], cg);
                                const float vu = __builtin_fmaf((float)acc[i][j][8 * gp + 4 + e], h2f(suh[e]) * sa_pre[j], cu);
                                oh[e] = gate_up_bits<BF>(vg, vu);
                            }
                            uint2 o;
                            o.x = (unsigned)oh[0] | ((unsigned)oh[1] << 16);
                            o.y = (unsigned)oh[2] | ((unsigned)oh[3] << 16);
                            *reinterpret_cast<uint2*>(static_cast<uint16_t*>(p.D) + (int64_t)m * p.n_out + gate_up_col(nb)) = o;
                        }
                    }
                }
                continue;
            }
            if (m < p.M) {
                const float sa = sa_pre[j];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int nb = nb0 + 8 * g;
                    if (nb < p.N) {
                        const uint2 swb = sw_pre[i][g];
                        const uint16_t swh[4] = {(uint16_t)(swb.x & 0xffffu), (uint16_t)(swb.x >> 16),
                                                 (uint16_t)(swb.y & 0xffffu), (uint16_t)(swb.y >> 16)};
                        uint16_t yh[4] = {0, 0, 0, 0};
                        if (p.Y != nullptr) {
                            const uint2 yb = *reinterpret_cast<const uint2*>(p.Y + (int64_t)m * p.N + nb);
                            yh[0] = (uint16_t)(yb.x & 0xffffu), yh[1] = (uint16_t)(yb.x >> 16);
                            yh[2] = (uint16_t)(yb.y & 0xffffu), yh[3] = (uint16_t)(yb.y >> 16);
                        }
                        uint16_t oh[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            // addend: the fp16-rounded outlier product (cuBLAS writes fp16) or the caller's y
                            constexpr bool BF = epi_bf16(EPI); // (bf16 call: P and the result in bf16, no addend)
                            const float c = has_outliers ? o2f<BF>(f2o_bits_of_f32_result<BF>(P[4 * g + e])) : h2f(yh[e]);
                            float v = __builtin_fmaf((float)acc[i][j][4 * g + e], h2f(swh[e]) * sa, c);
                            if (epi_has_silu(EPI)) v = silu_f32(v);
                            oh[e] = f2o_bits_of_f32_result<BF>(v);
                        }
                        if (epi_has_mul(EPI)) { // gate * up: one fp16 (bf16) multiply of the rounded result
                            const uint2 mb = *reinterpret_cast<const uint2*>(p.Mul + (int64_t)m * p.N + nb);
                            const uint16_t mh[4] = {(uint16_t)(mb.x & 0xffffu), (uint16_t)(mb.x >> 16),
                                                    (uint16_t)(mb.y & 0xffffu), (uint16_t)(mb.y >> 16)};
#pragma unroll
                            for (int e = 0; e < 4; ++e) oh[e] = omul_bits<epi_bf16(EPI)>(oh[e], mh[e]);
                        }
                        if constexpr (epi_bias(EPI)) { // the layer's bias: one fp16 (bf16) add of the rounded result
                            const uint2 bb = bias_pre[i][g];
                            const uint16_t bh[4] = {(uint16_t)(bb.x & 0xffffu), (uint16_t)(bb.x >> 16), (uint16_t)(bb.y & 0xffffu),
                                                    (uint16_t)(bb.y >> 16)};
#pragma unroll
                            for (int e = 0; e < 4; ++e) oh[e] = oadd_bits<epi_bf16(EPI)>(oh[e], bh[e]);
                        }
                        uint2 o;
                        o.x = (unsigned)oh[0] | ((unsigned)oh[1] << 16);
                        o.y = (unsigned)oh[2] | ((unsigned)oh[3] << 16);
                        *reinterpret_cast<uint2*>(static_cast<uint16_t*>(p.D) + (int64_t)m * p.N + nb) = o;
                    }
                }
            }
        }
    }
}

static std::atomic<int> g_tile_nt{0}; // 0 by rule (default) | 1 never | 2 whenever one tile row
template <int BM, int BN, int WAVES_M, int WAVES_N, int EPI, int NSTAGE = 2, int KG = 1, bool PREO = false, bool XSP = false,
          bool ADMA = false>
static hipError_t launch_cfg(const GemmParams& p, hipStream_t st)
{
    constexpr int T = WAVES_M * WAVES_N * KG * 64;
    constexpr size_t lds = (size_t)KG * NSTAGE * (size_t)(BM + BN) * KSLICE + (PREO ? (size_t)(BM + BN) * OSLICE : 0);
    static_assert(lds <= 160 * 1024, "LDS budget");
    auto kern = gemm_w8a8o16_kernel<BM, BN, WAVES_M, WAVES_N, EPI, NSTAGE, KG, PREO, XSP, ADMA>;
    static DeviceOnce once;
    if (hipError_t e = ensure_dynamic_lds(kern, lds, once); e != hipSuccess) return e;
    const int tiles = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
    GemmParams q = p;
    // one tile row: every weight line is read by exactly one workgroup -> non-temporal copies for weights of 32 MiB and more (knob 1290 / 1291 / 1292:
    // by that rule / never / whenever there is one tile row).  Operator us cold at 64 rows, plain -> non-temporal: 12288 x 4096 23.1 -> 22.1, 11008 x 4096
    // 23.0 -> 21.8, 18944 x 3584 28.4 -> 26.9, 3584 x 18944 33.4 -> 32.1; deep form at 97..128 rows -1 %; warm loops over one layer +5..+12 % by construction
    // (profiles/r05_tile_nontemporal.txt)
    const int ntm = g_tile_nt.load(std::memory_order_relaxed);
    if (p.M <= BM && EPI != EPI_INT32 && (ntm == 2 || (ntm == 0 && (int64_t)p.N * p.K >= ((int64_t)32 << 20)))) q.flags |= 2;
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles * (XSP ? p.xsplit : 1))), dim3(T), lds, st, q);
    return hipGetLastError();
}

void set_tile_nt(int mode) { g_tile_nt.store(mode); }

// ---- mid-M "deep" form: 128 x 128 tiles, 4 LDS stages really in flight (ADMA), plan.xs workgroups per tile along K (the rules: gemm_plan.hip) ----
template <int EPI>
static hipError_t launch_deep_epi(const GemmParams& p, const GemmPlan& pl, hipStream_t st)
{
    GemmParams q = p;
    q.xsplit = pl.xs;
    q.flags = pl.deep_early ? 1 : 0;
    if (pl.deep_build == 3) { // round 6: copy-only waves, two slices per barrier (gemm_mid_kernels.hip)
        q.flags = 0;
        return launch_gemm_mid(q, EPI, pl, st);
    }
    if (pl.deep_build == 2) { // five stages = the whole 160 KiB of LDS: four slices in flight
        if (pl.xs > 1) return launch_cfg<128, 128, 2, 4, EPI, 5, 1, false, true, true>(q, st);
        return launch_cfg<128, 128, 2, 4, EPI, 5, 1, false, false, true>(q, st);
    }
    if (pl.deep_build) {
        if (pl.xs > 1) return launch_cfg<128, 128, 2, 4, EPI, 4, 1, false, true, true>(q, st);
        return launch_cfg<128, 128, 2, 4, EPI, 4, 1, false, false, true>(q, st);
    }
    if (pl.xs > 1) return launch_cfg<128, 128, 2, 2, EPI, 4, 1, false, true, true>(q, st);
    return launch_cfg<128, 128, 2, 2, EPI, 4, 1, false, false, true>(q, st);
}
hipError_t launch_gemm_deep(const GemmParams& p, int epi, const GemmPlan& pl, hipStream_t st)
{
    return with_epi<false>(epi, [&](auto e) { return launch_deep_epi<decltype(e)::value>(p, pl, st); });
}

// ---- two-barrier tiles: plan.cfg picks the build (0..23: also measurement knob 10 + i; the last two: plan.xs workgroups per tile along K) ----
template <int EPI>
static hipError_t launch_epi(const GemmParams& p, const GemmPlan& pl, hipStream_t st)
{
    GemmParams q = p;
    q.xsplit = pl.xs;
    switch (pl.cfg) {
    case 0: return launch_cfg<32, 128, 1, 4, EPI>(p, st);
    case 1: return launch_cfg<128, 128, 2, 2, EPI>(p, st);
    case 2: return launch_cfg<256, 256, 2, 4, EPI>(p, st);
    case 3: return launch_cfg<64, 128, 2, 4, EPI>(p, st);
    case 4: return launch_cfg<128, 128, 2, 4, EPI>(p, st);
    case 5: return launch_cfg<128, 64, 4, 2, EPI>(p, st);
    case 6: return launch_cfg<256, 128, 2, 4, EPI>(p, st);
    case 7: return launch_cfg<64, 64, 2, 2, EPI>(p, st);
    case 8: return launch_cfg<64, 256, 2, 4, EPI>(p, st);
    case 9: return launch_cfg<64, 64, 2, 2, EPI, 4>(p, st);
    case 10: return launch_cfg<64, 64, 2, 2, EPI, 8>(p, st);
    case 11: return launch_cfg<64, 128, 2, 4, EPI, 4>(p, st);
    case 12: return launch_cfg<128, 64, 4, 2, EPI, 4>(p, st);
    case 13: return launch_cfg<64, 32, 2, 1, EPI, 8>(p, st);
    case 14: return launch_cfg<128, 128, 2, 4, EPI, 4>(p, st);
    case 15: return launch_cfg<32, 128, 1, 4, EPI, 4>(p, st);
    case 16: return launch_cfg<64, 64, 2, 2, EPI, 2, 4>(p, st);
    case 17: return launch_cfg<64, 64, 2, 2, EPI, 2, 2>(p, st);
    case 18: return launch_cfg<32, 64, 1, 2, EPI, 2, 4>(p, st);
    case 19: return launch_cfg<128, 64, 4, 2, EPI, 2, 2>(p, st);
    case 20: return launch_cfg<64, 32, 2, 1, EPI, 2, 4>(p, st);
    case 21: return launch_cfg<64, 128, 2, 4, EPI, 2, 2>(p, st);
    case 22: return launch_cfg<32, 64, 1, 2, EPI, 2, 4, true>(p, st);
    case 23: return launch_cfg<64, 64, 2, 2, EPI, 2, 4, true>(p, st);
    case kTileCfgXs32: return launch_cfg<32, 64, 1, 2, EPI, 2, 4, true, true>(q, st);
    case kTileCfgXs64: return launch_cfg<64, 64, 2, 2, EPI, 2, 4, true, true>(q, st);
    default: return hipErrorInvalidValue;
    }
}
hipError_t launch_gemm_tiles(const GemmParams& p, int epi, const GemmPlan& pl, hipStream_t st)
{
    return with_epi<true>(epi, [&](auto e) { return launch_epi<decltype(e)::value>(p, pl, st); });
}

// ---------------------------------------------------------------------------------------------------------
// Stand-alone pieces of the reference API surface that enqueue() no longer needs (kept for drop-in parity).

// gemmfp16 (TsinghuaMixQPlugin.cpp:122-161): Out[M,N] = fp16(fpA[M,O] . fpW[N,O]^T), fp32 accumulate.
// One wave per 32x32 output tile; operands straight from global (O is tiny, both panels stay in L2).
__global__ __launch_bounds__(256) void gemm_fp16_kernel(const uint16_t* __restrict__ fpA,
                                                         const uint16_t* __restrict__ fpW, uint16_t* __restrict__ Out,
                                                         int M, int N, int O)
{
    const int lane = threadIdx.x & 63, lr = lane & 31, lh = lane >> 5;
    const int tiles_n = (N + 31) / 32;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int tm = (int)(tile / tiles_n), tn = (int)(tile % tiles_n);
    if ((int64_t)tm * 32 >= M) return;
    const int mrow = min(tm * 32 + lr, M - 1), nrow = min(tn * 32 + lr, N - 1);
    v16f P;
#pragma unroll
    for (int e = 0; e < 16; ++e) P[e] = 0.f;
    for (int k0 = 0; k0 < O; k0 += 16) {
        const int k = k0 + lh * 8;
        v8h xf, yf;
        if ((O & 7) == 0) { // rows are 16-byte aligned: vector loads (k + 8 <= O always holds for k < O)
            if (k < O) {
                xf = *reinterpret_cast<const v8h*>(fpW + (int64_t)nrow * O + k);
                yf = *reinterpret_cast<const v8h*>(fpA + (int64_t)mrow * O + k);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) xf[e] = (_Float16)0.f, yf[e] = (_Float16)0.f;
            }
        } else { // any O (dynamic outlier sets of the P-flavour): element loads with a zero tail
            uint16_t xb[8], yb[8]; // (arrays, not vector-element lvalues: see mixq_device.h on __builtin_bit_cast)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool ok = k + e < O;
                xb[e] = ok ? fpW[(int64_t)nrow * O + k + e] : (uint16_t)0;
                yb[e] = ok ? fpA[(int64_t)mrow * O + k + e] : (uint16_t)0;
            }
            __builtin_memcpy(&xf, xb, 16);
            __builtin_memcpy(&yf, yb, 16);
        }
        P = __builtin_amdgcn_mfma_f32_32x32x16_f16(xf, yf, P, 0, 0, 0);
    }
    const int m = tm * 32 + lr;
    if (m >= M) return;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int nb = tn * 32 + 8 * g + 4 * lh;
        if (nb < N) {
            uint2 o;
            o.x = (unsigned)f2h_bits(P[4 * g]) | ((unsigned)f2h_bits(P[4 * g + 1]) << 16);
            o.y = (unsigned)f2h_bits(P[4 * g + 2]) | ((unsigned)f2h_bits(P[4 * g + 3]) << 16);
            *reinterpret_cast<uint2*>(Out + (int64_t)m * N + nb) = o;
        }
    }
}

hipError_t launch_gemm_fp16(const void* fpA, const void* fpW, void* Out, int M, int N, int O, hipStream_t st)
{
    if (M <= 0 || N <= 0) return hipSuccess;
    const int64_t tiles = (int64_t)((M + 31) / 32) * ((N + 31) / 32);
    hipLaunchKernelGGL(gemm_fp16_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, st,
                       static_cast<const uint16_t*>(fpA), static_cast<const uint16_t*>(fpW),
                       static_cast<uint16_t*>(Out), M, N, O);
    return hipGetLastError();
}

// dequantizationKernel (kernel/i8gemm.cu:258-279): out = hadd( fp16((float(x)*sRow[m])*sCol[n]), out ).
__global__ __launch_bounds__(256) void dequantization_kernel(uint16_t* __restrict__ out, const int32_t* __restrict__ x,
                                                              const uint16_t* __restrict__ sRow,
                                                              const uint16_t* __restrict__ sCol, int M, int N)
{
    const int64_t total = (int64_t)M * N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int m = (int)(i / N), n = (int)(i % N);
        const float t = ((float)x[i] * h2f(sRow[m])) * h2f(sCol[n]);
        out[i] = f2h_bits_of_f32_result(h2f(f2h_bits_of_f32_result(t)) + h2f(out[i]));
    }
}

hipError_t launch_dequantization(void* out, const int32_t* x, const void* sRow, const void* sCol, int M, int N,
                                 hipStream_t st)
{
    if (M <= 0 || N <= 0) return hipSuccess;
    const int64_t total = (int64_t)M * N;
    const int64_t want = (total + 255) / 256;
    const unsigned grid = (unsigned)(want < 2048 ? want : 2048);
    hipLaunchKernelGGL(dequantization_kernel, dim3(grid), dim3(256), 0, st, static_cast<uint16_t*>(out), x,
                       static_cast<const uint16_t*>(sRow), static_cast<const uint16_t*>(sCol), M, N);
    return hipGetLastError();
}

// dequantizationKernelSilu (quantkernel/mix_cuda/cult.cu:2305-2324, called by dequantizeInt8Silu :2341-2348 on the
// P-flavour's sm90 route, MixQ/src/mixquant/modules/linear.py:321-324):
//   out = fp16( silu( fma(fl32(float(x) * sRow[m]), sCol[n], float(y)) ) )   -- fp32 throughout, ONE rounding to fp16
// (unlike dequantizationKernel above, which rounds the product to fp16 before an fp16 add).
__global__ __launch_bounds__(256) void dequantization_silu_kernel(uint16_t* __restrict__ out,
                                                                   const int32_t* __restrict__ x,
                                                                   const uint16_t* __restrict__ sRow,
                                                                   const uint16_t* __restrict__ sCol,
                                                                   const uint16_t* __restrict__ y, int M, int N)
{
    const int64_t total = (int64_t)M * N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int m = (int)(i / N), n = (int)(i % N);
        // nvcc (default -fmad=true) contracts the LAST multiply with the add: fma(fl32(x * sRow), sCol, y) -- the first
        // product is rounded on its own (pinned: hipcc must not fold it into the fma), exactly as the oracle restates it
        float t = (float)x[i] * h2f(sRow[m]);
        asm("" : "+v"(t));
        out[i] = f2h_bits_of_f32_result(silu_f32(__builtin_fmaf(t, h2f(sCol[n]), h2f(y[i]))));
    }
}

hipError_t launch_dequantization_silu(void* out, const int32_t* x, const void* sRow, const void* sCol, const void* y,
                                      int M, int N, hipStream_t st)
{
    if (M <= 0 || N <= 0) return hipSuccess;
    const int64_t want = ((int64_t)M * N + 255) / 256;
    const unsigned grid = (unsigned)(want < 2048 ? want : 2048);
    hipLaunchKernelGGL(dequantization_silu_kernel, dim3(grid), dim3(256), 0, st, static_cast<uint16_t*>(out), x,
                       static_cast<const uint16_t*>(sRow), static_cast<const uint16_t*>(sCol),
                       static_cast<const uint16_t*>(y), M, N);
    return hipGetLastError();
}

} // namespace mixq
