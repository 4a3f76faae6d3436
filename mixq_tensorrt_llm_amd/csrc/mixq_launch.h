// Host-visible launch interface between mixq_api.hip (C ABI, orchestration) and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <string>
#include <type_traits>

namespace mixq {

// Per-device once-flags: attributes set with hipFuncSetAttribute (and device symbol addresses, CU counts) belong to the
// CURRENT device, and a process may drive several GPUs.  One bit per device ordinal (ordinals >= 64 are simply redone).
inline int current_device()
{
    int d = 0;
    return hipGetDevice(&d) == hipSuccess && d >= 0 ? d : 0;
}
struct DeviceOnce {
    std::atomic<uint64_t> mask{0};
    bool done(int dev) const { return dev < 64 && ((mask.load(std::memory_order_acquire) >> dev) & 1u); }
    void set(int dev)
    {
        if (dev < 64) mask.fetch_or(uint64_t{1} << dev, std::memory_order_release);
    }
};
// hipFuncAttributeMaxDynamicSharedMemorySize for `kern` on the current device, once per device (idempotent if raced).
template <class Kern>
inline hipError_t ensure_dynamic_lds(Kern kern, size_t bytes, DeviceOnce& once)
{
    const int dev = current_device();
    if (once.done(dev)) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)bytes);
    if (e == hipSuccess) once.set(dev);
    return e;
}
int num_cus(); // of the current device (cached per device)

enum { EPI_DEQUANT = 0, EPI_DEQUANT_SILU = 1, EPI_INT32 = 2, EPI_DEQUANT_SILU_MUL = 3,
       EPI_F16GEMM = 4,   // 4: the operands are fp16 (K counts BYTES), fp32 accumulation, D = fp16(A B^T): the ping-pong kernel
                          // with v_mfma_f32_32x32x16_f16 (second pass of the two-pass fpA_intB GEMM, w8a16_gemm_kernels.hip)
       EPI_DEQUANT_BIAS = 5 }; // 5: EPI_DEQUANT, then D = fp16(D + bias[n]) on the rounded value (GemmParams::bias, the layer's fp16 [N]
                               // bias; the reference adds it after the plugin, plugin.py:158-160).  Kernel choice: the same as EPI_DEQUANT
// 6 / 7: EPI_DEQUANT / EPI_DEQUANT_BIAS of a bf16 call (mixq_enqueue with inputDesc[0].type == MIXQ_TYPE_BF16): sA, fpA, fpW, the bias
// and D are bf16; the outlier product runs on the bf16 MFMA and is rounded to bf16, D = bf16(fma(acc, sW sA, P)) (+ one bf16 add of
// the bias).  sW stays fp16.  Kernel choice: the same as EPI_DEQUANT
enum { EPI_DEQUANT_BF16 = 6, EPI_DEQUANT_BIAS_BF16 = 7 };
// 8 / 9: EPI_DEQUANT_SILU / EPI_DEQUANT_SILU_MUL of a bf16 call (mixq_gemm_mixed_act_typed): g = bf16(silu(fma(acc, sW sA, P))) on the fp32
// value, D = g or D = bf16(fp32(g) * fp32(Mul)) -- one multiply of the ROUNDED g by the bf16 [M,N] multiplicand (the fp32 product of two bf16
// values is exact: one rounding, torch's bf16 multiply).  No addend, no bias, no peer writes, O <= 128.  Kernel choice: the same as EPI_DEQUANT
enum { EPI_DEQUANT_SILU_BF16 = 8, EPI_DEQUANT_SILU_MUL_BF16 = 9 };
// 10 / 11: the merged gate / up projection (mixq_gemm_mixed_gate_up_typed), fp16 / bf16: the GEMM is (M, GemmParams::N = 2 n_out, K) on the merged
// weight of include/mixq.h (blocks of 8 gate rows followed by their 8 up rows); of every 16 GEMM columns the first 8 are EPI_DEQUANT_SILU's g, the
// last 8 EPI_DEQUANT's u (each rounded to the call's type), and D[m, 8 (c / 16) + c % 8] = T_rn(fp32(g) * fp32(u)) with D [M, n_out] at row stride
// GemmParams::n_out -- the bits of EPI_DEQUANT for u followed by EPI_DEQUANT_SILU_MUL with Mul = u.  In the 32 x 32 MFMA families gate and up of a
// column are the same lane's column quads g and g ^ 1 (8 columns apart); in the skinny kernel lanes l and l ^ 32.  No addend, bias or peer writes,
// O <= 128.  Kernel choice: EPI_DEQUANT's on (M, 2 n_out, K)
enum { EPI_GATE_UP = 10, EPI_GATE_UP_BF16 = 11 };
constexpr bool epi_gate_up(int epi) { return epi == EPI_GATE_UP || epi == EPI_GATE_UP_BF16; }
constexpr bool epi_has_mul(int epi) { return epi == EPI_DEQUANT_SILU_MUL || epi == EPI_DEQUANT_SILU_MUL_BF16; }
constexpr bool epi_has_silu(int epi) { return epi == EPI_DEQUANT_SILU || epi == EPI_DEQUANT_SILU_BF16 || epi_has_mul(epi); }
constexpr bool epi_bf16(int epi)
{
    return epi == EPI_DEQUANT_BF16 || epi == EPI_DEQUANT_BIAS_BF16 || epi == EPI_DEQUANT_SILU_BF16 || epi == EPI_DEQUANT_SILU_MUL_BF16 ||
           epi == EPI_GATE_UP_BF16;
}
// output column of GEMM column c of a merged gate / up call (c % 16 < 8: the gate column; its up column is c + 8)
__host__ __device__ constexpr int gate_up_col(int c) { return ((c >> 4) << 3) + (c & 7); }
constexpr bool epi_bias(int epi) { return epi == EPI_DEQUANT_BIAS || epi == EPI_DEQUANT_BIAS_BF16; }
// f(std::integral_constant<int, EPI>{}) with the run-time `epi` as a compile-time constant: the ten dequantising epilogues; any other
// value is EPI_INT32 where the family has that build (INT32), else an error (and f is not instantiated for it)
template <bool INT32, class F>
inline hipError_t with_epi(int epi, F&& f)
{
    switch (epi) {
    case EPI_DEQUANT: return f(std::integral_constant<int, EPI_DEQUANT>{});
    case EPI_DEQUANT_SILU: return f(std::integral_constant<int, EPI_DEQUANT_SILU>{});
    case EPI_DEQUANT_SILU_MUL: return f(std::integral_constant<int, EPI_DEQUANT_SILU_MUL>{});
    case EPI_DEQUANT_BIAS: return f(std::integral_constant<int, EPI_DEQUANT_BIAS>{});
    case EPI_DEQUANT_BF16: return f(std::integral_constant<int, EPI_DEQUANT_BF16>{});
    case EPI_DEQUANT_BIAS_BF16: return f(std::integral_constant<int, EPI_DEQUANT_BIAS_BF16>{});
    case EPI_DEQUANT_SILU_BF16: return f(std::integral_constant<int, EPI_DEQUANT_SILU_BF16>{});
    case EPI_DEQUANT_SILU_MUL_BF16: return f(std::integral_constant<int, EPI_DEQUANT_SILU_MUL_BF16>{});
    case EPI_GATE_UP: return f(std::integral_constant<int, EPI_GATE_UP>{});
    case EPI_GATE_UP_BF16: return f(std::integral_constant<int, EPI_GATE_UP_BF16>{});
    }
    if constexpr (INT32) return f(std::integral_constant<int, EPI_INT32>{});
    else return hipErrorInvalidValue;
}

// TP all-gather fused into the GEMM's store path (gemm_pp_kernels.hip, TP = true): every finished 32-row block of a wave
// tile is written straight into this rank's column block of EVERY destination's [M, n_total] buffer (one-sided peer writes
// over xGMI, write-through at system scope), and when the last tile of an M chunk (`chunk_tile_rows` rows of 256 x 256
// tiles) has been acknowledged the chunk's flag word in every destination receives `seq`.  No separate push launch, no
// second read of the [M, N/tp] block, and the transfer runs under the GEMM itself.
constexpr int kTpMaxPeers = 8;
constexpr int kTpFlagWords = 64; // flag words per (parity, producer): word 0 = stand-alone push, one per M chunk when fused
struct TpEpilogue {
    int ndst;                      // 0: off
    int ldd;                       // row stride of every destination in elements (= n_total)
    void* base[kTpMaxPeers];       // destination r's [M, n_total] fp16 buffer + this rank's column offset
    unsigned* flag[kTpMaxPeers];   // this producer's kTpFlagWords flag words in destination r
    unsigned seq;
    unsigned* counters;            // this rank's per-chunk tile counters (kTpFlagWords words, zero; left zero)
    int chunk_tile_rows;           // tile rows (of 256 rows) per flag word
};
int tp_chunk_tile_rows(int M);     // tile rows per flag word for an M-row call: a multiple of the kernel's GROUP_M walk
int tp_flag_words(int M);          // flag words a consumer must wait for = ceil(tile rows / chunk_tile_rows) <= kTpFlagWords
bool gemm_tp_fused_supported(int M, int N, int K, int O); // the plan of the operator's call is the plain 256 x 256 ping-pong kernel

struct GemmParams {
    const int8_t* A;      // qA [M,K]
    const int8_t* B;      // W  [N,K]
    const uint16_t* sA;   // [M]
    const uint16_t* sW;   // [N]
    const uint16_t* fpA;  // [M,O] or null
    const uint16_t* fpW;  // [N,O] or null
    const uint16_t* Y;    // fp16 [M,N] addend or null (int8FusedDequantize API)
    const uint16_t* Mul;  // fp16 (bf16) [M,N] multiplicand of EPI_DEQUANT_SILU_MUL (_BF16): D = fp16(fp16(silu(..)) * Mul), else null
    void* D;              // fp16 [M,N] (EPI_DEQUANT*) or int32 [M,N] (EPI_INT32)
    const void* zeros;    // >= 16 B of device zeros (K / O tails)
    int M, N, K, O;
    int a_frag;           // layout of A: 0 row-major | 1 the skinny GEMM's fragment-major image (only valid when gemm_takes_skinny) |
                          // 2 K-slice-major [K/128][M][128 B] (read by the plain 256 x 256 ping-pong kernel only; no producer ships:
                          // measured a net loss, docs/LAB_NOTEBOOK.md R3.10); 1 is written by mixq_enqueue's quantiser (FRAG)
    const void* b_image;  // the registered fragment-major image of B this call may stream (resolved once per call by the API layer), or null
    int b_frag;           // (set by the skinny launcher from b_image, a_frag == 1 only) layout of B: 0 row-major [N,K] | 1 fragment-major image
                          // (1-KiB blocks [16-feature tile][64-byte k-step], lane l = feature % 16 + 16 * (k / 16 % 4) at l * 16) | 2 the same, non-temporal loads
    void* dbg;            // measurement only: 8 x uint64 s_memtime stamps per block (ping-pong kernel), else null
    int flags;            // (set by launch_gemm_deep) bit 0: measurement -- every wave issues its slice copies before its MFMAs
    int xsplit;           // (set by launch_epi) workgroups per tile of the small-tile kernels' K split, else 0
    int splitk_solo;      // (set by launch_gemm_pp_splitk) leading tiles that are not split
    unsigned splitk_patience; // (set by launch_gemm_pp_splitk) wall-clock ticks a workgroup waits for its partners before
                              // it defers its share to the last arriver
    TpEpilogue tp;        // (launch_gemm_pp_tp only) peer-write epilogue, else ndst == 0
    void* splitk_ws;      // device scratch of gemm_splitk_workspace_size bytes whose arrival words are zero, or null: lets
                          // launch_gemm split K over 2 / 4 workgroups per 256x256 tile when the tiles alone cover at
                          // most half / a quarter of the CUs (gemm_pp_kernels.hip)
    const uint16_t* bias; // fp16 [N] of EPI_DEQUANT_BIAS (bf16 [N] of EPI_DEQUANT_BIAS_BF16) (added once, by whoever runs the final epilogue of an element), else null
    int n_out;            // EPI_GATE_UP (_BF16): width and row stride of D = N / 2 (N is the GEMM's width, the merged weight's rows), else 0 (last: the older fields keep their offsets)
};

// What one int8 GEMM call launches: decided once by plan_gemm (gemm_plan.hip: the ladder of DESIGN.md §4), read by launch_gemm, the
// family launchers, describe_gemm_plan and every selection question of the API layer.  A plain value; fields of other families are 0.
enum { GEMM_TILES = 0, GEMM_SKINNY, GEMM_DEEP, GEMM_PP_ABLATE, GEMM_PP128, GEMM_PP_SPLITK, GEMM_PP };
enum { kTileCfgXs32 = 24, kTileCfgXs64 = 25 }; // GemmPlan::cfg of the two-barrier tiles with K split over workgroups (0..23: launch_gemm_tiles)
struct GemmPlan {
    int family;        // GEMM_*
    int xs;            // workgroups per tile along K: deep form 1 / 2 / 4 / 8, 256 x 256 split 2 / 4 / 8, two-barrier tiles 2..16; else 0
    int solo;          // GEMM_PP_SPLITK: leading tiles that are not split
    int cfg;           // GEMM_TILES: tile configuration; GEMM_PP_ABLATE: the ablation
    int tile_m, tile_n, kgroups; // GEMM_TILES: the configuration's tile and K groups inside the workgroup (0: forced by knob 10 + i)
    int deep_build;    // GEMM_DEEP: 0 = 4 waves x 64 x 64, 1 = 8 waves x 64 x 32 (4 stages), 2 = 8 waves, 5 stages, 3 = the mid kernel (gemm_mid_kernels.hip)
    bool deep_early;   // GEMM_DEEP builds 0..2: measurement -- every wave issues its slice copies before its MFMAs
    int mid_bn;        // build 3: tile width 128 | 96
    bool mid_rot;      // build 3: tile rows start at different K slices
    bool qa_frag;      // GEMM_SKINNY: qA is the fragment-major image
    int skinny_kw, skinny_abl;      // GEMM_SKINNY: K-split waves 4 / 8 / 16; measurement ablation or 0
    int skinny_route, skinny_tiles; // GEMM_SKINNY: GemmParams::b_frag (skinny_weight_route); 16-column feature tiles per workgroup, 1 | 2
    bool skinny_nt;    // GEMM_SKINNY route 3: non-temporal weight loads
    const char* name;  // what last_gemm_kernel reports (null: left as it is)
};
GemmPlan plan_gemm(const GemmParams& p, int epi); // pure host function; without a device num_cus() answers 256
hipError_t launch_gemm(const GemmParams& p, int epi, hipStream_t st, const GemmPlan* planned = nullptr); // planned: plan_gemm(p, epi) the caller already holds
void describe_gemm_plan(const GemmPlan& plan, char* buf, size_t len); // the plan as text (host only)
hipError_t launch_gemm_tiles(const GemmParams& p, int epi, const GemmPlan& plan, hipStream_t st); // two-barrier tiles (gemm_kernels.hip)
void set_tile_nt(int mode); // measurement knob 1290 by rule (default) / 1291 never / 1292 always: non-temporal weight copies on a single tile row
int skinny_weight_route(int a_frag, bool image, int M, int N, int K);         // GemmParams::b_frag of the skinny launch
bool skinny_runs_nontemporal(int N, int K);                                   // that route 3 loads non-temporally
hipError_t launch_gemm_pp(const GemmParams& p, int epi, hipStream_t st);  // 256x256 ping-pong schedule
hipError_t launch_gemm_pp128(const GemmParams& p, int epi, hipStream_t st);
hipError_t launch_gemm_pp_tp(const GemmParams& p, hipStream_t st); // EPI_DEQUANT (EPI_DEQUANT_BIAS when p.bias) with p.tp.ndst destinations instead of p.D
// D[M,N] fp16 = A[M,K] B[N,K]^T, fp16 operands (K % 8 == 0, N % 8 == 0, 16-byte aligned rows), fp32 accumulation
hipError_t launch_gemm_f16_pp(const void* A, const void* B, void* D, int M, int N, int K, const void* zeros, hipStream_t st);
hipError_t launch_gemm_f16_pp128(const void* A, const void* B, void* D, int M, int N, int K, const void* zeros, hipStream_t st); // 128 x 256 tiles // 128x256 ping-pong schedule (mid-size problems)
bool gemm_pp128_wins(int M, int N, int K); // the rule for taking the 128x256 tiles (then no K split, no scratch)
constexpr size_t kSplitkWordsBytes = 16384; // hand-over words (64 B per tile) of up to 256 split tiles, at the start of the scratch
struct SplitPlan {
    int s;    // workgroups per split tile: 0 (no split form for this shape) / 2 / 4 / 8
    int solo; // leading tiles (whole waves) computed by one workgroup each, inside the same launch
};
SplitPlan gemm_splitk_plan(int M, int N, int K);
size_t gemm_splitk_workspace_size(int M, int N, int K);   // 0: the shape does not use the split form (or it is off)
size_t gemm_splitk_workspace_bound();                     // max of the above over all shapes (for workspace sizing)
hipError_t launch_gemm_pp_splitk(const GemmParams& p, int epi, const GemmPlan& plan, hipStream_t st);
void set_splitk_patience(unsigned ticks); // test knob: 0 = every workgroup but the last arriver defers at once
void set_splitk_force(int v); // -1 automatic (default), 0 off, 2 / 4: that factor wherever the shape allows it
// the same idea for the small-tile kernels with in-workgroup split (gemm_kernels.hip, XS): few tiles, long K
size_t gemm_xsplit_workspace_size(int M, int N, int K);
size_t gemm_xsplit_workspace_bound();
// mid-M deep form (gemm_kernels.hip): 128 x 128 tiles, 4 stages in flight, K split over 1 / 2 / 4 / 8 workgroups per tile
size_t gemm_deep_workspace_size(int M, int N, int K); // 0: the form is not used for this shape, or needs no scratch
hipError_t launch_gemm_deep(const GemmParams& p, int epi, const GemmPlan& plan, hipStream_t st);
// round-6 schedule of the same tiles (gemm_mid_kernels.hip): 2 copy-only waves + 8 compute waves, one barrier per pair of slices; p.xsplit workgroups per tile
hipError_t launch_gemm_mid(const GemmParams& p, int epi, const GemmPlan& plan, hipStream_t st);
void set_mid_rot(int mode);  // measurement knob 1413 (default: 3 = by rule) / 1411 (0 = never) / 1410 (1 = unsplit tiles) / 1412 (2 = always)
void set_mid_bn(int mode);   // measurement knob 1430 (default: 0 = by rule) / 1431 (1 = 128-wide tiles always)
int gemm_mid_tile_width(int M, int N, int xsplit); // 128 | 96: the tile width of the mid kernel
bool gemm_mid_rotated_walk(int M, int xsplit);     // its tile rows start at different K slices
bool gemm_skinny_supported(const GemmParams& p);
hipError_t launch_gemm_skinny(const GemmParams& p, int epi, const GemmPlan& plan, hipStream_t st); // M <= 64: GEMV-like, HBM-bound on W
hipError_t launch_gemm_pp_ablate(const GemmParams& p, int abl, hipStream_t st);  // timing experiments only
void set_gemm_variant(int v);
bool w8a16_skinny_takes(int M, int N, int K); // the fpA_intB skinny form serves this shape (w8a16_gemm_kernels.hip)
// the same form with the layer's fp16 [N] bias added to the rounded result (M <= 16, w8a16_skinny_takes only)
hipError_t launch_w8a16_skinny_bias(const void* A, const uint8_t* Wq, const void* scale, void* Out, int M, int N, int K,
                                    const void* bias, hipStream_t st);
// the same form for a bf16 call (bf16 A / Out / bias, fp16 scale; bias may be null)
hipError_t launch_w8a16_skinny_bf16(const void* A, const uint8_t* Wq, const void* scale, void* Out, int M, int N, int K,
                                    const void* bias, hipStream_t st);
// fpA_intB measurement / test knobs (mixq_debug_set_gemm_variant 80..89, 831..834, 840..844, 850..858, 800 + ABL); `form`:
//   -1 everything automatic | 0 narrow form | 1..4 wide form with 32 / 64 / 128 / 256-row tiles | 100 + ABL ablation of the
//   256-row form | 200 / 201 / 202 two-pass form automatic / never / always, 203 / 204 its second pass on 256- / 128-row tiles
//   | 300 / 301 skinny form automatic / off, 302..305 one of its shapes | 306 / 307 / 308 1..4 tokens through the skinny form
//   always / never / automatic;  `ks`: -2 keep, -1 automatic, n = workgroups per tile along K.
void set_wo_force(int form, int ks);
const char* last_gemm_kernel(); // kernel family launch_gemm chose last (reporting only)
void set_skinny_nt(int nt);
void set_skinny_wrows(int on); // knob 884 on (default) / 885 off: row-major weights read in 256-byte runs (gemm_skinny_kernels.hip WFRAG == 3)
void set_skinny_wfrag(int mode); // knob 880 automatic | 881 weight images with plain loads | 882 with non-temporal loads | 883 images ignored
// weight images (gemm_skinny_kernels.hip): a fragment-major copy of an int8 [N, K] weight, registered under the weight's pointer
hipError_t launch_weight_image(const int8_t* W, int8_t* img, int N, int K, hipStream_t st);
hipError_t register_weight_image(const void* weight, const void* image, int N, int K, hipStream_t st); // records the weight's content tag; synchronises st
bool unregister_weight_image(const void* weight);
const void* resolve_weight_image(const void* weight, int N, int K, hipStream_t st); // once per call; verifies the content tag on first use
int verify_weight_image(const void* weight, hipStream_t st);  // 1 current | 0 stale (dropped) | -1 nothing registered; synchronises st
int weight_image_stale_count();
int skinny_feature_tiles(int M, int N, int K, bool image = false); // (image: the call streams a registered weight image) measurement knob 894 / 895 / 896: feature tiles per workgroup of the fragment-major form auto / 1 / 2
hipError_t launch_gemm_fp16(const void* fpA, const void* fpW, void* Out, int M, int N, int O, hipStream_t st);
hipError_t launch_dequantization(void* out, const int32_t* x, const void* sRow, const void* sCol, int M, int N,
                                 hipStream_t st);
hipError_t launch_dequantization_silu(void* out, const int32_t* x, const void* sRow, const void* sCol, const void* y,
                                      int M, int N, hipStream_t st);
hipError_t launch_quant_extract(void* A, int8_t* qA, void* sA, void* fpA, const int32_t* ind, int M, int K, int O,
                                bool zero, hipStream_t st,
                                void* zero_words = nullptr, // (kSplitkWordsBytes to clear on the way, or null)
                                int frag = 0,  // qA layout: 0 row-major | 1 the skinny GEMM's fragment order (quant_frag_layout_supported)
                                bool bf16 = false); // A, sA, fpA are bf16 (either flavour): sA = bf16(amax / 127), q = sat(rint(x / sA)) on the
                                                    // row as quantised (zero: the zeroed row); an ind[j] outside [0, K) gathers +0, zeroes nothing
void set_quant_block_rows(int m); // measurement knob 1300 (rules) / 1301..1312 (64 << n rows)
int quant_block_rows(int nvec, bool norm_producer); // rows up to which a whole 256-thread block takes one row of nvec 16-byte vectors
bool quant_frag_layout_supported(int M, int K);   // the quantiser can write the fragment-major image for this shape
bool gemm_takes_skinny(const GemmParams& p, int epi); // the plan of this problem is gemm_skinny_kernel
bool qa_frag_enabled(); // test knob 890 / 891 (default on)
void set_quant_stamp_buffer(void* device_u64_8_per_block); // measurement only (NULL in production)
// Activation producers (quantisers, outlier gathers, the fused RMSNorm producer): name of the form the most recent launch took,
// e.g. "quant_extract_kernel<TPR=64,MAXV=8,ZERO=1,FRAG=0> nt" (" nt": non-temporal qA stores).  Reporting only.
const char* last_producer_kernel();
void note_producer_kernel(const char* name); // (name: a string that lives as long as the process)
std::string producer_form_name(const char* kernel, int tpr, int maxv, const char* flag, int flag_value, int frag, bool nt);
hipError_t launch_quant_with_scale(const void* src, const void* scale, int8_t* dst, int M, int K, hipStream_t st);
hipError_t launch_extract(void* A, void* fpA, const int32_t* ind, int M, int K, int O, bool zero, hipStream_t st);
hipError_t launch_rmsnorm_quant(const void* X, const void* gamma, void* out, void* outl, const int32_t* ind, int8_t* q,
                                void* scale, float eps, int M, int K, int O, int quant /* 0, 8, 4 */, hipStream_t st,
                                int q_layout = 0 /* 1: fragment-major int8 rows (quant == 8, quant_frag_layout_supported) */,
                                // both or neither: the row is h = fp16(X + residual), written to h_out (may be X or residual, not out);
                                // same form and grid as without, so the same bits as an fp16 add followed by the plain call
                                const void* residual = nullptr, void* h_out = nullptr,
                                // x, residual, h, gamma, out, the outliers and the scale are bf16 (quant 0 / 8): same form table, no clamp,
                                // scale = bf16(amax / 127), q = sat(rint(out / scale)) -- launch_quant_extract's bf16 rules on the rounded row
                                bool bf16 = false);
hipError_t launch_find_outliers(const void* A, int M, int K, float sigma, unsigned* mask, int32_t* ind, int32_t* count,
                                int capacity, hipStream_t st, bool bf16 = false); // bf16: A is bf16 (|fp32(a)| > sigma)
hipError_t launch_dequant_columns(const int8_t* W, const void* sW, const int32_t* ind, int len, void* out, int N, int K,
                                  hipStream_t st, bool bf16 = false); // bf16: out is bf16 (sW stays fp16); ind[j] outside [0, K): a zero column
hipError_t launch_quant4_rows(const void* A, uint8_t* q, void* sA, int M, int K, hipStream_t st);
hipError_t launch_unpack_s4(const uint8_t* src, int8_t* dst, size_t packed_bytes, hipStream_t st);
// packed-int4 weight stream (int4_gemm_kernels.hip): p.A / p.B packed int4 [M, K] / [N, K], p.K = PACKED bytes per row, p.Y addend or null
void set_s4_wrows(int mode); // knob 872 by rule (default) / 873 off / 874 always: packed weights read in 256-byte runs (int4_gemm_kernels.hip WROWS)
bool gemm_skinny_s4_supported(int M, int N, int k_packed);
hipError_t launch_gemm_skinny_s4(const GemmParams& p, int epi, hipStream_t st);
// the same with the fp16 rows quantised inside the launch (M <= 16): p.A = fp16 [M, 2 p.K], p.sA = the row scales, WRITTEN (workgroup 0)
bool gemm_skinny_s4q_supported(int M, int N, int k_packed);
hipError_t launch_gemm_skinny_s4q(const GemmParams& p, int epi, hipStream_t st);
hipError_t launch_unpack_s4_columns(const uint8_t* weight, const int32_t* ind, int rows, int cols_packed, int n,
                                    void* out, hipStream_t st);
hipError_t launch_w8a16(const void* A, const uint8_t* Wq, const void* scale, void* Out, int M, int N, int K,
                        hipStream_t st, const void* bias = nullptr); // bias: fp16 [N] added to the rounded result, or null
// the same GEMV for bf16 A / Out / bias (scale stays fp16): Out = bf16(sum_k fp32(A) (q - 128) * scale[n]), fp32 throughout
hipError_t launch_w8a16_bf16(const void* A, const uint8_t* Wq, const void* scale, void* Out, int M, int N, int K,
                             hipStream_t st, const void* bias);

void note_gemm_kernel(const char* name);
// TP all-gather of the output columns as one-sided peer writes + flags (tp_kernels.hip)
// seq_word != null (capturable form): the call number is *seq_word + 1, read on the device; launch_tp_wait stores it back
hipError_t launch_tp_push(const void* src, void* const* dst_bases, unsigned* const* dst_flags, int ndst, int M, int n_loc,
                          int N, int col0, unsigned seq, int nflags, unsigned* done_counter, hipStream_t st,
                          const unsigned* seq_word = nullptr,
                          const unsigned* status = nullptr); // (capturable form) the sticky status word: raised -> nothing is stored or published
hipError_t launch_tp_wait(const unsigned* flags, int nprod, int word0, int nwords, unsigned seq, unsigned* status, int trap,
                          unsigned patience_ms, hipStream_t st, unsigned* seq_word = nullptr);
hipError_t launch_tp_arrive(unsigned* const* peer_acks, const unsigned* own_acks, int npeer, const unsigned* seq_word,
                            unsigned* status, int trap, unsigned patience_ms, hipStream_t st);
// fpA_intB GEMM (M > 4) on the interleaved qweight (w8a16_gemm_kernels.hip); scratch may be null (no K split)
size_t w8a16_gemm_workspace_size(int M, int N, int K, bool bf16 = false);
hipError_t launch_w8a16_gemm(const void* A, const uint8_t* Wq, const void* scale, void* Out, int M, int N, int K,
                             void* scratch, size_t scratch_bytes, const void* zeros, hipStream_t st);
// the bf16 call: A / Out bf16, scale fp16; Out = bf16(scale[n] * sum_k A[m,k] (q[k,n] - 128)), the form of the fp16 call of the same
// shape and scratch (the wide form where that is the two-pass form)
hipError_t launch_w8a16_gemm_bf16(const void* A, const uint8_t* Wq, const void* scale, void* Out, int M, int N, int K,
                                  void* scratch, size_t scratch_bytes, const void* zeros, hipStream_t st);

} // namespace mixq
