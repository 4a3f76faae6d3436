// Fused RMSNorm -> outlier extraction -> per-token int8 quantisation for gfx950 (the producer on
// the input side of the MixQ linear; removes one full pass over the activations compared with norm + quant).
//
// Replaces (reference, CUDA): quantkernel/mix_cuda/layernorm/layernorm.cu:122-198 generalT5LayerNorm_extract_outliers
// and :41-98 generalT5LayerNorm (mixlib ops layernorm_forward_cuda_extract_outliers / layernorm_forward_cuda):
//   rstd = rsqrt( sum x^2 / n + eps )                  fp32
//   out  = fp16( clamp( (x * rstd) * gamma, +-64504 ) )
//   outliers[j] = out[ind[j]] ; out[ind[j]] = 0        (P-flavour: outliers leave the int8 path)
//   scale = fp16(amax/127) ; q = int8(rn(out/scale))   same arithmetic as the stand-alone quantiser
//
// One wavefront (K <= 8192) or one 256-thread block (K <= 32768) owns a row and keeps it in registers: x is read once
// (16-byte loads), out / q / outliers / scale are written once.  The normalised row passes through LDS only so that
// the <= 128 outlier values can be picked by column index; the outlier columns are zeroed through a K-bit mask.
#include "mixq_device.h"
#include "mixq_launch.h"

namespace mixq {

constexpr int NBLOCK = 256;

// QUANT: 0 = plain RMSNorm, 8 = int8 rows (scale amax/127), 4 = packed int4 rows (scale amax/7, layernorm.cu:201-290)
// FRAG (QUANT == 8, decode batches): the int8 rows go out in the skinny GEMM's fragment-major order (quant_kernels.hip FRAG).
// ADD: the residual add in front of the norm rides in the same pass -- h = fp16(x + R), rounded once, goes out to H and IS the
// row from there on (sum of squares, normalisation, ... all see the rounded h), so every output has the bits of an fp16 add
// followed by the ADD == false launch of the same form.  A lane holds its x and R vectors in registers before it stores h for
// the same elements, and no lane reads another lane's: H may be X or R (not `out`).
// BF (QUANT 0 / 8 only): x, R, H, gamma, out, the outliers and the scale are bf16.  h = bf16(x + R); out = bf16((row * rstd) * gamma)
// without the clamp (bf16 has fp32's range: the +-64504 clamp is an fp16 overflow guard); scale = bf16(fp32(amax) / 127) and
// q = sat[-127, 127](rint(out / scale)) on the ROUNDED bf16 row, one IEEE quotient per element -- quant_extract_kernel's BF rules
// (quant_kernels.hip), so q and scale are what the bf16 quantiser makes of `out`.  Same TPR / MAXV / grid / reductions as the fp16 form.
template <bool ADD> struct norm_row_ptr { typedef const uint16_t* __restrict__ type; };
template <> struct norm_row_ptr<true> { typedef const uint16_t* type; }; // (H may alias it)

template <int TPR, int MAXV, int QUANT, bool FRAG = false, bool ADD = false, bool BF = false>
__global__ __launch_bounds__(NBLOCK) void rmsnorm_quant_kernel(typename norm_row_ptr<ADD>::type X,
                                                               const uint16_t* __restrict__ gamma,
                                                               uint16_t* __restrict__ out, uint16_t* __restrict__ outl,
                                                               const int32_t* __restrict__ ind, int8_t* __restrict__ q,
                                                               uint16_t* __restrict__ scale, float eps, int M, int K,
                                                               int O, const uint16_t* R = nullptr, uint16_t* H = nullptr)
{
    static_assert(!(BF && QUANT == 4), "there is no bf16 int4 producer");
    constexpr int INF_BITS = BF ? 0x7f80 : 0x7c00; // |x| bit pattern of +inf: larger patterns are NaNs
    constexpr int RPB = NBLOCK / TPR;
    __shared__ float redf[NBLOCK / 64];
    __shared__ int redi[NBLOCK / 64];
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[]; // [mask: K bits, 16-B padded][RPB rows x K fp16]
    const int tid = threadIdx.x;
    const int t = tid % TPR;
    const int rslot = tid / TPR;
    const int64_t row = (int64_t)blockIdx.x * RPB + rslot;
    const bool row_ok = row < M;
    const int nvec = K >> 3;
    const int mask_bytes = ((K + 127) / 128) * 16;
    unsigned* zmask = reinterpret_cast<unsigned*>(dyn);
    uint16_t* lrow = reinterpret_cast<uint16_t*>(dyn + mask_bytes) + (size_t)rslot * K;

    // the row (and, for short rows, gamma) is requested FIRST: its round trip runs under the outlier-mask phase below (a
    // decode batch is a chain of latencies: the mask phase alone is an `ind` round trip + two barriers)
    const uint4* src = reinterpret_cast<const uint4*>(X + (row_ok ? row : 0) * (int64_t)K);
    const uint4* res = ADD ? reinterpret_cast<const uint4*>(R + (row_ok ? row : 0) * (int64_t)K) : nullptr;
    const uint4* __restrict__ g4 = reinterpret_cast<const uint4*>(gamma);
    uint4 x[MAXV];
    uint4 r[ADD ? MAXV : 1]; // the residual's vectors travel with the row's: both round trips run under the mask phase
    constexpr bool GPRE = MAXV <= 4; // gamma prefetched into registers (16 more VGPRs at most)
    uint4 gpre[GPRE ? MAXV : 1];
#pragma unroll
    for (int v = 0; v < MAXV; ++v) {
        const int idx = v * TPR + t;
        x[v] = (row_ok && idx < nvec) ? src[idx] : make_uint4(0u, 0u, 0u, 0u);
        if (GPRE) gpre[v] = idx < nvec ? g4[idx] : make_uint4(0u, 0u, 0u, 0u);
        if (ADD) r[v] = (row_ok && idx < nvec) ? res[idx] : make_uint4(0u, 0u, 0u, 0u);
    }
    if (QUANT) {
        for (int i = tid; i < mask_bytes / 4; i += NBLOCK) zmask[i] = 0u;
        __syncthreads();
        for (int j = tid; j < O; j += NBLOCK) {
            const int c = ind[j];
            if (c >= 0 && c < K) atomicOr(zmask + (c >> 5), 1u << (c & 31));
        }
        __syncthreads();
    }
    if (ADD) { // h = fp16(x + R) (BF: bf16(x + R)): stored once, and the row from here on
        uint4* hdst = reinterpret_cast<uint4*>(H + (row_ok ? row : 0) * (int64_t)K);
#pragma unroll
        for (int v = 0; v < MAXV; ++v) {
            const int idx = v * TPR + t; // (lanes past the row hold 0 + 0)
            const unsigned a[4] = {x[v].x, x[v].y, x[v].z, x[v].w};
            const unsigned b[4] = {r[v].x, r[v].y, r[v].z, r[v].w};
            unsigned o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if constexpr (BF) o[e] = __builtin_bit_cast(unsigned, bf2_add(__builtin_bit_cast(v2h, a[e]), b[e])); // (packed: one conversion per pair)
                else o[e] = (unsigned)hadd_bits((uint16_t)(a[e] & 0xffffu), (uint16_t)(b[e] & 0xffffu)) |
                            ((unsigned)hadd_bits((uint16_t)(a[e] >> 16), (uint16_t)(b[e] >> 16)) << 16);
            x[v] = make_uint4(o[0], o[1], o[2], o[3]);
            if (row_ok && idx < nvec) hdst[idx] = x[v];
        }
    }

    float ss = 0.f;
#pragma unroll
    for (int v = 0; v < MAXV; ++v) {
        const unsigned w[4] = {x[v].x, x[v].y, x[v].z, x[v].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a = o2f<BF>((uint16_t)(w[e] & 0xffffu)), b = o2f<BF>((uint16_t)(w[e] >> 16));
            ss = __builtin_fmaf(a, a, ss);
            ss = __builtin_fmaf(b, b, ss);
        }
    }
    if constexpr (BF) { // the row stays PACKED across the reduction: bf16 -> fp32 is a shift, and without this the compiler keeps the
                        // widened copy of the whole row live for the normalisation (twice the registers, half the occupancy)
#pragma unroll
        for (int v = 0; v < MAXV; ++v) asm("" : "+v"(x[v].x), "+v"(x[v].y), "+v"(x[v].z), "+v"(x[v].w));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off, 64);
    if (TPR > 64) {
        if ((tid & 63) == 0) redf[tid >> 6] = ss;
        __syncthreads();
        ss = (redf[0] + redf[1]) + (redf[2] + redf[3]);
    }
    const float rstd = 1.0f / __builtin_sqrtf(ss / (float)K + eps);

    // normalise in place (registers now hold the fp16 result), stage the row in LDS for the gather
    unsigned m2 = 0u;
#pragma unroll
    for (int v = 0; v < MAXV; ++v) {
        const int idx = v * TPR + t;
        if (idx < nvec) {
            const uint4 gv = GPRE ? gpre[v] : g4[idx];
            const unsigned w[4] = {x[v].x, x[v].y, x[v].z, x[v].w};
            const unsigned gw[4] = {gv.x, gv.y, gv.z, gv.w};
            unsigned o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = (o2f<BF>((uint16_t)(w[e] & 0xffffu)) * rstd) * o2f<BF>((uint16_t)(gw[e] & 0xffffu));
                float b = (o2f<BF>((uint16_t)(w[e] >> 16)) * rstd) * o2f<BF>((uint16_t)(gw[e] >> 16));
                if (!BF) { // (fp16 overflow guard; bf16 has fp32's range)
                    a = a > 0.f ? __builtin_fminf(a, 64504.f) : __builtin_fmaxf(a, -64504.f);
                    b = b > 0.f ? __builtin_fminf(b, 64504.f) : __builtin_fmaxf(b, -64504.f);
                }
                // (plain norm: one packed conversion per pair keeps the store loop's registers at the fp16 form's; in front of the
                //  quantiser the per-element form allocates fewer -- profiles/bf16_norm_resource_usage.txt)
                if constexpr (BF && QUANT == 0) o[e] = __builtin_bit_cast(unsigned, f2bf2_of_f32_results(a, b));
                else if constexpr (BF) o[e] = (unsigned)f2bf_bits(a) | ((unsigned)f2bf_bits(b) << 16);
                else o[e] = (unsigned)f2h_bits_of_f32_result(a) | ((unsigned)f2h_bits_of_f32_result(b) << 16);
            }
            x[v] = make_uint4(o[0], o[1], o[2], o[3]);
            if (QUANT) reinterpret_cast<uint4*>(lrow)[idx] = x[v];
        }
    }
    if (QUANT) {
        if (TPR > 64) __syncthreads(); // the whole row is in LDS (one wave per row needs no barrier: LDS ops are in order)
        if (row_ok)
            for (int j = t; j < O; j += TPR) {
                const int c = ind[j];
                outl[row * (int64_t)O + j] = (c >= 0 && c < K) ? lrow[c] : (uint16_t)0;
            }
#pragma unroll
        for (int v = 0; v < MAXV; ++v) {
            const int idx = v * TPR + t;
            if (idx < nvec) {
                const unsigned m8 = (zmask[idx >> 2] >> ((idx & 3) * 8)) & 0xffu;
                unsigned w[4] = {x[v].x, x[v].y, x[v].z, x[v].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (m8 & (1u << (2 * e))) w[e] &= 0xffff0000u;
                    if (m8 & (2u << (2 * e))) w[e] &= 0x0000ffffu;
                    m2 = pk_max_u16(m2, w[e] & 0x7fff7fffu); // |x| bit patterns, NaN patterns included
                }
                x[v] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    }
    // the normalised row (outlier columns zeroed when quantising), one 16-byte store per vector
    uint4* __restrict__ dsto = reinterpret_cast<uint4*>(out + (row_ok ? row : 0) * (int64_t)K);
#pragma unroll
    for (int v = 0; v < MAXV; ++v) {
        const int idx = v * TPR + t;
        if (row_ok && idx < nvec) dsto[idx] = x[v];
    }
    if (!QUANT) return;

    auto row_max = [&](int val) __attribute__((always_inline)) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) val = max(val, __shfl_xor(val, off, 64));
        if (TPR > 64) {
            __syncthreads(); // (also orders a second use of redi[])
            if ((tid & 63) == 0) redi[tid >> 6] = val;
            __syncthreads();
            val = max(max(redi[0], redi[1]), max(redi[2], redi[3]));
        }
        return val;
    };
    const int amax_all = row_max((int)max(m2 & 0xffffu, m2 >> 16));
    int amax = amax_all;
    if (amax_all > INF_BITS) { // a NaN in the row: max with NaNs dropped (__hmax); -1 = every element is NaN
        amax = -1;
#pragma unroll
        for (int v = 0; v < MAXV; ++v) {
            const unsigned w[4] = {x[v].x, x[v].y, x[v].z, x[v].w};
            if (v * TPR + t < nvec) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int lo = (int)(w[e] & 0x7fffu), hi = (int)((w[e] >> 16) & 0x7fffu);
                    lo = lo > INF_BITS ? -1 : lo;
                    hi = hi > INF_BITS ? -1 : hi;
                    amax = max(amax, max(lo, hi));
                }
            }
        }
        amax = row_max(amax);
    }
    const uint16_t amax_bits = amax < 0 ? (uint16_t)0x7fffu : (uint16_t)amax;
    const uint16_t s_bits = BF ? f2bf_bits(bf2f(amax_bits) / 127.0f) : f2h_bits(h2f(amax_bits) / (QUANT == 4 ? 7.0f : 127.0f));
    const float s = o2f<BF>(s_bits);
    const float rs = 1.0f / s;
    if (row_ok && t == 0) scale[row] = s_bits;
    if (QUANT == 4) { // packed int4 pairs: element 2i in the low nibble (cutlass::int4b_t), low 4 bits of half2int_rn
        unsigned* __restrict__ dst4 = reinterpret_cast<unsigned*>(q + (row_ok ? row : 0) * (int64_t)(K >> 1));
        for (int v = 0; v < MAXV; ++v) {
            const int idx = v * TPR + t;
            if (row_ok && idx < nvec) {
                const unsigned w[4] = {x[v].x, x[v].y, x[v].z, x[v].w};
                unsigned o = 0u;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned q0 = (unsigned)quant_one(h2f((uint16_t)(w[e] & 0xffffu)), s) & 0xfu;
                    const unsigned q1 = (unsigned)quant_one(h2f((uint16_t)(w[e] >> 16)), s) & 0xfu;
                    o |= (q0 | (q1 << 4)) << (8 * e);
                }
                dst4[idx] = o;
            }
        }
        return;
    }
    uint2* __restrict__ dstq = reinterpret_cast<uint2*>(q + (row_ok ? row : 0) * (int64_t)K);
    auto slot = [&](int idx) __attribute__((always_inline)) -> uint2* { // 8-byte group idx of this row -> its place in the image
        if (!FRAG) return dstq + idx;
        const int64_t r = row_ok ? row : 0;
        const int64_t blk = (r >> 4) * ((K + 63) >> 6) + (idx >> 3);
        return reinterpret_cast<uint2*>(q + (blk << 10) + (((idx >> 1) & 3) << 8) + ((r & 15) << 4) + ((idx & 1) << 3));
    };
    const bool stream_out = !FRAG && (int64_t)M * K >= ((int64_t)8 << 20); // prefill-size images: non-temporal stores (launch-uniform)
    if constexpr (BF) { // one IEEE quotient per element, every case (quant_extract_kernel's BF form)
#pragma unroll
        for (int v = 0; v < MAXV; ++v) {
            const int idx = v * TPR + t;
            if (row_ok && idx < nvec) {
                typedef unsigned v2u_ __attribute__((ext_vector_type(2)));
                const unsigned w[4] = {x[v].x, x[v].y, x[v].z, x[v].w};
                unsigned o[2] = {0u, 0u};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int q0 = quant_one_bf16(bf2f((uint16_t)(w[e] & 0xffffu)), s);
                    const int q1 = quant_one_bf16(bf2f((uint16_t)(w[e] >> 16)), s);
                    o[e >> 1] |= (unsigned)(q0 | (q1 << 8)) << ((e & 1) * 16);
                }
                if (stream_out) __builtin_nontemporal_store(v2u_{o[0], o[1]}, reinterpret_cast<v2u_*>(slot(idx)));
                else *slot(idx) = make_uint2(o[0], o[1]);
            }
        }
    } else if (amax_all < 0x7c00 && s_bits != 0) { // every element finite, scale finite and non-zero (row-uniform)
#pragma unroll
        for (int v = 0; v < MAXV; ++v) {
            const int idx = v * TPR + t;
            if (row_ok && idx < nvec) {
                typedef unsigned v2u_ __attribute__((ext_vector_type(2)));
                const uint2 q8 = quant_vec8_finite(x[v], s, rs);
                if (stream_out) __builtin_nontemporal_store(v2u_{q8.x, q8.y}, reinterpret_cast<v2u_*>(slot(idx))); // (quant_kernels.hip)
                else *slot(idx) = q8;
            }
        }
    } else {
        for (int v = 0; v < MAXV; ++v) {
            const int idx = v * TPR + t;
            if (row_ok && idx < nvec) {
                const unsigned w[4] = {x[v].x, x[v].y, x[v].z, x[v].w};
                unsigned o[2] = {0u, 0u};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int q0 = quant_one(h2f((uint16_t)(w[e] & 0xffffu)), s);
                    const int q1 = quant_one(h2f((uint16_t)(w[e] >> 16)), s);
                    o[e >> 1] |= (unsigned)(q0 | (q1 << 8)) << ((e & 1) * 16);
                }
                *slot(idx) = make_uint2(o[0], o[1]);
            }
        }
    }
}

// one name per instantiation and store form, built on its first launch (reporting only: mixq_debug_last_producer_kernel);
// the ADD forms carry ",ADD=1" behind FRAG, the others keep the names they had; a bf16 launch is the fp16 form's name + " [bf16]"
// (the quantiser's convention), " nt" behind it
static std::string norm_form_name(int tpr, int maxv, int quant, bool frag, bool add, bool bf, bool nt)
{
    std::string n = producer_form_name("rmsnorm_quant_kernel", tpr, maxv, "QUANT", quant, frag, false);
    if (add) n.insert(n.size() - 1, ",ADD=1"); // "...,FRAG=0,ADD=1>"
    return n + (bf ? " [bf16]" : "") + (nt ? " nt" : "");
}

template <int TPR, int MAXV, int QUANT, bool FRAG, bool ADD, bool BF>
static void note_norm(bool nt)
{
    static const std::string n[2] = {norm_form_name(TPR, MAXV, QUANT, FRAG, ADD, BF, false),
                                     norm_form_name(TPR, MAXV, QUANT, FRAG, ADD, BF, true)};
    note_producer_kernel(n[nt ? 1 : 0].c_str());
}

template <int TPR, int MAXV, bool ADD, bool BF>
static hipError_t launch_norm(const uint16_t* X, const uint16_t* gamma, uint16_t* out, uint16_t* outl,
                              const int32_t* ind, int8_t* q, uint16_t* scale, float eps, int M, int K, int O,
                              int quant, hipStream_t st, int q_layout, const uint16_t* R, uint16_t* H)
{
    if constexpr (TPR == 256 && MAXV <= 8) {
        if (q_layout == 1 && quant == 8) {
            const size_t lds = (size_t)((K + 127) / 128) * 16 + (size_t)K * 2;
            static DeviceOnce oncef;
            if (hipError_t e = ensure_dynamic_lds(rmsnorm_quant_kernel<TPR, MAXV, 8, true, ADD, BF>, 160 * 1024 - 64, oncef); e != hipSuccess)
                return e;
            note_norm<TPR, MAXV, 8, true, ADD, BF>(false);
            hipLaunchKernelGGL((rmsnorm_quant_kernel<TPR, MAXV, 8, true, ADD, BF>), dim3((unsigned)M), dim3(NBLOCK), lds, st, X, gamma, out,
                               outl, ind, q, scale, eps, M, K, O, R, H);
            return hipGetLastError();
        }
    }
    if (q_layout != 0) return hipErrorInvalidValue;
    constexpr int RPB = NBLOCK / TPR;
    const dim3 grid((unsigned)((M + RPB - 1) / RPB)), block(NBLOCK);
    if (quant) {
        const size_t lds = (size_t)((K + 127) / 128) * 16 + (size_t)RPB * K * 2;
        // rows of 8192 x 4 waves need more than the default 64 KiB of dynamic LDS
        static DeviceOnce once8, once4;
        if (hipError_t e = ensure_dynamic_lds(rmsnorm_quant_kernel<TPR, MAXV, 8, false, ADD, BF>, 160 * 1024 - 64, once8); e != hipSuccess)
            return e;
        if constexpr (BF) { // (QUANT == 8 only)
            if (quant != 8) return hipErrorInvalidValue;
            note_norm<TPR, MAXV, 8, false, ADD, true>((int64_t)M * K >= ((int64_t)8 << 20));
            hipLaunchKernelGGL((rmsnorm_quant_kernel<TPR, MAXV, 8, false, ADD, true>), grid, block, lds, st, X, gamma, out, outl, ind, q,
                               scale, eps, M, K, O, R, H);
            return hipGetLastError();
        } else {
            if (hipError_t e = ensure_dynamic_lds(rmsnorm_quant_kernel<TPR, MAXV, 4, false, ADD>, 160 * 1024 - 64, once4); e != hipSuccess)
                return e;
            if (quant == 4) note_norm<TPR, MAXV, 4, false, ADD, false>(false);
            else note_norm<TPR, MAXV, 8, false, ADD, false>((int64_t)M * K >= ((int64_t)8 << 20)); // (the kernel's stream_out)
            if (quant == 4)
                hipLaunchKernelGGL((rmsnorm_quant_kernel<TPR, MAXV, 4, false, ADD>), grid, block, lds, st, X, gamma, out, outl, ind, q,
                                   scale, eps, M, K, O, R, H);
            else
                hipLaunchKernelGGL((rmsnorm_quant_kernel<TPR, MAXV, 8, false, ADD>), grid, block, lds, st, X, gamma, out, outl, ind, q,
                                   scale, eps, M, K, O, R, H);
        }
    } else {
        note_norm<TPR, MAXV, 0, false, ADD, BF>(false);
        hipLaunchKernelGGL((rmsnorm_quant_kernel<TPR, MAXV, 0, false, ADD, BF>), grid, block, 0, st, X, gamma, out, outl, ind, q,
                           scale, eps, M, K, O, R, H);
    }
    return hipGetLastError();
}

// The form rules, once for every call (ADD: with the residual add in front; BF: bf16 rows): the same (M, K, quant, q_layout) takes
// the same TPR / MAXV / grid either way, so the reduction order -- and with it every bit -- is that of the unfused sequence.
template <bool ADD, bool BF>
static hipError_t launch_rmsnorm_form(const uint16_t* x, const uint16_t* g, uint16_t* o, uint16_t* ol, const int32_t* ind, int8_t* q,
                                      uint16_t* sc, float eps, int M, int K, int O, int quant, hipStream_t st, int q_layout,
                                      const uint16_t* r, uint16_t* h)
{
    const int nvec = K / 8;
    // Decode batches (few rows: the launch is a chain of latencies, not a stream): a whole 256-thread block per row, so that
    // a row is ONE load round trip of 1-4 vectors per lane instead of 8-16 on a single wavefront -- the same rule as the
    // quantiser's (quant_kernels.hip); 32 x 4096: 11.0 -> ~4.5 us for the fused producer (profiles/r03_small_m_timeline.txt)
    if ((M <= quant_block_rows(nvec, true) || q_layout == 1) && nvec > 64 * 2) { // (round 5: at every size here -- the table in quant_kernels.hip)
        if (nvec <= 256 * 2) return launch_norm<256, 2, ADD, BF>(x, g, o, ol, ind, q, sc, eps, M, K, O, quant, st, q_layout, r, h);
        if (nvec <= 256 * 4) return launch_norm<256, 4, ADD, BF>(x, g, o, ol, ind, q, sc, eps, M, K, O, quant, st, q_layout, r, h);
    }
    if (nvec <= 64 * 2) return launch_norm<64, 2, ADD, BF>(x, g, o, ol, ind, q, sc, eps, M, K, O, quant, st, 0, r, h);
    if (nvec <= 64 * 4) return launch_norm<64, 4, ADD, BF>(x, g, o, ol, ind, q, sc, eps, M, K, O, quant, st, 0, r, h);
    if (nvec <= 64 * 8) return launch_norm<64, 8, ADD, BF>(x, g, o, ol, ind, q, sc, eps, M, K, O, quant, st, 0, r, h);
    if (nvec <= 64 * 16) return launch_norm<64, 16, ADD, BF>(x, g, o, ol, ind, q, sc, eps, M, K, O, quant, st, 0, r, h);
    if (nvec <= 256 * 8) return launch_norm<256, 8, ADD, BF>(x, g, o, ol, ind, q, sc, eps, M, K, O, quant, st, q_layout, r, h);
    if (nvec <= 256 * 16) return launch_norm<256, 16, ADD, BF>(x, g, o, ol, ind, q, sc, eps, M, K, O, quant, st, 0, r, h);
    return hipErrorInvalidValue;
}

// quant = 0: plain RMSNorm (only `out`), 8 / 4: fused producer.  hipErrorInvalidValue for rows longer than 32768.
// residual / h_out (both or neither): the row is h = fp16(X + residual), written to h_out (which may be X or residual).
// bf16: every 16-bit operand is bf16 (quant 0 / 8 only).
hipError_t launch_rmsnorm_quant(const void* X, const void* gamma, void* out, void* outl, const int32_t* ind, int8_t* q,
                                void* scale, float eps, int M, int K, int O, int quant, hipStream_t st, int q_layout,
                                const void* residual, void* h_out, bool bf16)
{
    if (bf16 && quant != 0 && quant != 8) return hipErrorInvalidValue;
    if (q_layout != 0 && !(q_layout == 1 && quant == 8 && quant_frag_layout_supported(M, K))) return hipErrorInvalidValue;
    if ((residual == nullptr) != (h_out == nullptr)) return hipErrorInvalidValue;
    if (M <= 0) return hipSuccess;
    const uint16_t* x = static_cast<const uint16_t*>(X);
    const uint16_t* g = static_cast<const uint16_t*>(gamma);
    uint16_t* o = static_cast<uint16_t*>(out);
    uint16_t* ol = static_cast<uint16_t*>(outl);
    uint16_t* sc = static_cast<uint16_t*>(scale);
    const uint16_t* r = static_cast<const uint16_t*>(residual);
    uint16_t* h = static_cast<uint16_t*>(h_out);
    if (bf16)
        return residual ? launch_rmsnorm_form<true, true>(x, g, o, ol, ind, q, sc, eps, M, K, O, quant, st, q_layout, r, h)
                        : launch_rmsnorm_form<false, true>(x, g, o, ol, ind, q, sc, eps, M, K, O, quant, st, q_layout, nullptr, nullptr);
    if (residual) return launch_rmsnorm_form<true, false>(x, g, o, ol, ind, q, sc, eps, M, K, O, quant, st, q_layout, r, h);
    return launch_rmsnorm_form<false, false>(x, g, o, ol, ind, q, sc, eps, M, K, O, quant, st, q_layout, nullptr, nullptr);
}

} // namespace mixq
