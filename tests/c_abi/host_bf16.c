/* A plain C99 host that negotiates a bf16 call of the MixQ operator (include/mixq.h MIXQ_TYPE_BF16): it asks
 * mixq_supports_format_combination for BF16 at positions 0 / 3 / 7 and mixq_get_output_data_type_for for the output type, then runs
 * one enqueue on raw device pointers.  Test infrastructure: tests/test_gpu_bf16_operator.py writes the inputs as raw files (A and
 * fp_weight as bf16 bit patterns), runs this once with M > 4 (prefill) and once with M <= 4 (decode), and compares out.bf16 with
 * the Python binding's result.
 *   usage: host_bf16 <dir> <M> <N> <K>      exit code 0 = negotiated and enqueued; writes <dir>/out.bf16 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include "mixq.h"

static void* read_file(const char* dir, const char* name, size_t bytes)
{
    char path[1024];
    snprintf(path, sizeof path, "%s/%s", dir, name);
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    void* p = malloc(bytes);
    if (fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "%s: short read (want %zu bytes)\n", path, bytes); exit(2); }
    fclose(f);
    return p;
}

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); exit(3); } } while (0)

static void* to_device(const void* host, size_t bytes)
{
    void* d = NULL;
    HIP_OK(hipMalloc(&d, bytes));
    HIP_OK(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
    return d;
}

static mixq_tensor_desc desc(int nb, int64_t d0, int64_t d1, int32_t type)
{
    mixq_tensor_desc t;
    memset(&t, 0, sizeof t);
    t.nbDims = nb;
    t.d[0] = d0;
    t.d[1] = d1;
    t.type = type;
    t.format = MIXQ_FORMAT_LINEAR;
    t.scale = 1.0f;
    return t;
}

int main(int argc, char** argv)
{
    if (argc != 5) return 1;
    const char* dir = argv[1];
    const int M = atoi(argv[2]), N = atoi(argv[3]), K = atoi(argv[4]);
    if (mixq_abi_version() != MIXQ_ABI_VERSION) return 9;
    mixq_handle* h = mixq_create(M, N, K);
    if (!h || mixq_initialize(h) != 0) return 5;

    /* negotiation, as TensorRT would run it: BF16 on A, fp_weight and the output; everything else HALF */
    mixq_tensor_desc io[8] = {desc(2, M, K, MIXQ_TYPE_BF16), desc(2, N, K / 2, MIXQ_TYPE_HALF), desc(1, N, 0, MIXQ_TYPE_HALF),
                              desc(2, N, 128, MIXQ_TYPE_BF16), desc(1, 256, 0, MIXQ_TYPE_HALF), desc(2, K, N / 2, MIXQ_TYPE_HALF),
                              desc(1, N, 0, MIXQ_TYPE_HALF), desc(2, M, N, MIXQ_TYPE_BF16)};
    for (int pos = 0; pos < 8; ++pos)
        if (mixq_supports_format_combination(h, pos, io, 7, 1) != 1) { fprintf(stderr, "position %d refused\n", pos); return 4; }
    int32_t types[7];
    for (int i = 0; i < 7; ++i) types[i] = io[i].type;
    const int out_type = mixq_get_output_data_type_for(h, 0, types, 7);
    if (out_type != MIXQ_TYPE_BF16) return 4;

    const size_t nA = (size_t)M * K, nO = (size_t)M * N;
    void* hA = read_file(dir, "A.bf16", nA * 2);
    void* hW = read_file(dir, "weight.i8", (size_t)N * K);
    void* hsw = read_file(dir, "sw.f16", (size_t)N * 2);
    void* hfpw = read_file(dir, "fp_weight.bf16", (size_t)N * 128 * 2);
    void* hind = read_file(dir, "fp_ind.i32", 128 * 4);
    void* hqw = read_file(dir, "qweight.u8", (size_t)K * N);
    void* dA = to_device(hA, nA * 2);
    void* dW = to_device(hW, (size_t)N * K);
    void* dsw = to_device(hsw, (size_t)N * 2);
    void* dfpw = to_device(hfpw, (size_t)N * 128 * 2);
    void* dind = to_device(hind, 128 * 4);
    void* dqw = to_device(hqw, (size_t)K * N);
    void* dO = NULL;
    HIP_OK(hipMalloc(&dO, nO * 2));
    void* ws = NULL;
    const size_t ws_bytes = mixq_workspace_size(h, M, N, K);
    if (ws_bytes) HIP_OK(hipMalloc(&ws, ws_bytes));
    hipStream_t st;
    HIP_OK(hipStreamCreate(&st));

    const void* inputs[7] = {dA, dW, dsw, dfpw, dind, dqw, dsw};
    void* outputs[1] = {dO};
    const int rc = mixq_enqueue(h, io, &io[7], inputs, outputs, ws, (void*)st);
    if (rc != 0) { fprintf(stderr, "mixq_enqueue: %s\n", mixq_error_string(rc)); return 6; }
    HIP_OK(hipStreamSynchronize(st));
    uint16_t* hO = (uint16_t*)malloc(nO * 2);
    HIP_OK(hipMemcpy(hO, dO, nO * 2, hipMemcpyDeviceToHost));
    char path[1024];
    snprintf(path, sizeof path, "%s/out.bf16", dir);
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(hO, 2, nO, f) != nO) return 2;
    fclose(f);
    printf("C host (bf16): M=%d N=%d K=%d, output type %d\n", M, N, K, out_type);

    HIP_OK(hipStreamDestroy(st));
    hipFree(dA); hipFree(dW); hipFree(dsw); hipFree(dfpw); hipFree(dind); hipFree(dqw); hipFree(dO);
    if (ws) hipFree(ws);
    free(hA); free(hW); free(hsw); free(hfpw); free(hind); free(hqw); free(hO);
    mixq_terminate(h);
    mixq_destroy(h);
    return 0;
}
