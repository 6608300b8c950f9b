// Encoder taps (sm_encoder_taps): launches that only READ the encoder's residual stream where it lies in the workspace after a
// block - VisionTransformer.forward's per-layer dict (vision_transformer.py:293-304) and the selections of get_tokens (:316-357),
// forward_return_n_last_blocks (:448-471) and return_patch_emb_from_n_last_blocks (:473-497).  forward.hip queues them.
#include "forward_pieces.h"

namespace sm {

// Rows of 384 floats, four rows per 64-lane wave: 16 lanes x 24 register-resident elements, the layout and the ln384_* arithmetic of
// forward_pieces.h - a normed row has the bits layernorm384_kernel gives it.  Selected row r = (image b, j < R) is read once from
// src[b * N + row0 + j] and written, normed (gamma != NULL) or raw, to dst + b * dst_image + j * 384; rows that are not selected are
// never touched.  HBM-bound: no LDS, no atomics.
__global__ __launch_bounds__(256) void encoder_tap_rows_kernel(EncoderTapRows a) {
    const int lane = threadIdx.x & 63, l16 = lane & 15;
    const int64_t rows = (int64_t)a.B * a.R;
    const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
    const bool live = row < rows;
    const int64_t rrow = live ? row : rows - 1;  // dead groups shadow the last row (they join the shuffles, never store)
    const int64_t b = rrow / a.R, j = rrow - b * a.R;
    const float* xr = a.src + (b * a.N + a.row0 + j) * SM_EMBED;
    float v[3][8];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float4 p0 = *reinterpret_cast<const float4*>(xr + (l16 + 16 * i) * 8);
        const float4 p1 = *reinterpret_cast<const float4*>(xr + (l16 + 16 * i) * 8 + 4);
        v[i][0] = p0.x; v[i][1] = p0.y; v[i][2] = p0.z; v[i][3] = p0.w;
        v[i][4] = p1.x; v[i][5] = p1.y; v[i][6] = p1.z; v[i][7] = p1.w;
    }
    const bool norm = a.gamma != nullptr;  // (kernel-uniform)
    float rstd = 0.f;
    if (norm) rstd = ln384_center(v, a.eps);
    if (!live) return;
    float* yr = a.dst + b * a.dst_image + j * SM_EMBED;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int k = (l16 + 16 * i) * 8;
        float o[8];
        if (norm) {
            ln384_affine(v[i], rstd, a.gamma, a.beta, k, o);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = v[i][e];
        }
        *reinterpret_cast<float4*>(yr + k) = make_float4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<float4*>(yr + k + 4) = make_float4(o[4], o[5], o[6], o[7]);
    }
}

// patch_mean[b][c] = mean over the n rows of tok[b] (B, n, 384), in ONE order whatever the batch: 32 columns per workgroup (a 128-B
// piece of every row), eight row segments of ceil(n / 8) rows walked top to bottom by one thread each, the eight partials added in
// segment order by the segment-0 thread.  No floating-point atomics.
constexpr int MEAN_COLS = 32, MEAN_SEGS = 8;
__global__ __launch_bounds__(MEAN_COLS* MEAN_SEGS) void encoder_patch_mean_kernel(const float* __restrict__ tok, float* __restrict__ mean,
                                                                                  int n) {
    __shared__ float part[MEAN_SEGS][MEAN_COLS];
    const int c = threadIdx.x % MEAN_COLS, seg = threadIdx.x / MEAN_COLS;
    const int col = blockIdx.x * MEAN_COLS + c, b = blockIdx.y;
    const int per = (n + MEAN_SEGS - 1) / MEAN_SEGS;
    const int r0 = seg * per, r1 = r0 + per < n ? r0 + per : n;
    const float* p = tok + (int64_t)b * n * SM_EMBED + col;
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += p[(int64_t)r * SM_EMBED];
    part[seg][c] = s;
    __syncthreads();
    if (seg == 0) {
        float t = part[0][c];
#pragma unroll
        for (int k = 1; k < MEAN_SEGS; ++k) t += part[k][c];
        mean[(int64_t)b * SM_EMBED + col] = t / (float)n;
    }
}

// the zeroed position table of the input-token tap (a kernel, not a memset node: see decoder_init_kernel in forward.hip)
__global__ __launch_bounds__(256) void encoder_tap_zero_kernel(float* __restrict__ dst, int64_t total4) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < total4) reinterpret_cast<float4*>(dst)[t] = make_float4(0.f, 0.f, 0.f, 0.f);
}

int encoder_tap_rows(const EncoderTapRows& a, hipStream_t st) {
    SM_REQUIRE(a.src && a.dst && a.B > 0 && a.N > 0 && a.R > 0 && a.row0 >= 0 && a.row0 + a.R <= a.N && a.dst_image >= (int64_t)a.R * SM_EMBED &&
                   a.dst_image % 4 == 0 && (a.gamma == nullptr) == (a.beta == nullptr),
               "encoder tap: bad rows (B=%d N=%d row0=%d R=%d)", a.B, a.N, a.row0, a.R);
    SM_REQUIRE(((uintptr_t)a.src | (uintptr_t)a.dst | (uintptr_t)a.gamma | (uintptr_t)a.beta) % 16 == 0, "encoder tap: pointers must be 16-B aligned");
    const int64_t rows = (int64_t)a.B * a.R;
    TapGuard tap(st, "encoder_tap_rows_kernel", 0.0, 2.0 * rows * SM_EMBED * 4);
    hipLaunchKernelGGL(encoder_tap_rows_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, a);
    return check_launch("encoder_tap_rows");
}

int encoder_patch_mean(const float* tok, float* mean, int B, int n, hipStream_t st) {
    SM_REQUIRE(tok && mean && B > 0 && n > 0, "encoder patch mean: bad arguments");
    TapGuard tap(st, "encoder_patch_mean_kernel", 0.0, ((double)B * n + B) * SM_EMBED * 4);
    hipLaunchKernelGGL(encoder_patch_mean_kernel, dim3(SM_EMBED / MEAN_COLS, B), dim3(MEAN_COLS * MEAN_SEGS), 0, st, tok, mean, n);
    return check_launch("encoder_patch_mean");
}

int encoder_tap_zero(float* dst, int64_t nfloat, hipStream_t st) {
    SM_REQUIRE(dst && nfloat > 0 && nfloat % 4 == 0 && (uintptr_t)dst % 16 == 0, "encoder tap: bad zero table");
    const int64_t total4 = nfloat / 4;
    hipLaunchKernelGGL(encoder_tap_zero_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, dst, total4);
    return check_launch("encoder_tap_zero");
}

}  // namespace sm
