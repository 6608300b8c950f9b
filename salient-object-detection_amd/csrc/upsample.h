// The bilinear up-sample of one query mask, shared by the evaluator's metric kernels (eval.hip) and the predictor's finish
// (predict.hip): both must give a pixel the same bits, so both evaluate it with these functions.
#pragma once
#include "common.h"

// The taps must round like torch's separate fp32 mul / add kernels: no contraction in a file that includes this header (the
// pragma holds for the rest of the translation unit).  Fused ops are written explicitly (__builtin_fmaf) where torch's CPU
// kernel fuses.
#pragma clang fp contract(off)

namespace sm {

struct UpIdx { int i0, i1; float l0, l1; };

// at::native::area_pixel_compute_source_index(scale, dst, align_corners=false, cubic=false) + the bilinear taps
__device__ __forceinline__ UpIdx up_index(int dst, float scale, int in_size) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    UpIdx u;
    u.i0 = (int)src;
    u.i1 = u.i0 + (u.i0 < in_size - 1 ? 1 : 0);
    u.l1 = src - (float)u.i0;
    u.l0 = 1.0f - u.l1;
    return u;
}

__device__ __forceinline__ float up_sample(const float* __restrict__ m, int mw, const UpIdx& uy, const UpIdx& ux) {
    const float p00 = m[uy.i0 * mw + ux.i0], p01 = m[uy.i0 * mw + ux.i1];
    const float p10 = m[uy.i1 * mw + ux.i0], p11 = m[uy.i1 * mw + ux.i1];
    // Bit-for-bit the arithmetic of torch-CPU's upsample_bilinear2d (ATen UpSampleKernel.cpp, compiled with fma
    // contraction; established by brute force against F.interpolate): along x then y, each level
    // fma(first_tap, w_first, second_tap * w_second).
    const float top = __builtin_fmaf(p00, ux.l0, p01 * ux.l1);
    const float bot = __builtin_fmaf(p10, ux.l0, p11 * ux.l1);
    return __builtin_fmaf(top, uy.l0, bot * uy.l1);
}

// the selected query's mask, up-sampled: value of pixel (y, x) (Ptr: LDS or global floats)
template <typename Ptr>
struct MaskSrc {
    Ptr m;
    int mh, mw;
    float sy, sx;
    __device__ __forceinline__ float value(int y, int x) const {
        const UpIdx uy = up_index(y, sy, mh), ux = up_index(x, sx, mw);
        // a pixel outside the up-sampled plane (H_b > scale * mh) is 0, as in eval_upsample_selected_native_kernel
        return uy.i0 < mh && ux.i0 < mw ? up_sample(m, mw, uy, ux) : 0.f;
    }
    __device__ __forceinline__ bool operator()(int y, int x) const { return value(y, x) > 0.5f; }
};

// the 8-bit soft value of a pixel: (mask * 255).astype(np.uint8) after clip(0, 1), truncating
__device__ __forceinline__ unsigned up_soft_u8(float v) { return (unsigned)(int)(fminf(fmaxf(v, 0.f), 1.f) * 255.0f); }

}  // namespace sm
