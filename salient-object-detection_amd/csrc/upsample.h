// The bilinear up-samples that more than one file needs.  align_corners=False on one query mask, shared by the evaluator's metric
// kernels (eval.hip), the predictor's finish (predict.hip), the object finder (objects.hip) and the selected-mask planes
// (selected.hip): all must give a pixel the same bits, so all evaluate it with these functions.  align_corners=True
// on channels-last features (upsample_aligned_kernel): one kernel for cluster.hip and conv.hip.
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
    // of a pixel that is known to lie inside the up-sampled plane
    __device__ __forceinline__ float inside(int y, int x) const { return up_sample(m, mw, up_index(y, sy, mh), up_index(x, sx, mw)); }
    __device__ __forceinline__ float value(int y, int x) const {
        const UpIdx uy = up_index(y, sy, mh), ux = up_index(x, sx, mw);
        // a pixel outside the up-sampled plane (H_b > scale * mh: not a size the crop can produce) is 0
        return uy.i0 < mh && ux.i0 < mw ? up_sample(m, mw, uy, ux) : 0.f;
    }
    __device__ __forceinline__ bool operator()(int y, int x) const { return value(y, x) > 0.5f; }
};

// source coordinate per destination pixel: F.interpolate's 1 / scale_factor, or in / out when the mask is resized to the image
__device__ __forceinline__ float source_scale(float scale, int in_size, int out_size) {
    return scale > 0.f ? 1.0f / scale : (float)in_size / (float)out_size;
}

// mask m (mh x mw) as image (H, W) sees it: scale > 0: F.interpolate(scale_factor=scale)[..., :H, :W]; 0: F.interpolate(size=(H, W))
template <typename Ptr>
__device__ __forceinline__ MaskSrc<Ptr> mask_src(Ptr m, int mh, int mw, float scale, int H, int W) {
    return {m, mh, mw, source_scale(scale, mh, H), source_scale(scale, mw, W)};
}

// F.interpolate(mode="bilinear", align_corners=True) by an integer factor on channels-last data, C % 4 == 0: image b's (gh, gw, C)
// rows start at in + b * strideb, up is dense (B, sf gh, sf gw, C).  Source coordinate o * (in - 1) / (out - 1) (ATen
// area_pixel_compute_scale / _source_index with align_corners: the scale is formed in fp32), the taps as torch-CPU writes them.
// Launched by the token up-sample of cluster.hip (strided batch) and the feature-map up-sample of conv.hip.  CT: the channel count
// when the caller knows it at compile time (cluster.hip's 384: the index split divides by a constant), 0 = the argument C.
template <int CT>
__global__ __launch_bounds__(256) void upsample_aligned_kernel(const float* __restrict__ in, int64_t strideb, float* __restrict__ up, int gh,
                                                               int gw, int c_arg, int sf, int64_t total4) {
    const int C = CT ? CT : c_arg;
    const int oh = sf * gh, ow = sf * gw, C4 = C / 4;
    const float sy = oh > 1 ? (float)(gh - 1) / (float)(oh - 1) : 0.f, sx = ow > 1 ? (float)(gw - 1) / (float)(ow - 1) : 0.f;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total4; t += (int64_t)gridDim.x * 256) {
        const int c = (int)(t % C4) * 4;
        const int64_t px = t / C4;
        const int ox = (int)(px % ow), oy = (int)((px / ow) % oh);
        const int64_t b = px / ((int64_t)ow * oh);
        const float syf = sy * oy, sxf = sx * ox;
        const int y0 = (int)syf, x0 = (int)sxf;
        const int y1 = y0 + (y0 < gh - 1 ? 1 : 0), x1 = x0 + (x0 < gw - 1 ? 1 : 0);
        const float ly1 = syf - y0, ly0 = 1.f - ly1, lx1 = sxf - x0, lx0 = 1.f - lx1;
        const float* base = in + b * strideb + c;
        const float4 p00 = *reinterpret_cast<const float4*>(base + ((int64_t)y0 * gw + x0) * C);
        const float4 p01 = *reinterpret_cast<const float4*>(base + ((int64_t)y0 * gw + x1) * C);
        const float4 p10 = *reinterpret_cast<const float4*>(base + ((int64_t)y1 * gw + x0) * C);
        const float4 p11 = *reinterpret_cast<const float4*>(base + ((int64_t)y1 * gw + x1) * C);
        float4 o;
        o.x = ly0 * (lx0 * p00.x + lx1 * p01.x) + ly1 * (lx0 * p10.x + lx1 * p11.x);
        o.y = ly0 * (lx0 * p00.y + lx1 * p01.y) + ly1 * (lx0 * p10.y + lx1 * p11.y);
        o.z = ly0 * (lx0 * p00.z + lx1 * p01.z) + ly1 * (lx0 * p10.z + lx1 * p11.z);
        o.w = ly0 * (lx0 * p00.w + lx1 * p01.w) + ly1 * (lx0 * p10.w + lx1 * p11.w);
        *reinterpret_cast<float4*>(up + px * C + c) = o;
    }
}

// the 8-bit soft value of a pixel: (mask * 255).astype(np.uint8) after clip(0, 1), truncating
__device__ __forceinline__ unsigned up_soft_u8(float v) { return (unsigned)(int)(fminf(fmaxf(v, 0.f), 1.f) * 255.0f); }

}  // namespace sm
