// The selected query's low-resolution mask up-sampled to image b's own size, as a plane: the bits the evaluator scored
// (upsample.h), written out for the bilateral refinement (fp64 targets) and for E-measure / weighted F (8-bit planes).  One kernel
// over where image b's plane lies and what a value is stored as, one launcher, the three entry points; and the byte-to-float copies
// that bring the solver's 0/1 result back as a one-query "mask_pred" for the metric kernels (BASELINE.json configs[2]).
#include "common.h"

// same discipline as eval.hip: no contraction, fused ops only where up_sample writes them
#pragma clang fp contract(off)
#include "upsample.h"

namespace sm {

constexpr int SEL_MAX_PIXELS = 1 << 22;  // of an 8-bit plane: sm_sod_metrics_u8's limit

// ---- layouts: where image b's plane lies in `out` and how large it is; scale(): what its entry point lets the `scale` argument
// be, told to the compiler - the walk is a few pixels per lane, and the general rule's four divisions ahead of it are a microsecond ----
struct Plane { int64_t off; int H, W; };
struct OneSize {  // one (OH, OW) for the whole batch, plane b at b * OH * OW; a size, never a factor
    int OH, OW;
    static constexpr bool covered = true;  // sy = mh / OH keeps the source row under mh - 0.5: no pixel lies outside the up-sampled plane
    __device__ __forceinline__ Plane plane(int b) const { return {(int64_t)b * OH * OW, OH, OW}; }
    __device__ __forceinline__ float scale(float) const { return 0.f; }
};
struct PackedPlanes {  // a MixedBatch / PackedImages table; a factor, never a size
    const sm_bilateral_image* __restrict__ images;
    static constexpr bool covered = false;
    __device__ __forceinline__ Plane plane(int b) const { const sm_bilateral_image im = images[b]; return {im.px_off, im.H, im.W}; }
    __device__ __forceinline__ float scale(float s) const { __builtin_assume(s > 0.f); return s; }
};
struct GtPlanes {  // a GtBatch table: the plane lies where the ground truth does; either mode
    const sm_eval_image* __restrict__ images;
    static constexpr bool covered = false;
    __device__ __forceinline__ Plane plane(int b) const { const sm_eval_image im = images[b]; return {im.gt_off, im.H, im.W}; }
    __device__ __forceinline__ float scale(float s) const { return s; }
};

// ---- stores: the solver's fp64 target (bilateral_solver.py:181: target cast to np.double), or the predictor's soft byte ----
__device__ __forceinline__ void plane_store(double* o, float v) { *o = (double)v; }
__device__ __forceinline__ void plane_store(unsigned char* o, float v) { *o = (unsigned char)up_soft_u8(v); }

// scale > 0: F.interpolate(scale_factor=scale)[..., :H_b, :W_b]; 0: F.interpolate(size=(H_b, W_b)) - mask_src, as sm_evaluate_masks_f32
template <typename Layout, typename T>
__global__ __launch_bounds__(256) void selected_plane_kernel(const float* __restrict__ masks, int64_t stride_b, const float* __restrict__ rows,
                                                             int sel_col, Layout layout, T* __restrict__ out, int mh, int mw, float scale) {
    const int b = blockIdx.y;
    const Plane pl = layout.plane(b);
    const int npx = pl.H * pl.W;
    if ((int)blockIdx.x * 256 >= npx) return;
    const int q = (int)rows[(int64_t)b * 16 + sel_col];  // query index written by eval_finalize_kernel (column 14 / 15)
    const auto src = mask_src<const float* __restrict__>(masks + (int64_t)b * stride_b + (int64_t)q * mh * mw, mh, mw, layout.scale(scale), pl.H, pl.W);
    T* __restrict__ o = out + pl.off;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < npx; p += gridDim.x * 256) {
        const int y = p / pl.W, x = p - y * pl.W;
        plane_store(o + p, Layout::covered ? src.inside(y, x) : src.value(y, x));
    }
}

// grid of the plane walks: 256-pixel workgroups over the largest image, at most 256 of them per image
static dim3 plane_grid(int max_pixels, int B) { return dim3((max_pixels + 255) / 256 < 256 ? (max_pixels + 255) / 256 : 256, B); }

// `ok`: what the entry point asks of its own arguments; `domain`: how its error text names that
template <typename Layout, typename T>
static int launch_selected(const char* name, bool ok, const char* domain, const float* masks, int64_t stride_b, const float* rows, int sel_col,
                           Layout layout, T* out, int B, int mh, int mw, float scale, int max_pixels, void* stream) {
    SM_REQUIRE(ok && masks && rows && out && B > 0 && B <= 65535 && mh > 0 && mw > 0 && max_pixels > 0 && (sel_col == 14 || sel_col == 15),
               "%s: bad arguments (sel_col 14 = picked query, 15 = upper bound%s)", name, domain);
    hipLaunchKernelGGL((selected_plane_kernel<Layout, T>), plane_grid(max_pixels, B), dim3(256), 0, (hipStream_t)stream, masks, stride_b, rows,
                       sel_col, layout, out, mh, mw, scale);
    return check_launch(name);
}

__global__ __launch_bounds__(256) void eval_u8_to_f32_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = (float)src[i];
}

__global__ __launch_bounds__(256) void eval_planes_u8_to_f32_kernel(const unsigned char* __restrict__ src,
                                                                   const sm_bilateral_image* __restrict__ images,
                                                                   float* __restrict__ dst, int Hmax, int Wmax) {
    const int b = blockIdx.y;
    const sm_bilateral_image im = images[b];
    const int npx = im.H * im.W;
    if ((int)blockIdx.x * 256 >= npx || im.H > Hmax || im.W > Wmax) return;
    const unsigned char* s = src + im.px_off;
    float* d = dst + (int64_t)b * Hmax * Wmax;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < npx; p += gridDim.x * 256) {
        const int y = p / im.W, x = p - y * im.W;
        d[(int64_t)y * Wmax + x] = (float)s[p];
    }
}

}  // namespace sm

extern "C" int sm_upsample_selected_f64(const float* masks, int64_t mask_stride_b, const float* rows, int32_t sel_col, double* out,
                                        int32_t B, int32_t mh, int32_t mw, int32_t OH, int32_t OW, void* stream) {
    return sm::launch_selected("sm_upsample_selected_f64", OH > 0 && OW > 0, "", masks, mask_stride_b, rows, sel_col, sm::OneSize{OH, OW}, out,
                               B, mh, mw, 0.f, OH * OW, stream);
}

extern "C" int sm_upsample_selected_native_f64(const float* masks, int64_t mask_stride_b, const float* rows, int32_t sel_col,
                                               const sm_bilateral_image* images, double* out, int32_t B, int32_t mh,
                                               int32_t mw, float scale, int32_t max_pixels, void* stream) {
    return sm::launch_selected("sm_upsample_selected_native_f64", images && scale > 0.f, "; scale > 0", masks, mask_stride_b, rows, sel_col,
                               sm::PackedPlanes{images}, out, B, mh, mw, scale, max_pixels, stream);
}

extern "C" int sm_upsample_selected_u8(const float* masks, int64_t mask_stride_b, const float* rows, int32_t sel_col,
                                       const sm_eval_image* images, uint8_t* out, int32_t B, int32_t mh, int32_t mw, float scale,
                                       int32_t max_pixels, void* stream) {
    static_assert(sm::SEL_MAX_PIXELS == 4194304, "the number in the error text");
    return sm::launch_selected("sm_upsample_selected_u8", images && scale >= 0.f && max_pixels <= sm::SEL_MAX_PIXELS,
                               "; scale >= 0; max_pixels <= 4194304", masks, mask_stride_b, rows, sel_col, sm::GtPlanes{images}, out, B, mh, mw,
                               scale, max_pixels, stream);
}

extern "C" int sm_mask_u8_to_f32(const uint8_t* src, float* dst, int64_t n, void* stream) {
    SM_REQUIRE(src && dst && n > 0, "sm_mask_u8_to_f32: bad arguments");
    const int64_t g = (n + 255) / 256;
    hipLaunchKernelGGL(sm::eval_u8_to_f32_kernel, dim3((int)(g < 2048 ? g : 2048)), dim3(256), 0, (hipStream_t)stream, src, dst, n);
    return sm::check_launch("sm_mask_u8_to_f32");
}

extern "C" int sm_mask_planes_u8_to_f32(const uint8_t* src, const sm_bilateral_image* images, float* dst, int32_t B,
                                        int32_t Hmax, int32_t Wmax, int32_t max_pixels, void* stream) {
    SM_REQUIRE(src && images && dst && B > 0 && B <= 65535 && Hmax > 0 && Wmax > 0 && max_pixels > 0,
               "sm_mask_planes_u8_to_f32: bad arguments");
    hipLaunchKernelGGL(sm::eval_planes_u8_to_f32_kernel, sm::plane_grid(max_pixels, B), dim3(256), 0, (hipStream_t)stream, src, images, dst,
                       Hmax, Wmax);
    return sm::check_launch("sm_mask_planes_u8_to_f32");
}
