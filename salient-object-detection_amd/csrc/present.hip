// The serving response's images on the device (SelfMaskInference.predict, app.py:296-311): the selected low-resolution mask
// -> 8 bits -> Pillow's LANCZOS resize to the upload's size -> jet colour table -> Image.blend with the upload ->
// ImageEnhance.Brightness, bit for bit what Pillow and matplotlib compute on the host.
//
// Resize = Pillow's ImagingResample on one 8-bit band, as preprocess.hip applies it to RGB: horizontal pass first, the
// intermediate rounded and clipped to uint8, then the vertical pass; a pass whose input and output lengths agree is skipped
// (ks = 0 in the image's descriptor), as Pillow's need_horizontal / need_vertical skip it.  The 22-bit taps come from the
// host (resample.pil_coeffs, bound as present.pil_lanczos_coeffs), the kernels apply them in int32 through resample.h.
//   P1  present_h_kernel   one workgroup per (row of the low-resolution mask, 256 output columns): the row is quantised into LDS
//                          once, every lane runs the tap loop of its output column -> uint8 intermediate (mh x W) in the workspace
//   P2  present_v_kernel   one lane per four consecutive pixels of the packed output, cut so that the lane's 4-byte mask store and
//                          16-byte RGBA store are aligned (the cut depends on px_off, not on W: a group may cross a row end, and
//                          the first / last group of an image may be partial - those store pixel by pixel).  Vertical taps on the
//                          intermediate, colour table from LDS, blend and brightness in fp32.
// The intermediate lives in the caller's workspace, not in LDS: it is mh x W bytes (54 KiB for a 28-row mask at 1920 columns, 8 MiB at
// the ABI's limits), every output row reads up to ks of its rows, and a per-tile recomputation would run the horizontal tap loop once
// per output row instead of once per mask row.  It is written once and read from the L2.
// Blend.c does not fuse its multiply and add: contraction is off for this file.
#include "resample.h"

#pragma clang fp contract(off)

namespace sm {

constexpr int PR_THREADS = 256;
constexpr int PR_MAX_MASK = SM_PRESENT_MAX_MASK;
constexpr int PR_MAX_PIXELS = SM_PRESENT_MAX_PIXELS;

__host__ __device__ __forceinline__ int pr_pitch(int max_w) { return (max_w + 3) & ~3; }

// (uint8)(m * 255.0f) of a value in [0, 1]; NaN gives 0
__device__ __forceinline__ int pr_quant(float m) {
    const float t = m * 255.0f;
    return t >= 255.0f ? 255 : (t >= 0.0f ? (int)t : 0);
}

// Blend.c: in1 + alpha * (in2 - in1) on the integer difference, the multiply and the add rounded separately (plain operators under
// the pragma above: the instructions carry no contraction flag, which the bodies of __fmul_rn / __fadd_rn, parsed before it, do)
__device__ __forceinline__ float pr_mix(int a, int b, float alpha) {
    const float p = alpha * (float)(b - a);
    return (float)a + p;
}

// one RGBA pixel of the heat map: blend(upload, colour, alpha) truncated, then blend(degenerate, that, brightness) clipped; the
// degenerate image of ImageEnhance.Brightness is black with the blended image's own alpha
__device__ __forceinline__ unsigned pr_heat(unsigned lut, int r, int g, int b, float alpha, float brightness) {
    const int o[4] = {r, g, b, 255};
    unsigned out = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int l = (int)((lut >> (8 * c)) & 255u);
        const int bl = (int)(unsigned char)pr_mix(o[c], l, alpha);
        const int d = c == 3 ? bl : 0;
        const float t = pr_mix(d, bl, brightness);
        const int v = t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
        out |= (unsigned)v << (8 * c);
    }
    return out;
}

__global__ __launch_bounds__(PR_THREADS) void present_h_kernel(const float* __restrict__ masks, int64_t mask_stride_b, int mh, int mw,
                                                               const sm_present_image* __restrict__ imgs, const int* __restrict__ coef,
                                                               unsigned char* __restrict__ ws, int pitch) {
    __shared__ int row[PR_MAX_MASK];
    const int b = blockIdx.z, y = blockIdx.y;
    const sm_present_image im = imgs[b];
    const int W = im.W;
    if (W <= 0 || W > pitch || (int)blockIdx.x * PR_THREADS >= W) return;  // (a device table that disagrees with the host's)
    const float* __restrict__ m = masks + (int64_t)b * mask_stride_b + (int64_t)y * mw;
    for (int x = threadIdx.x; x < mw; x += PR_THREADS) row[x] = pr_quant(m[x]);
    __syncthreads();
    const int xx = blockIdx.x * PR_THREADS + threadIdx.x;
    if (xx >= W) return;
    unsigned char* __restrict__ o = ws + ((int64_t)b * mh + y) * pitch;
    const RsTaps t = rs_taps(coef, im.coef_x, im.ksx, W, mw, xx);
    if (!t.k) {  // pass skipped: W == mw
        o[xx] = (unsigned char)row[t.first];
        return;
    }
    int s = RS_HALF;
    for (int i = 0; i < t.n; ++i) s += row[t.first + i] * t.k[i];
    o[xx] = (unsigned char)rs_clip8(s);
}

// the vertical taps of output row y (k == nullptr: pass skipped, H == mh)
__device__ __forceinline__ RsTaps pr_taps(const sm_present_image& im, const int* __restrict__ coef, int mh, int y) {
    return rs_taps(coef, im.coef_y, im.ksy, im.H, mh, y);
}

__device__ __forceinline__ int pr_vertical_1(const RsTaps& t, const unsigned char* __restrict__ tmp, int pitch, int x) {
    const unsigned char* __restrict__ p = tmp + (int64_t)t.first * pitch + x;
    if (!t.k) return p[0];
    int s = RS_HALF;
    for (int i = 0; i < t.n; ++i) s += (int)p[(int64_t)i * pitch] * t.k[i];
    return rs_clip8(s);
}

// columns x .. x + 3 of one output row (x + 3 < W <= pitch): four intermediate bytes per load -> the four mask bytes, packed
__device__ __forceinline__ unsigned pr_vertical_4(const RsTaps& t, const unsigned char* __restrict__ tmp, int pitch, int x) {
    const unsigned char* __restrict__ p = tmp + (int64_t)t.first * pitch + x;
    unsigned w;
    if (!t.k) {
        __builtin_memcpy(&w, p, 4);
        return w;
    }
    int s0 = RS_HALF, s1 = s0, s2 = s0, s3 = s0;
    for (int i = 0; i < t.n; ++i) {
        __builtin_memcpy(&w, p + (int64_t)i * pitch, 4);
        const int c = t.k[i];
        s0 += (int)(w & 255u) * c;
        s1 += (int)((w >> 8) & 255u) * c;
        s2 += (int)((w >> 16) & 255u) * c;
        s3 += (int)(w >> 24) * c;
    }
    return (unsigned)rs_clip8(s0) | ((unsigned)rs_clip8(s1) << 8) | ((unsigned)rs_clip8(s2) << 16) | ((unsigned)rs_clip8(s3) << 24);
}

__global__ __launch_bounds__(PR_THREADS) void present_v_kernel(const unsigned char* __restrict__ ws, int mh, int pitch,
                                                               const sm_present_image* __restrict__ imgs, const int* __restrict__ coef,
                                                               const unsigned char* __restrict__ rgb, const unsigned* __restrict__ lut_rgba,
                                                               float alpha, float brightness, unsigned char* __restrict__ mask_out,
                                                               unsigned char* __restrict__ heat_out) {
    __shared__ unsigned lut[256];
    const int b = blockIdx.y;
    const sm_present_image im = imgs[b];
    const int H = im.H, W = im.W;
    if (H <= 0 || W <= 0 || W > pitch || (int64_t)H * W > PR_MAX_PIXELS || im.px_off < 0) return;
    const int npx = H * W;
    // group g holds the pixels 4 g - lead .. 4 g - lead + 3 of the image: px_off + pixel is a multiple of 4 at a group's start
    const int lead = (int)(im.px_off & 3);
    const int g = blockIdx.x * PR_THREADS + threadIdx.x;
    if ((int64_t)blockIdx.x * PR_THREADS * 4 >= (int64_t)npx + lead) return;  // the whole workgroup lies past this image
    if (heat_out) {
        lut[threadIdx.x] = lut_rgba[threadIdx.x];  // PR_THREADS == 256 entries
        __syncthreads();
    }
    const int q0 = 4 * g - lead;
    if (q0 >= npx) return;
    const unsigned char* __restrict__ tmp = ws + (int64_t)b * mh * pitch;
    const unsigned char* __restrict__ src = rgb + im.img_off;
    const int qa = q0 < 0 ? 0 : q0;
    int y = qa / W, x = qa - y * W;
    if (q0 >= 0 && q0 + 3 < npx) {  // a whole group: one 4-byte and one 16-byte store
        unsigned m4;
        if (x + 3 < W) {
            m4 = pr_vertical_4(pr_taps(im, coef, mh, y), tmp, pitch, x);
        } else {  // the group crosses a row end
            m4 = 0;
            for (int j = 0; j < 4; ++j) {
                m4 |= (unsigned)pr_vertical_1(pr_taps(im, coef, mh, y), tmp, pitch, x) << (8 * j);
                if (++x == W) { x = 0; ++y; }
            }
        }
        if (mask_out) *reinterpret_cast<unsigned*>(mask_out + im.px_off + q0) = m4;
        if (heat_out) {
            unsigned c[3];
            __builtin_memcpy(c, src + (int64_t)q0 * 3, 12);  // R G B R | G B R G | B R G B
            uint4 h;
            h.x = pr_heat(lut[m4 & 255u], c[0] & 255u, (c[0] >> 8) & 255u, (c[0] >> 16) & 255u, alpha, brightness);
            h.y = pr_heat(lut[(m4 >> 8) & 255u], c[0] >> 24, c[1] & 255u, (c[1] >> 8) & 255u, alpha, brightness);
            h.z = pr_heat(lut[(m4 >> 16) & 255u], (c[1] >> 16) & 255u, c[1] >> 24, c[2] & 255u, alpha, brightness);
            h.w = pr_heat(lut[m4 >> 24], (c[2] >> 8) & 255u, (c[2] >> 16) & 255u, c[2] >> 24, alpha, brightness);
            *reinterpret_cast<uint4*>(heat_out + (im.px_off + q0) * 4) = h;
        }
        return;
    }
    // the image's first or last group, partial: pixel by pixel
    const int qe = q0 + 4 < npx ? q0 + 4 : npx;
    for (int q = qa; q < qe; ++q) {
        const unsigned v = (unsigned)pr_vertical_1(pr_taps(im, coef, mh, y), tmp, pitch, x);
        if (mask_out) mask_out[im.px_off + q] = (unsigned char)v;
        if (heat_out) {
            const unsigned char* __restrict__ p = src + (int64_t)q * 3;
            const unsigned h = pr_heat(lut[v], p[0], p[1], p[2], alpha, brightness);
            unsigned char* o = heat_out + (im.px_off + q) * 4;
            o[0] = (unsigned char)h; o[1] = (unsigned char)(h >> 8); o[2] = (unsigned char)(h >> 16); o[3] = (unsigned char)(h >> 24);
        }
        if (++x == W) { x = 0; ++y; }
    }
}

}  // namespace sm

extern "C" size_t sm_present_workspace_bytes(int32_t B, int32_t mh, int32_t max_w) {
    if (B <= 0 || B > 65535 || mh <= 0 || mh > sm::PR_MAX_MASK || max_w <= 0 || max_w > sm::PR_MAX_PIXELS) return 0;
    return ((size_t)B * mh * sm::pr_pitch(max_w) + 255) & ~(size_t)255;
}

extern "C" int sm_present_masks_u8(const float* masks, int64_t mask_stride_b, int32_t mh, int32_t mw, const uint8_t* rgb,
                                   const sm_present_image* images_host, const sm_present_image* images_dev, const int32_t* coef,
                                   const uint8_t* lut_rgba, float blend_alpha, float brightness, uint8_t* mask_out, uint8_t* heat_out,
                                   void* workspace, size_t workspace_bytes, int32_t B, void* stream) {
    SM_REQUIRE(masks && images_host && images_dev && coef && workspace,
               "sm_present_masks_u8: null pointer (masks, the host or device image table, coef or workspace)");
    SM_REQUIRE(mask_out || heat_out, "sm_present_masks_u8: null pointer (mask_out and heat_out: nothing to compute)");
    SM_REQUIRE(!heat_out || (rgb && lut_rgba), "sm_present_masks_u8: null pointer (rgb or lut_rgba, with heat_out)");
    SM_REQUIRE(B > 0 && B <= 65535, "sm_present_masks_u8: B=%d (1 .. 65535)", B);
    SM_REQUIRE(mh >= 1 && mh <= sm::PR_MAX_MASK && mw >= 1 && mw <= sm::PR_MAX_MASK, "sm_present_masks_u8: mask %d x %d (1 .. %d each)", mh, mw,
               sm::PR_MAX_MASK);
    SM_REQUIRE(mask_stride_b >= (int64_t)mh * mw || B == 1, "sm_present_masks_u8: mask_stride_b=%lld below mh*mw", (long long)mask_stride_b);
    SM_REQUIRE(blend_alpha >= 0.0f && blend_alpha <= 1.0f, "sm_present_masks_u8: blend_alpha=%g (0 .. 1: Pillow's unclipped blend)",
               (double)blend_alpha);
    SM_REQUIRE(brightness == brightness, "sm_present_masks_u8: brightness is NaN");
    SM_REQUIRE(((uintptr_t)mask_out % 4) == 0 && ((uintptr_t)heat_out % 16) == 0 && ((uintptr_t)lut_rgba % 4) == 0 &&
                   ((uintptr_t)workspace % 4) == 0,
               "sm_present_masks_u8: misaligned pointer (mask_out 4, heat_out 16, lut_rgba 4, workspace 4 bytes)");
    int max_w = 0;
    int64_t max_px = 0;
    for (int b = 0; b < B; ++b) {
        const sm_present_image& im = images_host[b];
        SM_REQUIRE(im.H > 0 && im.W > 0 && (int64_t)im.H * im.W <= sm::PR_MAX_PIXELS, "sm_present_masks_u8: image %d is %d x %d (at most %d pixels)",
                   b, im.H, im.W, sm::PR_MAX_PIXELS);
        SM_REQUIRE(im.img_off >= 0 && im.px_off >= 0, "sm_present_masks_u8: image %d has a negative offset", b);
        SM_REQUIRE((im.ksx == 0) == (im.W == mw) && (im.ksy == 0) == (im.H == mh) && im.ksx >= 0 && im.ksy >= 0 && im.coef_x >= 0 && im.coef_y >= 0,
                   "sm_present_masks_u8: image %d: ks = 0 marks a skipped pass (W == mw / H == mh) and nothing else (ksx=%d ksy=%d)", b, im.ksx,
                   im.ksy);
        max_w = im.W > max_w ? im.W : max_w;
        max_px = (int64_t)im.H * im.W > max_px ? (int64_t)im.H * im.W : max_px;
    }
    const size_t need = sm_present_workspace_bytes(B, mh, max_w);
    SM_REQUIRE(need && workspace_bytes >= need, "sm_present_masks_u8: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const int pitch = sm::pr_pitch(max_w);
    hipLaunchKernelGGL(sm::present_h_kernel, dim3((max_w + sm::PR_THREADS - 1) / sm::PR_THREADS, mh, B), dim3(sm::PR_THREADS), 0, st, masks,
                       mask_stride_b, mh, mw, images_dev, coef, (unsigned char*)workspace, pitch);
    const int groups = (int)((max_px + 3) / 4 + 1);  // + 1: the partial leading group of an image whose px_off is no multiple of 4
    hipLaunchKernelGGL(sm::present_v_kernel, dim3((groups + sm::PR_THREADS - 1) / sm::PR_THREADS, B), dim3(sm::PR_THREADS), 0, st,
                       (const unsigned char*)workspace, mh, pitch, images_dev, coef, rgb, (const unsigned*)lut_rgba, blend_alpha, brightness,
                       mask_out, heat_out);
    return sm::check_launch("sm_present_masks_u8");
}
