// The predictor's finish: from the last decoder layer's query masks and objectness to what a caller of a saliency model wants
// per image - the arg-max query, its mask at the image's own size as COCO run boundaries, and (when asked for) packed 0/1 or
// 8-bit planes - without an up-sampled plane in between.
//
// The source of every pixel is one low-resolution mask of a few kilobytes, so a pixel is COMPUTED wherever it is needed
// (upsample.h: the bits sm_evaluate_masks_f32 scores) and the kernels walk the output in the order that output wants:
//   P0  predict_best     arg-max objectness per image, first maximum (one wave per image)
//   P1  predict_runs<count>   column-major positions q = x H + y, cut into ranges of PR_WAVE_POS per wave, PR_WAVES waves per
//                        workgroup: 64 consecutive positions per step, one lane each; a ballot gives the 64 values as one mask,
//                        mask ^ (mask << 1 | carry) marks the positions that differ from the one before, a popcount counts them
//   P2  predict_runs<emit>    the same walk again; a wave first adds up the counts of the ranges before its own (at most 1024 per
//                        image), then every marked lane stores its position at offset + popcount(marks below it)
//   P3  predict_planes   row-major, four pixels per lane and one 4-byte store: the binary / soft planes, only when asked for
// No workgroup waits on another and no atomic decides an order: the output is ascending by construction.  The selected mask is
// staged in LDS once per workgroup when it has at most PR_LDS_FLOATS values and read through L2 otherwise.
// sm_rle_runs_packed_u8 and sm_rle_runs_u8 run P1 / P2 on byte planes (packed planes of different sizes; images in the top-left corner
// of padded planes of one size), each workgroup's chunk of its plane staged in LDS in place of the bilinear evaluation.
#include "common.h"

// same discipline as eval.hip: no contraction, fused ops only where up_sample writes them
#pragma clang fp contract(off)
#include "upsample.h"

namespace sm {

constexpr int PR_THREADS = 256;
constexpr int PR_WAVES = PR_THREADS / 64;
constexpr int PR_WAVE_POS = 4096;                    // positions per wave: 64 steps of 64
constexpr int PR_CHUNK = PR_WAVES * PR_WAVE_POS;     // positions per workgroup
constexpr int PR_LDS_FLOATS = 12288;                 // staging limit: 48 KiB, under the 64-KiB default of a workgroup
constexpr int PR_MAX_PIXELS = 1 << 22;               // as sm_evaluate_masks_f32; split_index needs positions < 2^24
constexpr int PR_MAX_QUERIES = 960;

__host__ __device__ inline int pr_units(int npx) { return (npx + PR_WAVE_POS - 1) / PR_WAVE_POS; }

// ---- pixel sources: value of pixel (y, x) as 0 / 1 -------------------------------------------------------------------------
// (MaskSrc, the selected query's mask up-sampled, comes from upsample.h)
struct TileSrc {  // a byte plane's column-major positions [base, ...) as a workgroup staged them in LDS (byte_runs_kernel)
    const unsigned char* t;
    int H, base;
    __device__ __forceinline__ bool operator()(int y, int x) const { return t[x * H + y - base] != 0; }
};

// ---- the chunked walk --------------------------------------------------------------------------------------------------------
// counts: this image's per-wave-range counts [pr_units(npx)]; starts / info: this image's rows.  EMIT false: write counts[unit];
// true: write the positions (the first `cap` of them) and, from the image's first wave, info = {count, pixel 0}.
template <bool EMIT, typename Src>
__device__ __forceinline__ void runs_chunk(const Src& src, int H, int npx, int chunk, int* __restrict__ counts, int* __restrict__ starts,
                                           int cap, int* __restrict__ info) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int unit = chunk * PR_WAVES + wv, q0 = unit * PR_WAVE_POS;
    if (q0 >= npx) return;
    const int q1 = q0 + PR_WAVE_POS < npx ? q0 + PR_WAVE_POS : npx;
    const float inv_h = 1.0f / (float)H;
    int at = 0;
    if (EMIT) {
        int s = 0;
        for (int u = lane; u < unit; u += 64) s += counts[u];
        at = wave_total(s);
        if (unit == 0) {  // the image's first wave also reports the total
            const int nu = pr_units(npx);
            int t = 0;
            for (int u = lane; u < nu; u += 64) t += counts[u];
            t = wave_total(t);
            if (lane == 0) { info[0] = t; info[1] = src(0, 0) ? 1 : 0; }
        }
    }
    // the pixel before the range (pixel 0 itself for the first range: no change there); a position is q = x * H + y
    int x, y;
    split_index(q0 > 0 ? q0 - 1 : 0, H, inv_h, x, y);
    unsigned long long carry = src(y, x) ? 1ull : 0ull;
    int n = 0;
    for (int qb = q0; qb < q1; qb += 64) {
        const int q = qb + lane;
        const bool in = q < q1;
        split_index(in ? q : q1 - 1, H, inv_h, x, y);
        const bool v = src(y, x);
        const unsigned long long m = __ballot(v), valid = __ballot(in);
        const unsigned long long c = (m ^ ((m << 1) | carry)) & valid;  // bit l: position qb + l differs from the one before
        carry = m >> 63;  // only the last step of a range can be partial, and nothing follows it
        const int nc = __popcll(c);
        if (EMIT) {
            if ((c >> lane) & 1ull) {
                const int i = at + __popcll(c & ((1ull << lane) - 1ull));
                if (i < cap) starts[i] = q;
            }
            at += nc;
        }
        n += nc;
    }
    if (!EMIT && lane == 0) counts[unit] = n;
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------
// Does candidate (ov, oi) displace (bv, bi)?  The order of sm_pick_mask_f32's scan `best = 0; if (o[q] > o[best]) best = q`: the
// first maximum; a NaN never wins, except at q = 0, where nothing displaces it.  PR_NONE marks a lane without a query.
constexpr int PR_NONE = 0x7fffffff;
__device__ __forceinline__ bool best_takes(float ov, int oi, float bv, int bi) {
    if (oi == PR_NONE) return false;
    if (bi == PR_NONE) return true;
    if (bv != bv) return bi != 0;           // a NaN away from q = 0 yields to anything; at q = 0 it stays
    if (ov != ov) return oi == 0;
    return ov > bv || (ov == bv && oi < bi);
}

__global__ __launch_bounds__(64) void predict_best_kernel(const float* __restrict__ obj, int64_t obj_stride_b, int nq, int* __restrict__ best) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* o = obj + (int64_t)b * obj_stride_b;
    float bv = 0.f;
    int bi = PR_NONE;
    for (int q = lane; q < nq; q += 64) {
        const float v = o[q];
        if (best_takes(v, q, bv, bi)) { bv = v; bi = q; }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const float ov = __shfl_xor(bv, s, 64);
        const int oi = __shfl_xor(bi, s, 64);
        const bool take = best_takes(ov, oi, bv, bi);
        bv = take ? ov : bv;
        bi = take ? oi : bi;
    }
    if (lane == 0) best[b] = bi;
}

extern __shared__ float pr_tile[];

// the selected query's mask of image b for this workgroup: staged in LDS (STAGED) or left in global memory
template <bool STAGED>
__device__ __forceinline__ auto selected_mask(const sm_predict_args& a, int b, const sm_bilateral_image& im) {
    const float* __restrict__ m = a.masks + (int64_t)b * a.mask_stride_b + (int64_t)a.best[b] * a.mh * a.mw;
    if constexpr (STAGED) {
        const auto src = mask_src<const float*>(pr_tile, a.mh, a.mw, a.scale, im.H, im.W);
        for (int t = threadIdx.x; t < a.mh * a.mw; t += PR_THREADS) pr_tile[t] = m[t];
        __syncthreads();
        return src;
    } else {
        return mask_src<const float* __restrict__>(m, a.mh, a.mw, a.scale, im.H, im.W);
    }
}

template <bool EMIT, bool STAGED>
__global__ __launch_bounds__(PR_THREADS) void predict_runs_kernel(sm_predict_args a, int* __restrict__ counts, int units_max) {
    const int b = blockIdx.y;
    const sm_bilateral_image im = a.images[b];
    const int npx = im.H * im.W;
    // (a device table that disagrees with the host table the grids and the workspace were sized from writes nothing)
    if (im.H <= 0 || im.W <= 0 || npx > a.max_pixels || (int64_t)blockIdx.x * PR_CHUNK >= npx) return;
    const auto src = selected_mask<STAGED>(a, b, im);
    runs_chunk<EMIT>(src, im.H, npx, blockIdx.x, counts + (int64_t)b * units_max, a.starts + (int64_t)b * a.cap, a.cap, a.info + 2 * b);
}

// Both byte sources in one kernel.  images: packed planes, image b's H_b x W_b bytes at planes + px_off_b; null: padded planes of
// Hp x Wp, image b the top-left sizes[b] = {H_b, W_b} (sizes null: all) of plane b.  A table or size entry that disagrees with what
// the host sized the grid and the workspace from writes nothing.
// Read where they lie, the 64 column-major positions of a step are bytes of 64 rows - 64 cache lines for 64 bytes.  So the workgroup
// first copies its chunk (and the position before it) into LDS along the rows, where the chunk's columns of a row are neighbours: the
// rows y0, y0 + 1, ... (wrapping at H) that the chunk touches, nc columns of each, and of those the positions inside the chunk.
template <bool EMIT>
__global__ __launch_bounds__(PR_THREADS) void byte_runs_kernel(const unsigned char* __restrict__ planes, const sm_bilateral_image* __restrict__ images,
                                                               int Hp, int Wp, const int* __restrict__ sizes, int* __restrict__ counts,
                                                               int units_max, int* __restrict__ starts, int cap, int* __restrict__ info) {
    __shared__ unsigned char tile[PR_CHUNK + 16];
    const int b = blockIdx.y;
    int H = Hp, W = Wp, pitch = Wp;
    const unsigned char* __restrict__ p = planes + (int64_t)b * Hp * Wp;
    if (images) {
        const sm_bilateral_image im = images[b];
        H = im.H; W = pitch = im.W; p = planes + im.px_off;
    } else if (sizes) {
        H = sizes[2 * b]; W = sizes[2 * b + 1];
        if (H > Hp || W > Wp) return;
    }
    const int npx = H * W;
    if (H <= 0 || W <= 0 || pr_units(npx) > units_max || (int64_t)blockIdx.x * PR_CHUNK >= npx) return;
    const int base = blockIdx.x ? blockIdx.x * PR_CHUNK - 1 : 0, end = base + PR_CHUNK + 1 < npx ? base + PR_CHUNK + 1 : npx;
    const int x0 = base / H, y0 = base - x0 * H, nc = (end - 1) / H - x0 + 1, nr = end - base < H ? end - base : H;
    const int dr = PR_THREADS / nc, dx = PR_THREADS - dr * nc;  // a thread's next (row, column): PR_THREADS further along the rows
    for (int r = threadIdx.x / nc, xr = threadIdx.x - r * nc; r < nr;) {
        const int y = y0 + r < H ? y0 + r : y0 + r - H, q = (x0 + xr) * H + y;
        if (q >= base && q < end) tile[q - base] = p[(int64_t)y * pitch + x0 + xr];
        r += dr; xr += dx;
        if (xr >= nc) { xr -= nc; ++r; }
    }
    __syncthreads();
    runs_chunk<EMIT>(TileSrc{tile, H, base}, H, npx, blockIdx.x, counts + (int64_t)b * units_max, starts + (int64_t)b * cap, cap, info + 2 * b);
}

// P3: groups of four packed bytes, aligned to 4 in the output buffer, one group per lane and pass: a wave writes 256 contiguous
// bytes per plane.  The groups that straddle the image's ends fall back to byte stores.
template <bool STAGED>
__global__ __launch_bounds__(PR_THREADS) void predict_planes_kernel(sm_predict_args a) {
    const int b = blockIdx.y;
    const sm_bilateral_image im = a.images[b];
    const int npx = im.H * im.W;
    const int lead = (int)((uintptr_t)((a.binary ? a.binary : a.soft) + im.px_off) & 3);  // bytes of the first group that lie before the image
    const int ngroups = (npx + lead + 3) >> 2;
    if (im.H <= 0 || im.W <= 0 || npx > a.max_pixels || (int)blockIdx.x * PR_THREADS >= ngroups) return;
    const auto src = selected_mask<STAGED>(a, b, im);
    unsigned char* __restrict__ ob = a.binary ? a.binary + im.px_off : nullptr;
    unsigned char* __restrict__ os = a.soft ? a.soft + im.px_off : nullptr;
    const bool al_b = ob && ((uintptr_t)(ob - lead) & 3) == 0, al_s = os && ((uintptr_t)(os - lead) & 3) == 0;
    for (int g = blockIdx.x * PR_THREADS + threadIdx.x; g < ngroups; g += gridDim.x * PR_THREADS) {
        const int p0 = 4 * g - lead;
        const int pf = p0 < 0 ? 0 : p0;
        int y = pf / im.W, x = pf - y * im.W;
        unsigned bin = 0, sft = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int p = p0 + e;
            if (p >= 0 && p < npx) {
                const float v = src.value(y, x);
                bin |= (v > 0.5f ? 1u : 0u) << (8 * e);
                sft |= up_soft_u8(v) << (8 * e);
                if (++x == im.W) { x = 0; ++y; }
            }
        }
        const bool full = p0 >= 0 && p0 + 3 < npx;
        if (ob) {
            if (full && al_b) *reinterpret_cast<unsigned*>(ob + p0) = bin;
            else
                for (int e = 0; e < 4; ++e)
                    if (p0 + e >= 0 && p0 + e < npx) ob[p0 + e] = (unsigned char)(bin >> (8 * e));
        }
        if (os) {
            if (full && al_s) *reinterpret_cast<unsigned*>(os + p0) = sft;
            else
                for (int e = 0; e < 4; ++e)
                    if (p0 + e >= 0 && p0 + e < npx) os[p0 + e] = (unsigned char)(sft >> (8 * e));
        }
    }
}

// largest H * W of a host table, or -1 when an entry is not an image (or lies outside `max_pixels`)
static int table_max_pixels(const sm_bilateral_image* images_host, int B, int max_pixels) {
    int mx = 0;
    for (int b = 0; b < B; ++b) {
        const sm_bilateral_image& im = images_host[b];
        if (im.H <= 0 || im.W <= 0 || im.px_off < 0 || (int64_t)im.H * im.W > max_pixels) return -1;
        mx = im.H * im.W > mx ? im.H * im.W : mx;
    }
    return mx;
}

}  // namespace sm

extern "C" size_t sm_predict_workspace_bytes(int32_t B, int32_t max_pixels) {
    if (B <= 0 || B > 65535 || max_pixels <= 0 || max_pixels > sm::PR_MAX_PIXELS) return 0;
    return ((size_t)B * sm::pr_units(max_pixels) * sizeof(int32_t) + 255) & ~(size_t)255;
}

extern "C" int sm_predict_masks_f32(const sm_predict_args* a, const sm_bilateral_image* images_host, void* stream) {
    SM_REQUIRE(a && images_host, "sm_predict_masks_f32: null pointer (args or the host image table)");
    SM_REQUIRE(a->masks && a->objectness && a->images && a->best, "sm_predict_masks_f32: null pointer (masks, objectness, images or best)");
    SM_REQUIRE(a->B > 0 && a->B <= 65535 && a->nq > 0 && a->nq <= sm::PR_MAX_QUERIES && a->mh > 0 && a->mw > 0 && a->scale >= 0.f,
               "sm_predict_masks_f32: bad shape (B=%d nq=%d (<= %d) mask %dx%d scale %g)", a->B, a->nq, sm::PR_MAX_QUERIES, a->mh, a->mw,
               (double)a->scale);
    SM_REQUIRE(a->max_pixels > 0 && a->max_pixels <= sm::PR_MAX_PIXELS, "sm_predict_masks_f32: max_pixels=%d (largest H*W of the batch, <= %d)",
               a->max_pixels, sm::PR_MAX_PIXELS);
    SM_REQUIRE((a->starts != nullptr) == (a->info != nullptr), "sm_predict_masks_f32: starts and info come together (both or neither)");
    const int mx = sm::table_max_pixels(images_host, a->B, a->max_pixels);
    SM_REQUIRE(mx > 0, "sm_predict_masks_f32: an image of the host table is empty or larger than max_pixels=%d", a->max_pixels);
    hipStream_t st = (hipStream_t)stream;
    const bool staged = a->mh * a->mw <= sm::PR_LDS_FLOATS;
    const size_t lds = staged ? (size_t)a->mh * a->mw * sizeof(float) : 0;
    if (a->starts) {
        SM_REQUIRE(a->cap > 0, "sm_predict_masks_f32: cap=%d", a->cap);
        SM_REQUIRE(a->workspace && ((uintptr_t)a->workspace % 256) == 0 &&
                       a->workspace_bytes >= sm_predict_workspace_bytes(a->B, a->max_pixels),
                   "sm_predict_masks_f32: workspace too small or misaligned");
    }
    hipLaunchKernelGGL(sm::predict_best_kernel, dim3(a->B), dim3(64), 0, st, a->objectness, a->obj_stride_b, a->nq, a->best);
    if (a->starts) {
        const int units_max = sm::pr_units(a->max_pixels);
        const dim3 grid((mx + sm::PR_CHUNK - 1) / sm::PR_CHUNK, a->B);
        int* counts = (int*)a->workspace;
        if (staged) {
            hipLaunchKernelGGL((sm::predict_runs_kernel<false, true>), grid, dim3(sm::PR_THREADS), lds, st, *a, counts, units_max);
            hipLaunchKernelGGL((sm::predict_runs_kernel<true, true>), grid, dim3(sm::PR_THREADS), lds, st, *a, counts, units_max);
        } else {
            hipLaunchKernelGGL((sm::predict_runs_kernel<false, false>), grid, dim3(sm::PR_THREADS), 0, st, *a, counts, units_max);
            hipLaunchKernelGGL((sm::predict_runs_kernel<true, false>), grid, dim3(sm::PR_THREADS), 0, st, *a, counts, units_max);
        }
    }
    if (a->binary || a->soft) {
        // a lane writes four pixels per pass; four passes per lane keep the staging of the mask a small part of a workgroup's work
        const int groups = (mx + 3) / 4 + 1;
        int gx = (groups + sm::PR_THREADS * 4 - 1) / (sm::PR_THREADS * 4);
        gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
        if (staged)
            hipLaunchKernelGGL(sm::predict_planes_kernel<true>, dim3(gx, a->B), dim3(sm::PR_THREADS), lds, st, *a);
        else
            hipLaunchKernelGGL(sm::predict_planes_kernel<false>, dim3(gx, a->B), dim3(sm::PR_THREADS), 0, st, *a);
    }
    return sm::check_launch("sm_predict_masks_f32");
}

extern "C" int sm_rle_runs_packed_u8(const uint8_t* planes, const sm_bilateral_image* images_dev, const sm_bilateral_image* images_host,
                                     int32_t B, int32_t* starts, int32_t cap, int32_t* info, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    SM_REQUIRE(planes && images_dev && images_host && starts && info && workspace, "sm_rle_runs_packed_u8: null pointer");
    SM_REQUIRE(B > 0 && B <= 65535 && cap > 0, "sm_rle_runs_packed_u8: %d images, cap %d", B, cap);
    const int mx = sm::table_max_pixels(images_host, B, sm::PR_MAX_PIXELS);
    SM_REQUIRE(mx > 0, "sm_rle_runs_packed_u8: an image of the host table is empty or has more than %d pixels", sm::PR_MAX_PIXELS);
    SM_REQUIRE(((uintptr_t)workspace % 256) == 0 && workspace_bytes >= sm_predict_workspace_bytes(B, mx),
               "sm_rle_runs_packed_u8: workspace too small or misaligned (sm_predict_workspace_bytes(B, largest H*W))");
    const int units_max = sm::pr_units(mx);
    const dim3 grid((mx + sm::PR_CHUNK - 1) / sm::PR_CHUNK, B);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sm::byte_runs_kernel<false>, grid, dim3(sm::PR_THREADS), 0, st, planes, images_dev, 0, 0, nullptr, (int*)workspace, units_max, starts, cap, info);
    hipLaunchKernelGGL(sm::byte_runs_kernel<true>, grid, dim3(sm::PR_THREADS), 0, st, planes, images_dev, 0, 0, nullptr, (int*)workspace, units_max, starts, cap, info);
    return sm::check_launch("sm_rle_runs_packed_u8");
}

extern "C" int sm_rle_runs_u8(const uint8_t* masks, int32_t B, int32_t H, int32_t W, const int32_t* sizes, int32_t* starts, int32_t cap,
                              int32_t* info, void* workspace, size_t workspace_bytes, void* stream) {
    SM_REQUIRE(masks && starts && info && workspace, "sm_rle_runs_u8: null pointer");
    SM_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= sm::PR_MAX_PIXELS && cap > 0,
               "sm_rle_runs_u8: %d masks of %dx%d, cap %d (at most 65535 masks of %d pixels)", B, H, W, cap, sm::PR_MAX_PIXELS);
    SM_REQUIRE(((uintptr_t)workspace % 256) == 0 && workspace_bytes >= sm_predict_workspace_bytes(B, H * W),
               "sm_rle_runs_u8: workspace too small or misaligned (sm_predict_workspace_bytes(B, H*W))");
    const int units_max = sm::pr_units(H * W);
    const dim3 grid((H * W + sm::PR_CHUNK - 1) / sm::PR_CHUNK, B);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sm::byte_runs_kernel<false>, grid, dim3(sm::PR_THREADS), 0, st, masks, nullptr, H, W, sizes, (int*)workspace, units_max, starts, cap, info);
    hipLaunchKernelGGL(sm::byte_runs_kernel<true>, grid, dim3(sm::PR_THREADS), 0, st, masks, nullptr, H, W, sizes, (int*)workspace, units_max, starts, cap, info);
    return sm::check_launch("sm_rle_runs_u8");
}
