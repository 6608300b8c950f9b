// E-measure and weighted F-measure of 8-bit saliency maps against binary ground truths (selfmask_amd/sod_metrics.py is the
// definition).  The 8-bit plane of the evaluator's selected query that they are computed from: sm_upsample_selected_u8, selected.hip.
//
// Per call, for B images of any mix of sizes (image b's bytes at images[b].gt_off in both `pred` and `gt`):
//   S1  histograms   a chunk of raster pixels per workgroup, two 256-bin histograms of p8 (foreground / background) in LDS by
//                    integer atomics, merged into the image's histograms by integer atomics: order-free, so a function of the
//                    input alone (as objects.hip argues).  G and sum(p8) are read off the histograms by the later launches.
//   S2  column pass  one lane per column walks the rows down and up: the row of the nearest foreground pixel of the column,
//                    the upper one on a tie, -1 where the column has none
//   S3  row pass     one lane per pixel minimises the key d^2 << 22 | source raster index over the columns' candidates as ONE
//                    64-bit integer (d^2 < 2^29, index < 2^22: a tie resolves to the lowest raster index by construction),
//                    searching outward from its own column until dx^2 exceeds the best d^2.  Out: d^2 (int32) and
//                    255 - p8[src] (a byte: Et is an integer over 255)
//   S4  weights      the 7 x 7 Gaussian of Et on the foreground pixels (49 taps in raster order of the window, zero padding, fp64)
//                    from an LDS copy of the raster window the chunk's taps reach (global reads when a row is too long for it),
//                    Ew = min-rule error x distance weight, and the chunk's two sums of Ew in a fixed order
//   S5  finish       one workgroup per image: partial sums added in a fixed order, E(t) with lanes as thresholds, the mean added
//                    in ascending t, the adaptive value, the four doubles
// An image without foreground skips S2 - S4 and gets wfm = 0.  No floating-point atomics anywhere; an image's chunks, partial
// sums and histograms are indexed by its own pixels only, so its four values do not depend on the batch around it.
#include "common.h"

#pragma clang fp contract(off)

#include <math.h>

namespace sm {

constexpr int SD_THREADS = 256;
constexpr int SD_PPT = 4;                         // pixels per thread
constexpr int SD_CHUNK = SD_THREADS * SD_PPT;     // raster pixels per workgroup
constexpr int SD_MAX_PIXELS = 1 << 22;
constexpr int SD_MAX_SIDE = 16384;                // H, W: d^2 <= 2 (2^14 - 1)^2 < 2^29
constexpr int SD_IDX_BITS = 22;
constexpr int SD_WINDOW = 16 * 1024;              // bytes of Et a workgroup stages: chunk + 3 rows and 3 pixels either side
constexpr double SD_EPS = 2.220446049250313e-16;  // 2^-52
constexpr unsigned long long SD_NO_KEY = ~0ull >> 1;

struct SdTaps { double k[49]; };  // fspecial('gaussian', 7, 5), row-major

struct SdWs { int* hist; int* fg; int* near; int* d2; unsigned char* et; double* part; size_t total; };

__host__ __device__ __forceinline__ int sd_chunks(int npx) { return (npx + SD_CHUNK - 1) / SD_CHUNK; }
static size_t sd_plane(int max_pixels) { return ((size_t)max_pixels + 255) & ~(size_t)255; }  // an image's stride in the planes

static SdWs carve_sod(int B, int max_pixels, char* base) {
    SdWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
    w.hist = (int*)take((size_t)B * 512 * sizeof(int));
    w.fg = (int*)take((size_t)B * sizeof(int));
    w.near = (int*)take((size_t)B * sd_plane(max_pixels) * sizeof(int));
    w.d2 = (int*)take((size_t)B * sd_plane(max_pixels) * sizeof(int));
    w.et = (unsigned char*)take((size_t)B * sd_plane(max_pixels));
    w.part = (double*)take((size_t)B * sd_chunks(max_pixels) * 2 * sizeof(double));
    w.total = off;
    return w;
}

__device__ __forceinline__ int sd_wave_total(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double sd_wave_total(double v) {  // a fixed tree: the same order whatever the batch
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- S1 ----
__global__ __launch_bounds__(SD_THREADS) void sod_hist_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ gt,
                                                              const sm_eval_image* __restrict__ images, int* __restrict__ hist) {
    __shared__ int h[512];
    const int b = blockIdx.y, tid = threadIdx.x;
    const sm_eval_image im = images[b];
    const int npx = im.H * im.W, p0 = blockIdx.x * SD_CHUNK;
    if (p0 >= npx) return;
    h[tid] = 0;
    h[tid + SD_THREADS] = 0;
    __syncthreads();
    const unsigned char* __restrict__ p8 = pred + im.gt_off;
    const unsigned char* __restrict__ g = gt + im.gt_off;
#pragma unroll
    for (int k = 0; k < SD_PPT; ++k) {
        const int p = p0 + k * SD_THREADS + tid;
        if (p < npx) atomicAdd(&h[(g[p] ? 0 : 256) + p8[p]], 1);
    }
    __syncthreads();
    int* out = hist + (int64_t)b * 512;
    for (int i = tid; i < 512; i += SD_THREADS)
        if (h[i]) atomicAdd(&out[i], h[i]);
}

// ---- S2 ----
__global__ __launch_bounds__(64) void sod_column_kernel(const unsigned char* __restrict__ gt, const sm_eval_image* __restrict__ images,
                                                        const int* __restrict__ hist, int* __restrict__ fg, int* __restrict__ near_all,
                                                        int64_t plane) {
    const int b = blockIdx.y, lane = threadIdx.x;
    const int* hf = hist + (int64_t)b * 512;
    const int G = sd_wave_total(hf[lane] + hf[lane + 64] + hf[lane + 128] + hf[lane + 192]);
    if (blockIdx.x == 0 && lane == 0) fg[b] = G;
    if (G == 0) return;
    const sm_eval_image im = images[b];
    const int H = im.H, W = im.W, x = blockIdx.x * 64 + lane;
    if (x >= W) return;
    const unsigned char* __restrict__ g = gt + im.gt_off;
    int* __restrict__ near = near_all + (int64_t)b * plane;
    int last = -1;
    for (int y = 0; y < H; ++y) {  // the nearest foreground row at or above
        if (g[y * W + x]) last = y;
        near[y * W + x] = last;
    }
    last = -1;
    for (int y = H - 1; y >= 0; --y) {  // against the nearest at or below: the upper row on a tie
        if (g[y * W + x]) last = y;
        const int up = near[y * W + x];
        near[y * W + x] = up < 0 ? last : (last < 0 || y - up <= last - y ? up : last);
    }
}

// ---- S3 ----
__global__ __launch_bounds__(SD_THREADS) void sod_row_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ gt,
                                                             const sm_eval_image* __restrict__ images, const int* __restrict__ fg,
                                                             const int* __restrict__ near_all, int* __restrict__ d2_all,
                                                             unsigned char* __restrict__ et_all, int64_t plane) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const sm_eval_image im = images[b];
    const int W = im.W, npx = im.H * im.W, p0 = blockIdx.x * SD_CHUNK;
    if (p0 >= npx || fg[b] == 0) return;
    const unsigned char* __restrict__ p8 = pred + im.gt_off;
    const unsigned char* __restrict__ g = gt + im.gt_off;
    const int* __restrict__ near = near_all + (int64_t)b * plane;
    int* __restrict__ d2 = d2_all + (int64_t)b * plane;
    unsigned char* __restrict__ et = et_all + (int64_t)b * plane;
    for (int k = 0; k < SD_PPT; ++k) {
        const int p = p0 + k * SD_THREADS + tid;
        if (p >= npx) break;
        if (g[p]) {
            d2[p] = 0;
            et[p] = (unsigned char)(255 - p8[p]);
            continue;
        }
        const int y = p / W, x = p - y * W;
        const int* __restrict__ nr = near + y * W;
        unsigned long long best = SD_NO_KEY;
        auto candidate = [&](int xc, unsigned long long dx2) {
            const int r = nr[xc];
            if (r < 0) return;
            const long long dy = y - r;
            const unsigned long long key = (((unsigned long long)(dy * dy) + dx2) << SD_IDX_BITS) | (unsigned)(r * W + xc);
            best = key < best ? key : best;
        };
        candidate(x, 0);
        for (int dx = 1;; ++dx) {
            const bool left = x - dx >= 0, right = x + dx < W;
            const unsigned long long dx2 = (unsigned long long)dx * dx;
            if ((!left && !right) || dx2 > (best >> SD_IDX_BITS)) break;
            if (left) candidate(x - dx, dx2);
            if (right) candidate(x + dx, dx2);
        }
        // fg[b] > 0: some column holds a foreground pixel, so a key was found and its index lies inside the image
        const int src = (int)(best & ((1u << SD_IDX_BITS) - 1));
        d2[p] = (int)(best >> SD_IDX_BITS);
        et[p] = (unsigned char)(255 - p8[src < npx ? src : p]);
    }
}

// ---- S4 ----
template <bool STAGED>
__device__ __forceinline__ double sd_smoothed(const unsigned char* __restrict__ e, int lo, const SdTaps& taps, int y, int x, int H, int W) {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const int yy = y + i - 3;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int xx = x + j - 3;
            const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
            const double v = in ? (double)e[yy * W + xx - (STAGED ? lo : 0)] / 255.0 : 0.0;
            acc = acc + taps.k[i * 7 + j] * v;
        }
    }
    return acc;
}

__global__ __launch_bounds__(SD_THREADS) void sod_weight_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ gt,
                                                                const sm_eval_image* __restrict__ images, const int* __restrict__ fg,
                                                                const int* __restrict__ d2_all, const unsigned char* __restrict__ et_all,
                                                                double* __restrict__ part, int64_t plane, int chunk_cap, SdTaps taps) {
    __shared__ unsigned char win[SD_WINDOW];
    __shared__ double wsum[2][SD_THREADS / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const sm_eval_image im = images[b];
    const int H = im.H, W = im.W, npx = H * W, p0 = blockIdx.x * SD_CHUNK;
    if (p0 >= npx || fg[b] == 0) return;
    const unsigned char* __restrict__ p8 = pred + im.gt_off;
    const unsigned char* __restrict__ g = gt + im.gt_off;
    const int* __restrict__ d2 = d2_all + (int64_t)b * plane;
    const unsigned char* __restrict__ et = et_all + (int64_t)b * plane;
    const int p1 = p0 + SD_CHUNK < npx ? p0 + SD_CHUNK : npx;
    // the raster window the taps of pixels p0 .. p1 - 1 reach: a tap inside the image is at p + i W + j, |i|, |j| <= 3
    const int64_t reach = 3 * (int64_t)W + 3;
    const int lo = p0 - reach > 0 ? (int)(p0 - reach) : 0, hi = p1 + reach < npx ? (int)(p1 + reach) : npx;
    const bool staged = hi - lo <= SD_WINDOW;  // uniform over the workgroup
    if (staged) {
        for (int i = tid; i < hi - lo; i += SD_THREADS) win[i] = et[lo + i];
        __syncthreads();
    }
    double s_fg = 0.0, s_bg = 0.0;
    for (int k = 0; k < SD_PPT; ++k) {
        const int p = p0 + k * SD_THREADS + tid;
        if (p >= npx) break;
        const int v = p8[p];
        if (g[p]) {
            const int y = p / W, x = p - y * W;
            const double e = (double)(255 - v) / 255.0;
            const double ea = staged ? sd_smoothed<true>(win, lo, taps, y, x, H, W) : sd_smoothed<false>(et, 0, taps, y, x, H, W);
            s_fg = s_fg + (ea < e ? ea : e);  // x 1: the foreground's weight
        } else {
            const double e = (double)v / 255.0;
            const double w = 2.0 - exp((-0.6931471805599453 / 5.0) * sqrt((double)d2[p]));
            s_bg = s_bg + e * w;
        }
    }
    s_fg = sd_wave_total(s_fg);
    s_bg = sd_wave_total(s_bg);
    if ((tid & 63) == 0) {
        wsum[0][tid >> 6] = s_fg;
        wsum[1][tid >> 6] = s_bg;
    }
    __syncthreads();
    if (tid < 2) {
        double s = 0.0;
        for (int w = 0; w < SD_THREADS / 64; ++w) s = s + wsum[tid][w];
        part[((int64_t)b * chunk_cap + blockIdx.x) * 2 + tid] = s;
    }
}

// ---- S5 ----
__device__ __forceinline__ double sd_e_value(long long a, long long b, long long G, long long n) {
    double s;
    if (G == 0) {
        s = (double)(n - b);
    } else if (G == n) {
        s = (double)a;
    } else {
        const double mu_f = (double)(a + b) / (double)n, mu_g = (double)G / (double)n;
        const double f[4] = {1.0, 1.0, 0.0, 0.0}, g[4] = {1.0, 0.0, 1.0, 0.0};
        const long long cnt[4] = {a, b, G - a, n - G - b};
        s = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double df = f[c] - mu_f, dg = g[c] - mu_g;
            const double align = ((2.0 * df) * dg) / ((df * df + dg * dg) + SD_EPS);
            s = s + (double)cnt[c] * (((align + 1.0) * (align + 1.0)) / 4.0);
        }
    }
    return s / (((double)n - 1.0) + SD_EPS);
}

__global__ __launch_bounds__(SD_THREADS) void sod_finish_kernel(const sm_eval_image* __restrict__ images, const int* __restrict__ hist,
                                                                const double* __restrict__ part, int chunk_cap, double* __restrict__ out) {
    __shared__ int hf[256], hb[256];
    __shared__ double ev[256], ps[2][SD_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const sm_eval_image im = images[b];
    const long long n = (long long)im.H * im.W;
    hf[t] = hist[(int64_t)b * 512 + t];
    hb[t] = hist[(int64_t)b * 512 + 256 + t];
    __syncthreads();
    long long G = 0;
    for (int v = 0; v < 256; ++v) G += hf[v];
    long long a = 0, bb = 0;
    for (int v = t; v < 256; ++v) {
        a += hf[v];
        bb += hb[v];
    }
    ev[t] = sd_e_value(a, bb, G, n);
    double s_fg = 0.0, s_bg = 0.0;
    if (G > 0) {
        const double* pp = part + (int64_t)b * chunk_cap * 2;
        const int nc = sd_chunks((int)n);
        for (int c = t; c < nc; c += SD_THREADS) {
            s_fg = s_fg + pp[2 * c];
            s_bg = s_bg + pp[2 * c + 1];
        }
    }
    ps[0][t] = s_fg;
    ps[1][t] = s_bg;
    __syncthreads();
    if (t != 0) return;
    double mean = 0.0, mx = ev[0];
    for (int v = 0; v < 256; ++v) {  // ascending t
        mean = mean + ev[v];
        mx = ev[v] > mx ? ev[v] : mx;
    }
    mean = mean / 256.0;
    long long total = 0;
    for (int v = 0; v < 256; ++v) total += (long long)v * (hf[v] + hb[v]);
    const long long bound = 2 * total < 255 * n ? 2 * total : 255 * n;
    const int thr = (int)((bound + n - 1) / n);  // the smallest byte v with v n >= bound; at most 255
    long long aa = 0, ab = 0;
    for (int v = thr; v < 256; ++v) {
        aa += hf[v];
        ab += hb[v];
    }
    double wfm = 0.0;
    if (G > 0) {
        s_fg = 0.0;
        s_bg = 0.0;
        for (int i = 0; i < SD_THREADS; ++i) {
            s_fg = s_fg + ps[0][i];
            s_bg = s_bg + ps[1][i];
        }
        const double tpw = (double)G - s_fg, fpw = s_bg;
        const double r = 1.0 - s_fg / (double)G;
        const double p = tpw / ((tpw + fpw) + SD_EPS);
        wfm = ((2.0 * r) * p) / ((r + p) + SD_EPS);
    }
    double* o = out + (int64_t)b * 4;
    o[0] = sd_e_value(aa, ab, G, n);
    o[1] = mean;
    o[2] = mx;
    o[3] = wfm;
}

static SdTaps sod_taps() {
    SdTaps t;
    double h[49], mx = 0.0, sum = 0.0;
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j) {
            const double y = i - 3, x = j - 3;
            h[i * 7 + j] = ::exp(-(y * y + x * x) / (2.0 * 5.0 * 5.0));
            mx = h[i * 7 + j] > mx ? h[i * 7 + j] : mx;
        }
    for (int k = 0; k < 49; ++k) {
        if (h[k] < SD_EPS * mx) h[k] = 0.0;
        sum += h[k];
    }
    for (int k = 0; k < 49; ++k) t.k[k] = h[k] / sum;
    return t;
}

}  // namespace sm

extern "C" size_t sm_sod_metrics_workspace_bytes(int32_t B, int32_t max_pixels) {
    if (B <= 0 || B > 65535 || max_pixels <= 0 || max_pixels > sm::SD_MAX_PIXELS) return 0;
    return sm::carve_sod(B, max_pixels, nullptr).total;
}

extern "C" int sm_sod_metrics_u8(const uint8_t* pred, const uint8_t* gt, const sm_eval_image* images, const sm_eval_image* images_host,
                                 int32_t B, int32_t max_pixels, double* out, int32_t* hist, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    SM_REQUIRE(pred && gt && images && images_host && out && workspace,
               "sm_sod_metrics_u8: null pointer (pred, gt, images, images_host, out or workspace)");
    SM_REQUIRE(B > 0 && B <= 65535, "sm_sod_metrics_u8: B=%d (1 .. 65535)", B);
    SM_REQUIRE(max_pixels > 0 && max_pixels <= sm::SD_MAX_PIXELS, "sm_sod_metrics_u8: max_pixels=%d (largest H*W of the batch, <= %d)",
               max_pixels, sm::SD_MAX_PIXELS);
    int max_w = 0;
    for (int b = 0; b < B; ++b) {
        const sm_eval_image& im = images_host[b];
        SM_REQUIRE(im.gt_off >= 0 && im.H >= 1 && im.W >= 1 && im.H <= sm::SD_MAX_SIDE && im.W <= sm::SD_MAX_SIDE &&
                       (int64_t)im.H * im.W <= max_pixels,
                   "sm_sod_metrics_u8: image %d is %d x %d (sides 1 .. %d, H*W <= max_pixels=%d)", b, im.H, im.W, sm::SD_MAX_SIDE, max_pixels);
        max_w = im.W > max_w ? im.W : max_w;
    }
    SM_REQUIRE(((uintptr_t)workspace % 256) == 0 && workspace_bytes >= sm_sod_metrics_workspace_bytes(B, max_pixels),
               "sm_sod_metrics_u8: workspace too small or misaligned");
    static const sm::SdTaps taps = sm::sod_taps();
    const sm::SdWs w = sm::carve_sod(B, max_pixels, (char*)workspace);
    hipStream_t st = (hipStream_t)stream;
    int* h = hist ? hist : w.hist;
    const int64_t plane = (int64_t)sm::sd_plane(max_pixels);
    const int nchunk = sm::sd_chunks(max_pixels);
    if (hipMemsetAsync(h, 0, (size_t)B * 512 * sizeof(int), st) != hipSuccess) return sm::check_launch("sm_sod_metrics_u8 (memset)");
    {
        sm::TapGuard tap(stream, "sod_hist_kernel");
        hipLaunchKernelGGL(sm::sod_hist_kernel, dim3(nchunk, B), dim3(sm::SD_THREADS), 0, st, pred, gt, images, h);
    }
    {
        sm::TapGuard tap(stream, "sod_column_kernel");
        hipLaunchKernelGGL(sm::sod_column_kernel, dim3((max_w + 63) / 64, B), dim3(64), 0, st, gt, images, h, w.fg, w.near, plane);
    }
    {
        sm::TapGuard tap(stream, "sod_row_kernel");
        hipLaunchKernelGGL(sm::sod_row_kernel, dim3(nchunk, B), dim3(sm::SD_THREADS), 0, st, pred, gt, images, w.fg, w.near, w.d2, w.et,
                           plane);
    }
    {
        sm::TapGuard tap(stream, "sod_weight_kernel");
        hipLaunchKernelGGL(sm::sod_weight_kernel, dim3(nchunk, B), dim3(sm::SD_THREADS), 0, st, pred, gt, images, w.fg, w.d2, w.et, w.part,
                           plane, nchunk, taps);
    }
    {
        sm::TapGuard tap(stream, "sod_finish_kernel");
        hipLaunchKernelGGL(sm::sod_finish_kernel, dim3(B), dim3(sm::SD_THREADS), 0, st, images, h, w.part, nchunk, out);
    }
    return sm::check_launch("sm_sod_metrics_u8");
}
