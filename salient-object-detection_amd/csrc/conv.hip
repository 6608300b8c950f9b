// Dilated ResNet-50 backbone (the MoCo-v2 / SwAV feature branch of the reference's pseudo-mask generator: networks/resnet.py:8-56,
// resnet_backbone.py:42-105, resnet_models.py:57-154).  Activations are NHWC, one row per pixel, so every convolution is a weight
// GEMM on sm_gemm_w16 (gemm_w16.hip, untouched): 1 x 1 convolutions read the activation rows as they lie, 3 x 3 (and the strided
// 1 x 1 down-sample) read rows gathered tap by tap into the GEMM's own operand format.  BatchNorm (eval) arrives folded into the
// weight and a bias (resnet.py of the package, fp64 on the host).  What is hand-written here are the streaming kernels between the
// GEMMs - 16-byte accesses per lane, no LDS: tap gather, stem gather, max-pool, ReLU + split, a channel-count-general bilinear
// up-sampler - and the launch sequence.
// upsample_aligned_kernel: torch-CPU arithmetic as written (the header switches a*b+c -> fma contraction off for this file)
#include "upsample.h"

#define TRY_RC(x)             \
    do {                      \
        int _rc = (x);        \
        if (_rc) return _rc;  \
    } while (0)

namespace sm {

// ---- tap gather: im2col in the F16X2 operand format ----------------------------------------------------------------------------
// in (B, H, W, C) F16X2 rows -> out (B, oh, ow, k*k*C): row (b, oy, ox) = the input rows (b, oy s - p + i d, ox s - p + j d), taps
// (i, j) row-major, laid end to end; a tap outside image b is zeros (the bounds are tested per image: never a row of image b +- 1).
// An F16X2 row is whole 32-B groups of 8 channels, so a tap moves as C / 4 16-byte vectors, bit for bit.  One thread per (output
// pixel, vector of the input row): it splits its index once and copies that vector of all k*k taps (independent loads; the lanes
// of a wave write consecutive vectors of one tap).
template <int K>
__global__ __launch_bounds__(256) void conv_gather_kernel(const uint4* __restrict__ in, uint4* __restrict__ out, int H, int W, int v_row,
                                                          int stride, int dil, int pad, int oh, int ow, int64_t total) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int v = (int)(t % v_row);
        const int64_t r = t / v_row;  // output pixel (b, oy, ox)
        const int ox = (int)(r % ow), oy = (int)((r / ow) % oh);
        const int64_t b = r / ((int64_t)ow * oh);
        const int y0 = oy * stride - pad, x0 = ox * stride - pad;
        uint4 val[K * K];
#pragma unroll
        for (int tap = 0; tap < K * K; ++tap) {
            const int y = y0 + (tap / K) * dil, x = x0 + (tap % K) * dil;
            val[tap] = make_uint4(0u, 0u, 0u, 0u);
            if (y >= 0 && y < H && x >= 0 && x < W) val[tap] = in[((b * H + y) * W + x) * v_row + v];
        }
#pragma unroll
        for (int tap = 0; tap < K * K; ++tap) out[(r * (K * K) + tap) * v_row + v] = val[tap];
    }
}

// ---- stem gather: the 7 x 7 x 3 taps of prefix.conv1 (stride 2, pad 3) from the fp32 NCHW input, written in F16X2 -----------------
// out (B, oh, ow, 160): column c * 49 + i * 7 + j = x[b, c, 2 oy - 3 + i, 2 ox - 3 + j] (the (64, 3, 7, 7) weight flattened as it lies),
// zeros outside the image and in the 13 pad columns 147..159.  One thread per 8-column group (20 per row).
constexpr int STEM_K = 147, STEM_KP = 160;
__global__ __launch_bounds__(256) void stem_gather_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W, int oh, int ow,
                                                          int64_t total) {
    constexpr int G = STEM_KP / 8;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int g = (int)(t % G);
        const int64_t r = t / G;
        const int ox = (int)(r % ow), oy = (int)((r / ow) % oh);
        const int64_t b = r / ((int64_t)ow * oh);
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int kx = g * 8 + e;
            const int c = kx / 49, ij = kx - c * 49, i = ij / 7, j = ij - i * 7;
            const int y = 2 * oy - 3 + i, xx = 2 * ox - 3 + j;
            v[e] = (kx < STEM_K && y >= 0 && y < H && xx >= 0 && xx < W) ? x[((b * 3 + c) * H + y) * W + xx] : 0.f;
        }
        f16x8 hi, lo;
        split8(v, hi, lo);
        char* p = reinterpret_cast<char*>(out) + t * 32;
        *reinterpret_cast<f16x8*>(p) = hi;
        *reinterpret_cast<f16x8*>(p + 16) = lo;
    }
}

// ---- max-pool 3 x 3, stride 2, pad 1 on NHWC (resnet_models.py:120) ----------------------------------------------------------------
// PyTorch semantics: the padding never wins (an all-negative window gives its largest negative value); every window holds at least
// its centre (2 oy, 2 ox).  Writes fp32 and / or the F16X2 copy layer1.0 reads.  One thread per 8-channel group.
__global__ __launch_bounds__(256) void maxpool_kernel(const float* __restrict__ in, float* __restrict__ out, float* __restrict__ outs, int H,
                                                      int W, int C8, int oh, int ow, int64_t total) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int g = (int)(t % C8);
        const int64_t r = t / C8;
        const int ox = (int)(r % ow), oy = (int)((r / ow) % oh);
        const int64_t b = r / ((int64_t)ow * oh);
        float m[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
        for (int i = 0; i < 3; ++i) {
            const int y = 2 * oy - 1 + i;
            if (y < 0 || y >= H) continue;
            for (int j = 0; j < 3; ++j) {
                const int x = 2 * ox - 1 + j;
                if (x < 0 || x >= W) continue;
                const float4* p = reinterpret_cast<const float4*>(in + (((b * H + y) * W + x) * C8 + g) * 8);
                const float4 a = p[0], c = p[1];
                m[0] = fmaxf(m[0], a.x); m[1] = fmaxf(m[1], a.y); m[2] = fmaxf(m[2], a.z); m[3] = fmaxf(m[3], a.w);
                m[4] = fmaxf(m[4], c.x); m[5] = fmaxf(m[5], c.y); m[6] = fmaxf(m[6], c.z); m[7] = fmaxf(m[7], c.w);
            }
        }
        if (out) {
            float4* q = reinterpret_cast<float4*>(out + t * 8);
            q[0] = make_float4(m[0], m[1], m[2], m[3]);
            q[1] = make_float4(m[4], m[5], m[6], m[7]);
        }
        if (outs) {
            f16x8 hi, lo;
            split8(m, hi, lo);
            char* p = reinterpret_cast<char*>(outs) + t * 32;
            *reinterpret_cast<f16x8*>(p) = hi;
            *reinterpret_cast<f16x8*>(p + 16) = lo;
        }
    }
}

// ---- ReLU + split: after a block's conv3 GEMM (residual epilogue, fp32) --------------------------------------------------------------
// One pass writes relu(x) in fp32 (the next block's residual and the map a caller sees; may be written in place) and in F16X2 (the
// next conv1's operand).  One thread per 8-element group; each group is read before it is written.
__global__ __launch_bounds__(256) void relu_split_kernel(const float* src, float* dst, float* __restrict__ dsts, int64_t total) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const float4* p = reinterpret_cast<const float4*>(src + t * 8);
        const float4 a = p[0], c = p[1];
        float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
        if (dst) {
            float4* q = reinterpret_cast<float4*>(dst + t * 8);
            q[0] = make_float4(v[0], v[1], v[2], v[3]);
            q[1] = make_float4(v[4], v[5], v[6], v[7]);
        }
        if (dsts) {
            f16x8 hi, lo;
            split8(v, hi, lo);
            char* q = reinterpret_cast<char*>(dsts) + t * 32;
            *reinterpret_cast<f16x8*>(q) = hi;
            *reinterpret_cast<f16x8*>(q + 16) = lo;
        }
    }
}

static int grid_for(int64_t total) {
    int64_t g = (total + 255) / 256;
    return (int)(g > 8192 ? 8192 : g);
}
static int conv_out(int n, int k, int stride, int dil, int pad) { return (n + 2 * pad - dil * (k - 1) - 1) / stride + 1; }

// ---- the network as a table --------------------------------------------------------------------------------------------------------
struct Block {
    int layer, inplanes, planes, stride, dil;  // stride of conv2 and of the down-sample; dil = pad of conv2
    bool down, last;                           // last: the layer's output map
    int ih, iw, oh, ow;
};
struct Plan {
    int B, H, W, h1, w1, h2, w2;  // input, after the stem, after the max-pool
    Block blk[SM_RESNET50_BLOCKS];
    size_t stemA, stemC, X, Xs, T1, T2, G, total;  // floats per region
    bool ok;
};

// resnet_models.py:122-125 ([3, 4, 6, 3] bottlenecks of 64..512 planes, the stride on conv2 of a layer's first block);
// resnet_backbone.py:49-55,72-85 with multi_grid None: layers 3 / 4 lose their stride, the convolution that had it gets
// dilation d / 2, every other 3 x 3 of the layer d (d = 2, 4)
static Plan make_plan(int B, int H, int W, int dilated) {
    Plan p = {};
    p.B = B; p.H = H; p.W = W;
    if (B < 1 || H < 1 || W < 1) return p;
    p.h1 = conv_out(H, 7, 2, 1, 3); p.w1 = conv_out(W, 7, 2, 1, 3);
    p.h2 = conv_out(p.h1, 3, 2, 1, 1); p.w2 = conv_out(p.w1, 3, 2, 1, 1);
    static const int planes[4] = {64, 128, 256, 512}, count[4] = {3, 4, 6, 3};
    const uint64_t lim = 1ull << 32;  // sm_gemm_w16 addresses its operands with 32-bit byte offsets
    const size_t m1 = (size_t)B * p.h1 * p.w1;
    p.stemA = m1 * STEM_KP; p.stemC = m1 * 64;
    bool ok = p.stemA * 4 < lim;
    int h = p.h2, w = p.w2, inpl = 64, n = 0;
    for (int l = 0; l < 4; ++l) {
        const int d = dilated ? (l == 2 ? 2 : l == 3 ? 4 : 1) : 1;
        for (int i = 0; i < count[l]; ++i, ++n) {
            Block& b = p.blk[n];
            b.layer = l; b.inplanes = inpl; b.planes = planes[l];
            b.stride = (i == 0 && l > 0) ? 2 : 1;
            b.dil = 1;
            if (d > 1) { b.dil = b.stride == 2 ? d / 2 : d; b.stride = 1; }
            b.down = i == 0; b.last = i == count[l] - 1;
            b.ih = h; b.iw = w;
            b.oh = conv_out(h, 3, b.stride, b.dil, b.dil); b.ow = conv_out(w, 3, b.stride, b.dil, b.dil);
            const size_t mi = (size_t)B * b.ih * b.iw, mo = (size_t)B * b.oh * b.ow;
            auto up = [](size_t& a, size_t v) { if (v > a) a = v; };
            up(p.X, mo * b.planes * 4); up(p.Xs, mo * b.planes * 4); up(p.Xs, mi * b.inplanes);
            up(p.T1, mi * b.planes); up(p.T2, mo * b.planes);
            up(p.G, mo * 9 * b.planes);
            if (b.down && b.stride == 2) up(p.G, mo * b.inplanes);
            h = b.oh; w = b.ow; inpl = b.planes * 4;
        }
    }
    // T1 and T2 need no test of their own: T2 = G / 9, and T1 <= 4 T2 (a strided block has four input pixels per output pixel) < G;
    // sm_gemm_w16 checks its operands again in any case
    ok = ok && p.G * 4 < lim && p.X * 4 < lim && p.Xs * 4 < lim;
    auto al = [](size_t nf) { return (nf + 63) & ~(size_t)63; };
    p.total = (al(p.stemA) + al(p.stemC) + al(p.X) + al(p.Xs) + al(p.T1) + al(p.T2) + al(p.G)) * sizeof(float);
    p.ok = ok;
    return p;
}

static int conv_gemm(hipStream_t st, const char* name, const float* A, const sm_conv_weight& cw, float* C, int64_t M, int N, int K, int epi,
                     bool out_s, const float* R = nullptr) {
    sm_gemm_args g = {};
    g.A = A; g.W = cw.w; g.bias = cw.bias; g.C = C; g.R = R;
    g.M = (int)M; g.N = N; g.K = K; g.lda = K; g.ldw = K; g.ldc = N; g.ldr = N;
    g.batch = 1; g.epilogue = epi; g.w_scale = cw.w_scale;
    TapGuard tap(st, name, 2.0 * M * N * K, 0.0);
    return sm_gemm_w16(&g, out_s ? 1 : 0, st);
}

}  // namespace sm

extern "C" int sm_conv_gather_f16x2(const float* in, float* out, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t k, int32_t stride,
                                    int32_t dilation, int32_t pad, void* stream) {
    SM_REQUIRE(in && out && B > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 8 == 0 && (k == 1 || k == 3) && stride >= 1 && dilation >= 1 && pad >= 0 &&
                   ((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0,
               "sm_conv_gather_f16x2: bad arguments (Cin %% 8 == 0, k 1 or 3, 16-B aligned pointers)");
    SM_REQUIRE(H + 2 * pad >= dilation * (k - 1) + 1 && W + 2 * pad >= dilation * (k - 1) + 1, "sm_conv_gather_f16x2: empty output");
    const int oh = sm::conv_out(H, k, stride, dilation, pad), ow = sm::conv_out(W, k, stride, dilation, pad);
    const int v_row = Cin / 4;
    const int64_t total = (int64_t)B * oh * ow * v_row;  // threads; each moves k*k vectors of 16 B in and out
    sm::TapGuard tap(stream, k == 1 ? "conv_gather_kernel (1x1)" : "conv_gather_kernel (3x3)", 0.0, 32.0 * total * k * k);
    const uint4* src = reinterpret_cast<const uint4*>(in);
    uint4* dst = reinterpret_cast<uint4*>(out);
    if (k == 1)
        hipLaunchKernelGGL(sm::conv_gather_kernel<1>, dim3(sm::grid_for(total)), dim3(256), 0, (hipStream_t)stream, src, dst, H, W, v_row, stride,
                           dilation, pad, oh, ow, total);
    else
        hipLaunchKernelGGL(sm::conv_gather_kernel<3>, dim3(sm::grid_for(total)), dim3(256), 0, (hipStream_t)stream, src, dst, H, W, v_row, stride,
                           dilation, pad, oh, ow, total);
    return sm::check_launch("sm_conv_gather_f16x2");
}

extern "C" int sm_resnet_stem_gather_f16x2(const float* x, float* out, int32_t B, int32_t H, int32_t W, void* stream) {
    SM_REQUIRE(x && out && B > 0 && H > 0 && W > 0 && ((uintptr_t)out % 16) == 0, "sm_resnet_stem_gather_f16x2: bad arguments");
    const int oh = sm::conv_out(H, 7, 2, 1, 3), ow = sm::conv_out(W, 7, 2, 1, 3);
    const int64_t total = (int64_t)B * oh * ow * (sm::STEM_KP / 8);
    sm::TapGuard tap(stream, "stem_gather_kernel", 0.0, 64.0 * total);
    hipLaunchKernelGGL(sm::stem_gather_kernel, dim3(sm::grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, out, H, W, oh, ow, total);
    return sm::check_launch("sm_resnet_stem_gather_f16x2");
}

extern "C" int sm_maxpool3x3s2_nhwc_f32(const float* in, float* out, float* out_f16x2, int32_t B, int32_t H, int32_t W, int32_t C,
                                        void* stream) {
    SM_REQUIRE(in && (out || out_f16x2) && B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && ((uintptr_t)in % 16) == 0 &&
                   ((uintptr_t)out % 16) == 0 && ((uintptr_t)out_f16x2 % 16) == 0,
               "sm_maxpool3x3s2_nhwc_f32: bad arguments (C %% 8 == 0, 16-B aligned pointers, at least one output)");
    const int oh = sm::conv_out(H, 3, 2, 1, 1), ow = sm::conv_out(W, 3, 2, 1, 1);
    const int64_t total = (int64_t)B * oh * ow * (C / 8);
    sm::TapGuard tap(stream, "maxpool_kernel", 0.0, 32.0 * total * 3.25);
    hipLaunchKernelGGL(sm::maxpool_kernel, dim3(sm::grid_for(total)), dim3(256), 0, (hipStream_t)stream, in, out, out_f16x2, H, W, C / 8, oh, ow,
                       total);
    return sm::check_launch("sm_maxpool3x3s2_nhwc_f32");
}

extern "C" int sm_relu_split_f16x2(const float* src, float* dst, float* dst_f16x2, int64_t rows, int32_t C, void* stream) {
    SM_REQUIRE(src && (dst || dst_f16x2) && rows > 0 && C > 0 && C % 8 == 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0 &&
                   ((uintptr_t)dst_f16x2 % 16) == 0 && (const float*)dst_f16x2 != src,
               "sm_relu_split_f16x2: bad arguments (C %% 8 == 0, 16-B aligned pointers, at least one output; only dst may alias src)");
    const int64_t total = rows * (C / 8);
    sm::TapGuard tap(stream, "relu_split_kernel", 0.0, 32.0 * total * 3);
    hipLaunchKernelGGL(sm::relu_split_kernel, dim3(sm::grid_for(total)), dim3(256), 0, (hipStream_t)stream, src, dst, dst_f16x2, total);
    return sm::check_launch("sm_relu_split_f16x2");
}

extern "C" int sm_upsample_nhwc_aligned_f32(const float* in, float* up, int32_t B, int32_t gh, int32_t gw, int32_t C, int32_t scale,
                                            void* stream) {
    SM_REQUIRE(in && up && B > 0 && gh > 0 && gw > 0 && C > 0 && C % 4 == 0 && scale >= 1 && scale <= 16 && ((uintptr_t)in % 16) == 0 &&
                   ((uintptr_t)up % 16) == 0,
               "sm_upsample_nhwc_aligned_f32: bad arguments (C %% 4 == 0, scale 1..16, 16-B aligned pointers)");
    const int64_t total4 = (int64_t)B * scale * scale * gh * gw * (C / 4);
    sm::TapGuard tap(stream, "upsample_aligned_kernel", 0.0, 16.0 * total4 * 5);
    hipLaunchKernelGGL(sm::upsample_aligned_kernel<0>, dim3(sm::grid_for(total4)), dim3(256), 0, (hipStream_t)stream, in, (int64_t)gh * gw * C, up, gh,
                       gw, C, scale, total4);
    return sm::check_launch("sm_upsample_nhwc_aligned_f32");
}

extern "C" size_t sm_resnet50_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t dilated) {
    const sm::Plan p = sm::make_plan(B, H, W, dilated);
    return p.ok ? p.total : 0;
}

extern "C" int sm_resnet50_forward(const sm_resnet50_weights* w, const float* x, int32_t B, int32_t H, int32_t W, int32_t dilated,
                                   float* out1, float* out2, float* out3, float* out4, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    using namespace sm;
    SM_REQUIRE(w && x && workspace, "sm_resnet50_forward: null pointer");
    const Plan p = make_plan(B, H, W, dilated);
    SM_REQUIRE(p.ok, "sm_resnet50_forward: bad shape (B, H, W >= 1; the largest gathered operand must stay below 4 GiB)");
    if (workspace_bytes < p.total) {
        set_error("sm_resnet50_forward: workspace of %zu bytes, %zu needed", workspace_bytes, p.total);
        return SM_ENOSPACE;
    }
    SM_REQUIRE(((uintptr_t)workspace % 256) == 0, "sm_resnet50_forward: the workspace must be 256-B aligned");
    SM_REQUIRE(w->stem.w && w->stem.bias, "sm_resnet50_forward: stem weights missing");
    for (int n = 0; n < SM_RESNET50_BLOCKS; ++n) {
        const sm_resnet_block& k = w->block[n];
        SM_REQUIRE(k.conv1.w && k.conv1.bias && k.conv2.w && k.conv2.bias && k.conv3.w && k.conv3.bias &&
                       (!p.blk[n].down || (k.down.w && k.down.bias)),
                   "sm_resnet50_forward: weights of block %d missing", n);
    }
    float* outs[4] = {out1, out2, out3, out4};
    for (int i = 0; i < 4; ++i) SM_REQUIRE(((uintptr_t)outs[i] % 16) == 0, "sm_resnet50_forward: output %d must be 16-B aligned", i + 1);
    hipStream_t st = (hipStream_t)stream;
    size_t off = 0;
    auto take = [&](size_t nf) {
        float* q = reinterpret_cast<float*>(workspace) + off;
        off += (nf + 63) & ~(size_t)63;
        return q;
    };
    float *A0 = take(p.stemA), *S = take(p.stemC), *X = take(p.X), *Xs = take(p.Xs), *T1 = take(p.T1), *T2 = take(p.T2), *G = take(p.G);

    // prefix (conv1 7 x 7 / 2 + bn1 + relu, resnet_models.py:114-118) and the max-pool (:120)
    TRY_RC(sm_resnet_stem_gather_f16x2(x, A0, B, H, W, stream));
    TRY_RC(conv_gemm(st, "resnet gemm: stem", A0, w->stem, S, (int64_t)B * p.h1 * p.w1, 64, STEM_KP, SM_EPI_RELU, false));
    TRY_RC(sm_maxpool3x3s2_nhwc_f32(S, nullptr, Xs, B, p.h1, p.w1, 64, stream));

    // bottlenecks (resnet_models.py:73-93).  Xs: the block's input in F16X2; X: the same in fp32, read only as an identity residual
    for (int n = 0; n < SM_RESNET50_BLOCKS; ++n) {
        const Block& b = p.blk[n];
        const sm_resnet_block& k = w->block[n];
        const int64_t mi = (int64_t)B * b.ih * b.iw, mo = (int64_t)B * b.oh * b.ow;
        const int cout = b.planes * 4;
        TRY_RC(conv_gemm(st, "resnet gemm: conv1", Xs, k.conv1, T1, mi, b.planes, b.inplanes, SM_EPI_RELU, true));
        TRY_RC(sm_conv_gather_f16x2(T1, G, B, b.ih, b.iw, b.planes, 3, b.stride, b.dil, b.dil, stream));
        TRY_RC(conv_gemm(st, "resnet gemm: conv2", G, k.conv2, T2, mo, b.planes, 9 * b.planes, SM_EPI_RELU, true));
        if (b.down) {  // the residual is downsample(x): it goes where the identity would lie
            const float* a = Xs;
            if (b.stride == 2) {
                TRY_RC(sm_conv_gather_f16x2(Xs, G, B, b.ih, b.iw, b.inplanes, 1, 2, 1, 0, stream));
                a = G;
            }
            TRY_RC(conv_gemm(st, "resnet gemm: downsample", a, k.down, X, mo, cout, b.inplanes, SM_EPI_BIAS, false));
        }
        TRY_RC(conv_gemm(st, "resnet gemm: conv3", T2, k.conv3, X, mo, cout, b.planes, SM_EPI_RESIDUAL, false, X));
        // out += residual; relu: fp32 in place - or, for a layer's last block, into the caller's map (the next layer's first block has
        // a down-sample and never reads the identity) - and the F16X2 operand of the next conv1
        float* dst = (b.last && outs[b.layer]) ? outs[b.layer] : X;
        const bool need_s = n + 1 < SM_RESNET50_BLOCKS;
        if (need_s || dst != X) TRY_RC(sm_relu_split_f16x2(X, dst, need_s ? Xs : nullptr, mo, cout, stream));
    }
    return SM_OK;
}
