// Baseline JPEG decode with the back half on the device, bit-identical to Pillow (libjpeg-turbo at its defaults: JDCT_ISLOW,
// fancy up-sampling, no draft mode).
//
// Host half (jpeg_host.h): markers + Huffman decode of the one interleaved scan into int16 coefficients; whatever it does not take
// is "unsupported" and stays with Pillow.  Device half (here): two launches for a batch whose images all differ in size and
// sampling, driven by a table of sm_jpeg_image:
//   jpeg_idct_kernel    one thread per 8 x 8 block: dequantise, the "islow" IDCT of jidctint.c (13-bit constants, PASS1_BITS = 2,
//                       columns then rows, descale with rounding, +128, clamp), 32-bit integers.  The 64 samples replace the
//                       first 64 bytes of the block's own 128 coefficient bytes, so no second buffer exists and no
//                       full-resolution chroma plane either: the samples of a component stay block-tiled at its own resolution.
//   jpeg_rgb_kernel     16 consecutive pixels (48 bytes, three 16-byte stores) per thread over the image's flat RGB bytes:
//                       chroma up-sampled on the fly (h2v1 / h2v2 "fancy" triangle filters of jdsample.c with their edge cases over
//                       the component's real width and height; plain replication where libjpeg picks it: down-sampled width <= 2),
//                       then jdcolor.c's 16-bit fixed-point YCbCr -> RGB.
// Every pixel depends on its own image's coefficients only: the bits do not depend on the batch.
#include "common.h"
#include "jpeg_host.h"

namespace sm {

constexpr int J_CONST_BITS = 13, J_PASS1_BITS = 2;
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373,
              F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819,
              F_2_562915447 = 20995, F_3_072711026 = 25172;

// one 8-point pass of jpeg_idct_islow: in[0..7] -> out[0..7], descaled by `shift` with rounding (arithmetic shift)
__device__ __forceinline__ void idct8(const int (&in)[8], int (&out)[8], int shift) {
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * F_0_541196100;
    int tmp2 = z1 + z3 * (-F_1_847759065);
    int tmp3 = z1 + z2 * F_0_765366865;
    int tmp0 = (in[0] + in[4]) * (1 << J_CONST_BITS);
    int tmp1 = (in[0] - in[4]) * (1 << J_CONST_BITS);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7], tmp1 = in[5], tmp2 = in[3], tmp3 = in[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F_1_175875602;
    tmp0 *= F_0_298631336, tmp1 *= F_2_053119869, tmp2 *= F_3_072711026, tmp3 *= F_1_501321110;
    z1 *= -F_0_899976223, z2 *= -F_2_562915447, z3 *= -F_1_961570560, z4 *= -F_0_390180644;
    z3 += z5, z4 += z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    const int r = 1 << (shift - 1);
    out[0] = (tmp10 + tmp3 + r) >> shift;
    out[7] = (tmp10 - tmp3 + r) >> shift;
    out[1] = (tmp11 + tmp2 + r) >> shift;
    out[6] = (tmp11 - tmp2 + r) >> shift;
    out[2] = (tmp12 + tmp1 + r) >> shift;
    out[5] = (tmp12 - tmp1 + r) >> shift;
    out[3] = (tmp13 + tmp0 + r) >> shift;
    out[4] = (tmp13 - tmp0 + r) >> shift;
}

__device__ __forceinline__ int clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const sm_jpeg_image* __restrict__ imgs, int16_t* __restrict__ coef,
                                                       const uint16_t* __restrict__ qt) {
    __shared__ int sq[192];
    const sm_jpeg_image im = imgs[blockIdx.y];
    const int ncomp = im.sampling == SM_JPEG_GRAY ? 1 : 3;
    if ((int)threadIdx.x < 64 * ncomp) sq[threadIdx.x] = qt[im.qt_off + threadIdx.x];
    __syncthreads();
    const int n0 = im.blocks_w[0] * im.blocks_h[0];
    const int n1 = ncomp == 3 ? im.blocks_w[1] * im.blocks_h[1] : 0;
    const int total = n0 + 2 * n1;  // both chroma components have one size
    for (int blk = blockIdx.x * 256 + threadIdx.x; blk < total; blk += gridDim.x * 256) {
        const int* q = sq + (blk < n0 ? 0 : (blk < n0 + n1 ? 64 : 128));
        char* p = reinterpret_cast<char*>(coef) + im.coef_off + (int64_t)blk * 128;
        int ws[64];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const i32x4 v = *reinterpret_cast<const i32x4*>(p + 16 * r);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ws[8 * r + 2 * e] = (int)(short)(v[e] & 0xffff) * q[8 * r + 2 * e];
                ws[8 * r + 2 * e + 1] = (v[e] >> 16) * q[8 * r + 2 * e + 1];
            }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) {  // pass 1: columns
            const int in[8] = {ws[c], ws[8 + c], ws[16 + c], ws[24 + c], ws[32 + c], ws[40 + c], ws[48 + c], ws[56 + c]};
            int out[8];
            idct8(in, out, J_CONST_BITS - J_PASS1_BITS);
#pragma unroll
            for (int r = 0; r < 8; ++r) ws[8 * r + c] = out[r];
        }
        unsigned w[16];
#pragma unroll
        for (int r = 0; r < 8; ++r) {  // pass 2: rows
            const int in[8] = {ws[8 * r], ws[8 * r + 1], ws[8 * r + 2], ws[8 * r + 3], ws[8 * r + 4], ws[8 * r + 5], ws[8 * r + 6], ws[8 * r + 7]};
            int out[8];
            idct8(in, out, J_CONST_BITS + J_PASS1_BITS + 3);
#pragma unroll
            for (int h = 0; h < 2; ++h)
                w[2 * r + h] = (unsigned)clamp8(out[4 * h] + 128) | ((unsigned)clamp8(out[4 * h + 1] + 128) << 8) |
                               ((unsigned)clamp8(out[4 * h + 2] + 128) << 16) | ((unsigned)clamp8(out[4 * h + 3] + 128) << 24);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // the block's coefficients are all in registers: its first 64 bytes take the samples
            const u32x4 v = {w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]};
            *reinterpret_cast<u32x4*>(p + 16 * k) = v;
        }
    }
}

// sample (y, x) of a component whose blocks are `bw` to a row, 64 bytes per block at a pitch of 128
__device__ __forceinline__ int jsample(const unsigned char* base, int bw, int y, int x) {
    return base[((int64_t)(y >> 3) * bw + (x >> 3)) * 128 + ((y & 7) << 3) + (x & 7)];
}

// one chroma component at full-resolution pixel (y, x); cw x ch = its real down-sampled size
__device__ __forceinline__ int jchroma(const unsigned char* base, int bw, int sampling, bool fancy, int cw, int ch, int y, int x) {
    if (sampling == SM_JPEG_444) return jsample(base, bw, y, x);
    const int cx = x >> 1;
    if (sampling == SM_JPEG_422) {
        const int s = jsample(base, bw, y, cx);
        if (!fancy) return s;
        if (x & 1) return cx == cw - 1 ? s : (3 * s + jsample(base, bw, y, cx + 1) + 2) >> 2;
        return cx == 0 ? s : (3 * s + jsample(base, bw, y, cx - 1) + 1) >> 2;
    }
    const int cy = y >> 1;
    if (!fancy) return jsample(base, bw, cy, cx);
    int fy = (y & 1) ? cy + 1 : cy - 1;  // the farther row; past the top / bottom the edge row repeats (libjpeg's context rows)
    fy = fy < 0 ? 0 : (fy > ch - 1 ? ch - 1 : fy);
    const int self = 3 * jsample(base, bw, cy, cx) + jsample(base, bw, fy, cx);
    if (x & 1) {
        if (cx == cw - 1) return (self * 4 + 7) >> 4;
        return (self * 3 + 3 * jsample(base, bw, cy, cx + 1) + jsample(base, bw, fy, cx + 1) + 7) >> 4;
    }
    if (cx == 0) return (self * 4 + 8) >> 4;
    return (self * 3 + 3 * jsample(base, bw, cy, cx - 1) + jsample(base, bw, fy, cx - 1) + 8) >> 4;
}

__global__ __launch_bounds__(256) void jpeg_rgb_kernel(const sm_jpeg_image* __restrict__ imgs, const int16_t* __restrict__ coef,
                                                      unsigned char* __restrict__ out) {
    const sm_jpeg_image im = imgs[blockIdx.y];
    const int64_t npx = (int64_t)im.H * im.W;
    const unsigned char* yb = reinterpret_cast<const unsigned char*>(coef) + im.coef_off;
    const int64_t n0 = (int64_t)im.blocks_w[0] * im.blocks_h[0];
    const unsigned char* cbb = yb + n0 * 128;
    const unsigned char* crb = cbb + (int64_t)im.blocks_w[1] * im.blocks_h[1] * 128;
    const int sampling = im.sampling;
    const int cw = sampling >= SM_JPEG_422 ? (im.W + 1) >> 1 : im.W;
    const int ch = sampling == SM_JPEG_420 ? (im.H + 1) >> 1 : im.H;
    const bool fancy = cw > 2;  // jinit_upsampler: the triangle filters need a down-sampled width above 2
    unsigned char* dst = out + im.out_off;
    for (int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16; p0 < npx; p0 += (int64_t)gridDim.x * 256 * 16) {
        int y = (int)(p0 / im.W), x = (int)(p0 - (int64_t)y * im.W);
        const int n = npx - p0 < 16 ? (int)(npx - p0) : 16;
        unsigned wv[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // 48 bytes: R G B of 16 pixels
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            int r = 0, g = 0, b = 0;
            if (i < n) {
                const int Y = jsample(yb, im.blocks_w[0], y, x);
                if (sampling == SM_JPEG_GRAY) {
                    r = g = b = Y;
                } else {
                    const int cb = jchroma(cbb, im.blocks_w[1], sampling, fancy, cw, ch, y, x) - 128;
                    const int cr = jchroma(crb, im.blocks_w[2], sampling, fancy, cw, ch, y, x) - 128;
                    // jdcolor.c build_ycc_rgb_table: FIX(1.40200), FIX(1.77200), -FIX(0.71414), -FIX(0.34414), ONE_HALF = 32768
                    r = clamp8(Y + ((91881 * cr + 32768) >> 16));
                    b = clamp8(Y + ((116130 * cb + 32768) >> 16));
                    g = clamp8(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
                }
                if (++x == im.W) x = 0, ++y;
            }
            wv[(3 * i) >> 2] |= (unsigned)r << (8 * ((3 * i) & 3));
            wv[(3 * i + 1) >> 2] |= (unsigned)g << (8 * ((3 * i + 1) & 3));
            wv[(3 * i + 2) >> 2] |= (unsigned)b << (8 * ((3 * i + 2) & 3));
        }
        unsigned char* o = dst + p0 * 3;  // out_off is a multiple of 16 and so is 48 * k
        if (n == 16) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const u32x4 v = {wv[4 * k], wv[4 * k + 1], wv[4 * k + 2], wv[4 * k + 3]};
                *reinterpret_cast<u32x4*>(o + 16 * k) = v;
            }
        } else {  // the image's last pixels
#pragma unroll
            for (int i = 0; i < 45; ++i)
                if (i < 3 * n) o[i] = (unsigned char)(wv[i >> 2] >> (8 * (i & 3)));
        }
    }
}

}  // namespace sm

extern "C" int sm_jpeg_probe(const uint8_t* bytes, size_t len, sm_jpeg_info* info) {
    SM_REQUIRE(bytes && info, "sm_jpeg_probe: null pointer");
    smjpeg::Frame f;
    smjpeg::parse_headers(bytes, len, f);
    *info = f.info;
    return SM_OK;
}

extern "C" int sm_jpeg_entropy_decode(const uint8_t* bytes, size_t len, int16_t* coef_out, size_t cap, uint16_t* qt_out,
                                      sm_jpeg_info* info) {
    SM_REQUIRE(bytes && info && coef_out && qt_out, "sm_jpeg_entropy_decode: null pointer");
    smjpeg::Frame f;
    const bool ok = smjpeg::parse_headers(bytes, len, f);
    *info = f.info;
    if (!ok) return SM_JPEG_UNSUPPORTED;
    if ((uint64_t)f.info.coef_bytes > (uint64_t)cap) {
        sm::set_error("sm_jpeg_entropy_decode: %lld coefficient bytes needed, room for %zu", (long long)f.info.coef_bytes, cap);
        return SM_ENOSPACE;
    }
    if (!smjpeg::decode_scan(bytes, len, f, coef_out)) {
        info->supported = 0;
        return SM_JPEG_UNSUPPORTED;
    }
    smjpeg::write_tables(f, qt_out);
    return SM_OK;
}

extern "C" size_t sm_jpeg_scan_bound(const sm_jpeg_info* info, size_t len) {
    if (!info) {
        sm::set_error("sm_jpeg_scan_bound: null pointer");
        return 0;
    }
    return smjpeg::scan_bound(*info, len);
}

extern "C" int sm_jpeg_scan_prepare(const uint8_t* bytes, size_t len, uint8_t* record_out, size_t cap, sm_jpeg_scan* scan, uint16_t* qt_out,
                                    sm_jpeg_info* info) {
    SM_REQUIRE(bytes && record_out && scan && info, "sm_jpeg_scan_prepare: null pointer");
    SM_REQUIRE(((uintptr_t)record_out & 15) == 0, "sm_jpeg_scan_prepare: record_out must be 16-byte aligned");
    smjpeg::Frame f;
    const bool ok = smjpeg::parse_headers(bytes, len, f);
    *info = f.info;
    memset(scan, 0, sizeof(*scan));
    if (!ok) return SM_JPEG_UNSUPPORTED;
    const int rc = smjpeg::prepare_scan(bytes, len, f, record_out, cap, *scan);
    if (rc == SM_ENOSPACE) sm::set_error("sm_jpeg_scan_prepare: room for %zu record bytes, sm_jpeg_scan_bound gives what suffices", cap);
    if (rc == SM_JPEG_UNSUPPORTED) info->supported = 0;
    if (rc == SM_OK && qt_out) smjpeg::write_tables(f, qt_out);
    return rc;
}

extern "C" int sm_jpeg_decode_batch_u8(const sm_jpeg_image* descr_host, const sm_jpeg_image* descr_dev, int32_t B, int16_t* coef,
                                       const uint16_t* qt, uint8_t* pixels_out, void* stream) {
    SM_REQUIRE(descr_host && descr_dev && coef && qt && pixels_out, "sm_jpeg_decode_batch_u8: null pointer");
    SM_REQUIRE(B > 0 && B <= 65535, "sm_jpeg_decode_batch_u8: 1 .. 65535 images per call (got %d)", B);
    int64_t max_blocks = 0, max_px = 0;
    for (int b = 0; b < B; ++b) {
        const sm_jpeg_image& im = descr_host[b];
        SM_REQUIRE(im.H >= 1 && im.W >= 1 && im.H <= smjpeg::MAX_DIM && im.W <= smjpeg::MAX_DIM, "sm_jpeg_decode_batch_u8: image %d is %d x %d", b,
                   im.H, im.W);
        SM_REQUIRE(im.sampling >= SM_JPEG_GRAY && im.sampling <= SM_JPEG_420, "sm_jpeg_decode_batch_u8: image %d: sampling %d", b, im.sampling);
        SM_REQUIRE(im.coef_off >= 0 && im.coef_off % 16 == 0 && im.out_off >= 0 && im.out_off % 16 == 0 && im.qt_off >= 0,
                   "sm_jpeg_decode_batch_u8: image %d: coef_off and out_off must be non-negative multiples of 16, qt_off non-negative", b);
        // the block grids the kernels index must be the ones the sizes imply: whole MCUs of the sampling
        const int hs = im.sampling >= SM_JPEG_422 ? 2 : 1, vs = im.sampling == SM_JPEG_420 ? 2 : 1;
        const int mx = (im.W + 8 * hs - 1) / (8 * hs), my = (im.H + 8 * vs - 1) / (8 * vs);
        const bool grey = im.sampling == SM_JPEG_GRAY;
        SM_REQUIRE(im.blocks_w[0] == mx * hs && im.blocks_h[0] == my * vs && im.blocks_w[1] == (grey ? 0 : mx) && im.blocks_h[1] == (grey ? 0 : my) &&
                       im.blocks_w[2] == im.blocks_w[1] && im.blocks_h[2] == im.blocks_h[1],
                   "sm_jpeg_decode_batch_u8: image %d: block grid does not match %d x %d at sampling %d", b, im.H, im.W, im.sampling);
        const int64_t blocks = (int64_t)im.blocks_w[0] * im.blocks_h[0] + 2 * (int64_t)im.blocks_w[1] * im.blocks_h[1];
        SM_REQUIRE(blocks < (1 << 30), "sm_jpeg_decode_batch_u8: image %d is too large", b);
        if (blocks > max_blocks) max_blocks = blocks;
        if ((int64_t)im.H * im.W > max_px) max_px = (int64_t)im.H * im.W;
    }
    hipStream_t st = (hipStream_t)stream;
    int64_t gx = (max_blocks + 255) / 256;
    if (gx > 2048) gx = 2048;
    sm::TapGuard tap(stream, "jpeg: idct + rgb");
    hipLaunchKernelGGL(sm::jpeg_idct_kernel, dim3((unsigned)gx, B), dim3(256), 0, st, descr_dev, coef, qt);
    gx = (max_px + 16 * 256 - 1) / (16 * 256);
    if (gx > 2048) gx = 2048;
    hipLaunchKernelGGL(sm::jpeg_rgb_kernel, dim3((unsigned)gx, B), dim3(256), 0, st, descr_dev, (const int16_t*)coef, pixels_out);
    return sm::check_launch("sm_jpeg_decode_batch_u8");
}
