// Pieces that several of the forward's kernels must agree on bit for bit, each written once: the LayerNorm arithmetic of a 384-wide
// row, the merge of the folded norm's twelve partials, the GEMMs' tile order and ring-row swizzle, and the F16X2 three-product step.
#pragma once
#include "common.h"

namespace sm {

// ---- GEMM scaffolding (gemm.hip, gemm_f16x2.hip, gemm_w16.hip) ---------------------------------------------------------------
// XCD-aware tile order (1-D grid): workgroups are dealt round-robin over the 8 XCDs (id % 8 labels the XCD, each with a private
// 4 MiB L2).  Give every XCD a CONTIGUOUS range of logical tiles (m-tile major, n-tile minor) so all n-tiles of an A row-panel
// run on one XCD and re-read it from that L2 instead of the Infinity Cache.
__device__ __forceinline__ int xcd_tile_order(int tile_id, int n_workgroups) {
    const int q8 = n_workgroups >> 3, r8 = n_workgroups & 7, xcd = tile_id & 7, slot = tile_id >> 3;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
}

// Ring image of the 32x32-MFMA GEMMs: 16-B chunk c of a 128-B stage row lives in slot c ^ ring32_swz(row).  The LDS-DMA
// destination is linear, so the XOR goes on the per-lane SOURCE chunk and again on the ds_read_b128 fragment offsets
// (conflict-free for all four 16-lane groups); an XOR is its own inverse.
__device__ __forceinline__ int ring32_swz(int row) { return (row >> 1) & 7; }

// ---- F16X2 products: x y ~= xh yh + 2^-11 (xh yl + xl yh), the 2^-22 lo*lo term dropped (gemm_f16x2.hip) -----------------------
constexpr float F16X2_LO = 1.0f / 2048.0f;  // weight of a lo half: x = hi + 2^-11 lo
// 2^-11 on every f16 lane: W16 kernels pre-scale the weight's hi fragment with it (whs = wh * 2^-11, exact)
__device__ __forceinline__ f16x8 f16x2_lo8() {
    const _Float16 d = (_Float16)F16X2_LO;
    return f16x8{d, d, d, d, d, d, d, d};
}
// One 16-deep step of a 32x32 block on v_mfma_f32_32x32x16_f16: hi*hi into `mn`, hi*lo then lo*hi into `cr` (a, b = MFMA A and
// B operands).  SWAP = the transposed block: every MFMA with its operands exchanged, the products in the SAME order - the fp32
// accumulation order, hence the bits, of the block the other way round.
template <bool SWAP = false>
__device__ __forceinline__ void f16x2_step32(f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl, f32x16& mn, f32x16& cr) {
    if constexpr (SWAP) {
        mn = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, ah, mn, 0, 0, 0);
        cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl, ah, cr, 0, 0, 0);
        cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, al, cr, 0, 0, 0);
    } else {
        mn = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, mn, 0, 0, 0);
        cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, cr, 0, 0, 0);
        cr = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, cr, 0, 0, 0);
    }
}
// main + cross / 2048 in ONE rounding.  (spectral.hip keeps a join of its own: that file compiles with contraction off.)
__device__ __forceinline__ float f16x2_join(float mn, float cr) { return fmaf(cr, F16X2_LO, mn); }

// ---- LayerNorm of a 384-wide row held by a 16-lane group (four rows per wave) --------------------------------------------------
// Lane l16 owns the three 8-element groups g = l16 + 16 i as v[3][8]: every access is a 16-B (fp32: 2 x 16 B) piece and an F16X2
// group leaves as one contiguous 32-B store; statistics are 4-step butterflies inside the group.  layernorm384_kernel (the norm
// and the chained norm) and the RESIDUAL_LN epilogue of gemm_f16x2_kernel promise the same bits: this is their one arithmetic.
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
    return v;
}
// centres v in place (two-pass, biased variance) and returns 1 / sqrt(var + eps); every lane of the group must take part
__device__ __forceinline__ float ln384_center(float (&v)[3][8], float eps) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) s += ((v[i][0] + v[i][1]) + (v[i][2] + v[i][3])) + ((v[i][4] + v[i][5]) + (v[i][6] + v[i][7]));
    const float mean = group16_sum(s) * (1.0f / 384.0f);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[i][e] -= mean;
            q += v[i][e] * v[i][e];
        }
    return 1.0f / sqrtf(group16_sum(q) * (1.0f / 384.0f) + eps);
}
// o = v * rstd * gamma + beta for the centred group of columns k .. k + 7
__device__ __forceinline__ void ln384_affine(const float (&v)[8], float rstd, const float* gamma, const float* beta, int k, float (&o)[8]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float4 gm = *reinterpret_cast<const float4*>(gamma + k + 4 * h);
        const float4 bt = *reinterpret_cast<const float4*>(beta + k + 4 * h);
        o[4 * h + 0] = v[4 * h + 0] * rstd * gm.x + bt.x; o[4 * h + 1] = v[4 * h + 1] * rstd * gm.y + bt.y;
        o[4 * h + 2] = v[4 * h + 2] * rstd * gm.z + bt.z; o[4 * h + 3] = v[4 * h + 3] * rstd * gm.w + bt.w;
    }
}

// ---- LayerNorm folded into the consuming product (gemm_w16m16_kernel, qkv_attention_m16_kernel) --------------------------------
// (mu r, r) of a row from the twelve 32-column partials (mean, M2) the producing residual GEMM left for it (24 floats), merged in
// segment order, stored to `out` (a float2 lvalue).  The fused and the unfused encoder path must give the same numbers: both
// expand this.  A macro, not a function: as an inlined function the same lines changed gemm_w16m16_kernel's register allocation
// (its code generation is fragile, see its K loop); expanded in place both kernels compile to the assembly they had before.
#define SM_LN_FOLD_ROW(stats24, eps, out)                                                          \
    do {                                                                                            \
        const float4* sp_ = reinterpret_cast<const float4*>(stats24);                              \
        float mean_s_[12], m2_ = 0.f, msum_ = 0.f;                                                 \
        _Pragma("unroll") for (int q_ = 0; q_ < 6; ++q_) {                                         \
            const float4 v_ = sp_[q_];                                                             \
            mean_s_[2 * q_] = v_.x; mean_s_[2 * q_ + 1] = v_.z;                                    \
            m2_ += v_.y; m2_ += v_.w;                                                              \
            msum_ += v_.x; msum_ += v_.z;                                                          \
        }                                                                                           \
        const float mu_ = msum_ * (1.0f / 12.0f);                                                  \
        float dev_ = 0.f;                                                                           \
        _Pragma("unroll") for (int q_ = 0; q_ < 12; ++q_) dev_ += (mean_s_[q_] - mu_) * (mean_s_[q_] - mu_); \
        const float rstd_ = 1.0f / sqrtf((m2_ + 32.0f * dev_) * (1.0f / 384.0f) + (eps));          \
        (out) = make_float2(mu_ * rstd_, rstd_);                                                    \
    } while (0)

}  // namespace sm
