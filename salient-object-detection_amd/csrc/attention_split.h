// What attention_f16x2_kernel and attention_probs_f16x2_kernel share: scores of F16X2 (split) Q and K, head_dim 64, on
// v_mfma_f32_32x32x16_f16 - three MFMAs per 16 head-dims (f16x2_step32), joined as main + cross / 2048.
//
// Staging: key (and value) rows travel as raw 256-B head slices of the F16X2 rows, HAT_CH keys per chunk, by LDS-DMA into a
// two-deep ring: the DMA of chunk c+1 flies under the MFMAs of chunk c and costs neither registers nor ds_writes.  An LDS-DMA
// writes 64 consecutive 16-B pieces, so rows cannot be padded; instead piece p of row r sits at slot p ^ hat_swz(r), a bit
// permutation of r & 15 chosen so that both the b128 key reads (16 rows, one piece index) and the transposed value reads of
// attention_f16x2.hip (4 consecutive rows x 4 alternate pieces) hit 64 banks.
// Each kernel keeps its own softmax, pass structure and output code.  Two call sites spell a piece out instead of calling it,
// because the call measured slower there (same bits; profiles/forward_pieces_ab.log): attention_f16x2_kernel its score block,
// attention_probs_f16x2_kernel its K-only ring feed.  A change to hat_scores32 / hat_feed belongs in those two places as well.
#pragma once
#include "forward_pieces.h"
#include <math.h>

namespace sm {

constexpr int HAT_CH = 64;                // keys per ring slot
constexpr int HAT_TENSOR = HAT_CH * 256;  // bytes of K (or V) per slot

// slot permutation of row r: bits (r0, r1, r2, r3) -> XOR mask bits (0, 3, 1, 2)
__device__ __forceinline__ int hat_swz(int r) { return (r & 1) | ((r & 2) << 2) | ((r & 4) >> 1) | ((r & 8) >> 1); }

// Ring fill of one chunk: 16 one-KiB pieces (a piece = 4 rows) per tensor - K alone (WITH_V = false), or K then V HAT_TENSOR
// bytes behind it - dealt round-robin over the NW waves, to the slot at LDS byte address `slot_lds`.  Kp / Vp: the head's slice
// of row 0; k_row / v_row: row strides in floats (an F16X2 row has its fp32 row's bytes).  Tail rows repeat the last key (finite
// data; masked or never stored).
template <int NW, bool WITH_V>
__device__ __forceinline__ void hat_feed(const char* Kp, int64_t k_row, const char* Vp, int64_t v_row, int n_k, int chunk,
                                         unsigned slot_lds, int wave, int lane) {
    constexpr int NP = WITH_V ? 32 : 16;
#pragma unroll
    for (int j = 0; j < (NP + NW - 1) / NW; ++j) {
        const int i = wave + NW * j;
        if (i < NP) {
            const int g = i & 15, row = 4 * g + (lane >> 4);
            int key = chunk * HAT_CH + row;
            key = key < n_k ? key : n_k - 1;
            const int piece = (lane & 15) ^ hat_swz(row);
            const char* src = ((!WITH_V || i < 16) ? Kp + (int64_t)key * k_row * 4 : Vp + (int64_t)key * v_row * 4) + piece * 16;
            lds_dma16(src, __builtin_amdgcn_readfirstlane(slot_lds + (i >> 4) * HAT_TENSOR + g * 1024));
        }
    }
}

// Q fragments of query row `q` (rows from q_end on repeat row q_end - 1): lane half h, 16-dim step t -> k-group 2t + h: hi
// chunk, lo chunk.  q_row: row stride in floats.
__device__ __forceinline__ void hat_q_frags(const char* Qp, int64_t q_row, int q, int q_end, int h, f16x8 (&qh)[4], f16x8 (&ql)[4]) {
    const int qrow = q < q_end ? q : q_end - 1;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const char* p = Qp + (int64_t)qrow * q_row * 4 + (2 * t + h) * 32;
        qh[t] = *reinterpret_cast<const f16x8*>(p);
        ql[t] = *reinterpret_cast<const f16x8*>(p + 16);
    }
}

// key fragment byte offsets inside a staged row: pieces 2(2t + h) [hi] and + 1 [lo], permuted by the row
__device__ __forceinline__ void hat_key_offsets(int r, int h, int (&k_hi)[4], int (&k_lo)[4]) {
    const int ksw = hat_swz(r & 15);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        k_hi[t] = ((2 * (2 * t + h)) ^ ksw) * 16;
        k_lo[t] = ((2 * (2 * t + h) + 1) ^ ksw) * 16;
    }
}

// Raw scores (before scale) of a 32-key block against the wave's 32 queries; kr = this lane's staged key row.
// QK = false: S^T = K Q^T - register v of lane (r, h) = key acc_row(v, h) of the block, query r;
// QK = true:  S = Q K^T, the same MFMAs with the operands exchanged - register v = query acc_row(v, h), key r.
template <bool QK>
__device__ __forceinline__ void hat_scores32(const char* kr, const int (&k_hi)[4], const int (&k_lo)[4], const f16x8 (&qh)[4],
                                             const f16x8 (&ql)[4], f32x16& s) {
    f32x16 mn, cr;
#pragma unroll
    for (int v = 0; v < 16; ++v) { mn[v] = 0.f; cr[v] = 0.f; }
    f16x8 kh[4], kl[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        kh[t] = *reinterpret_cast<const f16x8*>(kr + k_hi[t]);
        kl[t] = *reinterpret_cast<const f16x8*>(kr + k_lo[t]);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) f16x2_step32<QK>(kh[t], kl[t], qh[t], ql[t], mn, cr);
#pragma unroll
    for (int v = 0; v < 16; ++v) s[v] = f16x2_join(mn[v], cr[v]);
}

// S^T block kb of a chunk with ck valid keys: rows past ck -> -inf.  Only the last chunk's last block has any (wave-uniform branch).
__device__ __forceinline__ void hat_mask_tail(f32x16& s, int kb, int ck, int h) {
    if ((kb + 1) * 32 > ck) {
#pragma unroll
        for (int v = 0; v < 16; ++v)
            if (kb * 32 + acc_row(v, h) >= ck) s[v] = -INFINITY;
    }
}

}  // namespace sm
