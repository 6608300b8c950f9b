// P = softmax(scale * Q K^T) per (batch, head), head_dim 64, WRITTEN OUT: the post-softmax `attn` of Attention.forward
// (vision_transformer.py:122-123), which VisionTransformer.get_last_selfattention returns (:307-314).  Q and K arrive in the
// F16X2 split format (as the projection GEMMs write them); products are the three-MFMA split form of attention_split.h, shared
// with attention_f16x2.hip: (hi*hi + (hi*lo + lo*hi) / 2048) * scale * log2(e), then exp2.
//
// Every key's NORMALISED probability is needed, not a running sum, so the keys are walked twice (a score tile held resident
// would be 16 registers per 32 keys: 112 at 197 tokens, 400 at 785 - it does not fit the shapes the forward accepts, and one
// structure for every n_k keeps a row's arithmetic the same everywhere):
//   pass 1  S^T = K Q^T, keys on the accumulator rows, the query on the lane (the layout of attention_f16x2.hip): maximum and
//           sum of a query are register-local plus one swap between the wave's halves, kept PER QUERY (no wave-wide decision),
//           updated once per 32-key block in key order;
//   pass 2  S = Q K^T - the same MFMAs with the operands exchanged: now the key is on the lane and the queries on the rows, so
//           a store instruction writes, for each of two query rows, 32 consecutive floats (128 B) of P.  Each lane fetches the
//           (-max * c, 1 / sum) of its 16 query rows from the lanes that own them (ds_bpermute) once, between the passes.
// A query's numbers depend on its own Q row and on the keys only - not on its position in the 32-row tile, on q0 / nq or on
// the batch - so any launch that contains a row writes the same bits for it.  Keys past n_k are masked to -inf in pass 1
// (exp2 gives exactly 0) and never stored in pass 2.  No atomics.
//
// Staging: the two-deep ring of attention_split.h, K alone (2 x 16 KiB); it simply runs through the 2 * chunks iterations of
// both passes.  Four waves of 32 queries share a ring; waves past the last query block only help with the staging.
#include "attention_split.h"

namespace sm {

constexpr int AP_NW = 4;  // waves (32 queries each) per workgroup

__global__ __launch_bounds__(AP_NW * 64, 2) void attention_probs_f16x2_kernel(sm_attn_probs_args a, int groups) {
    __shared__ __attribute__((aligned(16))) char smem[2 * HAT_TENSOR];
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)smem;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int qg = blockIdx.x % groups, pair = blockIdx.x / groups;
    const int head = pair % a.heads;
    const int64_t b = pair / a.heads;
    const int q_end = a.q0 + a.nq;
    const int qw = a.q0 + (qg * AP_NW + wave) * 32;  // first query row of this wave
    const bool active = qw < q_end;

    const char* Qp = reinterpret_cast<const char*>(a.Q + b * a.sQb + head * SM_HEAD_DIM);
    const char* Kp = reinterpret_cast<const char*>(a.K + b * a.sKb + head * SM_HEAD_DIM);
    float* Pb = a.P + b * a.sPb + ((int64_t)head * a.nq - a.q0) * a.n_k;  // row i of the image's head at Pb + i * n_k

    // ring fill: 16 one-KiB pieces per chunk (a piece = 4 rows), four per wave.  hat_feed<AP_NW, false> of attention_split.h spelled
    // out: through the shared function this kernel wrote 1.5 % fewer GB/s (profiles/forward_pieces_ab.log, bisect), same bits.
    const int n_k = a.n_k;
    const int srow = lane >> 4;
    auto issue = [&](int chunk, int slot) {
#pragma unroll
        for (int j = 0; j < 16 / AP_NW; ++j) {
            const int g = wave + AP_NW * j, row = 4 * g + srow;
            int key = chunk * HAT_CH + row;
            key = key < n_k ? key : n_k - 1;  // tail rows repeat the last key (finite data; masked / not stored below)
            const int piece = (lane & 15) ^ hat_swz(row);
            lds_dma16(Kp + (int64_t)key * a.sKr * 4 + piece * 16, __builtin_amdgcn_readfirstlane(lds0 + slot * HAT_TENSOR + g * 1024));
        }
    };
    const int nch = (n_k + HAT_CH - 1) / HAT_CH, nit = 2 * nch;
    issue(0, 0);

    f16x8 qh[4], ql[4];
    hat_q_frags(Qp, a.sQr, qw + r, q_end, h, qh, ql);
    const float cs = a.scale * 1.44269504088896340736f;  // scores in log2 units

    int k_hi[4], k_lo[4];
    hat_key_offsets(r, h, k_hi, k_lo);

    float m_run = -INFINITY, l_run = 0.f;  // pass 1: this lane's query; l_run over the rows of this lane's half
    float rm[16], ri[16];                  // pass 2: -max * cs and 1 / sum of query row acc_row(v, h)
#pragma unroll
    for (int v = 0; v < 16; ++v) { rm[v] = 0.f; ri[v] = 0.f; }

    for (int it = 0; it < nit; ++it) {
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();  // the chunk of this iteration has landed for every wave; every wave is done with the previous one
        __builtin_amdgcn_sched_barrier(0);
        if (it + 1 < nit) issue(it + 1 < nch ? it + 1 : it + 1 - nch, (it + 1) & 1);
        if (!active) continue;
        const bool second = it >= nch;
        const int c = second ? it - nch : it;
        if (it == nch) {  // between the passes (wave-uniform): every lane collects the statistics of its 16 accumulator rows
            const float inv = 1.0f / halves_sum(l_run);
            const float mo = -m_run * cs;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                rm[v] = __shfl(mo, acc_row(v, h), 64);
                ri[v] = __shfl(inv, acc_row(v, h), 64);
            }
        }
        const int ck = min(HAT_CH, n_k - c * HAT_CH);
        const char* Ks = smem + (it & 1) * HAT_TENSOR;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            if (kb * 32 >= ck) break;
            const char* kr = Ks + (kb * 32 + r) * 256;
            if (!second) {
                f32x16 s;
                hat_scores32<false>(kr, k_hi, k_lo, qh, ql, s);
                hat_mask_tail(s, kb, ck, h);
                float bmax = s[0];
#pragma unroll
                for (int v = 1; v < 16; ++v) bmax = fmaxf(bmax, s[v]);
                bmax = halves_max(bmax);  // a block always holds a real key, so bmax is finite
                const float m_new = fmaxf(m_run, bmax);
                const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * cs);  // first block: exp2(-inf) = 0
                const float moff = -m_new * cs;
                float psum = 0.f;
#pragma unroll
                for (int v = 0; v < 16; ++v) psum += __builtin_amdgcn_exp2f(fmaf(s[v], cs, moff));  // masked: exp2(-inf) = 0
                l_run = l_run * alpha + psum;
                m_run = m_new;
            } else {
                f32x16 s;
                hat_scores32<true>(kr, k_hi, k_lo, qh, ql, s);
                const int key = c * HAT_CH + kb * 32 + r;
                if (key < n_k) {
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int qi = qw + acc_row(v, h);
                        if (qi < q_end) Pb[(int64_t)qi * n_k + key] = __builtin_amdgcn_exp2f(fmaf(s[v], cs, rm[v])) * ri[v];
                    }
                }
            }
        }
    }
    wait_vmcnt<0>();  // no DMA may outlive the workgroup's LDS allocation
}

}  // namespace sm

extern "C" int sm_attention_probs_f16x2(const sm_attn_probs_args* a, void* stream) {
    SM_REQUIRE(a && a->Q && a->K && a->P, "sm_attention_probs_f16x2: null pointer");
    SM_REQUIRE(a->batch > 0 && a->heads > 0 && a->heads <= SM_HEADS && a->n_q > 0 && a->n_k > 0,
               "sm_attention_probs_f16x2: bad shape (batch, n_q, n_k >= 1; 1 <= heads <= 6)");
    SM_REQUIRE(a->q0 >= 0 && a->nq > 0 && (int64_t)a->q0 + a->nq <= a->n_q, "sm_attention_probs_f16x2: query range [q0, q0 + nq) outside [0, n_q)");
    SM_REQUIRE(a->scale > 0.f, "sm_attention_probs_f16x2: scale must be positive");
    SM_REQUIRE(a->sQr % 8 == 0 && a->sKr % 8 == 0 && a->sQb % 8 == 0 && a->sKb % 8 == 0 && a->sQr >= SM_HEAD_DIM && a->sKr >= SM_HEAD_DIM,
               "sm_attention_probs_f16x2: strides must be multiples of 8 elements (F16X2 groups)");
    SM_REQUIRE(((uintptr_t)a->Q | (uintptr_t)a->K) % 32 == 0 && (uintptr_t)a->P % 4 == 0,
               "sm_attention_probs_f16x2: Q, K must be 32-B aligned (one F16X2 group), P 4-B aligned");
    const int64_t packed = (int64_t)a->heads * a->nq * a->n_k;
    SM_REQUIRE(a->sPb == 0 || a->sPb >= packed, "sm_attention_probs_f16x2: sPb smaller than one image's block (heads * nq * n_k)");
    sm_attn_probs_args k = *a;
    if (k.sPb == 0) k.sPb = packed;
    const int nqb = (a->nq + 31) / 32;
    const int groups = (nqb + sm::AP_NW - 1) / sm::AP_NW;
    const int64_t grid = (int64_t)groups * a->heads * a->batch;
    SM_REQUIRE(grid < ((int64_t)1 << 31), "sm_attention_probs_f16x2: too many workgroups");
    hipLaunchKernelGGL(sm::attention_probs_f16x2_kernel, dim3((unsigned)grid), dim3(sm::AP_NW * 64), 0, (hipStream_t)stream, k, groups);
    return sm::check_launch("sm_attention_probs_f16x2");
}
