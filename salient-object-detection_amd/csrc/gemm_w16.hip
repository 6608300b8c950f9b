// fp32-grade GEMM against a WEIGHT matrix on the f16 matrix cores with ONE fp32 accumulator: C = epilogue(A W^T + bias),
// A in the F16X2 split format (hi = f16(a), lo' = f16((a - hi) * 2^11), as every producer writes it), W in the
// "W16" format prepared once per checkpoint.
//
// Why a second weight format.  gemm_f16x2.hip evaluates a*w as hi*hi + 2^-11 (hi*lo' + lo'*hi) and therefore needs TWO
// accumulators (main, cross): 32 accumulator registers per 32x32 block.  That caps the tile a workgroup can own, and
// the kernel is fed through the texture path (LDS-DMA: ~16 cycles of the CU's single address unit per 1-KiB piece):
// at 128 x 128 the staging of both operands takes two thirds of the MFMA time and any stall shows.
// Weights are static, so they can be pre-scaled: W' = W * 2^s with s chosen per tensor so that max|W'| lies in
// [2^13, 2^14).  Then wl = f16(W' - f16(W')) is a NORMAL f16 number without its own 2^11 factor (or, for tiny weights,
// a subnormal whose absolute error is 2^-39 of the tensor's maximum), and
//     a * w' = ah*wh + ah*wl + al'*(wh * 2^-11)            (dropping al*wl, 2^-22 relative, as before)
// all three products in the SAME scale: one accumulator, three MFMAs.  whs = wh * 2^-11 is exact (wh >= 2^-3 after the
// scaling, far above the f16 subnormal range) and costs four v_pk_mul_f16 per weight fragment, hidden under the MFMAs.
// The epilogue multiplies the accumulator by 2^-s (exact) before the bias.  Half the accumulator registers buy a
// 256 x 128 tile per workgroup: 3/4 of the staged bytes per MFMA of the 128 x 128 tile at the same occupancy.
//
// Everything else is the structure of gemm_f16x2.hip: LDS-DMA ring with counted vmcnt + one raw barrier per K-tile, XOR swizzle on
// the DMA source address and the fragment reads, weights as the MFMA A operand (a lane owns one output row), epilogue
// turned through the idle ring so global accesses are contiguous row segments, XCD-aware tile order (forward_pieces.h).
#include "forward_pieces.h"
#include <type_traits>
#include <mutex>
#include <stdlib.h>

namespace sm {

// ---- 16x16x32 MFMA kernel ---------------------------------------------------------------------------------------------------
// The GEMM runs on v_mfma_f32_16x16x32_f16.  Why: with three batches in flight the chip sits at its power limit, and in
// an MFMA-dense loop on random operands the 16x16x32 shape sustains 12-14 % more FLOP/s than 32x32x16 at the same cycles
// per FLOP (scripts/mb/mfma_shape.hip: 1.75 vs 1.55 PFLOP/s; MI355X_MICROARCH.md, DVFS give-back item 7).  A 32x32x16 family
// of this kernel was measured and rejected.
// A / B operands: lane l holds row (l & 15), k-group (l >> 4) of a 32-k stage - one 16-B hi chunk and one 16-B lo chunk per
// fragment, so a stage is ONE MFMA step.  C: lane l holds output row m = l & 15 and four consecutive n = 4 (l >> 4) + reg.
// LDS image of a 128-B stage row (four k-groups x [hi | lo]): m16_slot of common.h, conflict-free for the fragment reads.  The
// LDS-DMA destination is linear, so the permutation goes on the per-lane SOURCE address (m16_chunk_of_slot).
typedef float f32x4v __attribute__((ext_vector_type(4)));

#ifdef SM_TUNING  // in-kernel stamps (tuning build only; a buffer nothing else reads): prologue / K loop / epilogue of a tile
__device__ unsigned long long g_gemm_stamps[2048 * 4];
__device__ int g_gemm_stamp_filter[3];  // (N, K, M) of the launches that stamp; N = 0: every launch (sm_gemm_stamp_filter)
// each workgroup keeps its stamps in registers and writes the record once, at the end: launches of several streams share the
// buffer, and a record must come from ONE workgroup
#define GEMM_STAMP(i)                                                                                                          \
    do {                                                                                                                       \
        asm volatile("" ::: "memory"); /* no load or store moves across a stamp */                                             \
        stamp_[i] = __builtin_amdgcn_s_memtime();                                                                              \
        asm volatile("" ::: "memory");                                                                                         \
    } while (0)
#define GEMM_STAMP_DECL unsigned long long stamp_[4] = {0, 0, 0, 0}
#define GEMM_STAMP_FLUSH                                                                                                         \
    do {                                                                                                                        \
        if (blockIdx.x < 2048 && tid == 0 && (g_gemm_stamp_filter[0] == 0 || (g.N == g_gemm_stamp_filter[0] && g.K == g_gemm_stamp_filter[1] && g.M == g_gemm_stamp_filter[2]))) \
            for (int i_ = 0; i_ < 4; ++i_) g_gemm_stamps[blockIdx.x * 4 + i_] = stamp_[i_];                                      \
    } while (0)
#else
#define GEMM_STAMP(i) do {} while (0)
#define GEMM_STAMP_DECL do {} while (0)
#define GEMM_STAMP_FLUSH do {} while (0)
#endif

// TERMS = 3: the fp32-grade product (wh*ah + wl*ah + whs*al').  TERMS = 1: "throughput mode"  - only wh*ah,
// plain f16 operands with fp32 accumulation: a DIAGNOSTIC of what the kernel structure reaches without the x3, never the
// metric (the results miss the 1e-4 gate by two orders of magnitude).  Same operand formats: the lo halves are staged and ignored.
// Ring feed.  Source addresses are a wave-uniform base (advanced per K-tile by scalar adds) + one 32-bit per-lane offset per
// piece.  Letting only the first half of the waves issue the pieces took 11 % off the fused QKV kernel's projection loop
// (qkv_attention.hip, shipped there) but nothing off these GEMMs: K loop of the 256 x 128 fc2 tile 102.5k cycles against 97.4k,
// pipeline 21.75k vs 21.75k images/s (profiles/r03_loader_half_ab.log) - four waves per SIMD already cover each other's issue time.
//
// Epilogue selection.  EPI_T >= 0: the epilogue (SM_EPI_*) and the output format (F16OUT: F16X2 instead of fp32) are fixed at
// compile time; EPI_T < 0: chosen at run time from g.epilogue / g.patch_n < 0, every epilogue in one kernel.  PLAIN: the launch
// uses none of ln_stats, C2, ln_stats_out, A_alt and split-K, and the kernel carries no code, registers or LDS for them.  The host
// instantiates <EPI_T, F16OUT, PLAIN = true> for the (tile, epilogue, format) combinations the forward launches and ONE generic
// <-1, false, false> kernel per tile for everything else (launch_gemm_m16): a specialisation's register allocation and the code
// behind its K loop are those of the one epilogue it runs.  Same arithmetic per element in both: results are bit-identical.
template <int BM, int BN, int NST, int NWM, int NWN, int WPS, int TERMS = 3, int EPI_T = -1, bool F16OUT = false, bool PLAIN = false>
__global__ __launch_bounds__(NWM * NWN * 64, WPS) void gemm_w16m16_kernel(sm_gemm_args g) {
    constexpr int NW = NWM * NWN, WTM = BM / NWM, WTN = BN / NWN;
    constexpr int TM = WTM / 16, TN = WTN / 16;       // 16x16 tiles per wave
    constexpr int ROWB = 128;
    // waves that feed the ring: all of them, or the first half where a stage's 8-row pieces do not divide among all (the 256 x 192 tile)
    constexpr int NL = ((BN / 8) % NW != 0 || (BM / 8) % NW != 0) ? NW / 2 : NW;
    constexpr int A_INST = BM / 8 / NL, W_INST = BN / 8 / NL;
    static_assert(A_INST * 8 * NL == BM && W_INST * 8 * NL == BN && TM * 16 * NWM == BM && TN * 16 * NWN == BN && (TM % 2) == 0, "tile split");
    constexpr int NI = A_INST + W_INST;
    constexpr int A_STAGE = BM * ROWB, W_STAGE = BN * ROWB, W_RING = NST * A_STAGE, RING_BYTES = NST * (A_STAGE + W_STAGE);
    extern __shared__ __attribute__((aligned(16))) char smemm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / NWN, wn = wave % NWN;
    const int r16 = lane & 15, kg = lane >> 4;
    const int tile_id = xcd_tile_order(blockIdx.x, gridDim.x);
    const int ntn = (g.N + BN - 1) / BN;
    const int n0 = (tile_id % ntn) * BN, m0 = (tile_id / ntn) * BM;
    const int M = g.M, N = g.N;
    const int split = (!PLAIN && g.split_k > 1) ? g.split_k : 1;
    const int nk = g.K / 32 / split;
    const int k_begin = split > 1 ? (int)blockIdx.z * nk * 32 : 0;
    const char* A = reinterpret_cast<const char*>(((!PLAIN && g.alt_from_n > 0 && n0 >= g.alt_from_n) ? g.A_alt : g.A) + k_begin);
    const char* W = reinterpret_cast<const char*>(g.W + k_begin);
    // DMA: lane -> (row = lane >> 3 of its 8-row piece, slot p = lane & 7); the slot holds chunk (2 kg + x) with
    // kg = ((p >> 1) + 2 * ((row >> 3) & 1)) & 3 (the pair rotation is its own inverse), x = (p & 1) ^ ((row >> 1) & 1)
    const bool loader = wave < NL;
    const int lw = loader ? wave : 0;  // (the offsets of a non-loader are never used)
    unsigned a_off[A_INST], w_off[W_INST];  // byte offsets from A / W (the host checks that M lda 4 and N ldw 4 fit in 32 bits)
    auto src_chunk = [&](int row) { return m16_chunk_of_slot(row, lane & 7); };
#pragma unroll
    for (int i = 0; i < A_INST; ++i) {
        const int row = (lw * A_INST + i) * 8 + (lane >> 3);
        int gm = m0 + row;
        gm = gm < M ? gm : M - 1;
        a_off[i] = (unsigned)gm * (unsigned)g.lda * 4u + src_chunk(row) * 16;
    }
#pragma unroll
    for (int i = 0; i < W_INST; ++i) {
        const int row = (lw * W_INST + i) * 8 + (lane >> 3);
        int gn = n0 + row;
        gn = gn < N ? gn : N - 1;
        w_off[i] = (unsigned)gn * (unsigned)g.ldw * 4u + src_chunk(row) * 16;
    }
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)smemm;
    auto issue_step = [&](int kt) {
        if (!loader) return;  // wave-uniform; a non-loader has no piece in flight, its vmcnt waits pass at once
        const int t = kt + NST - 1;
        const int tt = t < nk ? t : nk - 1, slot = t % NST;
        const char* wb = W + tt * ROWB;  // scalar: the K-tile's column block of both operands
        const char* ab = A + tt * ROWB;
        const unsigned sw = __builtin_amdgcn_readfirstlane(lds_base + W_RING + slot * W_STAGE + wave * W_INST * 1024);
#pragma unroll
        for (int i = 0; i < W_INST; ++i) lds_dma16_s(wb, w_off[i], sw + i * 1024);
        const unsigned sa = __builtin_amdgcn_readfirstlane(lds_base + slot * A_STAGE + wave * A_INST * 1024);
#pragma unroll
        for (int i = 0; i < A_INST; ++i) lds_dma16_s(ab, a_off[i], sa + i * 1024);
    };
    // fragment offsets: tile rows are multiples of 16, so the slot of (row = base + r16, kg) does not depend on the tile
    const int off_hi = r16 * ROWB + m16_slot(r16, kg, 0) * 16, off_lo = r16 * ROWB + m16_slot(r16, kg, 1) * 16;
    const int a_base = wm * WTM * ROWB, w_base = wn * WTN * ROWB;

    f32x4v acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[i][j][v] = 0.f;
    GEMM_STAMP_DECL;
    GEMM_STAMP(0);
#pragma unroll
    for (int v = -(NST - 1); v < 0; ++v) issue_step(v);
    // LayerNorm folded into this GEMM (g.ln_stats): A holds the RAW residual stream x (F16X2), W the weight times the norm's gain,
    // and LN(x) W^T + b = r (x W'^T - mu c) + b' with c = row sums of W', b' = b + W beta - applied in the epilogue.  Here, under
    // the latency of the first K-tile: (mu r, r) of this tile's rows (SM_LN_FOLD_ROW, forward_pieces.h) into LDS behind the ring (a PLAIN
    // launch has no such tail).
    float2* lnrow = reinterpret_cast<float2*>(smemm + RING_BYTES);
    if (!PLAIN && g.ln_stats && tid < BM) {
        int m = m0 + tid;
        m = m < M ? m : M - 1;
        SM_LN_FOLD_ROW(g.ln_stats + (int64_t)m * 24, g.ln_eps, lnrow[tid]);
    }
    const f16x8 down = f16x2_lo8();
    for (int kt = 0; kt < nk; ++kt) {
        wait_vmcnt<(NST - 2) * NI>();
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (kt == 0) GEMM_STAMP(1);
        issue_step(kt);
        const char* sta = smemm + (kt % NST) * A_STAGE + a_base;
        const char* stw = smemm + W_RING + (kt % NST) * W_STAGE + w_base;
        // Register plan: the W fragments of the step stay live (TN x 12 registers), the A fragments come in blocks of at most
        // four row tiles (32 registers) - with TM = 8 all sixteen A fragments do not fit beside 64 accumulator registers in a
        // 128-register budget, and left to itself the compiler re-read some of them from LDS in an order that changed from
        // build to build (a K loop of 42.5k or 51.6k cycles for the same source, scripts/gemm_stamps.py)
        f16x8 wh[TN], wl[TN], whs[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            wh[j] = *reinterpret_cast<const f16x8*>(stw + j * 16 * ROWB + off_hi);
            if constexpr (TERMS == 3) wl[j] = *reinterpret_cast<const f16x8*>(stw + j * 16 * ROWB + off_lo);
        }
        constexpr int IB = TM > 4 ? 4 : TM;
#pragma unroll
        for (int i0 = 0; i0 < TM; i0 += IB) {
            f16x8 ah[IB], al[IB];
#pragma unroll
            for (int ii = 0; ii < IB; ++ii) {
                ah[ii] = *reinterpret_cast<const f16x8*>(sta + (i0 + ii) * 16 * ROWB + off_hi);
                if constexpr (TERMS == 3) al[ii] = *reinterpret_cast<const f16x8*>(sta + (i0 + ii) * 16 * ROWB + off_lo);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if constexpr (TERMS == 3) {
                    if (i0 == 0) whs[j] = wh[j] * down;
                }
#pragma unroll
                for (int ii = 0; ii < IB; ++ii) {
                    acc[i0 + ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[j], ah[ii], acc[i0 + ii][j], 0, 0, 0);
                    if constexpr (TERMS == 3) {
                        acc[i0 + ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[j], ah[ii], acc[i0 + ii][j], 0, 0, 0);
                        acc[i0 + ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(whs[j], al[ii], acc[i0 + ii][j], 0, 0, 0);
                    }
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    wait_vmcnt<0>();
    GEMM_STAMP(2);

    float* C = g.C + (split > 1 ? (int64_t)blockIdx.z : 0) * g.strideC;
    const bool out_split = g.patch_n < 0;
    const float ws = g.w_scale;
    // Epilogue staging (the idle ring): 32 rows of this wave's WTN columns.  For 32-column slices (the 256 x 256 and 256 x 128
    // shapes) rows are 128 B with the 16-B piece c of row r at slot c ^ (r & 7) and, for F16X2 output, the two 8-B halves of a piece
    // swapped on rows with bit 3 set: the 8-lane groups of a float4 store, the 16-lane groups of an 8-B store and the four 16-lane
    // groups of the read-back each cover a bank row once.  (Rounds 2-3 padded rows to 144 B: lanes r and r + 8 of every 8-B store met on
    // one bank pair and two lanes of every read-back group shared a slot - the 0.14 conflict ratio of profiles/r03_pmc_sq_counters.txt
    // was this epilogue, not the K loop.)  Other slice widths keep the padded rows.
    constexpr bool SWZ = WTN == 32;
    constexpr int EPLD = SWZ ? 128 : WTN * 4 + 16;
    constexpr int PIECES = WTN / 4;
    static_assert(NW * 32 * EPLD <= RING_BYTES, "epilogue staging must fit in the ring");
    __builtin_amdgcn_s_barrier();
    char* ep = smemm + wave * (32 * EPLD);

    auto run = [&](auto epi_tag, auto fmt_tag, auto full_tag) {
        constexpr int EPI = decltype(epi_tag)::value;
        constexpr bool F = decltype(fmt_tag)::value;
        constexpr bool FULL = decltype(full_tag)::value;  // the whole tile lies inside C: no row / column guard on any load or store
        // The rows added in the epilogue (residual stream / position table) are fetched a 32-row block ahead, all of a
        // block's loads before any of its stores: C may alias R (in-place residual), so left in one loop every load would
        // wait behind the previous store: 16-24 exposed memory latencies per tile (scripts/gemm_stamps.py).
        constexpr int NIT = 32 * PIECES / 64;
        constexpr bool HASR = EPI == SM_EPI_RESIDUAL || EPI == SM_EPI_PATCH;
        // A PLAIN two-block tile (256 x 128: proj, fc2, patch) fetches the rows of BOTH blocks here, ahead of everything else: without
        // the other epilogues' registers in the allocation 2 x NIT float4 fit, and block 1 no longer waits a memory latency for its
        // rows behind block 0's stores.  Every load of the tile still precedes every store.
        constexpr bool ALLRES = HASR && PLAIN && TM / 2 == 2 && NIT <= 4;
        float4 res_[ALLRES ? 2 : 1][HASR ? NIT : 1];
        auto load_res = [&](int ib) {
            float4* res = res_[ALLRES ? ib : 0];
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int idx = it * 64 + lane, row = idx / PIECES, pc = idx % PIECES;
                const int m = m0 + wm * WTM + ib * 32 + row, n = n0 + wn * WTN + pc * 4;
                res[it] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (FULL || (m < M && n < N)) {
                    if constexpr (EPI == SM_EPI_RESIDUAL) res[it] = *reinterpret_cast<const float4*>(g.R + (int64_t)m * g.ldr + n);
                    else if constexpr (EPI == SM_EPI_PATCH) res[it] = *reinterpret_cast<const float4*>(g.R + (int64_t)(1 + m % g.patch_n) * g.ldr + n);
                }
            }
        };
        if constexpr (HASR) load_res(0);
        if constexpr (ALLRES) load_res(1);
        // this lane's bias values (columns 16 j + 4 kg .. + 3 of the wave's slice), fetched ONCE and all together: read per
        // element inside the loops below they were TM x TN x 4 guarded scalar loads, each waited for in its own branch
        float brow[TN][4];
        {
            const bool vec = g.bias && (reinterpret_cast<uintptr_t>(g.bias) & 15) == 0;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * WTN + j * 16 + 4 * kg;
                float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
                if (vec && (FULL || n + 3 < N)) {
                    bv = *reinterpret_cast<const float4*>(g.bias + n);
                } else if (g.bias) {
                    if (n < N) bv.x = g.bias[n];
                    if (n + 1 < N) bv.y = g.bias[n + 1];
                    if (n + 2 < N) bv.z = g.bias[n + 2];
                    if (n + 3 < N) bv.w = g.bias[n + 3];
                }
                brow[j][0] = bv.x; brow[j][1] = bv.y; brow[j][2] = bv.z; brow[j][3] = bv.w;
            }
        }
        // folded LayerNorm (consumer side): c[n] = sum_k W'[n][k] of this lane's columns (N % 4 == 0, c 16-B aligned: host-checked)
        constexpr bool CANFOLD = !HASR && !PLAIN;
        const bool fold = CANFOLD && g.ln_stats != nullptr;
        float crow[CANFOLD ? TN : 1][4];
        if constexpr (CANFOLD) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * WTN + j * 16 + 4 * kg;
                float4 cv = make_float4(0.f, 0.f, 0.f, 0.f);
                if (fold && n + 3 < N) cv = *reinterpret_cast<const float4*>(g.ln_c + n);
                crow[j][0] = cv.x; crow[j][1] = cv.y; crow[j][2] = cv.z; crow[j][3] = cv.w;
            }
        }
        // One 32-row block (two 16-row tiles) at a time goes through the staging area.  fill(ib, phase): phase 0 = the block's values
        // computed and written to the LDS piece by piece; 1 = register maths only (kept in the output format); 2 = those registers written
        float tq[F ? 1 : 2][F ? 1 : TN][4];
        f16x4 thi[F ? 2 : 1][F ? TN : 1], tlo[F ? 2 : 1][F ? TN : 1];
        auto fill = [&](int ib, auto phase_tag) {
            constexpr int PH = decltype(phase_tag)::value;
#pragma unroll
            for (int ii = 0; ii < 2; ++ii) {
                const int i = 2 * ib + ii, row = ii * 16 + r16;
                float rs = ws, mur = 0.f;  // fold: t = acc (2^-s r) + (b' - mu r c)
                if constexpr (CANFOLD) {
                    if (fold) {
                        const float2 lr = lnrow[wm * WTM + i * 16 + r16];
                        rs = ws * lr.y;
                        mur = lr.x;
                    }
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int nl = j * 16 + 4 * kg;  // this lane: columns nl .. nl+3 of its row
                    float t[4];
                    f16x4 hi, lo;
                    if constexpr (PH != 2) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if constexpr (CANFOLD) {  // (wave-uniform branch: the plain path keeps its one fma per element)
                                if (fold) t[e] = acc[i][j][e] * rs + (brow[j][e] - mur * crow[j][e]);
                                else t[e] = acc[i][j][e] * ws + brow[j][e];
                            } else {
                                t[e] = acc[i][j][e] * ws + brow[j][e];
                            }
                            if constexpr (EPI == SM_EPI_RELU) t[e] = fmaxf(t[e], 0.f);
                        }
                        if constexpr (EPI == SM_EPI_GELU) gelu4(t);
                        if constexpr (F) split4(t, hi, lo);
                        if constexpr (PH == 1) {
                            if constexpr (F) {
                                thi[ii][j] = hi; tlo[ii][j] = lo;
                            } else {
#pragma unroll
                                for (int e = 0; e < 4; ++e) tq[ii][j][e] = t[e];
                            }
                        }
                    } else {
                        if constexpr (F) {
                            hi = thi[ii][j]; lo = tlo[ii][j];
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) t[e] = tq[ii][j][e];
                        }
                    }
                    if constexpr (PH != 1) {
                        if constexpr (F) {  // F16X2: elements nl..nl+3 of group nl / 8: hi at 32 G + 8 (kg & 1), lo 16 B further
                            if constexpr (SWZ) {
                                const int pc = 2 * (nl >> 3), half = ((kg & 1) ^ ((row >> 3) & 1)) * 8;
                                char* p = ep + row * EPLD + half;
                                *reinterpret_cast<f16x4*>(p + ((pc ^ (row & 7)) * 16)) = hi;
                                *reinterpret_cast<f16x4*>(p + (((pc + 1) ^ (row & 7)) * 16)) = lo;
                            } else {
                                char* p = ep + row * EPLD + (nl >> 3) * 32 + (kg & 1) * 8;
                                *reinterpret_cast<f16x4*>(p) = hi;
                                *reinterpret_cast<f16x4*>(p + 16) = lo;
                            }
                        } else {
                            const int pc = SWZ ? ((nl >> 2) ^ (row & 7)) : (nl >> 2);
                            *reinterpret_cast<float4*>(ep + row * EPLD + pc * 16) = make_float4(t[0], t[1], t[2], t[3]);
                        }
                    }
                }
            }
        };
        using Ph0 = std::integral_constant<int, 0>;
        using Ph1 = std::integral_constant<int, 1>;
        using Ph2 = std::integral_constant<int, 2>;
        // PIPE (the PLAIN kernels): the next block's maths runs right behind this block's LDS writes, before the wave waits for
        // anything, and a block's pieces are ALL read back before the first is stored (read and stored one by one, each read was
        // waited for inside its store's guard: four exposed LDS latencies per block).  The staging area is this wave's own and the LDS
        // executes a wave's instructions in order, so between the writes, the reads and the next block's writes the compiler only has
        // to keep the program order (the empty asm); the one wait left per block is the one the stores' operands need.  Maths BETWEEN
        // the reads and the stores (four more float4 live) spilled in the 256 x 256 GELU kernel, and a second staging buffer - block
        // ib + 1 written before block ib is read - changed nothing: fc1 epilogue 12.15 k cycles against 12.12 k, and one spilled
        // register in its K loop (profiles/gemm_w16_epilogues.log).  The generic kernel keeps both full drains and its order.
        constexpr bool PIPE = PLAIN;
        if constexpr (PIPE) fill(0, Ph1{});
#pragma unroll
        for (int ib = 0; ib < TM / 2; ++ib) {
            if constexpr (PIPE) {
                fill(ib, Ph2{});
                asm volatile("" ::: "memory");
            } else {
                fill(ib, Ph0{});
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            auto store_piece = [&](int it, const float4& val) {
                const int idx = it * 64 + lane, row = idx / PIECES, pc = idx % PIECES;
                int m = m0 + wm * WTM + ib * 32 + row;
                const int n = n0 + wn * WTN + pc * 4;
                if (FULL || (m < M && n < N)) {
                    if constexpr (EPI == SM_EPI_PATCH) {
                        const int img = m / g.patch_n, p = m - img * g.patch_n;
                        m = img * (g.patch_n + 1) + 1 + p;
                    }
                    *reinterpret_cast<float4*>(C + (int64_t)m * g.ldc + n) = val;
                    if constexpr (EPI == SM_EPI_RESIDUAL && !PLAIN) {
                        if (g.C2) {  // the F16X2 copy of the new residual stream: A operand of the GEMM the next LayerNorm is folded into
                            const float vv[4] = {val.x, val.y, val.z, val.w};
                            store_f16x2_4(g.C2 + (int64_t)m * g.ldc, n, vv);
                        }
                    }
                }
                if constexpr (EPI == SM_EPI_RESIDUAL && WTN == 32 && !PLAIN) {
                    // ... and that norm's row statistics over this wave's 32 columns: (mean, M2) by two 8-lane butterflies (the
                    // eight lanes pc = 0..7 of a row are consecutive), two-pass, written to slot (row, column segment): fixed
                    // order everywhere, no atomics.  Rows past M join the shuffles (their staging rows hold finite values).
                    if (g.ln_stats_out) {
                        float sm_ = (val.x + val.y) + (val.z + val.w);
                        sm_ += __shfl_xor(sm_, 1, 64); sm_ += __shfl_xor(sm_, 2, 64); sm_ += __shfl_xor(sm_, 4, 64);
                        const float mean = sm_ * (1.0f / 32.0f);
                        const float dx = val.x - mean, dy = val.y - mean, dz = val.z - mean, dw = val.w - mean;
                        float q2 = (dx * dx + dy * dy) + (dz * dz + dw * dw);
                        q2 += __shfl_xor(q2, 1, 64); q2 += __shfl_xor(q2, 2, 64); q2 += __shfl_xor(q2, 4, 64);
                        if (pc == 0 && m < M && n < N)
                            *reinterpret_cast<float2*>(g.ln_stats_out + ((int64_t)m * 12 + (n0 + wn * WTN) / 32) * 2) = make_float2(mean, q2);
                    }
                }
            };
            const float4* res = res_[ALLRES ? ib : 0];
            auto staged = [&](int it) {
                const int idx = it * 64 + lane, row = idx / PIECES, pc = idx % PIECES;
                float4 val = *reinterpret_cast<const float4*>(ep + row * EPLD + (SWZ ? (pc ^ (row & 7)) : pc) * 16);
                if constexpr (SWZ && F) {  // rows with bit 3 set hold the halves of a piece swapped
                    if (row & 8) val = make_float4(val.z, val.w, val.x, val.y);
                }
                if constexpr (HASR) { val.x = res[it].x + val.x; val.y = res[it].y + val.y; val.z = res[it].z + val.z; val.w = res[it].w + val.w; }
                return val;
            };
            if constexpr (PIPE) {
                if (ib + 1 < TM / 2) fill(ib + 1, Ph1{});
                __builtin_amdgcn_sched_barrier(0);  // (left alone the scheduler pulls later blocks' maths up as well, and spills)
                float4 v[NIT];
#pragma unroll
                for (int it = 0; it < NIT; ++it) v[it] = staged(it);
                if constexpr (HASR && !ALLRES) {  // the next block's rows fly under this block's stores
                    if (ib + 1 < TM / 2) load_res(ib + 1);
                }
#pragma unroll
                for (int it = 0; it < NIT; ++it) store_piece(it, v[it]);
                asm volatile("" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
            } else {
#pragma unroll
                for (int it = 0; it < NIT; ++it) store_piece(it, staged(it));
                if constexpr (HASR && !ALLRES) {
                    if (ib + 1 < TM / 2) load_res(ib + 1);
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        }
    };
    using T = std::true_type;
    using Fa = std::false_type;
    if constexpr (EPI_T >= 0) {
        // interior tiles (all but the last row / column of tiles) take a copy of the epilogue without the per-piece guards
        const bool full = PLAIN && m0 + BM <= M && n0 + BN <= N;
        if (full) run(std::integral_constant<int, EPI_T>{}, std::integral_constant<bool, F16OUT>{}, T{});
        else run(std::integral_constant<int, EPI_T>{}, std::integral_constant<bool, F16OUT>{}, Fa{});
    } else switch (g.epilogue) {
        case SM_EPI_GELU: out_split ? run(std::integral_constant<int, SM_EPI_GELU>{}, T{}, Fa{}) : run(std::integral_constant<int, SM_EPI_GELU>{}, Fa{}, Fa{}); break;
        case SM_EPI_RELU: out_split ? run(std::integral_constant<int, SM_EPI_RELU>{}, T{}, Fa{}) : run(std::integral_constant<int, SM_EPI_RELU>{}, Fa{}, Fa{}); break;
        case SM_EPI_RESIDUAL: run(std::integral_constant<int, SM_EPI_RESIDUAL>{}, Fa{}, Fa{}); break;
        case SM_EPI_PATCH: run(std::integral_constant<int, SM_EPI_PATCH>{}, Fa{}, Fa{}); break;
        default: out_split ? run(std::integral_constant<int, SM_EPI_BIAS>{}, T{}, Fa{}) : run(std::integral_constant<int, SM_EPI_BIAS>{}, Fa{}, Fa{}); break;
    }
#ifdef SM_TUNING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stamp sees the stores retired (tuning build only)
    GEMM_STAMP(3);
    GEMM_STAMP_FLUSH;
#endif
}

template <int BM, int BN, int NST, int NWM, int NWN, int WPS, int TERMS = 3, int EPI_T = -1, bool F16OUT = false, bool PLAIN = false>
static int launch_gemm_m16_terms(const sm_gemm_args& g, hipStream_t st) {
    dim3 grid(((g.N + BN - 1) / BN) * ((g.M + BM - 1) / BM), 1, (!PLAIN && g.split_k > 1) ? g.split_k : 1);
    // ring + (generic kernel) (mu r, r) of the tile's rows (folded LayerNorm)
    constexpr size_t lds = (size_t)NST * (BM + BN) * 128 + (PLAIN ? 0 : (size_t)BM * 8);
    if (lds > 64 * 1024) {
        static std::once_flag attr_once;
        std::call_once(attr_once, [] {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_w16m16_kernel<BM, BN, NST, NWM, NWN, WPS, TERMS, EPI_T, F16OUT, PLAIN>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            (void)hipGetLastError();
        });
    }
    hipLaunchKernelGGL((gemm_w16m16_kernel<BM, BN, NST, NWM, NWN, WPS, TERMS, EPI_T, F16OUT, PLAIN>), grid, dim3(NWM * NWN * 64), lds, st, g);
    return check_launch("sm_gemm_w16 (16x16x32)");
}
// One (epilogue, output format) a tile has a PLAIN specialisation for.  The lists in sm_gemm_w16_tile name what the forward
// (forward.hip, W16 mode) launches on that tile; anything else - another epilogue, the LayerNorm fold on either side, the second A
// operand, split-K, throughput mode - runs the tile's generic kernel.
template <int E, bool F>
struct EpiSpec {
    static constexpr int epi = E;
    static constexpr bool f16 = F;
};
template <int BM, int BN, int NST, int NWM, int NWN, int WPS, class... Specs>
static int launch_gemm_m16(const sm_gemm_args& g, bool f16, hipStream_t st) {
    if (g.mfma_terms == 1) return launch_gemm_m16_terms<BM, BN, NST, NWM, NWN, WPS, 1>(g, st);
    const bool plain = !g.ln_stats && !g.C2 && !g.ln_stats_out && !(g.alt_from_n > 0) && !(g.split_k > 1);
    if (plain) {
        int rc = SM_OK;
        const bool done = (... || (Specs::epi == g.epilogue && Specs::f16 == f16
                                       ? (rc = launch_gemm_m16_terms<BM, BN, NST, NWM, NWN, WPS, 3, Specs::epi, Specs::f16, true>(g, st), true)
                                       : false));
        if (done) return rc;
    }
    return launch_gemm_m16_terms<BM, BN, NST, NWM, NWN, WPS, 3>(g, st);
}

// fp32 weights (rows, K) -> W16: per group of 8 k, 16 B of wh = f16(w * scale) then 16 B of wl = f16(w * scale - wh)
__global__ __launch_bounds__(256) void split_w16_kernel(const float* __restrict__ src, int64_t lds_, float* __restrict__ dst,
                                                        int64_t ldd, int K, int64_t total_groups, float scale) {
    const int gpr = K / 8;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total_groups; t += (int64_t)gridDim.x * 256) {
        const int64_t row = t / gpr;
        const int gidx = (int)(t - row * gpr);
        const float4 a = *reinterpret_cast<const float4*>(src + row * lds_ + gidx * 8);
        const float4 b = *reinterpret_cast<const float4*>(src + row * lds_ + gidx * 8 + 4);
        const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        f16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = x[e] * scale;  // exact: scale is a power of two
            _Float16 hh;
            float hf;
            asm volatile("v_cvt_f16_f32 %0, %1" : "=v"(hh) : "v"(v));
            asm volatile("v_cvt_f32_f16 %0, %1" : "=v"(hf) : "v"(hh));
            hi[e] = hh;
            lo[e] = (_Float16)(v - hf);
        }
        char* p = reinterpret_cast<char*>(dst + row * ldd) + gidx * 32;
        *reinterpret_cast<f16x8*>(p) = hi;
        *reinterpret_cast<f16x8*>(p + 16) = lo;
    }
}

}  // namespace sm

extern "C" int sm_split_w16(const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int64_t rows, int32_t K, float scale,
                            void* stream) {
    SM_REQUIRE(src && dst && rows > 0 && K > 0 && K % 8 == 0 && ld_src % 4 == 0 && ld_dst % 4 == 0 && ld_src >= K &&
                   ld_dst >= K,
               "sm_split_w16: bad arguments (K %% 8 == 0, strides %% 4 == 0)");
    int ex = 0;
    SM_REQUIRE(scale > 0.f && frexpf(scale, &ex) == 0.5f, "sm_split_w16: scale must be a power of two");
    const int64_t groups = rows * (K / 8);
    int64_t grid = (groups + 255) / 256;
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(sm::split_w16_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, src, ld_src, dst, ld_dst, K,
                       groups, scale);
    return sm::check_launch("sm_split_w16");
}

extern "C" int sm_gemm_w16_tile(const sm_gemm_args* g, int out_f16x2, int variant, void* stream) {
    SM_REQUIRE(g && g->A && g->W && g->C, "sm_gemm_w16: null pointer");
    SM_REQUIRE(g->M > 0 && g->N > 0 && g->K > 0 && g->K % 32 == 0 && g->batch <= 1, "sm_gemm_w16: bad shape (K %% 32, batch 1)");
    SM_REQUIRE(g->N % 4 == 0 && g->ldc % 4 == 0 && ((uintptr_t)g->C % 16 == 0), "sm_gemm_w16: N, ldc must be multiples of 4");
    SM_REQUIRE(g->lda % 8 == 0 && g->ldw % 8 == 0 && ((uintptr_t)g->A % 16 == 0) && ((uintptr_t)g->W % 16 == 0),
               "sm_gemm_w16: lda/ldw must be multiples of 8, pointers 16-B aligned");
    SM_REQUIRE(g->epilogue == SM_EPI_BIAS || g->epilogue == SM_EPI_GELU || g->epilogue == SM_EPI_RELU ||
                   g->epilogue == SM_EPI_RESIDUAL || g->epilogue == SM_EPI_PATCH, "sm_gemm_w16: unsupported epilogue");
    int ex = 0;
    SM_REQUIRE(g->w_scale > 0.f && frexpf(g->w_scale, &ex) == 0.5f, "sm_gemm_w16: w_scale must be the weight tensor's 2^-s");
    SM_REQUIRE((uint64_t)g->M * (uint64_t)g->lda * 4 < (1ull << 32) && (uint64_t)g->N * (uint64_t)g->ldw * 4 < (1ull << 32),
               "sm_gemm_w16: operands beyond 4 GiB (the ring's source addresses are 32-bit offsets from A / W)");
    if (g->ln_stats || g->ln_stats_out || g->C2) {
        SM_REQUIRE(variant >= 40 && variant < 50 && (variant != 43 || !(g->ln_stats_out || g->C2)), "sm_gemm_w16: the LayerNorm fold needs the 16x16x32 kernels with 32-column wave tiles");
        if (g->ln_stats)
            SM_REQUIRE(g->K == SM_EMBED && g->ln_c && ((uintptr_t)g->ln_c % 16) == 0 && ((uintptr_t)g->ln_stats % 16) == 0 && g->ln_eps > 0.f &&
                           g->epilogue != SM_EPI_RESIDUAL && g->epilogue != SM_EPI_PATCH && !(g->split_k > 1) && g->alt_from_n == 0,
                       "sm_gemm_w16: folded LayerNorm needs K = 384, ln_c (16-B aligned), ln_eps and a BIAS / GELU / RELU epilogue");
        if (g->ln_stats_out || g->C2)
            SM_REQUIRE(g->epilogue == SM_EPI_RESIDUAL && g->N == SM_EMBED && g->ldc % 8 == 0 && !(g->split_k > 1) &&
                           (!g->C2 || ((uintptr_t)g->C2 % 32) == 0) && (!g->ln_stats_out || ((uintptr_t)g->ln_stats_out % 8) == 0),
                       "sm_gemm_w16: the F16X2 copy / row statistics come from a RESIDUAL epilogue with N = 384");
    }
    SM_REQUIRE(sm_gemm_w16_variant_name(variant) != nullptr, "sm_gemm_w16_tile: unknown variant %d (40, 42, 43, 44, 45, 47)", variant);
    SM_REQUIRE(g->mfma_terms == 0 || g->mfma_terms == 3 || g->mfma_terms == 1,
               "sm_gemm_w16: mfma_terms must be 0/3 (fp32-grade) or 1 (throughput mode)");
    if (out_f16x2)
        SM_REQUIRE(g->N % 8 == 0 && g->ldc % 8 == 0 && (g->epilogue == SM_EPI_BIAS || g->epilogue == SM_EPI_GELU ||
                                                      g->epilogue == SM_EPI_RELU) && !(g->split_k > 1),
                   "sm_gemm_w16: F16X2 output needs N %% 8 == 0 and a BIAS/GELU/RELU epilogue");
    if (g->epilogue == SM_EPI_RESIDUAL) SM_REQUIRE(g->R && g->ldr % 4 == 0, "sm_gemm_w16: residual needs R, ldr %% 4 == 0");
    if (g->epilogue == SM_EPI_PATCH) SM_REQUIRE(g->R && g->patch_n > 0, "sm_gemm_w16: PATCH needs R/patch_n");
    if (g->alt_from_n > 0) SM_REQUIRE(g->A_alt && g->alt_from_n % 256 == 0, "sm_gemm_w16: bad A_alt (multiple of 256)");
    if (g->split_k > 1)
        SM_REQUIRE(g->epilogue == SM_EPI_BIAS && !g->bias && (g->K / 32) % g->split_k == 0, "sm_gemm_w16: bad split_k");
    sm_gemm_args a = *g;
    if (out_f16x2) a.patch_n = -1;
    hipStream_t st = (hipStream_t)stream;
    const bool f = out_f16x2 != 0;
    using sm::EpiSpec;
    using GeluS = EpiSpec<SM_EPI_GELU, true>;          // fc1
    using BiasS = EpiSpec<SM_EPI_BIAS, true>;          // all-layer K/V, qkv, decoder projections, the head's last layer
    using ReluS = EpiSpec<SM_EPI_RELU, true>;          // decoder linear1, the head
    using Relu = EpiSpec<SM_EPI_RELU, false>;          // the head's middle layer when its output leaves as fp32
    using Resid = EpiSpec<SM_EPI_RESIDUAL, false>;     // proj, fc2, decoder output projections, linear2
    using Patch = EpiSpec<SM_EPI_PATCH, false>;        // patch embedding
    switch (variant) {
        case 40: return sm::launch_gemm_m16<256, 256, 2, 2, 8, 4, GeluS, BiasS>(a, f, st);   // 16 waves of 128x32 (fc1, all-layer K/V)
        case 42: return sm::launch_gemm_m16<128, 128, 2, 2, 4, 4>(a, f, st);   // 8 waves of 64x32
        case 43: return sm::launch_gemm_m16<256, 192, 2, 4, 4, 4>(a, f, st);   // 16 waves of 64x48: N = 1536 / 4608 in 400 / 1200 tiles
        case 44: return sm::launch_gemm_m16<64, 64, 3, 2, 2, 3, BiasS, ReluS, Relu, Resid>(a, f, st);  // 4 waves of 32x32 (decoder, batch 1)
        case 45: return sm::launch_gemm_m16<128, 64, 2, 2, 2, 3>(a, f, st);    // 4 waves of 64x32
        case 47: return sm::launch_gemm_m16<256, 128, 3, 4, 4, 4, Resid, Patch, BiasS, GeluS>(a, f, st);  // 16 waves of 64x32, ring of three (proj, fc2, qkv, patch)
    }
    sm::set_error("sm_gemm_w16_tile: unknown variant %d", variant);
    return SM_EINVAL;
}

extern "C" const char* sm_gemm_w16_variant_name(int variant) {
    switch (variant) {
        case 40: return "gemm_w16m16_kernel<256, 256, 2, 2, 8, 4, 3>";
        case 42: return "gemm_w16m16_kernel<128, 128, 2, 2, 4, 4, 3>";
        case 43: return "gemm_w16m16_kernel<256, 192, 2, 4, 4, 4, 3>";
        case 44: return "gemm_w16m16_kernel<64, 64, 3, 2, 2, 3, 3>";
        case 45: return "gemm_w16m16_kernel<128, 64, 2, 2, 2, 3, 3>";
        case 47: return "gemm_w16m16_kernel<256, 128, 3, 4, 4, 4, 3>";
    }
    return nullptr;
}

// Tile choice.  Alone on the GPU every shape from 128 x 64 to 256 x 256 lands within a few per cent of the others
// (scripts/gemm_w16_sweep.py; 128 x 64 is even the fastest for N = 384 because it fills the CUs best).  What ships is
// decided by the quantity the bench measures - three batches in flight, the chip at its power limit (1.9 GHz), other
// streams' kernels filling every idle CU: there the shapes that stage the fewest bytes per MFMA win (profiles/
// r02_pipeline_variant_sweep.log): 256 x 256 tiles (one workgroup of 16 waves per CU) for outputs that are a multiple of
// 256 wide, 256 x 128 with a three-stage ring otherwise - +3...6 % images/s over 128 x 128 / 128 x 64 although a lone
// launch is no faster.  Small problems (decoder, batch 1) keep 128 x 128 / 128 x 64 / 64 x 64 by workgroup count.
extern "C" int sm_gemm_w16_pick(const sm_gemm_args* g) {
    if (!g) return -1;
#ifdef SM_TUNING  // tuning knobs (same results): force a variant for the wide (N > 384) / narrow GEMMs
    static const int forced_w = getenv("SM_W16_VARIANT_WIDE") ? atoi(getenv("SM_W16_VARIANT_WIDE")) : -1;
    static const int forced_n = getenv("SM_W16_VARIANT_NARROW") ? atoi(getenv("SM_W16_VARIANT_NARROW")) : -1;
#else
    constexpr int forced_w = -1, forced_n = -1;
#endif
    const long nb = g->split_k > 1 ? g->split_k : 1;
    const long wg128x64 = (long)((g->M + 127) / 128) * ((g->N + 63) / 64) * nb;
    const long wg128 = (long)((g->M + 127) / 128) * ((g->N + 127) / 128) * nb;
    const long wg256x128 = (long)((g->M + 255) / 256) * ((g->N + 127) / 128) * nb;
    const long wg256 = (long)((g->M + 255) / 256) * ((g->N + 255) / 256) * nb;
    // (Small launches are latency chains - a 64 x 64 tile walks 12 K-tiles behind a ring of three - but a ring of six, five stages in
    // flight before the first MFMA, is SLOWER: the batch-1 forward 1.209 -> 1.256 ms, serving p50 1.20 -> 1.25 ms: issuing 80 KiB of
    // LDS-DMA per workgroup up front costs more address-unit time than the waits it removes.  profiles/r04_deep_ring_ab.log.)
    if (wg128x64 < 512) return 44;
    const bool narrow = g->N <= 384;
    if (narrow && forced_n >= 0) return forced_n;
    if (!narrow && forced_w >= 0) return forced_w;
    if (g->alt_from_n == 0 || g->alt_from_n % 256 == 0) {
        // (256 x 192, variant 43: fc1 in 400 tiles = 1.56 rounds of 0.75-size tiles instead of 1.17 rounds in 2.  Measured, three
        // alternations, profiles/r04_tile_256x192_ab.log: the lone launch 79.9 -> 70.7 us (0.086 -> 0.097 of the f16 roof), ONE stream
        // 16.1 k -> 16.7 k images/s (+3.8 %), the three-stream pipeline the metric is quoted on 22.43 k -> 22.20 k (-1.0 %: 17 % more
        // staged bytes per MFMA).  The pick follows the pipeline; sm_gemm_w16_tile selects 43.)
        if (g->N % 256 == 0 && g->N >= 1024 && wg256 >= 128) return 40;  // 256 x 256
        if (wg256x128 >= 128) return 47;                                  // 256 x 128, ring of three, 16 waves
    }
    if (wg128 >= 256) return 42;
    return 45;
}

extern "C" int sm_gemm_w16(const sm_gemm_args* g, int out_f16x2, void* stream) {
    const int v = sm_gemm_w16_pick(g);
    if (v < 0) { sm::set_error("sm_gemm_w16: null arguments"); return SM_EINVAL; }
    return sm_gemm_w16_tile(g, out_f16x2, v, stream);
}

#ifdef SM_TUNING
extern "C" int sm_gemm_stamp_filter(int N, int K, int M) {
    const int f[3] = {N, K, M};
    return hipMemcpyToSymbol(HIP_SYMBOL(sm::g_gemm_stamp_filter), f, sizeof(f)) == hipSuccess ? 0 : 1;
}
extern "C" int sm_gemm_stamps(unsigned long long* host_out, int count) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(sm::g_gemm_stamps), sizeof(unsigned long long) * count) == hipSuccess ? 0 : 1;
}
#endif
