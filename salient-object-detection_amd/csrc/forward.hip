// MaskFormer.forward (maskformer.py:164-251; return_intermediate=True, use_binary_classifier=True) as one
// stream-ordered sequence of the kernels of this library.  No allocation, no synchronisation: the caller owns the
// workspace and the stream, so the whole forward can be captured into a hipGraph.
//
// Four GEMM back ends behind sm_weights.gemm_mode:
//   0  exact-fp32 MFMA (gemm.hip): every buffer fp32;
//   1  split-operand f16 MFMA (gemm_f16x2.hip, fp32-grade, ~2.2x faster): every tensor that only feeds a GEMM is
//      produced directly in the F16X2 format by its producer (LayerNorm, attention, GELU/ReLU epilogues, im2col,
//      up-sample); tensors that are also residuals / outputs exist in fp32 as well.  "(S)" marks them below.
//   2  W16 (gemm_w16.hip, the default): activations as in mode 1, the weights in the W16 format with a per-tensor 2^-s, so every
//      weight GEMM sums in one fp32 accumulator; products of two activations (the mask einsum) stay on the mode-1 kernel.  Only
//      this mode and mode 3 have the fused QKV + attention kernel, the folded pre-norms and the encoder's split-K fc2;
//   3  the W16 kernels with ONE f16 MFMA per product instead of three (sm_gemm_args.mfma_terms = 1): the throughput-mode
//      diagnostic, two orders of magnitude outside the 1e-4 logit gate - never the metric, and without attention maps.
#include "common.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <utility>
#include <vector>

namespace sm {

// ---- timing taps (sm_forward_timing): event pairs around the heavy launches, on the launch sequence's stream ----------
struct Tap {
    hipStream_t st;
    hipEvent_t e0, e1;
    std::string name;
    double flops, bytes;
};
static bool g_timing = false;
static std::vector<Tap> g_taps;

// begin returns a handle (-1 when timing is off: nothing is created or recorded then); TapGuard (common.h) pairs the two
int tap_begin(void* stream, const char* name, double flops, double bytes) {
    if (!g_timing) return -1;
    Tap t;
    t.st = (hipStream_t)stream; t.name = name; t.flops = flops; t.bytes = bytes;
    if (hipEventCreate(&t.e0) != hipSuccess || hipEventCreate(&t.e1) != hipSuccess) return -1;
    (void)hipEventRecord(t.e0, t.st);
    g_taps.push_back(t);
    return (int)g_taps.size() - 1;
}
void tap_end(int handle) {
    if (handle >= 0 && handle < (int)g_taps.size()) (void)hipEventRecord(g_taps[handle].e1, g_taps[handle].st);
}

// Forwards this small (batch 1-2 at 224^2: serving) run the encoder's fc2 - K = 1536 on M/64 x 6 workgroups, a 48-step serial K
// loop of ~20 us - split four ways along K; the LayerNorm launch that follows sums the slices (as the decoder's does).  Only on
// the automatic path (sm_forward_io.attn_path = 0): the Evaluator pins a path so that rows do not depend on the batch size.
// And only below 16 images: from there on the automatic path IS the large-batch kernel set, to the bit (the "fused" pin) - a
// caller who pins for a ragged last batch gets what the full batches gave.  (The split would be 0.10 ms of 1.1 - 1.8 ms faster at
// 16 - 100 images of 32^2 - 80^2 pixels, profiles/auto_vs_fused_pin_small_grids.log: given up for that equality.)
static const int64_t SM_SPLIT_FC2_ROWS = 512;

struct Shape {
    int B, H, W, P, gh, gw, n, N, L, nq, sf, KVW;  // sf: the pixel decoder's scale_factor (2 as shipped); KVW: row width of ws.KV
    int64_t M, Mp, Md, Mo;  // tokens, patch tokens, decoder rows, objectness rows
};

static Shape make_shape(const sm_weights* w, int B, int H, int W) {
    Shape s;
    s.B = B; s.H = H; s.W = W; s.P = w->patch;
    s.gh = (H + s.P - 1) / s.P; s.gw = (W + s.P - 1) / s.P;
    s.n = s.gh * s.gw; s.N = s.n + 1; s.L = w->n_dec_layers; s.nq = w->n_queries;
    s.sf = w->scale_factor > 0 ? w->scale_factor : 2;
    s.KVW = s.L * 2 * SM_EMBED;
    s.M = (int64_t)B * s.N; s.Mp = (int64_t)B * s.n; s.Md = (int64_t)B * s.nq; s.Mo = s.Md * s.L;
    return s;
}

// workspace carve-up (floats, every region 256-B aligned)
struct Ws {
    float *pos, *X, *Xn, *QKV, *AO, *HID, *TOK, *TOKs, *KV, *UP, *TGT, *TGTs, *TGTQ, *T2, *QK, *Qc, *AOd, *HIDd, *PART, *QD,
        *QDs, *LOG, *O1, *O2, *ST;
    size_t total;
};

static Ws carve(const Shape& s, float* base) {
    Ws w;
    size_t off = 0;
    auto take = [&](size_t nfloat) {
        float* p = base ? base + off : nullptr;
        off += (nfloat + 63) & ~(size_t)63;
        return p;
    };
    const size_t D = SM_EMBED;
    w.pos = take((size_t)s.N * D);
    w.X = take(s.M * D);
    w.Xn = take(s.M * D);               // (S)
    w.QKV = take(s.M * 3 * D);
    w.AO = take(s.M * D);               // (S)
    // HID (S) doubles as the im2col buffer (S) (consumed by the patch GEMM before fc1 first writes HID)
    size_t hid = s.M * SM_MLP, cols = (size_t)s.Mp * 3 * s.P * s.P;
    w.HID = take(hid > cols ? hid : cols);
    w.TOK = take(s.Mp * D);
    w.TOKs = take(s.Mp * D);            // F16X2 copy of TOK (A operand of the all-layer K/V GEMM)
    w.KV = take(s.Mp * 2 * D * s.L);    // cross-attention K|V of ALL decoder layers: (B*n, L*768)
    w.UP = take(s.Mp * s.sf * s.sf * D);  // (S)
    w.TGT = take(s.Md * D);
    w.TGTs = take(s.Md * D);            // F16X2 copy of TGT
    w.TGTQ = take(s.Md * D);            // (S) tgt + query_pos
    w.T2 = take(s.Md * D);
    w.QK = take(s.Md * 3 * D);
    w.Qc = take(s.Md * D);
    w.AOd = take(s.Md * D);             // (S)
    w.HIDd = take(s.Md * SM_MLP);       // (S)
    // split-K partials: the decoder's linear2, and the encoder's fc2 on forwards of at most SM_SPLIT_FC2_ROWS token rows
    w.PART = take((s.M <= SM_SPLIT_FC2_ROWS && s.M > s.Md ? s.M : s.Md) * D * 4);
    w.QD = take(s.Mo * D);
    w.QDs = take(s.Mo * D);             // F16X2 copy of QD
    w.LOG = take(s.Mo * s.sf * s.sf * s.n);
    w.O1 = take(s.Mo * D);              // (S)
    w.O2 = take(s.Mo * D);
    w.ST = take(s.M * 24);              // folded LayerNorm: (mean, M2) of the twelve 32-column segments of every token row
    w.total = off * sizeof(float);
    return w;
}

#define TRY(x)                \
    do {                      \
        int _rc = (x);        \
        if (_rc) return _rc;  \
    } while (0)

struct Ctx {
    bool S;    // split-operand GEMM mode (activations that only feed GEMMs are F16X2)
    bool W16;  // ... with the weights in the W16 format: weight GEMMs run the single-accumulator kernel (gemm_w16.hip)
    hipStream_t st;
    int terms;  // MFMAs per product in the W16 kernels: 3 (fp32-grade) or 1 (gemm_mode 3: the throughput-mode diagnostic)
};

// ---- launchers: the tap and the mode dispatch; their arguments are the ABI structs themselves -------------------------
// C = epilogue(A W^T + b).  `ws` = the weight tensor's 2^-s (W16 mode; 0 = W is not a W16 weight: an activation operand, or another
// mode).  Call sites set the optional fields (the LayerNorm fold, A_alt, split_k) under their sm_gemm_args names.
static sm_gemm_args linear_args(const float* A, int lda, const float* W, float ws, const float* b, float* C, int ldc, int64_t M,
                                int N, int K, int epi, const float* R = nullptr, int ldr = 0) {
    sm_gemm_args g = {};
    g.A = A; g.W = W; g.bias = b; g.C = C; g.R = R;
    g.M = (int)M; g.N = N; g.K = K; g.lda = lda; g.ldw = K; g.ldc = ldc; g.ldr = ldr;
    g.batch = 1; g.epilogue = epi; g.w_scale = ws;
    return g;
}
static bool use_w16(const Ctx& c, const sm_gemm_args& g) { return c.W16 && g.w_scale > 0.f; }
static bool pow2(float s) {
    int ex = 0;
    return s > 0.f && frexpf(s, &ex) == 0.5f;
}
static std::string gemm_name(const Ctx& c, const sm_gemm_args& g) {
    if (!g_timing) return std::string();
    char buf[64];
    int bm = 0, bn = 0, nst = 0;
    if (use_w16(c, g)) {
        const char* nm = sm_gemm_w16_variant_name(sm_gemm_w16_pick(&g));
        std::string s = nm ? nm : "gemm_w16_kernel<?>";
        if (c.terms == 1 && s.size() > 3 && s.compare(s.size() - 3, 3, " 3>") == 0) s.replace(s.size() - 2, 1, "1");  // the TERMS template argument
        return s;
    }
    if (c.S) {
        sm_gemm_f16x2_pick_tile(&g, &bm, &bn, &nst);
        snprintf(buf, sizeof buf, "gemm_f16x2_kernel<%d, %d, %d, 2, %d, %d, 0>", bm, bn, nst, bn == 128 ? 4 : 2, bn == 128 ? 2 : 3);
    } else {
        sm_gemm_f32_pick_tile(&g, &bm, &bn);
        snprintf(buf, sizeof buf, "gemm_f32_kernel<%d, %d, %d>", bm, bn, bm == 128 ? (bn == 128 ? 2 : 3) : 4);
    }
    return buf;
}
// in split mode A and W are F16X2 / W16 and `out_s` asks for an F16X2 C
static int gemm(const Ctx& c, const sm_gemm_args& g, bool out_s = false) {
    TapGuard tap(c.st, gemm_name(c, g).c_str(), 2.0 * g.M * g.N * g.K * (g.batch > 0 ? g.batch : 1), 0.0);
    if (use_w16(c, g)) {
        sm_gemm_args gt = g;
        gt.mfma_terms = c.terms;
        return sm_gemm_w16(&gt, out_s ? 1 : 0, c.st);
    }
    return c.S ? sm_gemm_f16x2(&g, out_s ? 1 : 0, c.st) : sm_gemm_f32(&g, c.st);
}
// in split mode Q, K and V are F16X2 (written so by the projection GEMMs) and the f16 matrix cores do the work
static int attn(const Ctx& c, sm_attn_args a) {
    TapGuard tap(c.st, c.S ? "attention_f16x2_kernel<4, false>" : "attention_f32_kernel", 4.0 * a.batch * a.heads * a.n_q * (double)a.n_k * SM_HEAD_DIM,
                 8.0 * a.batch * a.heads * SM_HEAD_DIM * ((double)a.n_q + a.n_k));  // Q, O and K, V once, 4 B per element
    a.out_f16x2 = c.S;
    return c.S ? sm_attention_f16x2(&a, c.st) : sm_attention_f32(&a, c.st);
}
// LayerNorm of packed 384-float rows, identity row maps; call sites set the optional fields under their sm_ln_args names
static sm_ln_args ln_args(const float* x, const float* gamma, const float* beta, float* y, int64_t rows, float eps) {
    sm_ln_args a = {};
    a.x = x; a.gamma = gamma; a.beta = beta; a.y = y; a.rows = (int)rows; a.eps = eps;
    a.ldx = a.ldy = a.ldy2 = a.chain_ldy = SM_EMBED;
    return a;
}
static int ln(const Ctx& c, const sm_ln_args& a) {
    TapGuard tap(c.st, "layernorm384_kernel", 0.0, 2.0 * a.rows * SM_EMBED * 4);
    return sm_layernorm_rows_f32(&a, c.st);
}

// ---- the blocks that repeat -------------------------------------------------------------------------------------------
// self-attention over a packed (B * n, 1152) buffer: Q | K | V are its column thirds, n tokens per image
static sm_attn_args self_attn_args(const float* qkv, int B, int n, float* O) {
    const int D = SM_EMBED;
    sm_attn_args a = {};
    a.Q = qkv; a.K = qkv + D; a.V = qkv + 2 * D; a.O = O;
    a.sQb = a.sKb = a.sVb = (int64_t)n * 3 * D; a.sQr = a.sKr = a.sVr = 3 * D;
    a.sOb = (int64_t)n * D; a.sOr = D;
    a.batch = B; a.heads = SM_HEADS; a.n_q = n; a.n_k = n; a.scale = 0.125f;
    return a;
}
// K = 1536 products with only M/64 x 6 output tiles (encoder fc2, decoder linear2), split 4-way along K: the GEMM writes four raw
// slices into PART, the LayerNorm launch that follows sums them in slice order with the bias and the residual
static sm_gemm_args split_k4_args(const float* A, const float* W, float ws, float* PART, int64_t M) {
    sm_gemm_args g = linear_args(A, SM_MLP, W, ws, nullptr, PART, SM_EMBED, M, SM_EMBED, SM_MLP, SM_EPI_BIAS);
    g.split_k = 4; g.strideC = M * SM_EMBED;
    return g;
}
static sm_ln_args split_k4_ln_args(const float* PART, const float* bias, const float* residual, const float* gamma, const float* beta,
                                   float* y, int64_t M, float eps) {
    sm_ln_args a = ln_args(PART, gamma, beta, y, M, eps);
    a.n_partials = 4; a.partial_stride = M * SM_EMBED; a.pre_bias = bias; a.residual = residual;
    return a;
}

// decoder start state in one launch: tgt = 0 (fp32 and F16X2 - zero bytes in both), tgt + query_pos = query_pos broadcast
// over the batch (fp32, or F16X2 in split mode).  A kernel rather than hipMemsetAsync: memset nodes in a captured
// hipGraph misbehaved on replay (graphs.py), and it saves three launches.
template <bool SPLIT>
__global__ __launch_bounds__(256) void decoder_init_kernel(const float* __restrict__ qpos, float* __restrict__ tgt,
                                                          float* __restrict__ tgts, float* __restrict__ tgtq, int rows_per,
                                                          int64_t total4) {
    const int64_t per4 = (int64_t)rows_per * (SM_EMBED / 4);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total4; t += (int64_t)gridDim.x * 256) {
        reinterpret_cast<float4*>(tgt)[t] = z;
        reinterpret_cast<float4*>(tgts)[t] = z;
        const float4 q = reinterpret_cast<const float4*>(qpos)[t % per4];
        if constexpr (SPLIT) {
            const int64_t e = t * 4, row = e / SM_EMBED;
            const float v[4] = {q.x, q.y, q.z, q.w};
            store_f16x2_4(tgtq + row * SM_EMBED, e - row * SM_EMBED, v);
        } else {
            reinterpret_cast<float4*>(tgtq)[t] = q;
        }
    }
}

// ---- one forward: what its stages share, and the stages ---------------------------------------------------------------
namespace {
struct Fwd {
    static constexpr int D = SM_EMBED;
    const sm_weights* w;
    const sm_forward_io* io;
    const sm_encoder_taps* tp;  // encoder taps, or NULL: then every launch below is the plain forward's
    Shape s;
    Ws ws;
    Ctx c;
    float* tok;          // final-normed patch tokens (the caller's buffer when it asks for them) ...
    const float* tok_a;  // ... and their GEMM-operand view
    float* QD;           // normed decoder outputs of every layer, (B, L, nq, 384) (the caller's buffer when it asks for them) ...
    const float* qd_a;   // ... and their GEMM-operand view

    int tokens() const;
    int encoder() const;  // returns inside block 12 when io->attn_only, after the last requested tap when tp->stop
    int block_attention(int i, const sm_gemm_args& qkv) const;
    // encoder taps (sm_encoder_taps): launches that only read
    int tap_rows(const float* src, float* dst, int slot, int slots, bool norm) const;
    int tap_input_tokens() const;
    int decoder() const;
    int heads() const;
    // the steps of a decoder layer (transformer_decoder.py:260-327); `tgt` is the fp32 residual stream
    // a norm also writes tgt + query_pos (with_pos_embed): the q = k operand of self-attention, the query operand of cross-attention
    void also_plus_query_pos(sm_ln_args& a) const { a.y2 = ws.TGTQ; a.y2_f16x2 = c.S ? 1 : 0; a.add = w->query_embed; a.add_rows = s.nq; }
    int self_attention_block(const sm_dec_layer& d, const float* value, const float* tgt, float* out) const;
    int cross_attention_block(const sm_dec_layer& d, int l, const float* tgt, float* out) const;
    int decoder_layer_pre(int l) const;
    int decoder_layer_post(int l, float* tgt, float* t2) const;
    sm_row_map layer_rows(int l) const { return {s.nq, s.L * s.nq, l * s.nq}; }  // rows of decoder layer l in the (B, L, nq, 384) stack
    int ffn01(const float* A, bool out_s) const;
};

// ---- tokens: patch embedding + cls + position (vision_transformer.py:269-281) ----------------------------
int Fwd::tokens() const {
    const float* pos = w->pos_embed;
    if (s.n != w->pos_grid * w->pos_grid) {  // interpolate_pos_encoding compares token COUNTS (:386-388)
        TRY(sm_pos_embed_bicubic_f32(w->pos_embed, w->pos_grid, ws.pos, s.gh, s.gw, c.st));
        pos = ws.pos;
    }
    float* cols = ws.HID;
    TRY(c.S ? sm_im2col_patches_f16x2(io->x, cols, s.B, s.H, s.W, s.P, c.st)
            : sm_im2col_patches_f32(io->x, cols, s.B, s.H, s.W, s.P, c.st));
    TRY(sm_cls_rows_f32(w->cls_token, pos, ws.X, s.B, s.N, c.st));
    const int K = 3 * s.P * s.P;
    sm_gemm_args g = linear_args(cols, K, w->patch_w, w->patch_s, w->patch_b, ws.X, D, s.Mp, D, K, SM_EPI_PATCH, pos, D);
    g.patch_n = s.n;
    TRY(gemm(c, g));
    if (tp && tp->post_pe) TRY(tap_rows(ws.X, tp->post_pe, 0, 1, false));
    if (tp && tp->input_tokens) TRY(tap_input_tokens());
    return SM_OK;
}

// Rows `select` picks of src (B, N, 384) - the stream where it lies - into slot `slot` of a (B, slots, R, 384) stack, through the
// final norm or as they are
int Fwd::tap_rows(const float* src, float* dst, int slot, int slots, bool norm) const {
    EncoderTapRows a = {};
    a.row0 = tp->select == SM_TAP_PATCH ? 1 : 0;
    a.R = tp->select == SM_TAP_ALL ? s.N : tp->select == SM_TAP_CLS ? 1 : s.n;
    a.src = src; a.dst = dst + (int64_t)slot * a.R * D; a.dst_image = (int64_t)slots * a.R * D;
    a.B = s.B; a.N = s.N; a.eps = 1e-6f;
    if (norm) { a.gamma = w->enc_norm_w; a.beta = w->enc_norm_b; }
    return encoder_tap_rows(a, c.st);
}

// cat(cls_token, patch_embed(x)) before the position embedding (get_tokens(input_tokens=True), vision_transformer.py:329-336): the
// patch epilogue once more over the im2col columns still in ws.HID, with a zeroed position table (the head of ws.QKV) and ws.Xn
// as the destination - both free until block 1's norm1 - so ws.X is not disturbed; then the selected rows to the caller
int Fwd::tap_input_tokens() const {
    float *zero = ws.QKV, *T = ws.Xn;
    TRY(encoder_tap_zero(zero, (int64_t)s.N * D, c.st));
    TRY(sm_cls_rows_f32(w->cls_token, zero, T, s.B, s.N, c.st));
    const int K = 3 * s.P * s.P;
    sm_gemm_args g = linear_args(ws.HID, K, w->patch_w, w->patch_s, w->patch_b, T, D, s.Mp, D, K, SM_EPI_PATCH, zero, D);
    g.patch_n = s.n;
    TRY(gemm(c, g));
    return tap_rows(T, tp->input_tokens, 0, 1, false);
}

// Block i + 1's attention matrix (sm_forward_io.last_attn / last_attn_cls for block 12, vision_transformer.py:307-314;
// sm_encoder_taps.attn / attn_cls for any block, :433-439): Q|K of the block - rows [0, 768) of its qkv weight, a prefix of the same
// tensor in every weight format, with the same fold arguments - into ws.QKV as (M, 768), then the probabilities kernel once per
// requested output.  `qkv` is the block's own qkv projection.
int Fwd::block_attention(int i, const sm_gemm_args& qkv) const {
    float* QK = ws.QKV;
    sm_gemm_args g = qkv;
    g.N = g.ldc = 2 * D;
    if (c.S) {
        g.C = QK;
        TRY(gemm(c, g, true));
    } else {  // exact-fp32 mode: the projection is fp32 (into ws.HID), the kernel's operands are its F16X2 split
        g.C = ws.HID;
        TRY(gemm(c, g));
        TRY(sm_split_f16x2(ws.HID, 2 * D, QK, 2 * D, s.M, 2 * D, c.st));
    }
    sm_attn_probs_args a = {};
    a.Q = QK; a.K = QK + D;
    a.sQb = a.sKb = (int64_t)s.N * 2 * D; a.sQr = a.sKr = 2 * D;
    a.batch = s.B; a.heads = SM_HEADS; a.n_q = s.N; a.n_k = s.N; a.scale = 0.125f;
    const bool last = i + 1 == SM_ENC_DEPTH, tapped = tp && (tp->attn_mask >> i & 1u);
    const int64_t slot = tapped ? __builtin_popcount(tp->attn_mask & ((1u << i) - 1u)) : 0;  // blocks stack in ascending order
    const int64_t per_block = (int64_t)s.B * SM_HEADS * s.N;  // rows of one block's slot
    float* const dst[4] = {last ? io->last_attn : nullptr, last ? io->last_attn_cls : nullptr,
                           tapped && tp->attn ? tp->attn + slot * per_block * s.N : nullptr,
                           tapped && tp->attn_cls ? tp->attn_cls + slot * per_block : nullptr};
    for (int pass = 0; pass < 4; ++pass) {
        a.P = dst[pass];
        if (!a.P) continue;
        a.q0 = 0; a.nq = pass & 1 ? 1 : s.N;
        // both walks over the keys count: 2 x (2 nq n_k 64) per head; bytes: Q, K once + P
        TapGuard tap(c.st, "attention_probs_f16x2_kernel", 4.0 * s.B * SM_HEADS * a.nq * (double)s.N * SM_HEAD_DIM,
                     4.0 * s.B * SM_HEADS * (SM_HEAD_DIM * ((double)a.nq + s.N) + (double)a.nq * s.N));
        TRY(sm_attention_probs_f16x2(&a, c.st));
    }
    return SM_OK;
}

// ---- 12 pre-norm blocks (vision_transformer.py:164-170), then the final norm ------------------------------------
int Fwd::encoder() const {
    const bool S = c.S;
    // (Split mode could carry the two pre-norms of a block on the GEMM that produces their input, on the 64 x 384 full-row tile
    // of SM_EPI_RESIDUAL_LN.  Measured with three batches in flight: 17.3k images/s against 18.0k unfused - the full-row tile
    // needs 112 KiB of LDS (one workgroup per CU, 197 of them).)
#ifdef SM_TUNING
    static const int fused_qkv_env = getenv("SM_FUSED_QKV") ? atoi(getenv("SM_FUSED_QKV")) : 1;
#else
    constexpr int fused_qkv_env = 1;
#endif
    // W16 mode, token grids of <= 208 (ViT-S/16 at 224^2): the qkv projection and the attention are ONE launch
    // (qkv_attention.hip); SM_FUSED_QKV=0 (tuning build only) keeps the two-launch path (same results to rounding)
    // ... and at least 96 (image, head) workgroups: the fused kernel is one workgroup per pair with a ~30 us life, so a small batch
    // leaves most CUs idle for that long - below B = 16 the two-launch path is faster (B = 1: 1.25 vs 1.38 ms per forward, B = 4:
    // 1.40 vs 1.96, B = 8: 1.53 vs 2.10, B = 16: 1.94 vs 1.93; profiles/r03_fused_vs_unfused_by_batch.log)
    const bool fused_qkv = c.W16 && fused_qkv_env != 0 && s.N <= sm_qkv_attention_max_tokens() && io->attn_path != 2 &&
                           (io->attn_path == 1 || s.B * SM_HEADS >= 96);
    // sm_weights.ln_fold: norm2 rides on proj -> fc1 and the next block's norm1 on fc2 -> qkv: the residual epilogues also write the
    // raw stream as F16X2 (into Xn) with its row statistics, the consuming GEMM carries the gain in its weights and applies
    // r (x W'^T - mu c) + b' in its epilogue.  Block 0's norm1 (its input comes from the patch embedding) stays a launch.
    // Measured (profiles/r03_ln_fold_ab.log): the fold wins where the forward is latency-bound (B = 1: 1.24 -> 1.20 ms, B = 8: 1.45 -> 1.34)
    // and loses where it is throughput-bound (B = 64, three streams: 21.55k -> 21.3k images/s: the extra F16X2 stream of the residual
    // epilogues and the statistics cost more than 23 co-resident LayerNorm launches) - so it follows the same batch rule and the same
    // pin as the attention path (sm_forward_io.attn_path: 2 = the small-batch kernels, 1 = the large-batch ones).
    const bool lnf = c.W16 && w->ln_fold != 0 && io->attn_path != 1 && (io->attn_path == 2 || s.B * SM_HEADS < 96);
    const bool split_fc2 = c.W16 && S && io->attn_path == 0 && s.M <= SM_SPLIT_FC2_ROWS && s.B * SM_HEADS < 96;  // see SM_SPLIT_FC2_ROWS

    auto pre_norm = [&](const float* gamma, const float* beta) {  // X -> Xn; the LN output only feeds a GEMM: F16X2 in split mode
        sm_ln_args a = ln_args(ws.X, gamma, beta, S ? nullptr : ws.Xn, s.M, 1e-6f);
        a.ys = S ? ws.Xn : nullptr;
        return ln(c, a);
    };
    // taps: which blocks' outputs / attention are asked for, and with tp->stop the block the forward returns in - after its token
    // tap (stop_tok; patch_mean needs block 12's) or, when the last thing asked for is an attention, right after that (stop_attn)
    const uint32_t lmask = tp ? tp->layer_mask : 0u, amask = tp ? tp->attn_mask : 0u;
    const int n_layers = __builtin_popcount(lmask);
    int stop_tok = -1, stop_attn = -1;
    if (tp && tp->stop) {
        const int hi_tok = tp->patch_mean ? SM_ENC_DEPTH - 1 : lmask ? 31 - __builtin_clz(lmask) : -1;
        const int hi_attn = amask ? 31 - __builtin_clz(amask) : -1;
        if (hi_tok < 0 && hi_attn < 0) return SM_OK;  // only post_pe / input_tokens: written by tokens()
        if (hi_attn > hi_tok) stop_attn = hi_attn; else stop_tok = hi_tok;
    }
    for (int i = 0; i < SM_ENC_DEPTH; ++i) {
        const sm_enc_layer& e = w->enc[i];
        const bool last = i + 1 == SM_ENC_DEPTH;
        const bool n1_done = split_fc2 && i > 0;  // the previous block's split fc2 ended in this block's norm1
        const bool f1 = lnf && i > 0 && !n1_done;  // this block's norm1 is folded into its qkv projection
        if (!f1 && !n1_done) TRY(pre_norm(e.norm1_w, e.norm1_b));
        sm_gemm_args qkv = linear_args(ws.Xn, D, f1 ? e.qkv_fw : e.qkv_w, f1 ? e.qkv_fs : e.qkv_s, f1 ? e.qkv_fb : e.qkv_b, ws.QKV,
                                       3 * D, s.M, 3 * D, D, SM_EPI_BIAS);
        if (f1) { qkv.ln_stats = ws.ST; qkv.ln_c = e.qkv_c; qkv.ln_eps = 1e-6f; }
        if ((last && (io->last_attn || io->last_attn_cls)) || (amask >> i & 1u)) {
            // ws.HID is free here (the previous block's fc2 - for block 1 the patch GEMM - has consumed it), ws.QKV is rewritten by
            // this block's own projection below
            TRY(block_attention(i, qkv));
            if ((last && io->attn_only) || i == stop_attn) return SM_OK;
        }
        if (fused_qkv) {
            sm_qkv_attn_args q = {};
            q.Xn = qkv.A; q.Wqkv = qkv.W; q.bias = qkv.bias; q.O = ws.AO; q.ldx = D; q.ldo = D;
            q.B = s.B; q.N = s.N; q.w_scale = qkv.w_scale; q.scale = 0.125f; q.out_f16x2 = 1; q.mfma_terms = c.terms;
            q.ln_stats = qkv.ln_stats; q.ln_c = qkv.ln_c; q.ln_eps = qkv.ln_eps;
            // algorithmic work of SURVEY.md 8d: 2 N 384 1152 + 4 N^2 384 FLOPs, x in + o out bytes per image
            TapGuard tap(c.st, sm_qkv_attention_kernel_name(c.terms), (double)s.B * (2.0 * s.N * D * 3 * D + 4.0 * s.N * s.N * D),
                         2.0 * s.M * D * 4);
            TRY(sm_qkv_attention_w16(&q, c.st));
        } else {
            TRY(gemm(c, qkv, S));
            TRY(attn(c, self_attn_args(ws.QKV, s.B, s.N, ws.AO)));
        }
        sm_gemm_args proj = linear_args(ws.AO, D, e.proj_w, e.proj_s, e.proj_b, ws.X, D, s.M, D, D, SM_EPI_RESIDUAL, ws.X, D);
        if (lnf) { proj.C2 = ws.Xn; proj.ln_stats_out = ws.ST; }
        TRY(gemm(c, proj));
        if (!lnf) TRY(pre_norm(e.norm2_w, e.norm2_b));
        sm_gemm_args fc1 = linear_args(ws.Xn, D, lnf ? e.fc1_fw : e.fc1_w, lnf ? e.fc1_fs : e.fc1_s, lnf ? e.fc1_fb : e.fc1_b, ws.HID,
                                       SM_MLP, s.M, SM_MLP, D, SM_EPI_GELU);
        if (lnf) { fc1.ln_stats = ws.ST; fc1.ln_c = e.fc1_c; fc1.ln_eps = 1e-6f; }
        TRY(gemm(c, fc1, S));
        if (split_fc2 && !last) {
            const sm_enc_layer& nx = w->enc[i + 1];
            TRY(gemm(c, split_k4_args(ws.HID, e.fc2_w, e.fc2_s, ws.PART, s.M)));
            // x += fc2 (slices + bias + residual, written back as the stream) and the next block's norm1 of it
            sm_ln_args a = split_k4_ln_args(ws.PART, e.fc2_b, ws.X, nx.norm1_w, nx.norm1_b, nullptr, s.M, 1e-6f);
            a.ys = ws.Xn; a.raw = ws.X;
            TRY(ln(c, a));
        } else {
            sm_gemm_args fc2 = linear_args(ws.HID, SM_MLP, e.fc2_w, e.fc2_s, e.fc2_b, ws.X, D, s.M, D, SM_MLP, SM_EPI_RESIDUAL, ws.X, D);
            if (lnf && !last) { fc2.C2 = ws.Xn; fc2.ln_stats_out = ws.ST; }
            TRY(gemm(c, fc2));
        }
        // ws.X is block i + 1's output from here until the next block's proj
        if (lmask >> i & 1u) TRY(tap_rows(ws.X, tp->tokens, __builtin_popcount(lmask & ((1u << i) - 1u)), n_layers, tp->norm != 0));
        if (i == stop_tok && !tp->patch_mean) return SM_OK;  // (patch_mean stops behind the final norm below)
    }
    // final norm on the last layer only (the other 11 per-layer norms of :299 are dead work when
    // lateral_connection=False: a caller who wants them asks through sm_encoder_taps), dropping the cls row on the way
    // (maskformer.py:107-108,177)
    sm_ln_args a = ln_args(ws.X, w->enc_norm_w, w->enc_norm_b, tok, s.Mp, 1e-6f);
    a.in_map = {s.n, s.N, 1};
    a.ys = S ? ws.TOKs : nullptr;
    TRY(ln(c, a));
    // return_patch_avgpool (vision_transformer.py:466-470): the mean of exactly these rows
    if (tp && tp->patch_mean) TRY(encoder_patch_mean(tok, tp->patch_mean, s.B, s.n, c.st));
    return SM_OK;
}

// ---- decoder layers (transformer_decoder.py:260-327) -----------------------------------------------------------------
// out = tgt + self_attn(q = k = tgt + query_pos, v = `value`)  ->  the in-projection is ONE launch: columns [0,768) read TGTQ,
// [768,1152) the value operand
int Fwd::self_attention_block(const sm_dec_layer& d, const float* value, const float* tgt, float* out) const {
    sm_gemm_args g = linear_args(ws.TGTQ, D, d.sa_in_w, d.sa_in_s, d.sa_in_b, ws.QK, 3 * D, s.Md, 3 * D, D, SM_EPI_BIAS);
    g.A_alt = value; g.alt_from_n = 2 * D;
    TRY(gemm(c, g, c.S));
    TRY(attn(c, self_attn_args(ws.QK, s.B, s.nq, ws.AOd)));
    return gemm(c, linear_args(ws.AOd, D, d.sa_out_w, d.sa_out_s, d.sa_out_b, out, D, s.Md, D, D, SM_EPI_RESIDUAL, tgt, D));
}
// out = tgt + cross_attn(q = tgt + query_pos, k = v = memory (pos = None)); K | V of layer l: columns [l*768, (l+1)*768) of ws.KV
int Fwd::cross_attention_block(const sm_dec_layer& d, int l, const float* tgt, float* out) const {
    TRY(gemm(c, linear_args(ws.TGTQ, D, d.ca_in_w, d.ca_in_s, d.ca_in_b, ws.Qc, D, s.Md, D, D, SM_EPI_BIAS), c.S));
    sm_attn_args a = {};
    a.Q = ws.Qc; a.K = ws.KV + (int64_t)l * 2 * D; a.V = a.K + D; a.O = ws.AOd;
    a.sQb = (int64_t)s.nq * D; a.sQr = D; a.sKb = a.sVb = (int64_t)s.n * s.KVW; a.sKr = a.sVr = s.KVW;
    a.sOb = (int64_t)s.nq * D; a.sOr = D;
    a.batch = s.B; a.heads = SM_HEADS; a.n_q = s.nq; a.n_k = s.n; a.scale = 0.125f;
    TRY(attn(c, a));
    return gemm(c, linear_args(ws.AOd, D, d.ca_out_w, d.ca_out_s, d.ca_out_b, out, D, s.Md, D, D, SM_EPI_RESIDUAL, tgt, D));
}

// forward_pre (transformer_decoder.py:299-327): tgt2 = norm_k(tgt) feeds the sub-block, tgt += sub-block(tgt2); the
// residual stream ws.TGT (fp32) is updated in place by the RESIDUAL epilogues and never normalised in the layer
int Fwd::decoder_layer_pre(int l) const {
    const sm_dec_layer& d = w->dec[l];
    const bool S = c.S;
    float* tgt = ws.TGT;
    const float* nrm_a = S ? ws.TGTs : ws.T2;  // GEMM-operand view of the normed tgt: F16X2, or the fp32 copy (fp32 mode only)
    auto norm = [&](const float* gamma, const float* beta, bool plus_query_pos) {
        sm_ln_args a = ln_args(tgt, gamma, beta, S ? nullptr : ws.T2, s.Md, 1e-5f);
        a.ys = S ? ws.TGTs : nullptr;
        if (plus_query_pos) also_plus_query_pos(a);
        return ln(c, a);
    };
    TRY(norm(d.norm1_w, d.norm1_b, true));  // norm1 -> tgt2 (value operand) and tgt2 + query_pos (q = k operand)
    TRY(self_attention_block(d, nrm_a, tgt, tgt));
    TRY(norm(d.norm2_w, d.norm2_b, true));  // norm2 -> only tgt2 + query_pos is needed (cross-attention query; key = value = memory)
    TRY(cross_attention_block(d, l, tgt, tgt));
    TRY(norm(d.norm3_w, d.norm3_b, false));  // norm3 -> operand of linear1
    TRY(gemm(c, linear_args(nrm_a, D, d.lin1_w, d.lin1_s, d.lin1_b, ws.HIDd, SM_MLP, s.Md, SM_MLP, D, SM_EPI_RELU), S));
    TRY(gemm(c, linear_args(ws.HIDd, SM_MLP, d.lin2_w, d.lin2_s, d.lin2_b, tgt, D, s.Md, D, SM_MLP, SM_EPI_RESIDUAL, tgt, D)));
    // intermediate.append(self.norm(output)) (:138-139), scattered into (B, L, nq, 384) (+ F16X2 copy)
    sm_ln_args fin = ln_args(tgt, w->dec_norm_w, w->dec_norm_b, QD, s.Md, 1e-5f);
    fin.out_map = layer_rows(l);
    fin.ys = S ? ws.QDs : nullptr;
    return ln(c, fin);
}

// forward_post (transformer_decoder.py:260-297): tgt = norm_k(tgt + sub-block(tgt)).  The residual epilogues write the sums into
// `t2` and the norms the new tgt back into `tgt` - except norm3, which leaves the layer's output in `t2`: the caller swaps the two
int Fwd::decoder_layer_post(int l, float* tgt, float* t2) const {
    const sm_dec_layer& d = w->dec[l];
    const bool S = c.S;
    const float* tgt_a = S ? ws.TGTs : tgt;  // GEMM-operand view of tgt
    TRY(self_attention_block(d, tgt_a, tgt, t2));
    sm_ln_args n1 = ln_args(t2, d.norm1_w, d.norm1_b, tgt, s.Md, 1e-5f);  // norm1 -> tgt (fp32: residual of the next block) + tgt + query_pos (cross-attention query operand)
    also_plus_query_pos(n1);
    TRY(ln(c, n1));
    TRY(cross_attention_block(d, l, tgt, t2));
    sm_ln_args n2 = ln_args(t2, d.norm2_w, d.norm2_b, tgt, s.Md, 1e-5f);  // norm2 -> tgt (residual of the FFN) (+ F16X2 copy: operand of linear1)
    n2.ys = S ? ws.TGTs : nullptr;
    TRY(ln(c, n2));
    // FFN: linear2 (K = 1536, only M/64 x 6 tiles) is split 4-way along K; norm3 sums the slices + bias + residual
    TRY(gemm(c, linear_args(tgt_a, D, d.lin1_w, d.lin1_s, d.lin1_b, ws.HIDd, SM_MLP, s.Md, SM_MLP, D, SM_EPI_RELU), S));
    TRY(gemm(c, split_k4_args(ws.HIDd, d.lin2_w, d.lin2_s, ws.PART, s.Md)));
    // norm3(sum of slices + bias + tgt) -> new tgt (fp32 + F16X2) and tgt + query_pos
    sm_ln_args n3 = split_k4_ln_args(ws.PART, d.lin2_b, tgt, d.norm3_w, d.norm3_b, t2, s.Md, 1e-5f);
    n3.ys = S ? ws.TGTs : nullptr;
    also_plus_query_pos(n3);
    // ... and, chained in the same launch, the shared final norm on this layer's output, scattered into (B, L, nq, 384)
    // (+ F16X2 copy): transformer_decoder.py:138-139.  Six launches fewer on the critical chain of a forward (serving).
    n3.chain_gamma = w->dec_norm_w; n3.chain_beta = w->dec_norm_b; n3.chain_y = QD; n3.chain_ys = S ? ws.QDs : nullptr;
    n3.chain_map = layer_rows(l); n3.chain_eps = 1e-5f;
    return ln(c, n3);
}

// ---- 6 decoder layers, post-norm as shipped (transformer_decoder.py:112-150) -----------------------------------------
int Fwd::decoder() const {
    const int64_t total4 = s.Md * D / 4;
    const int grid = (int)((total4 + 255) / 256 < 2048 ? (total4 + 255) / 256 : 2048);
    if (c.S)
        hipLaunchKernelGGL(decoder_init_kernel<true>, dim3(grid), dim3(256), 0, c.st, w->query_embed, ws.TGT, ws.TGTs, ws.TGTQ, s.nq, total4);
    else
        hipLaunchKernelGGL(decoder_init_kernel<false>, dim3(grid), dim3(256), 0, c.st, w->query_embed, ws.TGT, ws.TGTs, ws.TGTQ, s.nq, total4);
    TRY(check_launch("decoder_init"));
    // cross-attention keys/values of every layer depend only on the encoder memory: one large GEMM
    // (B*n x 384) x (384 x L*768) instead of L small ones on the critical chain
    TRY(gemm(c, linear_args(tok_a, D, w->dec_kv_w, w->dec_kv_s, w->dec_kv_b, ws.KV, s.KVW, s.Mp, s.KVW, D, SM_EPI_BIAS), c.S));
    float *tgt = ws.TGT, *t2 = ws.T2;
    for (int l = 0; l < s.L; ++l) {
        if (w->normalize_before) {
            TRY(decoder_layer_pre(l));
        } else {
            TRY(decoder_layer_post(l, tgt, t2));
            std::swap(tgt, t2);  // norm3 wrote the new tgt into t2: TGT / T2 swap roles every layer
        }
    }
    return SM_OK;
}

// ---- heads --------------------------------------------------------------------------------------------------
// relu(ffn1(relu(ffn0(A)))) into ws.O2 (through ws.O1): the first two layers of the 3-layer MLP `ffn` (MLP.forward :265-268), shared
// by the mask head and the objectness head; `out_s`: O2 in F16X2 (it feeds another GEMM) or in fp32 (it feeds the row dot product)
int Fwd::ffn01(const float* A, bool out_s) const {
    TRY(gemm(c, linear_args(A, D, w->ffn0_w, w->ffn0_s, w->ffn0_b, ws.O1, D, s.Mo, D, D, SM_EPI_RELU), c.S));
    return gemm(c, linear_args(ws.O1, D, w->ffn1_w, w->ffn1_s, w->ffn1_b, ws.O2, D, s.Mo, D, D, SM_EPI_RELU), out_s);
}

int Fwd::heads() const {
    const bool S = c.S;
    const float* q_a = qd_a;
    TRY(sm_query_mean_f32(QD, io->features, s.B, s.L, s.nq, c.st));
    if (w->mask_head_ffn) {
        // return_intermediate=True with use_binary_classifier=False (maskformer.py:225): the mask einsum takes
        // ffn(queries), a 384->384->384->384 MLP with ReLU between the layers (MLP.forward :265-268), not the queries
        TRY(ffn01(q_a, S));
        TRY(gemm(c, linear_args(ws.O2, D, w->ffn2_w, w->ffn2_s, w->ffn2_b, ws.O1, D, s.Mo, D, D, SM_EPI_BIAS), S));
        q_a = ws.O1;
    }
    // return_intermediate=False (the 3-D path, maskformer.py:219-220): the decoder hands back its last layer only, so only that
    // layer's queries reach the mask einsum; the outputs are then (B, 1, nq, 2gh, 2gw)
    const int Lm = io->last_layer_only ? 1 : s.L;
    const float* qm_a = q_a + (io->last_layer_only ? (int64_t)(s.L - 1) * s.nq * D : 0);
    if (s.n % 4 == 0) {
        // mask_pred = sigmoid(up(Q . tok^T)): the einsum of maskformer.py:223 commutes with the bilinear x2 of the pixel
        // decoder (:144-162) - both linear - so the GEMM runs on the token grid (N = n instead of 4n) and the (B, 4n,
        // 384) up-sampled feature map is never built
        sm_gemm_args g = {};
        g.A = qm_a; g.W = tok_a; g.C = ws.LOG;
        g.M = Lm * s.nq; g.N = s.n; g.K = D; g.lda = D; g.ldw = D; g.ldc = s.n;
        g.strideA = (int64_t)s.L * s.nq * D; g.strideW = (int64_t)s.n * D; g.strideC = (int64_t)Lm * s.nq * s.n;
        g.batch = s.B; g.epilogue = SM_EPI_BIAS;
        TRY(gemm(c, g));
        TRY(sm_upsample_logits_sigmoid_f32(ws.LOG, io->mask_logits, io->mask_pred, (int64_t)s.B * Lm * s.nq, s.gh, s.gw, s.sf, c.st));
    } else {  // token counts that are not a multiple of 4 (float4 rows of the GEMM output): the literal order
        TRY(S ? sm_upsample_tokens_f16x2(tok, (int64_t)s.n * D, ws.UP, s.B, s.gh, s.gw, s.sf, c.st)
              : sm_upsample_tokens_f32(tok, (int64_t)s.n * D, ws.UP, s.B, s.gh, s.gw, s.sf, c.st));
        // mask_pred[b] = sigmoid(Q[b] (L*nq x 384) . up[b]^T (384 x 4n))   (maskformer.py:223)
        sm_gemm_args g = {};
        g.A = qm_a; g.W = ws.UP; g.C = io->mask_logits ? io->mask_logits : ws.LOG; g.C2 = io->mask_pred;
        const int up_n = s.sf * s.sf * s.n;
        g.M = Lm * s.nq; g.N = up_n; g.K = D; g.lda = D; g.ldw = D; g.ldc = up_n;
        g.strideA = (int64_t)s.L * s.nq * D; g.strideW = (int64_t)up_n * D; g.strideC = (int64_t)Lm * s.nq * up_n;
        g.batch = s.B; g.epilogue = SM_EPI_SIGMOID2;
        TRY(gemm(c, g));
    }
    if (w->mask_head_ffn || w->no_objectness) return SM_OK;  // no objectness on these paths (maskformer.py:246-249, :219-220)
    TRY(ffn01(q_a, false));
    return sm_rowdot_sigmoid_f32(ws.O2, w->ffn2_w, w->ffn2_b, io->objectness, (int)s.Mo, c.st);
}

}  // namespace

static int forward(const sm_weights* w, const sm_forward_io* io, const sm_encoder_taps* tp, float* wsbase, hipStream_t st) {
    const Shape s = make_shape(w, io->B, io->H, io->W);
    const Ws ws = carve(s, wsbase);
    const Ctx c = {w->gemm_mode >= 1, w->gemm_mode >= 2, st, w->gemm_mode == 3 ? 1 : 3};
    float* tok = io->patch_tokens ? io->patch_tokens : ws.TOK;
    float* QD = io->queries ? io->queries : ws.QD;
    const Fwd f = {w, io, tp, s, ws, c, tok, c.S ? ws.TOKs : tok, QD, c.S ? ws.QDs : QD};
    TRY(f.tokens());
    TRY(f.encoder());
    if (io->attn_only || io->encoder_only || (tp && tp->stop)) return SM_OK;  // attn_only / stop: the encoder returned early
    TRY(f.decoder());
    return f.heads();
}

static int validate(const sm_weights* w, const sm_forward_io* io, const sm_encoder_taps* tp) {
    SM_REQUIRE(w && io, "sm_maskformer_forward: null arguments");
    SM_REQUIRE(w->patch == 8 || w->patch == 16, "sm_maskformer_forward: patch=%d (8 or 16)", w->patch);
    SM_REQUIRE(w->gemm_mode >= 0 && w->gemm_mode <= 3, "sm_maskformer_forward: gemm_mode=%d (0..3)", w->gemm_mode);
    SM_REQUIRE(w->n_dec_layers >= 1 && w->n_dec_layers <= SM_MAX_DEC_LAYERS, "sm_maskformer_forward: n_dec_layers=%d",
               w->n_dec_layers);
    SM_REQUIRE(w->n_queries >= 1 && w->pos_grid >= 1, "sm_maskformer_forward: bad n_queries/pos_grid");
    SM_REQUIRE(w->scale_factor >= 0 && w->scale_factor <= 16, "sm_maskformer_forward: scale_factor=%d (1..16; 0 = the shipped 2)", w->scale_factor);
    SM_REQUIRE(w->dec_kv_w && w->dec_kv_b, "sm_maskformer_forward: dec_kv_w/dec_kv_b (packed cross-attention K/V) missing");
    SM_REQUIRE(io->x && io->B > 0 && io->H > 0 && io->W > 0, "sm_maskformer_forward: bad input shape");
    if (w->gemm_mode >= 1) {
        const int gh = (io->H + w->patch - 1) / w->patch, gw = (io->W + w->patch - 1) / w->patch;
        const int sf = w->scale_factor > 0 ? w->scale_factor : 2;
        SM_REQUIRE((gh * gw) % 4 == 0 || (sf * sf * gh * gw) % 4 == 0,
                   "sm_maskformer_forward: the token count or the mask size must be a multiple of 4 (scale_factor %d on a %d x %d grid)", sf, gh, gw);
    }
    if (w->gemm_mode >= 2) {
        // W16 weights carry their 2^-s in the *_s fields; a zero (a caller that filled the pointers but not the scales) would
        // otherwise send W16 bytes through the F16X2 kernel: wrong results, no error
        bool ok = pow2(w->patch_s) && pow2(w->dec_kv_s) && pow2(w->ffn0_s) && pow2(w->ffn1_s) && (!w->mask_head_ffn || pow2(w->ffn2_s));
        for (int i = 0; i < SM_ENC_DEPTH && ok; ++i)
            ok = pow2(w->enc[i].qkv_s) && pow2(w->enc[i].proj_s) && pow2(w->enc[i].fc1_s) && pow2(w->enc[i].fc2_s);
        for (int l = 0; l < w->n_dec_layers && ok; ++l) {
            const sm_dec_layer& d = w->dec[l];
            ok = pow2(d.sa_in_s) && pow2(d.sa_out_s) && pow2(d.ca_in_s) && pow2(d.ca_out_s) && pow2(d.lin1_s) && pow2(d.lin2_s);
        }
        SM_REQUIRE(ok, "sm_maskformer_forward: gemm_mode 2/3 needs every weight's 2^-s (*_s fields) to be a positive power of two");
        if (w->ln_fold) {
            for (int i = 0; i < SM_ENC_DEPTH && ok; ++i) {
                const sm_enc_layer& e = w->enc[i];
                ok = e.fc1_fw && e.fc1_fb && e.fc1_c && pow2(e.fc1_fs) && (i == 0 || (e.qkv_fw && e.qkv_fb && e.qkv_c && pow2(e.qkv_fs)));
            }
            SM_REQUIRE(ok, "sm_maskformer_forward: ln_fold needs the gain-scaled weights, folded biases and row sums (*_fw, *_fb, *_c, *_fs) of every encoder layer");
        }
    }
    const bool want_attn = io->last_attn || io->last_attn_cls;
    SM_REQUIRE(io->attn_only == 0 || io->attn_only == 1, "sm_maskformer_forward: attn_only=%d (0 or 1)", io->attn_only);
    SM_REQUIRE(!io->attn_only || want_attn, "sm_maskformer_forward: attn_only needs last_attn or last_attn_cls");
    SM_REQUIRE(!want_attn || w->gemm_mode != 3,
               "sm_maskformer_forward: last_attn / last_attn_cls are not available in gemm_mode 3 (the one-MFMA diagnostic)");
    if (io->attn_only || (tp && tp->stop))
        ;  // the forward stops inside the encoder: no other output is written
    else if (!io->encoder_only)
        SM_REQUIRE(io->mask_pred && (io->objectness || w->mask_head_ffn || w->no_objectness) && io->features,
                   "sm_maskformer_forward: null output");
    else
        SM_REQUIRE(io->patch_tokens, "sm_maskformer_forward: encoder_only needs patch_tokens");
    SM_REQUIRE(io->attn_path >= 0 && io->attn_path <= 2, "sm_maskformer_forward: attn_path=%d (0 auto, 1 fused, 2 two launches)", io->attn_path);
    SM_REQUIRE(!(io->last_layer_only && w->mask_head_ffn), "sm_maskformer_forward: last_layer_only is the 3-D path (no ffn mask head)");
    if (!tp) return SM_OK;
    const uint32_t depth_bits = (1u << SM_ENC_DEPTH) - 1u;
    SM_REQUIRE(w->gemm_mode != 3, "sm_maskformer_forward_taps: encoder taps are not available in gemm_mode 3 (the one-MFMA diagnostic)");
    SM_REQUIRE(!(tp->layer_mask & ~depth_bits) && !(tp->attn_mask & ~depth_bits),
               "sm_maskformer_forward_taps: layer_mask=0x%x attn_mask=0x%x (bits 0..%d: blocks 1..%d)", tp->layer_mask, tp->attn_mask,
               SM_ENC_DEPTH - 1, SM_ENC_DEPTH);
    SM_REQUIRE(tp->layer_mask || tp->attn_mask || tp->post_pe || tp->input_tokens || tp->patch_mean,
               "sm_maskformer_forward_taps: nothing requested (empty masks, no post_pe / input_tokens / patch_mean)");
    SM_REQUIRE((tp->layer_mask != 0) == (tp->tokens != nullptr), "sm_maskformer_forward_taps: layer_mask and tokens go together (mask 0x%x, tokens %s)",
               tp->layer_mask, tp->tokens ? "set" : "NULL");
    SM_REQUIRE((tp->attn_mask != 0) == (tp->attn || tp->attn_cls), "sm_maskformer_forward_taps: attn_mask and attn / attn_cls go together (mask 0x%x)",
               tp->attn_mask);
    SM_REQUIRE(tp->select >= SM_TAP_ALL && tp->select <= SM_TAP_PATCH, "sm_maskformer_forward_taps: select=%d (SM_TAP_ALL, _CLS, _PATCH)", tp->select);
    SM_REQUIRE((tp->norm == 0 || tp->norm == 1) && (tp->stop == 0 || tp->stop == 1), "sm_maskformer_forward_taps: norm=%d stop=%d (0 or 1)",
               tp->norm, tp->stop);
    SM_REQUIRE(((uintptr_t)tp->tokens | (uintptr_t)tp->post_pe | (uintptr_t)tp->input_tokens | (uintptr_t)tp->patch_mean) % 16 == 0,
               "sm_maskformer_forward_taps: token outputs must be 16-B aligned");
    SM_REQUIRE(!io->attn_only, "sm_maskformer_forward_taps: attn_only with taps (set stop and ask for block 12 through attn_mask)");
    SM_REQUIRE(!tp->stop || !(want_attn || io->encoder_only),
               "sm_maskformer_forward_taps: stop with last_attn / last_attn_cls / encoder_only (ask for block 12 through attn_mask)");
    return SM_OK;
}

}  // namespace sm

extern "C" size_t sm_forward_workspace_bytes(const sm_weights* w, int32_t B, int32_t H, int32_t W) {
    if (!w || B <= 0 || H <= 0 || W <= 0 || (w->patch != 8 && w->patch != 16)) return 0;
    return sm::carve(sm::make_shape(w, B, H, W), nullptr).total;
}

extern "C" int sm_maskformer_forward_taps(const sm_weights* w, const sm_forward_io* io, const sm_encoder_taps* taps, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    int rc = sm::validate(w, io, taps);
    if (rc) return rc;
    const size_t need = sm_forward_workspace_bytes(w, io->B, io->H, io->W);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace % 256) != 0) {
        sm::set_error("sm_maskformer_forward: workspace %zu B < %zu B needed (or not 256-B aligned)", workspace_bytes, need);
        return SM_ENOSPACE;
    }
    return sm::forward(w, io, taps, (float*)workspace, (hipStream_t)stream);
}

extern "C" int sm_maskformer_forward(const sm_weights* w, const sm_forward_io* io, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    return sm_maskformer_forward_taps(w, io, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int sm_forward_timing(int enable) {
    for (auto& t : sm::g_taps) {
        (void)hipEventDestroy(t.e0);
        (void)hipEventDestroy(t.e1);
    }
    sm::g_taps.clear();
    sm::g_timing = enable != 0;
    return SM_OK;
}

extern "C" int sm_forward_timing_read(sm_kernel_time* out, int max_entries) {
    SM_REQUIRE(out && max_entries > 0, "sm_forward_timing_read: null output");
    int n = 0;
    // calibration: an event pair with nothing between it still measures the command processor's event handling
    double overhead_us = 0.0;
    if (!sm::g_taps.empty()) {
        hipStream_t st = sm::g_taps.front().st;
        (void)hipEventSynchronize(sm::g_taps.back().e1);
        const int reps = 16;
        hipEvent_t ev[2 * reps];
        for (auto& e : ev) (void)hipEventCreate(&e);
        for (auto& e : ev) (void)hipEventRecord(e, st);
        (void)hipEventSynchronize(ev[2 * reps - 1]);
        for (int i = 0; i < reps; ++i) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]);
            overhead_us += ms * 1e3 / reps;
        }
        for (auto& e : ev) (void)hipEventDestroy(e);
    }
    for (auto& t : sm::g_taps) {
        float ms = 0.f;
        if (hipEventSynchronize(t.e1) != hipSuccess || hipEventElapsedTime(&ms, t.e0, t.e1) != hipSuccess) {
            sm::set_error("sm_forward_timing_read: event query failed");
            return SM_ELAUNCH;
        }
        int k = 0;
        while (k < n && t.name != out[k].name) ++k;
        if (k == n) {
            if (n == max_entries) continue;
            memset(&out[n], 0, sizeof out[n]);
            strncpy(out[n].name, t.name.c_str(), sizeof out[n].name - 1);
            ++n;
        }
        out[k].launches += 1;
        out[k].overhead_us = overhead_us;
        out[k].total_us += ms * 1e3 > overhead_us ? ms * 1e3 - overhead_us : 0.0;
        out[k].flops += t.flops;
        out[k].bytes += t.bytes;
    }
    return n;
}
