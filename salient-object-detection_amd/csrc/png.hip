// PNG encoding of 8-bit grey / RGB / RGBA images on the device: the serving response's three pictures without their raw pixels crossing
// to the host.  The output is DEFINED by selfmask_amd/png.py (encode_reference): every step is a function of the input alone - integer
// histograms, integer LDS atomics and scans, no floating point - and the tests hold these kernels to its bytes.
//   G0  png_plan_kernel    one workgroup: per image the offset of its region of the workspace (a prefix sum over the table)
//   G1  png_filter_kernel  one workgroup per image row: the five filters' sums of |signed byte|, the pick (ties to the lowest id), the
//                          filtered row -> the image's filtered stream in the workspace
//   G2  png_deflate_kernel one workgroup per PNG_CHUNK bytes of the stream = one deflate block = one IDAT: chunk -> LDS, run starts /
//                          ends by two scans, tokens in closed form (literal, 258-matches, remainder; distance 1 only), histogram,
//                          length-limited Huffman lengths (rank sort by all lanes; two-queue merge and depth walk by one lane; repair
//                          on the 16 per-length counts), the cheapest of stored / fixed / dynamic, bits ORed into LDS words at offsets
//                          from a prefix sum, sync-flush block, the chunk's Adler-32 sums and the CRC-32 of "IDAT" + data (per-lane
//                          slices combined by multiplication with x^(8 n) mod the CRC polynomial) -> the chunk's slot
//   G3  png_gather_kernel  one workgroup per chunk: prefix sum of the chunk lengths -> its place in the file; framing, the combined
//                          Adler-32 behind the last chunk, signature + IHDR by chunk 0, IEND and the file's size by the last
// Workspace: [plan: B x 16 bytes | per image: filtered stream | chunk slots (PNG_SLOT bytes each) | chunk records (16 bytes each)].
#include "common.h"

namespace sm {

constexpr int PNG_THREADS = 256;
constexpr int PNG_CHUNK = 16384;           // png.py: PNG_CHUNK
constexpr int PNG_SEG = PNG_CHUNK / PNG_THREADS;  // consecutive positions per lane
constexpr int PNG_SLOT = PNG_CHUNK + 64;   // "IDAT" 4 + zlib header 2 + stored block 5 + PNG_CHUNK + sync block 5, rounded up
constexpr int PNG_SLOT_WORDS = PNG_SLOT / 4;
constexpr int PNG_MAX_PIXELS = 1 << 24;
constexpr int PNG_NSYM = 288;              // literal/length symbols of the fixed code; 286 can occur
constexpr unsigned PNG_CRC_POLY = 0xEDB88320u;
constexpr unsigned PNG_ADLER = 65521u;

struct PngPlan {
    int64_t ws_off;  // the image's region inside the workspace; 0 (the plan itself lives there) = the image is skipped
    int32_t nch, pad;
};
struct PngChunkRec {
    unsigned len, s1, s2, crc;  // bytes of IDAT data; sum d_i and sum (n - i) d_i mod 65521; CRC register after "IDAT" + data
};

__host__ __device__ __forceinline__ bool png_dims_ok(int H, int W, int C) {
    return H >= 1 && W >= 1 && (int64_t)H * W <= PNG_MAX_PIXELS && (C == 1 || C == 3 || C == 4);
}
__host__ __device__ __forceinline__ int64_t png_stream_bytes(int H, int W, int C) { return (int64_t)H * ((int64_t)W * C + 1); }
__host__ __device__ __forceinline__ int png_chunks(int64_t n) { return (int)((n + PNG_CHUNK - 1) / PNG_CHUNK); }
__host__ __device__ __forceinline__ int64_t png_align16(int64_t n) { return (n + 15) & ~(int64_t)15; }
__host__ __device__ __forceinline__ int64_t png_region_bytes(int64_t n) {
    return (png_align16(n) + (int64_t)png_chunks(n) * (PNG_SLOT + (int64_t)sizeof(PngChunkRec)) + 255) & ~(int64_t)255;
}
__host__ __device__ __forceinline__ int64_t png_plan_bytes(int B) { return ((int64_t)B * (int64_t)sizeof(PngPlan) + 255) & ~(int64_t)255; }
__host__ __device__ __forceinline__ int64_t png_bound(int H, int W, int C) {  // png.py: bound
    if (!png_dims_ok(H, W, C)) return 0;
    const int64_t n = png_stream_bytes(H, W, C);
    return n + 22 * (int64_t)png_chunks(n) + 51;
}
__host__ __device__ __forceinline__ bool png_image_ok(const sm_png_image& im) {
    return png_dims_ok(im.H, im.W, im.channels) && im.filter_mode >= -1 && im.filter_mode <= 4 && im.pix_off >= 0 && im.out_off >= 0 &&
           im.out_cap >= png_bound(im.H, im.W, im.channels);
}

// ---- G0 ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PNG_THREADS) void png_plan_kernel(const sm_png_image* __restrict__ imgs, int B, PngPlan* __restrict__ plan,
                                                               int64_t ws_bytes) {
    __shared__ int64_t part[PNG_THREADS];
    const int t = threadIdx.x, per = (B + PNG_THREADS - 1) / PNG_THREADS;
    const int b0 = t * per < B ? t * per : B, b1 = b0 + per < B ? b0 + per : B;
    int64_t sum = 0;
    for (int b = b0; b < b1; ++b) {
        const sm_png_image im = imgs[b];
        if (png_image_ok(im)) sum += png_region_bytes(png_stream_bytes(im.H, im.W, im.channels));
    }
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < PNG_THREADS; d <<= 1) {  // inclusive scan
        const int64_t v = part[t] + (t >= d ? part[t - d] : 0);
        __syncthreads();
        part[t] = v;
        __syncthreads();
    }
    int64_t off = png_plan_bytes(B) + part[t] - sum;
    for (int b = b0; b < b1; ++b) {
        const sm_png_image im = imgs[b];
        PngPlan p = {0, 0, 0};
        if (png_image_ok(im)) {
            const int64_t n = png_stream_bytes(im.H, im.W, im.channels), r = png_region_bytes(n);
            if (off + r <= ws_bytes) {
                p.ws_off = off;
                p.nch = png_chunks(n);
            }
            off += r;
        }
        plan[b] = p;
    }
}

// the image's table entry and plan, checked: false = skip it (a device table that disagrees with the host's)
__device__ __forceinline__ bool png_fetch(const sm_png_image* __restrict__ imgs, const PngPlan* __restrict__ plan, int b, int64_t ws_bytes,
                                          sm_png_image& im, PngPlan& pl, int64_t& n) {
    im = imgs[b];
    pl = plan[b];
    if (!png_image_ok(im)) return false;
    n = png_stream_bytes(im.H, im.W, im.channels);
    return pl.ws_off > 0 && pl.nch == png_chunks(n) && pl.ws_off + png_region_bytes(n) <= ws_bytes;
}

// ---- G1 ---------------------------------------------------------------------------------------------------------------------------------
// bytes x .. x + 3 of a row of rb bytes, zero where the index falls outside it (or there is no row): one 4-byte load inside the row
__device__ __forceinline__ unsigned png_get4(const unsigned char* __restrict__ row, int x, int rb) {
    if (!row) return 0;
    unsigned w = 0;
    if (x >= 0 && x + 4 <= rb) {
        __builtin_memcpy(&w, row + x, 4);
        return w;
    }
    for (int i = 0; i < 4; ++i)
        if (x + i >= 0 && x + i < rb) w |= (unsigned)row[x + i] << (8 * i);
    return w;
}
__device__ __forceinline__ int png_abs_diff(int a, int b) { return a > b ? a - b : b - a; }
__device__ __forceinline__ int png_filter_byte(int mode, int x, int a, int b, int c) {
    int pred = 0;
    if (mode == 1) pred = a;
    else if (mode == 2) pred = b;
    else if (mode == 3) pred = (a + b) >> 1;
    else if (mode == 4) {
        const int p = a + b - c, pa = png_abs_diff(p, a), pb = png_abs_diff(p, b), pc = png_abs_diff(p, c);
        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    }
    return (x - pred) & 255;
}

__global__ __launch_bounds__(PNG_THREADS) void png_filter_kernel(const unsigned char* __restrict__ pixels, const sm_png_image* __restrict__ imgs,
                                                                 const PngPlan* __restrict__ plan, unsigned char* __restrict__ ws,
                                                                 int64_t ws_bytes) {
    __shared__ unsigned long long tot[5];
    __shared__ int s_mode;
    sm_png_image im;
    PngPlan pl;
    int64_t n;
    const int y = blockIdx.x, t = threadIdx.x;
    if (!png_fetch(imgs, plan, blockIdx.y, ws_bytes, im, pl, n) || y >= im.H) return;
    const int C = im.channels, rb = im.W * C;  // <= 2^26
    const unsigned char* __restrict__ cur = pixels + im.pix_off + (int64_t)y * rb;
    const unsigned char* __restrict__ up = y ? cur - rb : nullptr;
    unsigned char* __restrict__ dst = ws + pl.ws_off + (int64_t)y * (rb + 1);
    int mode = im.filter_mode;
    if (mode < 0) {
        if (t < 5) tot[t] = 0;
        __syncthreads();
        unsigned s[5] = {0, 0, 0, 0, 0};  // a lane sees at most 2^26 / 256 bytes x 128
        for (int x = 4 * t; x < rb; x += 4 * PNG_THREADS) {
            const unsigned wx = png_get4(cur, x, rb), wa = png_get4(cur, x - C, rb), wb = png_get4(up, x, rb), wc = png_get4(up, x - C, rb);
            const int m = rb - x < 4 ? rb - x : 4;
            for (int i = 0; i < m; ++i) {
                const int vx = (wx >> (8 * i)) & 255, va = (wa >> (8 * i)) & 255, vb = (wb >> (8 * i)) & 255, vc = (wc >> (8 * i)) & 255;
#pragma unroll
                for (int f = 0; f < 5; ++f) {
                    const int v = png_filter_byte(f, vx, va, vb, vc);
                    s[f] += (unsigned)(v < 128 ? v : 256 - v);
                }
            }
        }
#pragma unroll
        for (int f = 0; f < 5; ++f) {
            unsigned long long v = s[f];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if ((t & 63) == 0) atomicAdd(&tot[f], v);
        }
        __syncthreads();
        if (t == 0) {
            int best = 0;
            for (int f = 1; f < 5; ++f)
                if (tot[f] < tot[best]) best = f;
            s_mode = best;
        }
        __syncthreads();
        mode = s_mode;
    }
    if (t == 0) dst[0] = (unsigned char)mode;
    for (int x = 4 * t; x < rb; x += 4 * PNG_THREADS) {
        const unsigned wx = png_get4(cur, x, rb), wa = png_get4(cur, x - C, rb), wb = png_get4(up, x, rb), wc = png_get4(up, x - C, rb);
        const int m = rb - x < 4 ? rb - x : 4;
        unsigned w = 0;
        for (int i = 0; i < m; ++i)
            w |= (unsigned)png_filter_byte(mode, (wx >> (8 * i)) & 255, (wa >> (8 * i)) & 255, (wb >> (8 * i)) & 255, (wc >> (8 * i)) & 255) << (8 * i);
        if (m == 4) __builtin_memcpy(dst + 1 + x, &w, 4);
        else
            for (int i = 0; i < m; ++i) dst[1 + x + i] = (unsigned char)(w >> (8 * i));
    }
}

// ---- G2 ---------------------------------------------------------------------------------------------------------------------------------
struct PngCodeScratch {            // the length-limited Huffman construction of one alphabet
    unsigned w[PNG_NSYM];          // counts in (count, symbol) order
    unsigned node_w[PNG_NSYM];     // internal nodes, in the order they are made
    unsigned short ord[PNG_NSYM];  // symbols in that order
    unsigned short leaf_parent[PNG_NSYM], node_parent[PNG_NSYM], depth[PNG_NSYM];
    unsigned per_len[16];
    unsigned n;
};

// counts cnt[0 .. nsym) -> lens[0 .. nsym), at most `limit` bits: png.py code_lengths.  Called by every lane of the workgroup.
__device__ void png_code_lengths(const unsigned* cnt, int nsym, int limit, unsigned char* lens, PngCodeScratch& s) {
    const int t = threadIdx.x;
    if (t == 0) s.n = 0;
    if (t < 16) s.per_len[t] = 0;
    __syncthreads();
    for (int sym = t; sym < nsym; sym += PNG_THREADS) {
        const unsigned c = cnt[sym];
        lens[sym] = 0;
        if (!c) continue;
        int rank = 0;
        for (int o = 0; o < nsym; ++o) {
            const unsigned co = cnt[o];
            rank += (co && (co < c || (co == c && o < sym))) ? 1 : 0;
        }
        s.ord[rank] = (unsigned short)sym;
        s.w[rank] = c;
        atomicAdd(&s.n, 1u);
    }
    __syncthreads();
    const int n = (int)s.n;
    if (n == 0) return;
    if (n == 1) {
        if (t == 0) lens[s.ord[0]] = 1;
        __syncthreads();
        return;
    }
    if (t == 0) {  // two queues: a leaf before an internal node of equal weight
        int i = 0, h = 0;
        for (int k = 0; k < n - 1; ++k) {
            unsigned tot = 0;
            for (int r = 0; r < 2; ++r) {
                if (i < n && (h >= k || s.w[i] <= s.node_w[h])) {
                    tot += s.w[i];
                    s.leaf_parent[i++] = (unsigned short)k;
                } else {
                    tot += s.node_w[h];
                    s.node_parent[h++] = (unsigned short)k;
                }
            }
            s.node_w[k] = tot;
        }
        s.depth[n - 2] = 0;
        for (int k = n - 3; k >= 0; --k) s.depth[k] = (unsigned short)(s.depth[s.node_parent[k]] + 1);
    }
    __syncthreads();
    for (int j = t; j < n; j += PNG_THREADS) {
        const int d = s.depth[s.leaf_parent[j]] + 1;
        atomicAdd(&s.per_len[d < limit ? d : limit], 1u);
    }
    __syncthreads();
    if (t == 0) {  // the repair: until the Kraft sum is exact
        unsigned total = 0;
        for (int l = 1; l <= limit; ++l) total += s.per_len[l] << (limit - l);
        while (total > (1u << limit)) {
            s.per_len[limit]--;
            for (int l = limit - 1; l > 0; --l)
                if (s.per_len[l]) {
                    s.per_len[l]--;
                    s.per_len[l + 1] += 2;
                    break;
                }
            total--;
        }
    }
    __syncthreads();
    for (int j = t; j < n; j += PNG_THREADS) {  // the rarest symbols the longest codes
        unsigned acc = 0;
        int len = 1;
        for (int l = limit; l >= 1; --l) {
            acc += s.per_len[l];
            if ((unsigned)j < acc) {
                len = l;
                break;
            }
        }
        lens[s.ord[j]] = (unsigned char)len;
    }
    __syncthreads();
}

// lens -> canonical codes, bit-reversed (png.py canonical_codes).  per_len: 16 words of scratch.  Every lane calls it.
__device__ void png_codes(const unsigned char* lens, int nsym, unsigned short* codes, unsigned* per_len) {
    const int t = threadIdx.x;
    if (t < 16) per_len[t] = 0;
    __syncthreads();
    for (int sym = t; sym < nsym; sym += PNG_THREADS)
        if (lens[sym]) atomicAdd(&per_len[lens[sym] & 15], 1u);
    __syncthreads();
    for (int sym = t; sym < nsym; sym += PNG_THREADS) {
        const int len = lens[sym] & 15;
        unsigned code = 0;
        if (len) {
            for (int l = 1; l <= len; ++l) code = (code + (l > 1 ? per_len[l - 1] : 0u)) << 1;
            for (int o = 0; o < sym; ++o) code += lens[o] == len ? 1u : 0u;
            code = __brev(code) >> (32 - len);
        }
        codes[sym] = (unsigned short)code;
    }
    __syncthreads();
}

__device__ __forceinline__ void png_put(unsigned* out, unsigned pos, unsigned v, int nb) {  // nb <= 25 bits of v at bit `pos`
    const unsigned wd = pos >> 5, sh = pos & 31;
    if (nb <= 0 || wd + 1 >= (unsigned)PNG_SLOT_WORDS) return;
    atomicOr(&out[wd], v << sh);
    if (sh + nb > 32) atomicOr(&out[wd + 1], v >> (32 - sh));
}

// match length 3 .. 258 -> symbol, extra bits, their value (png.py length_symbol)
__device__ __forceinline__ void png_length_symbol(int len, int& sym, int& eb, int& ev) {
    const int m = len - 3;
    if (m == 255) { sym = 285; eb = 0; ev = 0; return; }
    if (m < 8) { sym = 257 + m; eb = 0; ev = 0; return; }
    eb = 29 - __clz(m);  // floor(log2 m) - 2
    sym = 261 + 4 * eb + ((m >> eb) & 3);
    ev = m & ((1 << eb) - 1);
}

// the tokens that start at positions a .. b - 1 of the chunk (png.py position_tokens): s_in = the last run start before a, e_out = the
// first run start at or after b (the chunk's length if there is none); f(symbol, extra bits, their value, is a match)
template <class F>
__device__ __forceinline__ void png_walk(const unsigned char* in, int a, int b, int s_in, int e_out, F f) {
    if (a >= b) return;
    int s = (a == 0 || in[a] != in[a - 1]) ? a : s_in;
    int p = a;
    while (p < b) {
        const unsigned char v = in[p];
        int q = p + 1;
        while (q < b && in[q] == v) ++q;
        const int e = q < b ? q : e_out;
        const int r = e - s - 1, nfull = r / 258, rem = r - nfull * 258;
        for (; p < q; ++p) {
            const int k = p - s, j = k - 1;
            if (k == 0) {
                f((int)v, 0, 0, false);
            } else if (j < nfull * 258) {
                if (j % 258 == 0) f(285, 0, 0, true);
            } else if (rem < 3) {
                f((int)v, 0, 0, false);
            } else if (j == nfull * 258) {
                int sym, eb, ev;
                png_length_symbol(rem, sym, eb, ev);
                f(sym, eb, ev, true);
            }
        }
        s = q;
    }
}

__device__ __forceinline__ int png_fixed_len(int sym) { return sym < 144 ? 8 : (sym < 256 ? 9 : (sym < 280 ? 7 : 8)); }

__device__ __forceinline__ unsigned png_crc_mul(unsigned a, unsigned b) {  // a * b mod the CRC polynomial, reflected bit order
    unsigned p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (PNG_CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}
__device__ __forceinline__ unsigned png_crc_byte(unsigned reg, unsigned byte) {
    reg ^= byte;
    for (int i = 0; i < 8; ++i) reg = (reg >> 1) ^ (PNG_CRC_POLY & (0u - (reg & 1u)));
    return reg;
}
// x^(8 * 2^j) mod the CRC polynomial, j = 0 .. 15
__constant__ unsigned PNG_X8N[16] = {0x00800000u, 0x00008000u, 0xedb88320u, 0xb1e6b092u, 0xa06a2517u, 0xed627daeu, 0x88d14467u, 0xd7bbfe6au,
                                     0xec447f11u, 0x8e7ea170u, 0x6427800eu, 0x4d47bae0u, 0x09fe548fu, 0x83852d0fu, 0x30362f1au, 0x7b5a9cc3u};

#ifdef SM_PNG_STAMPS  // experiment build (build.py --variant=pngstamps -DSM_PNG_STAMPS, scripts/png_stamps.py): cycles of lane 0 between marks
#define PNG_MARK(k) do { if (threadIdx.x == 0) { const unsigned long long now_ = __builtin_readcyclecounter(); s_dbg[k] += now_ - s_dbg[15]; s_dbg[15] = now_; } } while (0)
#else
#define PNG_MARK(k)
#endif

constexpr int PNG_CRC_SLICE = 68;  // bytes per lane: 256 x 68 >= PNG_SLOT
static_assert(PNG_CRC_SLICE * PNG_THREADS >= PNG_SLOT && PNG_CRC_SLICE % 4 == 0, "CRC slices cover a slot");

__global__ __launch_bounds__(PNG_THREADS) void png_deflate_kernel(const sm_png_image* __restrict__ imgs, const PngPlan* __restrict__ plan,
                                                                  unsigned char* __restrict__ ws, int64_t ws_bytes) {
    __shared__ uint4 s_in4[PNG_CHUNK / 16];
    __shared__ unsigned s_out[PNG_SLOT_WORDS];
    __shared__ unsigned s_cnt[PNG_NSYM], s_clcnt[19];
    __shared__ unsigned char s_ll[PNG_NSYM], s_cl[19];
    __shared__ unsigned short s_code[PNG_NSYM], s_clcode[19];
    __shared__ PngCodeScratch s_hs;
    __shared__ int s_fwd[PNG_THREADS], s_bwd[PNG_THREADS];
    __shared__ unsigned s_scan[PNG_THREADS];
    // [0] extra bits, [1] matches, [2] fixed cost, [3] dynamic cost, [4] hlit, [5] hclen, [6] kind, [7] header bits, [8] s1, [9] s2, [10] crc
    __shared__ unsigned s_v[12];
#ifdef SM_PNG_STAMPS
    __shared__ unsigned long long s_dbg[16];
    if (threadIdx.x == 0) { for (int i = 0; i < 15; ++i) s_dbg[i] = 0; s_dbg[15] = __builtin_readcyclecounter(); }
#endif
    sm_png_image im;
    PngPlan pl;
    int64_t nstream;
    const int k = blockIdx.x, t = threadIdx.x;
    if (!png_fetch(imgs, plan, blockIdx.y, ws_bytes, im, pl, nstream) || k >= pl.nch) return;
    const bool last = k == pl.nch - 1;
    const int n = last ? (int)(nstream - (int64_t)k * PNG_CHUNK) : PNG_CHUNK;  // 1 .. PNG_CHUNK
    unsigned char* __restrict__ region = ws + pl.ws_off;
    const unsigned char* __restrict__ src = region + (int64_t)k * PNG_CHUNK;  // 16-byte aligned
    unsigned char* in = reinterpret_cast<unsigned char*>(s_in4);
    unsigned char* out8 = reinterpret_cast<unsigned char*>(s_out);

    // ---- the chunk and an empty output -----------------------------------------------------------------------------------------------
    for (int i = t; i < PNG_CHUNK / 16; i += PNG_THREADS) {
        uint4 v = {0, 0, 0, 0};
        if (16 * i + 16 <= n) v = reinterpret_cast<const uint4*>(src)[i];
        s_in4[i] = v;
    }
    for (int i = t; i < PNG_SLOT_WORDS; i += PNG_THREADS) s_out[i] = 0;
    for (int i = t; i < PNG_NSYM; i += PNG_THREADS) s_cnt[i] = 0;
    if (t < 19) s_clcnt[t] = 0;
    if (t < 12) s_v[t] = 0;
    __syncthreads();
    for (int i = (n & ~15) + t; i < n; i += PNG_THREADS) in[i] = src[i];  // the tail of the last chunk
    __syncthreads();
    PNG_MARK(0);  // load

    // ---- run starts before / after every lane's segment ------------------------------------------------------------------------------
    const int a = t * PNG_SEG < n ? t * PNG_SEG : n, b = a + PNG_SEG < n ? a + PNG_SEG : n;
    {
        int lastst = -1, firstst = n;
        for (int p = a; p < b; ++p)
            if (p == 0 || in[p] != in[p - 1]) {
                lastst = p;
                if (firstst == n) firstst = p;
            }
        s_fwd[t] = lastst;
        s_bwd[t] = firstst;
        __syncthreads();
        for (int d = 1; d < PNG_THREADS; d <<= 1) {  // inclusive max scan forward, min scan backward
            int f = s_fwd[t], g = s_bwd[t];
            if (t >= d) f = max(f, s_fwd[t - d]);
            if (t + d < PNG_THREADS) g = min(g, s_bwd[t + d]);
            __syncthreads();
            s_fwd[t] = f;
            s_bwd[t] = g;
            __syncthreads();
        }
    }
    const int s_in = t ? max(s_fwd[t - 1], 0) : 0, e_out = t + 1 < PNG_THREADS ? s_bwd[t + 1] : n;
    PNG_MARK(1);  // run scans

    // ---- histogram, Adler-32 sums -------------------------------------------------------------------------------------------------------
    {
        unsigned ebits = 0, nmatch = 0;
        png_walk(in, a, b, s_in, e_out, [&](int sym, int eb, int, bool match) {
            atomicAdd(&s_cnt[sym], 1u);
            ebits += (unsigned)eb;
            nmatch += match ? 1u : 0u;
        });
        if (ebits) atomicAdd(&s_v[0], ebits);
        if (nmatch) atomicAdd(&s_v[1], nmatch);
        unsigned s1 = 0, s2 = 0;  // s2 < 64 x 255 x 16384 < 2^32
        for (int p = a; p < b; ++p) {
            s1 += in[p];
            s2 += (unsigned)(n - p) * in[p];
        }
        if (s1) {
            atomicAdd(&s_v[8], s1);  // < 256 x 16320
            atomicAdd(&s_v[9], s2 % PNG_ADLER);
        }
        if (t == 0) s_cnt[256] = 1;  // end of block (no token adds to it)
    }
    __syncthreads();
    PNG_MARK(2);  // histogram walk, Adler sums

    // ---- the dynamic code and the three costs -----------------------------------------------------------------------------------------
    png_code_lengths(s_cnt, 286, 15, s_ll, s_hs);
    PNG_MARK(3);  // literal/length code lengths
    if (t < 2) s_ll[286 + t] = 0;  // the two symbols only the fixed code has
    __syncthreads();
    const int dist_len = s_v[1] ? 1 : 0;
    for (int sym = t; sym < 286; sym += PNG_THREADS) {
        const unsigned c = s_cnt[sym];
        if (c) {
            atomicAdd(&s_v[2], c * (unsigned)png_fixed_len(sym));
            atomicAdd(&s_v[3], c * (unsigned)s_ll[sym]);
            atomicMax(&s_v[4], (unsigned)sym + 1u);
        }
    }
    __syncthreads();
    const int hlit = min(max((int)s_v[4], 257), 286);
    if (t == 0) {  // the code-length sequence's histogram: zero runs in closed form (png.py code_length_sequence)
        for (int i = 0; i < hlit;) {
            if (s_ll[i]) {
                s_clcnt[s_ll[i]]++;
                ++i;
                continue;
            }
            int z = i;
            while (z < hlit && s_ll[z] == 0) ++z;
            z -= i;
            i += z;
            s_clcnt[18] += (unsigned)(z / 138);
            z %= 138;
            if (z >= 11) s_clcnt[18]++;
            else if (z >= 3) s_clcnt[17]++;
            else s_clcnt[0] += (unsigned)z;
        }
        s_clcnt[dist_len]++;
    }
    __syncthreads();
    PNG_MARK(4);  // costs, code-length histogram
    png_code_lengths(s_clcnt, 19, 7, s_cl, s_hs);
    png_codes(s_cl, 19, s_clcode, s_hs.per_len);
    PNG_MARK(5);  // code-length code
    if (t == 0) {
        const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int hclen = 4;
        for (int i = 4; i < 19; ++i)
            if (s_cl[order[i]]) hclen = i + 1;
        unsigned head = 3 + 14 + 3 * (unsigned)hclen;
        for (int c = 0; c < 19; ++c) head += s_clcnt[c] * (s_cl[c] + (c == 18 ? 7u : (c == 17 ? 3u : 0u)));
        const unsigned body = s_v[0], nm = s_v[1];
        const unsigned cost_dyn = head + s_v[3] + body + nm * (unsigned)dist_len;
        const unsigned cost_fix = 3 + s_v[2] + body + 5 * nm;
        const unsigned cost_sto = 8u * (5u + (unsigned)n);
        int kind = 0;
        unsigned best = cost_sto;
        if (cost_fix < best) { kind = 1; best = cost_fix; }
        if (cost_dyn < best) { kind = 2; best = cost_dyn; }
        s_v[5] = (unsigned)hclen;
        s_v[6] = (unsigned)kind;
        s_v[7] = kind == 2 ? head : 3u;
        s_v[11] = best;
        s_v[8] %= PNG_ADLER;
        s_v[9] %= PNG_ADLER;
    }
    __syncthreads();
    const int kind = (int)s_v[6];
    const unsigned base = 32u + (k == 0 ? 16u : 0u);  // "IDAT", and the zlib header in front of the first chunk
    if (t == 0) {
        s_out[0] = 0x54414449u;            // I D A T
        if (k == 0) s_out[1] = 0x00000178u;  // 78 01
    }
    __syncthreads();

    // ---- the block ------------------------------------------------------------------------------------------------------------------------
    if (kind == 0) {
        const unsigned o = base >> 3;
        if (t == 0) {
            out8[o] = last ? 1 : 0;
            out8[o + 1] = (unsigned char)n;
            out8[o + 2] = (unsigned char)(n >> 8);
            out8[o + 3] = (unsigned char)~n;
            out8[o + 4] = (unsigned char)(~n >> 8);
        }
        for (int p = a; p < b; ++p) out8[o + 5 + p] = in[p];
    } else {
        if (kind == 1)
            for (int sym = t; sym < PNG_NSYM; sym += PNG_THREADS) s_ll[sym] = (unsigned char)png_fixed_len(sym);
        __syncthreads();
        png_codes(s_ll, PNG_NSYM, s_code, s_hs.per_len);
        PNG_MARK(6);  // choice, canonical codes
        const int dl = kind == 1 ? 5 : dist_len;
        unsigned bits = 0;
        png_walk(in, a, b, s_in, e_out, [&](int sym, int eb, int, bool match) { bits += (unsigned)s_ll[sym] + (unsigned)eb + (match ? (unsigned)dl : 0u); });
        s_scan[t] = bits;
        __syncthreads();
        for (int d = 1; d < PNG_THREADS; d <<= 1) {
            const unsigned v = s_scan[t] + (t >= d ? s_scan[t - d] : 0u);
            __syncthreads();
            s_scan[t] = v;
            __syncthreads();
        }
        unsigned pos = base + s_v[7] + s_scan[t] - bits;
        PNG_MARK(7);  // bit-length walk, prefix sum
        png_walk(in, a, b, s_in, e_out, [&](int sym, int eb, int ev, bool match) {
            const int len = s_ll[sym];
            png_put(s_out, pos, (unsigned)s_code[sym] | ((unsigned)ev << len), len + eb + (match ? dl : 0));
            pos += (unsigned)(len + eb + (match ? dl : 0));
        });
        if (t == PNG_THREADS - 1) png_put(s_out, base + s_v[7] + s_scan[t], s_code[256], s_ll[256]);  // end of block
        PNG_MARK(8);  // deposit walk
        if (t == 0) {
            unsigned hp = base;
            png_put(s_out, hp, (last ? 1u : 0u) | ((unsigned)kind << 1), 3);
            hp += 3;
            if (kind == 2) {
                const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                const int hclen = (int)s_v[5];
                png_put(s_out, hp, (unsigned)(hlit - 257) | (0u << 5) | ((unsigned)(hclen - 4) << 10), 14);
                hp += 14;
                for (int i = 0; i < hclen; ++i, hp += 3) png_put(s_out, hp, s_cl[order[i]], 3);
                auto emit = [&](int c, int eb, int ev) {
                    png_put(s_out, hp, (unsigned)s_clcode[c] | ((unsigned)ev << s_cl[c]), s_cl[c] + eb);
                    hp += (unsigned)(s_cl[c] + eb);
                };
                for (int i = 0; i < hlit;) {
                    if (s_ll[i]) {
                        emit(s_ll[i], 0, 0);
                        ++i;
                        continue;
                    }
                    int z = i;
                    while (z < hlit && s_ll[z] == 0) ++z;
                    z -= i;
                    i += z;
                    for (; z >= 138; z -= 138) emit(18, 7, 127);
                    if (z >= 11) emit(18, 7, z - 11);
                    else if (z >= 3) emit(17, 3, z - 3);
                    else
                        for (; z > 0; --z) emit(0, 0, 0);
                }
                emit(dist_len, 0, 0);
            }
        }
    }
    // the sync block (3 zero bits, padding, 00 00 FF FF) behind every chunk but the last; the output was zero all over
    unsigned end_bits = base + s_v[11] + (last ? 0u : 3u);
    unsigned nbytes = (end_bits + 7) >> 3;  // of "IDAT" + data
    __syncthreads();  // every bit of the block is in place
    PNG_MARK(9);  // header bits (lane 0), everyone arrived
    if (!last) {
        if (t == 0 && nbytes + 4 <= (unsigned)PNG_SLOT) {
            out8[nbytes + 2] = 0xFF;
            out8[nbytes + 3] = 0xFF;
        }
        nbytes += 4;
    }
    nbytes = nbytes < (unsigned)PNG_SLOT ? nbytes : (unsigned)PNG_SLOT;
    __syncthreads();

    // ---- CRC-32 of "IDAT" + data: a slice per lane from a zero register, each times x^(8 x the bytes behind it), XORed ------------------
    {
        const unsigned lo = (unsigned)t * PNG_CRC_SLICE, hi = min(lo + (unsigned)PNG_CRC_SLICE, nbytes);
        if (lo < hi) {
            unsigned reg = 0;
            unsigned i = lo;
            for (; i + 4 <= hi; i += 4) {
                reg ^= s_out[i >> 2] ^ (i == 0 ? 0xFFFFFFFFu : 0u);  // the initial register, folded into the first four bytes
                for (int r = 0; r < 32; ++r) reg = (reg >> 1) ^ (PNG_CRC_POLY & (0u - (reg & 1u)));
            }
            for (; i < hi; ++i) reg = png_crc_byte(reg, out8[i]);
            const unsigned after = nbytes - hi;
            for (int j = 0; j < 16; ++j)
                if ((after >> j) & 1u) reg = png_crc_mul(PNG_X8N[j], reg);
            atomicXor(&s_v[10], reg);
        }
    }
    __syncthreads();

    PNG_MARK(10);  // CRC-32
    // ---- the slot and its record ------------------------------------------------------------------------------------------------------------
    unsigned char* __restrict__ slots = region + png_align16(nstream);
    uint4* __restrict__ slot = reinterpret_cast<uint4*>(slots + (int64_t)k * PNG_SLOT);
    const uint4* o4 = reinterpret_cast<const uint4*>(s_out);
    for (unsigned i = t; i < (nbytes + 15) / 16; i += PNG_THREADS) slot[i] = o4[i];
    if (t == 0) {
        PngChunkRec* rec = reinterpret_cast<PngChunkRec*>(slots + (int64_t)pl.nch * PNG_SLOT) + k;
        PngChunkRec r;
        r.len = nbytes - 4;
        r.s1 = s_v[8];
        r.s2 = s_v[9];
        r.crc = s_v[10];
        *rec = r;
    }
#ifdef SM_PNG_STAMPS
    __syncthreads();
    PNG_MARK(11);  // stores
    if (t == 0 && k == 0 && blockIdx.y == 0)  // into the unused tail of the plan's 256 bytes
        for (int i = 0; i < 12; ++i) reinterpret_cast<unsigned long long*>(ws + 64)[i] = s_dbg[i];
#endif
}

// ---- G3 ---------------------------------------------------------------------------------------------------------------------------------
struct PngOut {
    unsigned char* p;
    int64_t cap;
    __device__ __forceinline__ void put(int64_t at, unsigned v) const {
        if (at >= 0 && at < cap) p[at] = (unsigned char)v;
    }
    __device__ __forceinline__ void be32(int64_t at, unsigned v) const {
        put(at, v >> 24);
        put(at + 1, v >> 16);
        put(at + 2, v >> 8);
        put(at + 3, v);
    }
};

__global__ __launch_bounds__(PNG_THREADS) void png_gather_kernel(const sm_png_image* __restrict__ imgs, const PngPlan* __restrict__ plan,
                                                                 const unsigned char* __restrict__ ws, int64_t ws_bytes,
                                                                 unsigned char* __restrict__ out, int64_t* __restrict__ sizes_out) {
    __shared__ unsigned long long s_sum;
    sm_png_image im;
    PngPlan pl;
    int64_t nstream;
    const int k = blockIdx.x, t = threadIdx.x, b = blockIdx.y;
    if (!png_fetch(imgs, plan, b, ws_bytes, im, pl, nstream) || k >= pl.nch) return;
    const unsigned char* __restrict__ slots = ws + pl.ws_off + png_align16(nstream);
    const PngChunkRec* __restrict__ rec = reinterpret_cast<const PngChunkRec*>(slots + (int64_t)pl.nch * PNG_SLOT);
    if (t == 0) s_sum = 0;
    __syncthreads();
    unsigned long long part = 0;
    for (int j = t; j < k; j += PNG_THREADS) part += 12ull + min(rec[j].len, (unsigned)(PNG_SLOT - 4));
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if ((t & 63) == 0 && part) atomicAdd(&s_sum, part);
    __syncthreads();
    const bool last = k == pl.nch - 1;
    const unsigned len = min(rec[k].len, (unsigned)(PNG_SLOT - 4)), data = len + (last ? 4u : 0u);
    const int64_t pos = 33 + (int64_t)s_sum;  // behind the signature and IHDR
    const PngOut o = {out + im.out_off, im.out_cap};
    const unsigned char* __restrict__ slot = slots + (int64_t)k * PNG_SLOT;
    for (unsigned i = t; i < 4 + len; i += PNG_THREADS) o.put(pos + 4 + i, slot[i]);
    if (t != 0) return;
    o.be32(pos, data);
    unsigned reg = rec[k].crc;
    if (last) {  // the Adler-32 of the whole stream from the chunks' sums
        unsigned A = 1, B = 0;
        for (int j = 0; j < pl.nch; ++j) {
            const unsigned nj = j == pl.nch - 1 ? (unsigned)(nstream - (int64_t)j * PNG_CHUNK) : (unsigned)PNG_CHUNK;
            B = (B + nj * A + rec[j].s2 % PNG_ADLER) % PNG_ADLER;  // nj * A < 2^14 x 2^16
            A = (A + rec[j].s1 % PNG_ADLER) % PNG_ADLER;
        }
        const unsigned adler = (B << 16) | A;
        o.be32(pos + 8 + len, adler);
        for (int i = 3; i >= 0; --i) reg = png_crc_byte(reg, (adler >> (8 * i)) & 255u);
    }
    o.be32(pos + 8 + data, ~reg);
    if (k == 0) {
        const unsigned char colour = im.channels == 1 ? 0 : (im.channels == 3 ? 2 : 6);
        const unsigned char head[29] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R',
                                        (unsigned char)(im.W >> 24), (unsigned char)(im.W >> 16), (unsigned char)(im.W >> 8), (unsigned char)im.W,
                                        (unsigned char)(im.H >> 24), (unsigned char)(im.H >> 16), (unsigned char)(im.H >> 8), (unsigned char)im.H,
                                        8, colour, 0, 0, 0};
        unsigned c = 0xFFFFFFFFu;
        for (int i = 0; i < 29; ++i) {
            o.put(i, head[i]);
            if (i >= 12) c = png_crc_byte(c, head[i]);
        }
        o.be32(29, ~c);
    }
    if (last) {
        const int64_t e = pos + 12 + data;
        const unsigned char iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
        for (int i = 0; i < 12; ++i) o.put(e + i, iend[i]);
        sizes_out[b] = e + 12;
    }
}

}  // namespace sm

extern "C" size_t sm_png_bound(int32_t H, int32_t W, int32_t channels) { return (size_t)sm::png_bound(H, W, channels); }

extern "C" size_t sm_png_workspace_bytes(const sm_png_image* images_host, int32_t B) {
    if (!images_host || B <= 0 || B > 65535) return 0;
    int64_t total = sm::png_plan_bytes(B);
    for (int b = 0; b < B; ++b) {
        const sm_png_image& im = images_host[b];
        if (!sm::png_dims_ok(im.H, im.W, im.channels)) return 0;
        total += sm::png_region_bytes(sm::png_stream_bytes(im.H, im.W, im.channels));
    }
    return (size_t)total;
}

extern "C" int sm_png_encode_batch_u8(const uint8_t* pixels, const sm_png_image* images_host, const sm_png_image* images_dev, int32_t B,
                                      uint8_t* out, int64_t* sizes_out, void* workspace, size_t workspace_bytes, void* stream) {
    SM_REQUIRE(pixels && images_host && images_dev && out && sizes_out && workspace,
               "sm_png_encode_batch_u8: null pointer (pixels, the host or device image table, out, sizes_out or workspace)");
    SM_REQUIRE(B > 0 && B <= 65535, "sm_png_encode_batch_u8: B=%d (1 .. 65535)", B);
    SM_REQUIRE(((uintptr_t)workspace % 16) == 0 && ((uintptr_t)sizes_out % 8) == 0,
               "sm_png_encode_batch_u8: misaligned pointer (workspace 16, sizes_out 8 bytes)");
    int max_h = 0, max_chunks = 0;
    for (int b = 0; b < B; ++b) {
        const sm_png_image& im = images_host[b];
        SM_REQUIRE(sm::png_dims_ok(im.H, im.W, im.channels), "sm_png_encode_batch_u8: image %d is %d x %d x %d (1, 3 or 4 channels, at most %d pixels)",
                   b, im.H, im.W, im.channels, sm::PNG_MAX_PIXELS);
        SM_REQUIRE(im.filter_mode >= -1 && im.filter_mode <= 4, "sm_png_encode_batch_u8: image %d: filter_mode=%d (-1 adaptive, 0 .. 4)", b,
                   im.filter_mode);
        SM_REQUIRE(im.pix_off >= 0 && im.out_off >= 0, "sm_png_encode_batch_u8: image %d has a negative offset", b);
        if (im.out_cap < sm::png_bound(im.H, im.W, im.channels)) {
            sm::set_error("sm_png_encode_batch_u8: image %d: out_cap=%lld below sm_png_bound=%lld", b, (long long)im.out_cap,
                          (long long)sm::png_bound(im.H, im.W, im.channels));
            return SM_ENOSPACE;
        }
        max_h = im.H > max_h ? im.H : max_h;
        const int nch = sm::png_chunks(sm::png_stream_bytes(im.H, im.W, im.channels));
        max_chunks = nch > max_chunks ? nch : max_chunks;
    }
    const size_t need = sm_png_workspace_bytes(images_host, B);
    if (!need || workspace_bytes < need) {
        sm::set_error("sm_png_encode_batch_u8: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return SM_ENOSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    sm::PngPlan* plan = (sm::PngPlan*)workspace;
    unsigned char* ws = (unsigned char*)workspace;
    const int64_t wsb = (int64_t)need;  // what the layout was sized for: the kernels stay inside it
    {
        sm::TapGuard tap(stream, "png_plan");
        hipLaunchKernelGGL(sm::png_plan_kernel, dim3(1), dim3(sm::PNG_THREADS), 0, st, images_dev, B, plan, wsb);
    }
    {
        sm::TapGuard tap(stream, "png_filter");
        hipLaunchKernelGGL(sm::png_filter_kernel, dim3(max_h, B), dim3(sm::PNG_THREADS), 0, st, pixels, images_dev, plan, ws, wsb);
    }
    {
        sm::TapGuard tap(stream, "png_deflate");
        hipLaunchKernelGGL(sm::png_deflate_kernel, dim3(max_chunks, B), dim3(sm::PNG_THREADS), 0, st, images_dev, plan, ws, wsb);
    }
    {
        sm::TapGuard tap(stream, "png_gather");
        hipLaunchKernelGGL(sm::png_gather_kernel, dim3(max_chunks, B), dim3(sm::PNG_THREADS), 0, st, images_dev, plan, (const unsigned char*)ws, wsb,
                           out, sizes_out);
    }
    return sm::check_launch("sm_png_encode_batch_u8");
}
