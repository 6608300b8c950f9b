// Entropy decode of baseline JPEG scans on the device: the Huffman decode that csrc/jpeg_host.h's decode_scan does on a host thread,
// into the same int16 coefficient layout, with the same verdict.  Input: the records of sm_jpeg_scan_prepare (unstuffed scan bytes, one
// table entry per restart interval, the Huffman tables in the host decoder's own form - walked by the host decoder's own lookup, the quantisation tables).
//
// The self-synchronising scheme of Weissenberger & Schmidt, "Accelerating JPEG Decompression on GPUs", cut so that all
// synchronisation stays inside one workgroup: ONE WORKGROUP PER IMAGE (1024 lanes), which walks the image's restart intervals, each
// in chunks of `chunk_subseqs` sub-sequences of `subseq_bits` bits, one lane per sub-sequence:
//   1. every lane decodes its sub-sequence from a guessed state ("a block starts at my first bit"); the chunk's first lane starts from
//      the true state (the interval's start, or the exit state of the chunk before).  The exit state (bit position of the first symbol
//      that starts behind the sub-sequence, block inside the MCU, zig-zag index) and the number of blocks completed are stored in the LDS;
//   2. rounds, a barrier apart: lane i decodes on into the next sub-sequence from its own exit state, always stores the block count it
//      saw there, and stops when its exit state equals the stored one, else replaces it.  An earlier lane reaches a sub-sequence in a later
//      round, so the chunk's first lane - the true one - has the last word; at most as many rounds as sub-sequences;
//   3. a prefix sum of the block counts gives every sub-sequence its first block;
//   4. every lane decodes its sub-sequence once more from the now-true entry state and writes the coefficients, de-zigzagged, to the
//      block's place in the component planes (DC values as differences);
// then, over the whole image, a segmented scan per component undoes the DC prediction, and one thread per block applies the host's
// range checks.  "Never guesses" stays the rule: only pass 4 and what follows it decide the verdict - a lane of pass 1 / 2 that meets an
// impossible code from a guessed state is merely unsynchronised (its exit state becomes JE_ERR, which no true state equals).  A flagged
// image's coefficients are zeroed.
//
// Memory safety on hostile bytes: bits are read through JeReader, which returns zero outside the record's padded scan; a symbol that
// would end behind its interval's last bit is an error, so no state ever points past it; a block's address is formed from a block
// number that is checked against the interval's block count; every loop runs over a bit range or a count that the record fixes.
// The Huffman tables (8.3 KiB at most) sit in the LDS; the scan bytes are read from memory, 4 bytes per 32 bits consumed.
#include "common.h"
#include "jpeg_host.h"

namespace sm {

constexpr int JE_THREADS = 1024, JE_MAX_HUFF = 6;
constexpr uint32_t JE_ERR = 0xFFFFFFFFu;

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct JeReader {
    const uint32_t* w;  // the image's scan, 16-byte aligned
    uint32_t nw;        // dwords that lie inside the record (scan + zero padding)
    uint32_t idx;       // dword index of the window's upper half
    uint64_t win;
    __device__ __forceinline__ uint32_t ld(uint32_t i) const { return i < nw ? __builtin_bswap32(w[i]) : 0u; }
    __device__ __forceinline__ void seek(uint32_t bit) {
        idx = bit >> 5;
        win = ((uint64_t)ld(idx) << 32) | ld(idx + 1);
    }
    // the 32 bits from bit position `bit` on, most significant first
    __device__ __forceinline__ uint32_t peek32(uint32_t bit) {
        const uint32_t i = bit >> 5;
        if (i != idx) {
            if (i == idx + 1) win = (win << 32) | ld(i + 1), idx = i;
            else seek(bit);
        }
        return (uint32_t)((win << (bit & 31)) >> 32);
    }
};

struct JeState {
    uint32_t p;   // bit position inside the image's scan of the next symbol; JE_ERR: no decode goes on from here
    uint32_t bi;  // block inside the MCU
    uint32_t z;   // zig-zag index of the next coefficient, 0: the DC symbol comes next
};

// what the lanes of one image share
struct JeBlock {     // per block inside the MCU
    int64_t base;    // element offset of its component's plane inside the image's coefficients
    int dc, ac;      // the component's tables
    int h, v, bw;    // the component's sampling factors and blocks per row
    int dv, dh;      // the block's place inside the MCU
    int comp;
};
struct JeImage {
    const smjpeg::HuffTable* huff;  // LDS
    const uint8_t* zigzag;        // LDS
    const JeBlock* blk;           // LDS
    int nb;                       // blocks per MCU
    int mcus_x;
};

// Decodes the symbols that start in [st.p, limit) of the interval that ends at bit seg_end; -> blocks completed.  WRITE: `blk0` is the
// number inside the interval of the block that is open at entry; coefficients go to coef (the image's), nothing is decoded once
// seg_blocks blocks are complete, and the lane that completes the last one reports the bits left behind it in *tail_bits.
template <bool WRITE>
__device__ int je_run(const JeImage& im, JeReader& rd, JeState& st, uint32_t limit, uint32_t seg_end, int blk0, int seg_blocks, int mcu0,
                      int16_t* coef, int* tail_bits) {
    int done = 0;
    if (st.p == JE_ERR) return 0;
    int16_t* blk = nullptr;
    int blk_of = -1;
    while (st.p < limit) {
        if (WRITE && blk0 + done >= seg_blocks) break;  // what follows the interval's last block is padding
        const JeBlock& kb = im.blk[st.bi];
        const uint32_t bits = rd.peek32(st.p);
        int len, s, r = 0;
        const int sym = smjpeg::huff_lookup(im.huff[st.z == 0 ? kb.dc : kb.ac], bits, len);
        bool bad = len == 0, store = false, eob = false;
        if (st.z == 0) {
            s = sym;
            bad |= s > 11;
            store = true;
        } else {
            r = sym >> 4, s = sym & 15;
            if (s == 0) {
                if (r == 15) bad |= st.z + 16 > 64;  // ZRL
                else if (r != 0) bad = true;         // EOBn belongs to progressive scans
                else eob = true;
            } else {
                bad |= st.z + r > 63 || s > 10;
                store = true;
            }
        }
        const uint32_t total = (uint32_t)(len + s);
        if (bad || total > seg_end - st.p) {  // no code, an impossible run, or a symbol that ends behind the interval's data
            st.p = JE_ERR;
            break;
        }
        uint32_t z = st.z;
        if (store) {
            z += r;
            if (WRITE) {
                int val = 0;
                if (s) {
                    const int raw = (int)((bits << len) >> (32 - s));
                    val = smjpeg::extend(raw, s);
                }
                if (blk_of != done) {  // the block's place: MCU by MCU in the scan, raster order in the component's plane
                    const int bn = blk0 + done, mcu = mcu0 + bn / im.nb;
                    const int my = mcu / im.mcus_x, mx = mcu - my * im.mcus_x;
                    blk = coef + kb.base + ((int64_t)(my * kb.v + kb.dv) * kb.bw + (mx * kb.h + kb.dh)) * 64;
                    blk_of = done;
                }
                blk[im.zigzag[z]] = (int16_t)val;  // z == 0: the DC difference
            }
            z += 1;
        } else if (eob) {
            z = 64;
        } else {
            z += 16;
        }
        st.p += total;
        if (z >= 64) {
            z = 0;
            st.bi = st.bi + 1 == (uint32_t)im.nb ? 0 : st.bi + 1;
            ++done;
            if (WRITE && blk0 + done == seg_blocks) *tail_bits = (int)(seg_end - st.p);
        }
        st.z = z;
    }
    return done;
}

// inclusive segmented scan over JE_THREADS (value, reset flag) pairs: out = the sum since the last pair whose flag is set, that pair included
__device__ __forceinline__ int je_scan(int* s_val, int* s_flag, int v, int f, int n) {
    const int t = threadIdx.x;
    s_val[t] = v, s_flag[t] = f;
    __syncthreads();
    for (int d = 1; d < n; d <<= 1) {
        int pv = 0, pf = 1;
        if (t >= d) pv = s_val[t - d], pf = s_flag[t - d];
        __syncthreads();
        if (t >= d) {
            if (!f) v += pv;
            f |= pf;
            s_val[t] = v, s_flag[t] = f;
        }
        __syncthreads();
    }
    return v;
}

__global__ __launch_bounds__(JE_THREADS) void jpeg_entropy_kernel(const sm_jpeg_scan* __restrict__ descr, const uint8_t* __restrict__ scans,
                                                                  int16_t* __restrict__ coef_out, int32_t* __restrict__ status,
                                                                  int32_t* __restrict__ stats, int subseq_bits, int chunk_subseqs) {
    __shared__ smjpeg::HuffTable s_huff[JE_MAX_HUFF];
    __shared__ uint32_t s_p[JE_THREADS], s_bz[JE_THREADS];
    __shared__ int s_cnt[JE_THREADS], s_val[JE_THREADS], s_rst[JE_THREADS];
    __shared__ int s_qt[192];
    __shared__ uint8_t s_zigzag[64];
    __shared__ JeBlock s_blk[8];
    __shared__ int s_flag, s_tail;
    const int t = threadIdx.x;
    const sm_jpeg_scan sc = descr[blockIdx.x];
    const uint8_t* rec = scans + sc.rec_off;
    int16_t* coef = reinterpret_cast<int16_t*>(reinterpret_cast<char*>(coef_out) + sc.coef_off);
    const int nc = sc.components;

    JeImage im;
    im.huff = s_huff, im.zigzag = s_zigzag, im.blk = s_blk;
    im.mcus_x = sc.mcus_x;
    int nb = 0;
    int64_t blocks = 0, comp_base[3] = {0, 0, 0};
    for (int c = 0; c < nc; ++c) {
        comp_base[c] = blocks * 64;
        blocks += (int64_t)sc.blocks_w[c] * sc.blocks_h[c];
        nb += sc.h[c] * sc.v[c];
    }
    im.nb = nb;
    // tables into the LDS, the image's coefficients to zero
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(rec + sc.huff_off);
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_huff);
        for (int i = t; i < sc.n_huff * (int)(sizeof(smjpeg::HuffTable) / 4); i += JE_THREADS) dst[i] = src[i];
        const uint16_t* q = reinterpret_cast<const uint16_t*>(rec + sc.qt_off);
        if (t < 192) s_qt[t] = q[t];
        if (t < 64) s_zigzag[t] = smjpeg::ZIGZAG[t];
        if (t == 0) {
            int k = 0;
            for (int c = 0; c < nc; ++c)
                for (int vv = 0; vv < sc.v[c]; ++vv)
                    for (int hh = 0; hh < sc.h[c]; ++hh, ++k) {
                        JeBlock& kb = s_blk[k];
                        kb.base = comp_base[c], kb.dc = sc.dc[c], kb.ac = sc.ac[c], kb.h = sc.h[c], kb.v = sc.v[c], kb.bw = sc.blocks_w[c];
                        kb.dv = vv, kb.dh = hh, kb.comp = c;
                    }
            s_flag = 0;
        }
        i32x4* z = reinterpret_cast<i32x4*>(coef);
        const i32x4 zero = {0, 0, 0, 0};
        for (int64_t i = t; i < blocks * 8; i += JE_THREADS) z[i] = zero;
    }
    __syncthreads();

    JeReader rd;
    rd.w = reinterpret_cast<const uint32_t*>(rec + sc.scan_off);
    rd.nw = (uint32_t)((sc.scan_len + 3) / 4 + 2);  // the record pads its scan with at least 8 zero bytes
    const sm_jpeg_segment* segs = reinterpret_cast<const sm_jpeg_segment*>(rec + sc.seg_off);
    const int64_t n_mcu = (int64_t)sc.mcus_x * sc.mcus_y;
    const int ri = sc.restart_interval > 0 && sc.restart_interval < n_mcu ? sc.restart_interval : (int)n_mcu;
    int rounds_all = 0, chunks_all = 0;
    bool bad_record = false;

    for (int k = 0; k < sc.n_seg; ++k) {
        const sm_jpeg_segment sg = segs[k];
        const int64_t want0 = (int64_t)k * ri, want_n = n_mcu - want0 < ri ? n_mcu - want0 : ri;
        if (sg.byte_off < 0 || sg.byte_len < 0 || (int64_t)sg.byte_off + sg.byte_len > sc.scan_len || sg.mcu0 != want0 || sg.mcus != want_n) {
            bad_record = true;  // not a table sm_jpeg_scan_prepare wrote: nothing is decoded from it
            break;
        }
        const uint32_t seg_bit0 = (uint32_t)sg.byte_off * 8u, seg_end = seg_bit0 + (uint32_t)sg.byte_len * 8u;
        const int seg_blocks = sg.mcus * nb;
        const int nsub = (int)(((uint32_t)sg.byte_len * 8u + (uint32_t)subseq_bits - 1) / (uint32_t)subseq_bits);
        if (t == 0) s_tail = -1;
        JeState carry = {seg_bit0, 0, 0};
        int carry_blocks = 0;
        for (int c0 = 0; c0 < nsub; c0 += chunk_subseqs) {
            const int n = nsub - c0 < chunk_subseqs ? nsub - c0 : chunk_subseqs;
            ++chunks_all;
            // 1: every lane its own sub-sequence
            JeState st = {JE_ERR, 0, 0};
            bool active = false;
            int cur = t;
            if (t < n) {
                const uint32_t lo = seg_bit0 + (uint32_t)(c0 + t) * (uint32_t)subseq_bits;
                const uint32_t hi = seg_end - lo > (uint32_t)subseq_bits ? lo + (uint32_t)subseq_bits : seg_end;
                if (t == 0) st = carry;
                else st.p = lo;
                if (st.p != JE_ERR) rd.seek(st.p);
                s_cnt[t] = je_run<false>(im, rd, st, hi, seg_end, 0, 0, 0, nullptr, nullptr);
                s_p[t] = st.p, s_bz[t] = (st.bi << 8) | st.z;
                active = t + 1 < n && st.p != JE_ERR;
            }
            __syncthreads();
            // 2: on into the following sub-sequences until the exit state is the stored one
            for (int round = 1; round < n; ++round) {
                if (active) {
                    const int nxt = cur + 1;
                    const uint32_t lo = seg_bit0 + (uint32_t)(c0 + nxt) * (uint32_t)subseq_bits;
                    const uint32_t hi = seg_end - lo > (uint32_t)subseq_bits ? lo + (uint32_t)subseq_bits : seg_end;
                    s_cnt[nxt] = je_run<false>(im, rd, st, hi, seg_end, 0, 0, 0, nullptr, nullptr);
                    const uint32_t bz = (st.bi << 8) | st.z;
                    if (s_p[nxt] == st.p && s_bz[nxt] == bz) active = false;
                    else s_p[nxt] = st.p, s_bz[nxt] = bz;
                    cur = nxt;
                    if (cur + 1 >= n || st.p == JE_ERR) active = false;
                }
                ++rounds_all;
                if (!__syncthreads_or(active)) break;
            }
            // 3: first block of every sub-sequence
            const int incl = je_scan(s_val, s_rst, t < n ? s_cnt[t] : 0, 0, n);
            // 4: decode again from the true entry states, writing
            if (t < n) {
                JeState en = carry;
                if (t > 0) en.p = s_p[t - 1], en.bi = s_bz[t - 1] >> 8, en.z = s_bz[t - 1] & 255;
                if (en.p != JE_ERR) {
                    const uint32_t lo = seg_bit0 + (uint32_t)(c0 + t) * (uint32_t)subseq_bits;
                    const uint32_t hi = seg_end - lo > (uint32_t)subseq_bits ? lo + (uint32_t)subseq_bits : seg_end;
                    const int blk0 = carry_blocks + incl - s_cnt[t];
                    int tail = -1;
                    rd.seek(en.p);
                    if (blk0 >= 0 && blk0 < seg_blocks) je_run<true>(im, rd, en, hi, seg_end, blk0, seg_blocks, sg.mcu0, coef, &tail);
                    if (en.p == JE_ERR) s_flag = 1;
                    if (tail >= 0) s_tail = tail;
                }
            }
            __syncthreads();
            carry.p = s_p[n - 1], carry.bi = s_bz[n - 1] >> 8, carry.z = s_bz[n - 1] & 255;
            carry_blocks += s_val[n - 1];
            __syncthreads();
            if (carry.p == JE_ERR || carry_blocks >= seg_blocks) break;  // nothing true lies behind either
        }
        __syncthreads();
        // the interval's MCUs must all be there, and less than a byte of padding behind them
        if (t == 0 && (s_tail < 0 || s_tail >= 8)) s_flag = 1;
        __syncthreads();
    }

    // DC prediction per component: a scan over its blocks in the order of the stream, restarted with every interval
    for (int c = 0; c < nc && !bad_record; ++c) {
        const int ch = sc.h[c], cv = sc.v[c], cbw = sc.blocks_w[c], hv = ch * cv;
        const int64_t items = n_mcu * hv;
        const int64_t per = (items + JE_THREADS - 1) / JE_THREADS;
        const int64_t a = (int64_t)t * per, b = a + per < items ? a + per : items;
        int16_t* plane = coef + comp_base[c];
        auto at = [&](int64_t i) -> int16_t* {
            const int64_t mcu = i / hv;
            const int sub = (int)(i - mcu * hv), vv = sub / ch, hh = sub - vv * ch;
            const int my = (int)(mcu / sc.mcus_x), mx = (int)(mcu - (int64_t)my * sc.mcus_x);
            return plane + ((int64_t)(my * cv + vv) * cbw + (mx * ch + hh)) * 64;
        };
        int sum = 0, rst = 0;
        for (int64_t i = a; i < b; ++i) {
            if (i % ((int64_t)ri * hv) == 0) sum = 0, rst = 1;
            sum += *at(i);
        }
        const int incl = je_scan(s_val, s_rst, sum, rst, JE_THREADS);
        (void)incl;
        int pred = t > 0 ? s_val[t - 1] : 0;  // what the lanes before carry in; a restart inside the run drops it
        bool out = false;
        for (int64_t i = a; i < b; ++i) {
            if (i % ((int64_t)ri * hv) == 0) pred = 0;
            int16_t* p = at(i);
            pred += *p;
            out |= pred < -32768 || pred > 32767;
            *p = (int16_t)pred;
        }
        if (out) s_flag = 1;
        __syncthreads();
    }

    // the host decoder's range checks, block by block (COL_SUM_MAX / BLOCK_SUM_MAX: see jpeg_host.h)
    for (int64_t bk = t; bk < blocks && !bad_record; bk += JE_THREADS) {
        int c = 0;
        if (nc == 3) c = bk * 64 >= comp_base[2] ? 2 : (bk * 64 >= comp_base[1] ? 1 : 0);
        const int* q = s_qt + 64 * c;
        const i32x4* p = reinterpret_cast<const i32x4*>(coef + bk * 64);
        int col[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        bool out = false;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const i32x4 v = p[r];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int lo = (int)(short)(v[e] & 0xffff) * q[8 * r + 2 * e], hi = (v[e] >> 16) * q[8 * r + 2 * e + 1];
                out |= lo < -32768 || lo > 32767 || hi < -32768 || hi > 32767;
                col[2 * e] += lo < 0 ? -lo : lo;
                col[2 * e + 1] += hi < 0 ? -hi : hi;
            }
        }
        int total = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            out |= col[i] > smjpeg::COL_SUM_MAX;
            total += col[i];
        }
        if (out || total > smjpeg::BLOCK_SUM_MAX) s_flag = 1;
    }
    __syncthreads();
    const bool flagged = s_flag != 0 || bad_record;
    if (flagged) {
        i32x4* z = reinterpret_cast<i32x4*>(coef);
        const i32x4 zero = {0, 0, 0, 0};
        for (int64_t i = t; i < blocks * 8; i += JE_THREADS) z[i] = zero;
    }
    if (t == 0) {
        status[blockIdx.x] = bad_record ? SM_EINVAL : (flagged ? SM_JPEG_UNSUPPORTED : SM_OK);
        stats[2 * blockIdx.x] = rounds_all, stats[2 * blockIdx.x + 1] = chunks_all;
    }
}

static bool params_ok(int32_t& subseq_bits, int32_t& chunk_subseqs) {
    if (subseq_bits == 0) subseq_bits = SM_JPEG_SUBSEQ_BITS_DEFAULT;
    if (chunk_subseqs == 0) chunk_subseqs = SM_JPEG_CHUNK_SUBSEQS_MAX;
    return subseq_bits >= SM_JPEG_SUBSEQ_BITS_MIN && subseq_bits <= SM_JPEG_SUBSEQ_BITS_MAX && subseq_bits % 32 == 0 && chunk_subseqs >= 1 &&
           chunk_subseqs <= SM_JPEG_CHUNK_SUBSEQS_MAX;
}

}  // namespace sm

extern "C" size_t sm_jpeg_entropy_workspace_bytes(const sm_jpeg_scan* descr_host, int32_t B, int32_t subseq_bits, int32_t chunk_subseqs) {
    if (!descr_host || B < 1 || !sm::params_ok(subseq_bits, chunk_subseqs)) {
        sm::set_error("sm_jpeg_entropy_workspace_bytes: null table, no image, or subseq_bits / chunk_subseqs out of range");
        return 0;
    }
    return ((size_t)B * 2 * sizeof(int32_t) + 15) & ~(size_t)15;
}

extern "C" int sm_jpeg_entropy_decode_batch(const sm_jpeg_scan* descr_host, const sm_jpeg_scan* descr_dev, int32_t B, const uint8_t* scans,
                                            int16_t* coef_out, int32_t* status, void* workspace, size_t workspace_bytes, int32_t subseq_bits,
                                            int32_t chunk_subseqs, void* stream) {
    SM_REQUIRE(descr_host && descr_dev && scans && coef_out && status && workspace, "sm_jpeg_entropy_decode_batch: null pointer");
    SM_REQUIRE(B > 0 && B <= 65535, "sm_jpeg_entropy_decode_batch: 1 .. 65535 images per call (got %d)", B);
    SM_REQUIRE(sm::params_ok(subseq_bits, chunk_subseqs),
               "sm_jpeg_entropy_decode_batch: subseq_bits must be 0 or a multiple of 32 in %d .. %d (at least the longest symbol, 27 bits), "
               "chunk_subseqs 0 or 1 .. %d",
               SM_JPEG_SUBSEQ_BITS_MIN, SM_JPEG_SUBSEQ_BITS_MAX, SM_JPEG_CHUNK_SUBSEQS_MAX);
    SM_REQUIRE(((uintptr_t)scans & 15) == 0 && ((uintptr_t)coef_out & 15) == 0, "sm_jpeg_entropy_decode_batch: scans and coef_out must be 16-byte aligned");
    if (workspace_bytes < (((size_t)B * 2 * sizeof(int32_t) + 15) & ~(size_t)15)) {
        sm::set_error("sm_jpeg_entropy_decode_batch: workspace of %zu bytes, sm_jpeg_entropy_workspace_bytes gives what is needed", workspace_bytes);
        return SM_ENOSPACE;
    }
    for (int b = 0; b < B; ++b) {
        const sm_jpeg_scan& s = descr_host[b];
        const char* what = nullptr;
        const int nc = s.components;
        const int64_t n_mcu = (int64_t)s.mcus_x * s.mcus_y;
        if (s.rec_off < 0 || s.rec_off % 16 || s.coef_off < 0 || s.coef_off % 16) what = "rec_off and coef_off must be non-negative multiples of 16";
        else if (nc != 1 && nc != 3) what = "1 or 3 components";
        else if (s.mcus_x < 1 || s.mcus_y < 1 || s.mcus_x > 8192 || s.mcus_y > 8192 || s.restart_interval < 0) what = "MCU grid or restart interval";
        else if (s.scan_len < 0 || s.scan_len >= SM_JPEG_MAX_SCAN_BYTES || s.rec_bytes < 0) what = "scan_len";
        if (!what) {
            const int64_t segs = s.restart_interval > 0 ? (n_mcu + s.restart_interval - 1) / s.restart_interval : 1;
            int nb = 0;
            for (int c = 0; c < nc && !what; ++c) {
                const bool luma = c == 0 && nc == 3;
                if (s.h[c] < 1 || s.v[c] < 1 || s.h[c] > (luma ? 2 : 1) || s.v[c] > (luma ? s.h[c] : 1)) what = "sampling factors";
                else if (s.blocks_w[c] != s.mcus_x * s.h[c] || s.blocks_h[c] != s.mcus_y * s.v[c]) what = "block grid does not match the MCU grid";
                else if (s.dc[c] < 0 || s.dc[c] >= s.n_huff || s.ac[c] < 0 || s.ac[c] >= s.n_huff) what = "Huffman table index";
                nb += s.h[c] * s.v[c];
            }
            if (what) {
            } else if (s.n_seg != segs) what = "n_seg does not match the restart interval";
            else if (s.n_huff < 1 || s.n_huff > sm::JE_MAX_HUFF) what = "n_huff";
            else if (n_mcu * nb >= (1 << 30)) what = "too many blocks";
            else if (s.scan_off < 0 || s.scan_off % 16 || (int64_t)s.scan_off + ((s.scan_len + 3) / 4 + 2) * 4 > s.rec_bytes) what = "scan bytes lie outside the record";
            else if (s.seg_off < 0 || s.seg_off % 16 || (int64_t)s.seg_off + segs * (int64_t)sizeof(sm_jpeg_segment) > s.rec_bytes) what = "segment table lies outside the record";
            else if (s.huff_off < 0 || s.huff_off % 16 || (int64_t)s.huff_off + (int64_t)s.n_huff * SM_JPEG_HUFF_BYTES > s.rec_bytes) what = "Huffman tables lie outside the record";
            else if (s.qt_off < 0 || s.qt_off % 16 || (int64_t)s.qt_off + 384 > s.rec_bytes) what = "quantisation tables lie outside the record";
        }
        SM_REQUIRE(!what, "sm_jpeg_entropy_decode_batch: image %d: %s", b, what);
    }
    sm::TapGuard tap(stream, "jpeg: entropy decode");
    hipLaunchKernelGGL(sm::jpeg_entropy_kernel, dim3((unsigned)B), dim3(sm::JE_THREADS), 0, (hipStream_t)stream, descr_dev, scans, coef_out, status,
                       (int32_t*)workspace, subseq_bits, chunk_subseqs);
    return sm::check_launch("sm_jpeg_entropy_decode_batch");
}
