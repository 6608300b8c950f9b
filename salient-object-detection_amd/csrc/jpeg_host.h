// Host half of the device JPEG decode: marker parser and baseline Huffman decoder (plain C++, no HIP: csrc/jpeg.hip wraps it
// in the C ABI, scripts/jpeg_host_check.cpp drives it stand-alone under the sanitizers).
//
// This is the only code of the library that reads untrusted bytes, so every read goes through a bounds check and the
// decoder NEVER GUESSES: whatever is not a plain single-scan baseline file, and whatever looks wrong inside one (a code that
// is in no table, a run past coefficient 63, entropy data that ends early, a marker where none belongs, bytes between the
// last MCU and EOI), ends the call with "unsupported".  The caller then hands the file to Pillow, so behaviour on every file is
// Pillow's - also on damaged ones, which libjpeg partly tolerates.
//
// Output: int16 coefficients in NATURAL (de-zigzagged, row-major 8 x 8) order, DC prediction undone, component after component,
// each component's blocks in raster order over its MCU-padded block grid; and the quantisation tables, natural order, one per
// component.  A last guard keeps the device's 32-bit IDCT inside the range where it, libjpeg's C code (64-bit long) and
// libjpeg-turbo's SIMD code (16-bit dequantisation and pass-1 workspace) are the same function - see COL_SUM_MAX.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/selfmask_hip.h"
#include "host_common.h"

// what the device's entropy decoder (csrc/jpeg_entropy.hip) shares with the host's compiles for both
#if defined(__HIPCC__)
#define SMJPEG_HD __host__ __device__ __forceinline__
#else
#define SMJPEG_HD inline
#endif

namespace smjpeg {

using sm::align16;

constexpr int FAST_BITS = 9;
constexpr int MAX_DIM = 65500;  // libjpeg's JPEG_MAX_DIMENSION

static const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// One Huffman table, in the form both decoders walk: prepare_scan sends it to the device whole (SM_JPEG_HUFF_BYTES each)
struct HuffTable {
    uint16_t fast[1 << FAST_BITS];  // (length << 8) | symbol for codes of at most FAST_BITS bits, 0 = longer / none
    int32_t maxcode[17];            // largest code of each length, -1 = none; [0] = -1: lengths start at 1
    int32_t valoff[17];             // index of the first symbol of a length minus its first code; [0] = 0
    uint8_t vals[256];
};
static_assert(sizeof(HuffTable) == SM_JPEG_HUFF_BYTES, "sm_jpeg_scan's table size");

struct Huff : HuffTable {
    bool defined;
};

struct Component {
    int id, h, v, tq, td, ta;
};

struct Frame {
    sm_jpeg_info info;
    Component comp[3];
    uint16_t qt[4][64];  // natural order
    bool qt_defined[4];
    Huff dc[4], ac[4];
    bool have_sof, adobe;
    int adobe_transform;
    int restart_interval;
    size_t scan_pos;  // first byte of entropy-coded data
};

// counts[1..16] codes per length, vals: the symbols in code order.  false: not a prefix code libjpeg would accept
inline bool build_huff(Huff& h, const uint8_t* counts, const uint8_t* vals, int nvals) {
    memset(h.fast, 0, sizeof(h.fast));
    memset(h.vals, 0, sizeof(h.vals));  // the table travels to the device whole (prepare_scan): no byte of it is left undefined
    memcpy(h.vals, vals, (size_t)nvals);
    h.maxcode[0] = -1, h.valoff[0] = 0;
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = counts[l - 1];
        h.valoff[l] = k - code;
        for (int i = 0; i < n; ++i, ++k, ++code) {
            if (l <= FAST_BITS) {
                const int lo = code << (FAST_BITS - l);
                if (lo + (1 << (FAST_BITS - l)) > (1 << FAST_BITS)) return false;
                for (int j = 0; j < (1 << (FAST_BITS - l)); ++j) h.fast[lo + j] = (uint16_t)((l << 8) | vals[k]);
            }
        }
        if (code >= (1 << l)) return false;  // jpeg_make_d_derived_tbl's check
        h.maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
    h.defined = true;
    return true;
}

struct Bits {
    const uint8_t* p;
    size_t pos, end;
    uint64_t buf;  // the next bits of the stream, most significant first
    int cnt;       // valid bits in buf
    int fake;      // zero bits appended after the data ran into a marker or the end of the buffer
    bool stopped;

    void reset(size_t at) { pos = at, buf = 0, cnt = 0, fake = 0, stopped = false; }

    inline void fill() {
        while (cnt <= 56) {
            if (!stopped && cnt <= 32 && pos + 4 <= end) {  // four bytes at once when none of them is 0xFF
                const uint32_t w = ((uint32_t)p[pos] << 24) | ((uint32_t)p[pos + 1] << 16) | ((uint32_t)p[pos + 2] << 8) | p[pos + 3];
                const uint32_t nw = ~w;
                if (!((nw - 0x01010101u) & ~nw & 0x80808080u)) {
                    buf |= (uint64_t)w << (32 - cnt);
                    cnt += 32;
                    pos += 4;
                    continue;
                }
            }
            if (!stopped && pos < end) {
                const uint8_t b = p[pos];
                if (b == 0xFF) {
                    if (pos + 1 < end && p[pos + 1] == 0x00) {
                        pos += 2;  // a stuffed 0xFF data byte
                    } else {
                        stopped = true;  // a marker (or the buffer's last byte): pos stays on its 0xFF
                        continue;
                    }
                } else {
                    pos += 1;
                }
                buf |= (uint64_t)b << (56 - cnt);
                cnt += 8;
            } else {
                stopped = true;
                fake += 8;
                cnt += 8;
            }
        }
    }
    inline uint32_t peek(int n) const { return (uint32_t)(buf >> (64 - n)); }
    inline void drop(int n) { buf <<= n, cnt -= n; }
    bool used_fake_bits() const { return cnt < fake; }
    int real_bits_left() const { return cnt - fake; }
};

// One symbol's code on the next 32 bits of the stream, most significant first: -> the symbol, len = the code's length (0: no code of
// up to 16 bits matches).  THE table walk: the host decoder and the device's kernel both decode with it.  The codes behind the fast
// table first, on their own: the host decoder reads the fast table with its own 9-bit peek and comes here for the rest.
SMJPEG_HD int huff_lookup_long(const HuffTable& h, uint32_t bits, int& len) {
    for (int l = FAST_BITS + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)(bits >> (32 - l));
        if (code <= h.maxcode[l]) {
            const int i = code + h.valoff[l];
            if (i < 0 || i > 255) break;
            len = l;
            return h.vals[i];
        }
    }
    len = 0;
    return 0;
}

SMJPEG_HD int huff_lookup(const HuffTable& h, uint32_t bits, int& len) {
    const uint32_t e = h.fast[bits >> (32 - FAST_BITS)];
    if (e) {
        len = (int)(e >> 8);
        return (int)(e & 255);
    }
    return huff_lookup_long(h, bits, len);
}

// the value of the s >= 1 bits `raw` that follow a symbol (T.81 F.2.2.1 EXTEND)
SMJPEG_HD int extend(int raw, int s) { return raw < (1 << (s - 1)) ? raw - (1 << s) + 1 : raw; }

// one Huffman symbol, or -1 (no code).  A fast-table hit returns at once - through huff_lookup the host decoder measured 5 - 9 % slower
// on one thread - and the long codes go through the shared walk: decode_scan refills below 32 valid bits, so 32 bits, fake zeros
// included, are there to peek
inline int decode_symbol(Bits& b, const Huff& h) {
    const uint16_t e = h.fast[b.peek(FAST_BITS)];
    if (e) {
        b.drop(e >> 8);
        return e & 255;
    }
    int len;
    const int sym = huff_lookup_long(h, b.peek(32), len);
    if (!len) return -1;
    b.drop(len);
    return sym;
}

inline int receive_extend(Bits& b, int s) {
    const int v = (int)b.peek(s);
    b.drop(s);
    return extend(v, s);
}

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Markers up to and including SOS.  Returns true when the file is one the device path takes; info is filled as far as the
// header could be read either way (width / height / components of any SOFn frame).
inline bool parse_headers(const uint8_t* p, size_t n, Frame& f) {
    memset(&f.info, 0, sizeof(f.info));
    memset(f.qt_defined, 0, sizeof(f.qt_defined));
    for (int i = 0; i < 4; ++i) f.dc[i].defined = f.ac[i].defined = false;
    f.have_sof = f.adobe = false;
    f.adobe_transform = -1;
    f.restart_interval = 0;
    f.scan_pos = 0;
    if (!p || n < 4 || p[0] != 0xFF || p[1] != 0xD8) return false;
    size_t pos = 2;
    for (;;) {
        if (pos >= n || p[pos] != 0xFF) return false;  // libjpeg would resynchronise: not ours to guess
        while (pos < n && p[pos] == 0xFF) ++pos;       // fill bytes
        if (pos >= n) return false;
        const int m = p[pos++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return false;  // stuffing, TEM, RSTn, SOI, EOI before a scan
        if (pos + 2 > n) return false;
        const int L = be16(p + pos);
        if (L < 2 || pos + (size_t)L > n) return false;
        const uint8_t* d = p + pos + 2;
        const int dl = L - 2;
        pos += (size_t)L;
        if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {  // SOFn
            if (f.have_sof || dl < 6) return false;
            f.have_sof = true;
            const int prec = d[0], nc = d[5];
            f.info.height = be16(d + 1);
            f.info.width = be16(d + 3);
            f.info.components = nc;
            if (dl != 6 + 3 * nc) return false;
            for (int c = 0; c < nc && c < 4; ++c) {
                f.info.h_samp[c] = d[7 + 3 * c] >> 4;
                f.info.v_samp[c] = d[7 + 3 * c] & 15;
            }
            if (m != 0xC0 || prec != 8 || (nc != 1 && nc != 3)) return false;  // progressive, arithmetic, 12-bit, CMYK / YCCK, ...
            if (f.info.width < 1 || f.info.height < 1 || f.info.width > MAX_DIM || f.info.height > MAX_DIM) return false;
            for (int c = 0; c < nc; ++c) {
                Component& k = f.comp[c];
                k.id = d[6 + 3 * c], k.h = d[7 + 3 * c] >> 4, k.v = d[7 + 3 * c] & 15, k.tq = d[8 + 3 * c];
                if (k.tq > 3) return false;
            }
            int sampling;
            if (nc == 1) {
                if (f.comp[0].h != 1 || f.comp[0].v != 1) return false;  // a lone component is never interleaved: other MCU rules
                sampling = SM_JPEG_GRAY;
            } else {
                if (f.comp[1].h != 1 || f.comp[1].v != 1 || f.comp[2].h != 1 || f.comp[2].v != 1) return false;
                const int h = f.comp[0].h, v = f.comp[0].v;
                if (h == 1 && v == 1) sampling = SM_JPEG_444;
                else if (h == 2 && v == 1) sampling = SM_JPEG_422;
                else if (h == 2 && v == 2) sampling = SM_JPEG_420;
                else return false;
                if (f.comp[0].id == 'R' && f.comp[1].id == 'G' && f.comp[2].id == 'B') return false;  // libjpeg: RGB, no transform
            }
            f.info.sampling = sampling;
            const int hmax = f.comp[0].h, vmax = f.comp[0].v;
            const int mx = (f.info.width + 8 * hmax - 1) / (8 * hmax), my = (f.info.height + 8 * vmax - 1) / (8 * vmax);
            f.info.mcus_x = mx, f.info.mcus_y = my;
            int64_t blocks = 0;
            for (int c = 0; c < nc; ++c) {
                f.info.blocks_w[c] = mx * f.comp[c].h;
                f.info.blocks_h[c] = my * f.comp[c].v;
                blocks += (int64_t)f.info.blocks_w[c] * f.info.blocks_h[c];
            }
            f.info.coef_bytes = blocks * 128;
        } else if (m == 0xC4) {  // DHT
            int o = 0;
            while (o < dl) {
                if (o + 17 > dl) return false;
                const int tc = d[o] >> 4, th = d[o] & 15;
                if (tc > 1 || th > 3) return false;
                int nv = 0;
                for (int i = 0; i < 16; ++i) nv += d[o + 1 + i];
                if (nv > 256 || o + 17 + nv > dl) return false;
                Huff& h = tc ? f.ac[th] : f.dc[th];
                h.defined = false;
                if (!build_huff(h, d + o + 1, d + o + 17, nv)) return false;
                o += 17 + nv;
            }
        } else if (m == 0xDB) {  // DQT
            int o = 0;
            while (o < dl) {
                const int pq = d[o] >> 4, tq = d[o] & 15;
                if (pq > 1 || tq > 3) return false;
                const int need = 1 + 64 * (pq + 1);
                if (o + need > dl) return false;
                for (int i = 0; i < 64; ++i) f.qt[tq][ZIGZAG[i]] = (uint16_t)(pq ? be16(d + o + 1 + 2 * i) : d[o + 1 + i]);
                f.qt_defined[tq] = true;
                o += need;
            }
        } else if (m == 0xDD) {  // DRI
            if (dl != 2) return false;
            f.restart_interval = be16(d);
        } else if (m == 0xEE) {
            if (dl >= 12 && !memcmp(d, "Adobe", 5)) f.adobe = true, f.adobe_transform = d[11];
        } else if (m == 0xDA) {  // SOS
            if (!f.have_sof) return false;
            const int nc = f.info.components;
            if (dl != 4 + 2 * nc || d[0] != nc) return false;  // several scans: one component each
            for (int c = 0; c < nc; ++c) {
                Component& k = f.comp[c];
                if (d[1 + 2 * c] != k.id) return false;  // scan order = frame order
                k.td = d[2 + 2 * c] >> 4, k.ta = d[2 + 2 * c] & 15;
                if (k.td > 3 || k.ta > 3 || !f.dc[k.td].defined || !f.ac[k.ta].defined || !f.qt_defined[k.tq]) return false;
            }
            if (d[1 + 2 * nc] != 0 || d[2 + 2 * nc] != 63 || d[3 + 2 * nc] != 0) return false;
            if (nc == 3 && f.adobe && f.adobe_transform != 1) return false;  // Adobe RGB (0) or an unknown transform
            f.info.restart_interval = f.restart_interval;
            f.scan_pos = pos;
            f.info.supported = 1;
            return true;
        } else if (m == 0xFE || (m >= 0xE0 && m <= 0xEF)) {
            // COM, APPn: skipped
        } else {
            return false;  // DNL, DHP, EXP, DAC, JPGn, reserved
        }
    }
}

// The device computes the IDCT in 32-bit integers; libjpeg's C code uses 64-bit longs, libjpeg-turbo's SIMD code 16-bit
// dequantised values and a 16-bit pass-1 workspace (saturating).  The three agree while nothing overflows:
//   * every dequantised value fits int16;
//   * pass 1: an output is sum_i g_i v_i / 2^11 over the column's inputs with |g_i| <= 8192 sqrt(2) cos(..) < 11400, so a column
//     whose |v| sum to at most 5800 gives |ws| <= 5.57 * 5800 + 1 < 32767; its 32-bit intermediates stay below 5800 * 4 * 25172;
//   * pass 2: no intermediate collects more than 33000 (the constants one input meets, absolute values summed) per unit of
//     input, the inputs of a row sum to at most 5.57 * sum|v| + 8: a block whose |v| sum to at most 11000 stays below 2^31.
// The forward DCT of any 8 x 8 block of 8-bit samples has column sums <= sqrt(8) * 1024 and a block sum <= 8192 before
// quantisation, so what an encoder writes passes; blocks that do not are left to Pillow.
constexpr int COL_SUM_MAX = 5800, BLOCK_SUM_MAX = 11000;

// Entropy-coded segment of the one interleaved scan.  true: all MCUs decoded and EOI follows directly.
inline bool decode_scan(const uint8_t* p, size_t n, Frame& f, int16_t* coef) {
    const sm_jpeg_info& in = f.info;
    const int nc = in.components;
    int16_t* base[3];
    int64_t off = 0;
    for (int c = 0; c < nc; ++c) {
        base[c] = coef + off;
        off += (int64_t)in.blocks_w[c] * in.blocks_h[c] * 64;
    }
    memset(coef, 0, (size_t)off * sizeof(int16_t));
    Bits b;
    b.p = p, b.end = n;
    b.reset(f.scan_pos);
    int pred[3] = {0, 0, 0};
    const int ri = f.restart_interval;
    int next_rst = 0;
    const int64_t n_mcu = (int64_t)in.mcus_x * in.mcus_y;
    int mxi = 0, myi = 0;
    for (int64_t mcu = 0; mcu < n_mcu; ++mcu) {
        if (ri && mcu && mcu % ri == 0) {
            // the interval must have ended inside its own data, with less than a byte of padding, right in front of RSTn
            if (b.used_fake_bits() || b.real_bits_left() >= 8) return false;
            size_t q = b.pos;
            if (q >= n || p[q] != 0xFF) return false;
            while (q < n && p[q] == 0xFF) ++q;
            if (q >= n || p[q] != 0xD0 + next_rst) return false;
            next_rst = (next_rst + 1) & 7;
            b.reset(q + 1);
            pred[0] = pred[1] = pred[2] = 0;
        }
        for (int c = 0; c < nc; ++c) {
            const Component& k = f.comp[c];
            const Huff &hd = f.dc[k.td], &ha = f.ac[k.ta];
            const uint16_t* qt = f.qt[k.tq];
            for (int vv = 0; vv < k.v; ++vv)
                for (int hh = 0; hh < k.h; ++hh) {
                    int16_t* blk = base[c] + ((int64_t)(myi * k.v + vv) * in.blocks_w[c] + (mxi * k.h + hh)) * 64;
                    int colsum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    if (b.cnt < 32) b.fill();
                    int s = decode_symbol(b, hd);
                    if (s < 0 || s > 11) return false;
                    if (s) pred[c] += receive_extend(b, s);
                    if (pred[c] < -32768 || pred[c] > 32767) return false;
                    blk[0] = (int16_t)pred[c];
                    {
                        const int v = pred[c] * (int)qt[0];
                        if (v < -32768 || v > 32767) return false;
                        colsum[0] = v < 0 ? -v : v;
                    }
                    for (int kk = 1; kk < 64;) {
                        if (b.cnt < 32) b.fill();
                        const int rs = decode_symbol(b, ha);
                        if (rs < 0) return false;
                        const int r = rs >> 4;
                        s = rs & 15;
                        if (s == 0) {
                            if (r == 15) {
                                kk += 16;
                                if (kk > 64) return false;
                                continue;
                            }
                            if (r != 0) return false;  // EOBn belongs to progressive scans
                            break;
                        }
                        kk += r;
                        if (kk > 63 || s > 10) return false;
                        const int cv = receive_extend(b, s);
                        const int nat = ZIGZAG[kk++];
                        blk[nat] = (int16_t)cv;
                        const int v = cv * (int)qt[nat];
                        if (v < -32768 || v > 32767) return false;
                        colsum[nat & 7] += v < 0 ? -v : v;
                    }
                    int total = 0;
                    for (int i = 0; i < 8; ++i) {
                        if (colsum[i] > COL_SUM_MAX) return false;
                        total += colsum[i];
                    }
                    if (total > BLOCK_SUM_MAX) return false;
                }
        }
        if (b.used_fake_bits()) return false;  // the data ended inside this MCU: stop here, whatever the header promised
        if (++mxi == in.mcus_x) mxi = 0, ++myi;
    }
    if (b.used_fake_bits() || b.real_bits_left() >= 8) return false;
    size_t q = b.pos;
    if (q >= n || p[q] != 0xFF) return false;
    while (q < n && p[q] == 0xFF) ++q;
    return q < n && p[q] == 0xD9;  // EOI: one scan, nothing after it
}

inline void write_tables(const Frame& f, uint16_t* qt_out) {
    for (int c = 0; c < f.info.components; ++c) memcpy(qt_out + 64 * c, f.qt[f.comp[c].tq], 64 * sizeof(uint16_t));
}

// ---- preparation of a scan for the device's entropy decoder (csrc/jpeg_entropy.hip): no Huffman decoding here ---------------------
// restart intervals the header implies; 0 when the header is not one parse_headers accepted
inline int64_t scan_segments(const sm_jpeg_info& in) {
    const int64_t n_mcu = (int64_t)in.mcus_x * in.mcus_y;
    if (!in.supported || n_mcu < 1) return 0;
    return in.restart_interval > 0 ? (n_mcu + in.restart_interval - 1) / in.restart_interval : 1;
}

// bytes of everything in a record but the scan bytes, for `segs` table entries
inline size_t record_fixed_bytes(int64_t segs) { return align16((size_t)segs * sizeof(sm_jpeg_segment)) + align16(6 * sizeof(HuffTable)) + 384; }

inline size_t scan_bound(const sm_jpeg_info& in, size_t len) {
    int64_t segs = scan_segments(in);
    if (segs > (int64_t)(len / 2) + 1) segs = (int64_t)(len / 2) + 1;  // every interval but the last ends in a two-byte marker
    return record_fixed_bytes(segs) + align16(len + 8);
}

// SM_OK, SM_JPEG_UNSUPPORTED or SM_ENOSPACE.  f: what parse_headers filled (it returned true).  Record layout:
// [segment table | Huffman tables | quantisation tables | unstuffed scan bytes + >= 8 zero bytes].
inline int prepare_scan(const uint8_t* p, size_t n, const Frame& f, uint8_t* rec, size_t cap, sm_jpeg_scan& sc) {
    const sm_jpeg_info& in = f.info;
    memset(&sc, 0, sizeof(sc));
    const int nc = in.components;
    const int64_t n_mcu = (int64_t)in.mcus_x * in.mcus_y, segs = scan_segments(in);
    const size_t raw = n - f.scan_pos;  // parse_headers: scan_pos <= n
    if (segs < 1 || (size_t)(segs - 1) > raw / 2 || raw >= (size_t)SM_JPEG_MAX_SCAN_BYTES) return SM_JPEG_UNSUPPORTED;
    // the tables the components name, each once
    int n_huff = 0, slot_dc[4] = {-1, -1, -1, -1}, slot_ac[4] = {-1, -1, -1, -1};
    for (int c = 0; c < nc; ++c) {
        if (slot_dc[f.comp[c].td] < 0) slot_dc[f.comp[c].td] = n_huff++;
        if (slot_ac[f.comp[c].ta] < 0) slot_ac[f.comp[c].ta] = n_huff++;
    }
    const size_t seg_at = 0, huff_at = align16((size_t)segs * sizeof(sm_jpeg_segment)), qt_at = huff_at + align16((size_t)n_huff * sizeof(HuffTable)),
                 scan_at = qt_at + 384;
    if ((uint64_t)scan_at + align16(raw + 8) >= ((uint64_t)1 << 31)) return SM_JPEG_UNSUPPORTED;  // the record's offsets are 32-bit
    if (cap < scan_at + align16(raw + 8)) return SM_ENOSPACE;
    memset(rec + huff_at, 0, qt_at - huff_at);
    for (int t = 0; t < 4; ++t)
        for (int k = 0; k < 2; ++k) {
            const int slot = k ? slot_ac[t] : slot_dc[t];
            if (slot < 0) continue;
            const HuffTable& h = k ? f.ac[t] : f.dc[t];
            memcpy(rec + huff_at + (size_t)slot * sizeof(HuffTable), &h, sizeof(HuffTable));
        }
    memset(rec + qt_at, 0, 384);
    for (int c = 0; c < nc; ++c) memcpy(rec + qt_at + 128 * c, f.qt[f.comp[c].tq], 128);
    // one pass: runs between 0xFF bytes are copied, FF 00 becomes FF, anything else behind an FF ends the interval
    uint8_t* dst = rec + scan_at;
    size_t pos = f.scan_pos, w = 0, seg_start = 0;
    const int64_t ri = in.restart_interval > 0 ? in.restart_interval : n_mcu;
    for (int64_t k = 0;;) {
        const uint8_t* q = pos < n ? (const uint8_t*)memchr(p + pos, 0xFF, n - pos) : nullptr;
        const size_t run = q ? (size_t)(q - (p + pos)) : n - pos;
        memcpy(dst + w, p + pos, run);  // w + run <= raw: the copy never outruns what it read
        w += run, pos += run;
        if (!q) return SM_JPEG_UNSUPPORTED;  // the file ends inside the scan
        if (pos + 1 < n && p[pos + 1] == 0x00) {
            dst[w++] = 0xFF;
            pos += 2;
            continue;
        }
        size_t t = pos;
        while (t < n && p[t] == 0xFF) ++t;  // fill bytes
        if (t >= n) return SM_JPEG_UNSUPPORTED;
        sm_jpeg_segment s;
        s.byte_off = (int32_t)seg_start, s.byte_len = (int32_t)(w - seg_start);
        s.mcu0 = (int32_t)(k * ri), s.mcus = (int32_t)(n_mcu - k * ri < ri ? n_mcu - k * ri : ri);
        memcpy(rec + seg_at + (size_t)k * sizeof(s), &s, sizeof(s));
        if (k == segs - 1) {
            if (p[t] != 0xD9) return SM_JPEG_UNSUPPORTED;  // EOI belongs here and nothing else
            break;
        }
        if (p[t] != 0xD0 + (int)(k & 7)) return SM_JPEG_UNSUPPORTED;
        ++k, seg_start = w, pos = t + 1;
    }
    memset(dst + w, 0, align16(w + 8) - w);
    sc.scan_off = (int32_t)scan_at, sc.scan_len = (int32_t)w;
    sc.seg_off = (int32_t)seg_at, sc.n_seg = (int32_t)segs;
    sc.huff_off = (int32_t)huff_at, sc.n_huff = n_huff;
    sc.qt_off = (int32_t)qt_at;
    sc.rec_bytes = (int32_t)(scan_at + align16(w + 8));
    sc.components = nc, sc.mcus_x = in.mcus_x, sc.mcus_y = in.mcus_y, sc.restart_interval = in.restart_interval;
    for (int c = 0; c < nc; ++c) {
        sc.blocks_w[c] = in.blocks_w[c], sc.blocks_h[c] = in.blocks_h[c];
        sc.h[c] = f.comp[c].h, sc.v[c] = f.comp[c].v;
        sc.td[c] = f.comp[c].td, sc.ta[c] = f.comp[c].ta;
        sc.dc[c] = slot_dc[f.comp[c].td], sc.ac[c] = slot_ac[f.comp[c].ta];
    }
    return SM_OK;
}

}  // namespace smjpeg
