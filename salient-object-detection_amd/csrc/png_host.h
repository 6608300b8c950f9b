// Host half of the device PNG decode: signature, IHDR and the chunk walk (plain C++, no HIP: csrc/png_decode.hip wraps it in the
// C ABI, scripts/png_host_check.cpp drives it stand-alone under the sanitizers).
//
// It reads untrusted bytes, so every read goes through a bounds check, and it DECODES NOTHING: the IDAT payloads are concatenated,
// the two-byte zlib header is validated and stripped, the stored Adler-32 is noted, and the deflate bytes travel to the device with
// at least 8 zero bytes behind them.  Whatever is not a plain 8-bit non-interlaced grey / RGB / grey + alpha / RGBA file, and
// whatever looks wrong between the chunks, ends the call with "unsupported": the caller hands the file to Pillow, so such a file
// decodes, or raises, as it does in Pillow.  An ancillary chunk is passed on its CRC alone: what is inside it is not looked at.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/selfmask_hip.h"
#include "host_common.h"

namespace smpng {

using sm::align16;

struct CrcTable {
    uint32_t t[256];
    CrcTable() {
        for (uint32_t n = 0; n < 256; ++n) {
            uint32_t c = n;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[n] = c;
        }
    }
};
inline uint32_t crc32(const uint8_t* p, size_t n) {
    static const CrcTable table;
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = table.t[(c ^ p[i]) & 255] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
inline bool is_type(const uint8_t* p, const char* name) { return memcmp(p, name, 4) == 0; }

// signature + IHDR; info is filled as far as the header could be read (0 x 0 when it is no PNG).  true: a supported header
inline bool probe(const uint8_t* p, size_t n, sm_png_info& info) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    memset(&info, 0, sizeof(info));
    if (!p || n < 8 + 12 + 13 || memcmp(p, sig, 8) != 0) return false;
    if (be32(p + 8) != 13 || !is_type(p + 12, "IHDR")) return false;
    const uint8_t* d = p + 16;
    const uint32_t w = be32(d), h = be32(d + 4);
    if (w > 0x7FFFFFFFu || h > 0x7FFFFFFFu) return false;
    info.width = (int32_t)w, info.height = (int32_t)h;
    info.bit_depth = d[8], info.colour_type = d[9], info.interlace = d[12];
    if (d[10] != 0 || d[11] != 0) return false;  // compression / filter method
    const int ct = info.colour_type;
    if (ct != 0 && ct != 2 && ct != 4 && ct != 6) return false;
    if (info.bit_depth != 8 || info.interlace != 0) return false;
    if (w < 1 || h < 1 || (uint64_t)w * h > (uint64_t)SM_PNG_MAX_PIXELS) return false;
    if (be32(d + 13) != crc32(p + 12, 4 + 13)) return false;
    info.bpp = ct == 0 ? 1 : ct == 2 ? 3 : ct == 4 ? 2 : 4;
    info.inflated_bytes = (int64_t)h * ((int64_t)w * info.bpp + 1);
    info.supported = 1;
    return true;
}

inline size_t stream_bound(const sm_png_info& info, size_t len) { return info.supported ? align16(len + 8) : 0; }

// SM_OK, SM_PNG_UNSUPPORTED or SM_ENOSPACE.  info: what probe filled (it returned true).  Two walks over the chunks: the first checks
// everything and sizes the data stream, the second copies - so a short record stays untouched
inline int prepare_stream(const uint8_t* p, size_t n, const sm_png_info& info, uint8_t* rec, size_t cap, sm_png_stream& st) {
    memset(&st, 0, sizeof(st));
    size_t pos = 8, first_idat = 0;
    uint64_t total = 0;
    bool seen_ihdr = false, in_idat = false, idat_over = false, seen_iend = false;
    while (!seen_iend) {
        if (n - pos < 12) return SM_PNG_UNSUPPORTED;  // pos <= n always
        const uint32_t len = be32(p + pos);
        if (len > 0x7FFFFFFFu || (size_t)len > n - pos - 12) return SM_PNG_UNSUPPORTED;
        const uint8_t* type = p + pos + 4;
        if (be32(p + pos + 8 + len) != crc32(type, 4 + (size_t)len)) return SM_PNG_UNSUPPORTED;
        const bool idat = is_type(type, "IDAT");
        if (in_idat && !idat) in_idat = false, idat_over = true;
        if (!seen_ihdr) {
            if (!is_type(type, "IHDR") || len != 13) return SM_PNG_UNSUPPORTED;
            seen_ihdr = true;
        } else if (is_type(type, "IHDR")) {
            return SM_PNG_UNSUPPORTED;
        } else if (idat) {
            if (idat_over) return SM_PNG_UNSUPPORTED;
            if (!in_idat && total == 0) first_idat = pos;
            in_idat = true;
            total += len;
        } else if (is_type(type, "IEND")) {
            seen_iend = true;
        } else if (is_type(type, "PLTE")) {
            if (info.colour_type == 3) return SM_PNG_UNSUPPORTED;  // a suggested palette in a colour file: Pillow ignores it too
        } else if (is_type(type, "tRNS") || is_type(type, "acTL") || is_type(type, "fcTL") || is_type(type, "fdAT")) {
            return SM_PNG_UNSUPPORTED;
        } else if (!(type[0] & 0x20)) {
            return SM_PNG_UNSUPPORTED;  // a critical chunk this reader does not know
        }
        pos += 12 + (size_t)len;
    }
    if (total < 6 || total - 6 >= (uint64_t)SM_PNG_MAX_DATA_BYTES) return SM_PNG_UNSUPPORTED;
    // the zlib wrapper (RFC 1950): the first two and the last four bytes of the stream, wherever the IDAT borders fall
    uint8_t head[2] = {0, 0}, tail[4] = {0, 0, 0, 0};
    const size_t data_len = (size_t)(total - 6), need = align16(data_len + 8);
    const bool copy = cap >= need;
    uint64_t k = 0;  // position in the concatenated stream
    for (pos = first_idat; k < total;) {
        const uint32_t len = be32(p + pos);  // checked above: these are the consecutive IDAT chunks
        const uint8_t* d = p + pos + 8;
        for (uint32_t i = 0; i < len && k + i < 2; ++i) head[k + i] = d[i];
        for (uint64_t j = k > total - 4 ? k : total - 4; j < k + len; ++j) tail[j - (total - 4)] = d[j - k];
        if (copy) {  // the part of this payload inside [2, total - 4)
            const uint64_t lo = k < 2 ? 2 : k, hi = k + len < total - 4 ? k + len : total - 4;
            if (hi > lo) memcpy(rec + (lo - 2), d + (lo - k), (size_t)(hi - lo));
        }
        k += len;
        pos += 12 + (size_t)len;
    }
    const int cmf = head[0], flg = head[1];
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) return SM_PNG_UNSUPPORTED;
    if (!copy) return SM_ENOSPACE;
    memset(rec + data_len, 0, need - data_len);
    st.data_len = (int32_t)data_len, st.rec_bytes = (int32_t)need;
    st.adler = be32(tail);
    st.H = info.height, st.W = info.width, st.colour_type = info.colour_type, st.bpp = info.bpp;
    st.inflated_bytes = (int32_t)info.inflated_bytes;  // <= 5 * 2^24
    st.magic = SM_PNG_STREAM_MAGIC;
    return SM_OK;
}

}  // namespace smpng
