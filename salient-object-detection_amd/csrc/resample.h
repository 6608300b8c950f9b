// Pillow's 8-bit two-pass resampler (libImaging/Resample.c: ImagingResample) on the device, the part every kernel shares:
// the fixed-point format, the clip, and the read of one output element's taps from the host's table
// (selfmask_amd/resample.py: pil_coeffs, laid out by CoefTable).  preprocess.hip applies it to RGB with the BILINEAR filter,
// present.hip to one band with LANCZOS; the tap loops stay in their kernels, where the data lives.
#pragma once
#include "common.h"

namespace sm {

constexpr int RS_PRECISION_BITS = 32 - 8 - 2;          // Pillow: PRECISION_BITS
constexpr int RS_HALF = 1 << (RS_PRECISION_BITS - 1);  // an accumulator starts here: the shift rounds to nearest

// clip8 of Resample.c on an accumulator: for a kernel that stores each result as a byte of its own (preprocess.hip)
__device__ __forceinline__ int rs_clip8_plain(int v) {
    v >>= RS_PRECISION_BITS;  // arithmetic shift, as the C code's table index
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// ... for a kernel that packs results into the bytes of a word (present.hip).  The empty asm keeps the clipped value opaque: left to
// itself hipcc fuses two shift-and-clip results that are packed into neighbouring bytes into one v_ashr_pk_u8_i32 and ORs further bytes
// on top as if the instruction had cleared bits 16-31 of its destination, which gfx950 leaves as they were (seen on the MI355X: bytes 0
// and 1 of a packed group right, 2 and 3 ORed with stale register bits).  The RGB resize keeps the plain clip: its three
// byte stores compile to v_med3_i32 per channel and a 16-bit merge of two of them, no v_ashr_pk_u8_i32 (checked in the ISA; the bytes are
// Pillow's in every test), and the opaque values cost it 4 % (62.4 against the plain clip's 60.4 us for both launches at B = 64,
// 350 x 350 -> 224: profiles/resample_refactor_ab.log).  A change of its stores that packs bytes into a word needs rs_clip8.
__device__ __forceinline__ int rs_clip8(int v) {
    v = rs_clip8_plain(v);
    asm volatile("" : "+v"(v));
    return v;
}

// The taps of output element i of a pass from n_in to n_out elements: out[i] = clip8(RS_HALF + sum_j in[first + j] * k[j], j < n).
// A pass the host marked as skipped (ks = 0: n_in == n_out) has k == nullptr and out[i] = in[first].
struct RsTaps {
    const int* k;
    int first, n;
};

// coef + coef_off: [n_out][2] bounds (first input index, tap count), then [n_out][ks] taps.  first is clamped into [0, n_in] and n
// into [0, min(ks, n_in - first)]: nothing is read past the row or column, whatever the table holds (a table that lives on the
// device alone is never seen by the host's checks).
__device__ __forceinline__ RsTaps rs_taps(const int* __restrict__ coef, int coef_off, int ks, int n_out, int n_in, int i) {
    RsTaps t;
    if (ks == 0) {
        t.k = nullptr;
        t.first = i < n_in ? i : n_in - 1;
        t.n = 0;
        return t;
    }
    const int* __restrict__ cb = coef + coef_off;
    int first = cb[2 * i], n = cb[2 * i + 1];
    first = first < 0 ? 0 : (first > n_in ? n_in : first);
    n = n < n_in - first ? n : n_in - first;
    n = n < ks ? n : ks;
    t.k = cb + 2 * (int64_t)n_out + (int64_t)i * ks;
    t.first = first;
    t.n = n;
    return t;
}

}  // namespace sm
