// Salient objects from run codes: the connected components of a run-coded mask with their boxes, areas, centroids and scores,
// found on the runs themselves - a few thousand items per image - without touching a pixel plane.
//
// The input is what the predictor's finish leaves on the device (predict.hip): ascending column-major run boundaries
// q = x H + y per image and info = {count, pixel 0}.  One workgroup per image:
//   O1  segments     a foreground run is cut at every column end it crosses: a table of vertical segments (q, length), ascending
//                    by construction; offsets from a workgroup prefix sum over per-run segment counts
//   O2  union        segment i of column x is joined to the segments of column x - 1 whose rows overlap its own (widened by one
//                    row at connectivity 8): binary search for the first candidate, then a walk; union-find with atomicMin on the
//                    parents (as uf_union in bilateral.hip): parents only decrease, so every loop is bounded
//   O3  rank         area and first raster pixel per root by integer atomics; K rounds of "largest (area, -first) below the
//                    previous one" pick the objects in order (as bs_post_best / bs_post_second)
//   O4  statistics   box and coordinate sums of the kept objects by integer atomics in LDS; the whole mask's box alongside
// and, when the low-resolution mask is given, a second launch spread over many workgroups:
//   O5  mass         one wave per kept segment walks its pixels and sums their 8-bit soft values (upsample.h: the bits
//                    predict_planes_kernel stores); per-object sums by 64-bit integer atomics
// Everything is an integer accumulated by commutative atomics, so the output is a function of the input alone.
// The tables of an image live in LDS when its segment bound fits OB_LDS_SEGS and in the caller's workspace otherwise: the same
// code runs against either (the STAGED pattern of predict.hip).
#include "common.h"

#pragma clang fp contract(off)
#include "upsample.h"

namespace sm {

constexpr int OB_THREADS = 256;
constexpr int OB_WAVES = OB_THREADS / 64;
constexpr int OB_LDS_SEGS = 3072;       // five int tables of this length: 60 KiB of the 64 KiB a workgroup gets without opt-in
constexpr int OB_MAX_OBJECTS = SM_OBJ_MAX_OBJECTS;
constexpr int OB_MAX_WIDTH = SM_OBJ_MAX_WIDTH;
constexpr int OB_MAX_PIXELS = 1 << 22;  // as the run kernels
constexpr int OB_NONE = 0x7fffffff;
constexpr int OB_MASS_BLOCKS = 256;     // workgroups per image of the mass launch, at most

constexpr int OB_WIDE_RUN = 8;          // a run of more segments than this is emitted by its whole wave

// rows of an image's segment table: the bound ceil(count / 2) + W at count = cap and the widest image (sm_mask_objects_seg_cap)
__host__ __device__ __forceinline__ int ob_seg_cap(int cap, int max_width) { return (cap + 1) / 2 + max_width; }

// tables modified by atomics are read through the L2 as well (the global path; in LDS this is a plain read)
__device__ __forceinline__ int ob_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ob_sync() {
    __threadfence();
    __syncthreads();
}

__device__ __forceinline__ int ob_find(int* parent, int i) {
    int p;
    while ((p = ob_load(&parent[i])) != i) i = p;
    return i;
}
__device__ __forceinline__ void ob_union(int* parent, int a, int b) {
    for (;;) {
        a = ob_find(parent, a);
        b = ob_find(parent, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }  // a < b: hang b under a
        const int old = atomicMin(&parent[b], a);
        if (old == b) return;
        b = old;
    }
}

__device__ __forceinline__ int ob_wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

struct ObShared {  // the workgroup's small state
    int wsum[OB_WAVES];
    unsigned long long wkey[OB_WAVES];
    int widx[OB_WAVES];
    int ncomp;
    int root[OB_MAX_OBJECTS], area[OB_MAX_OBJECTS], first[OB_MAX_OBJECTS];
    int x0[OB_MAX_OBJECTS + 1], y0[OB_MAX_OBJECTS + 1], x1[OB_MAX_OBJECTS + 1], y1[OB_MAX_OBJECTS + 1];  // [OB_MAX_OBJECTS]: the whole mask
    unsigned long long sum_x[OB_MAX_OBJECTS], sum_y[OB_MAX_OBJECTS];
    int mask_area;
};

// boundary i of the run list with its two implied ends
__device__ __forceinline__ int ob_bound(const int* __restrict__ starts, int n, int npx, int i) {
    if (i < 0) return 0;
    if (i >= n) return npx;
    const int q = starts[i];
    return q < 0 ? 0 : (q > npx ? npx : q);
}

// row i of the tables: the part of run [s, e) that lies in column x (nothing is written past the S rows of the tables)
__device__ __forceinline__ void ob_emit(int* Q, int* L, int* P, int* A, int* F, int S, int H, int s, int e, int x, int i) {
    if (i < 0 || i >= S) return;
    const int lo = x * H, hi = lo + H;
    const int q = s > lo ? s : lo;
    Q[i] = q;
    L[i] = (e < hi ? e : hi) - q;
    P[i] = i;
    A[i] = 0;
    F[i] = OB_NONE;
}

// O1 - O4 of one image against tables Q (segment start), L (length), P (parent), A (area per root, then rank per root), F (first
// pixel per root, then rank per segment), each of S entries.  Returns the segment count, or -1 when the table would not hold them.
__device__ __forceinline__ int ob_components(const sm_objects_args& a, ObShared& sh, int b, int H, int W, int n, int p0, int* Q, int* L,
                                             int* P, int* A, int* F, int S) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int npx = H * W;
    const int* __restrict__ starts = a.starts + (int64_t)b * a.cap;
    // ---- O1: segments ----
    const int nf = (n + 1 + p0) / 2;  // foreground runs: run j spans [bound(2j - p0), bound(2j + 1 - p0))
    int nseg = 0;
    for (int base = 0; base < nf; base += OB_THREADS) {
        const int j = base + tid;
        int s = 0, e = 0, xs = 0, cnt = 0;
        if (j < nf) {
            s = ob_bound(starts, n, npx, 2 * j - p0);
            e = ob_bound(starts, n, npx, 2 * j + 1 - p0);
            if (e > s) {
                xs = s / H;
                cnt = (e - 1) / H - xs + 1;
            }
        }
        const int incl = ob_wave_incl_scan(cnt, lane);
        if (lane == 63) sh.wsum[wv] = incl;
        __syncthreads();
        int off = nseg + incl - cnt, total = 0;
#pragma unroll
        for (int w = 0; w < OB_WAVES; ++w) {
            off += w < wv ? sh.wsum[w] : 0;
            total += sh.wsum[w];
        }
        __syncthreads();
        // a run of a few segments is emitted by its own lane; one that crosses many columns (an all-ones plane is ONE run of W
        // segments) by the 64 lanes of its wave, one such run after the other
        const bool wide = cnt > OB_WIDE_RUN;
        if (!wide)
            for (int t = 0; t < cnt; ++t) ob_emit(Q, L, P, A, F, S, H, s, e, xs + t, off + t);
        for (unsigned long long todo = __ballot(wide); todo; todo &= todo - 1) {
            const int from = __ffsll((long long)todo) - 1;
            const int rs = __shfl(s, from, 64), re = __shfl(e, from, 64), rx = __shfl(xs, from, 64), rn = __shfl(cnt, from, 64),
                      ro = __shfl(off, from, 64);
            for (int t = lane; t < rn; t += 64) ob_emit(Q, L, P, A, F, S, H, rs, re, rx + t, ro + t);
        }
        nseg += total;
        if (nseg > S || nseg < 0) return -1;  // (only a run list that is not ascending gets here; uniform over the workgroup)
    }
    ob_sync();
    // ---- O2: union with the overlapping segments of the column before ----
    const int widen = a.connectivity == 8 ? 1 : 0;
    for (int i = tid; i < nseg; i += OB_THREADS) {
        const int q = Q[i], x = q / H;
        if (x == 0) continue;
        const int y0 = q - x * H, y1 = y0 + L[i] - 1;
        const int colq = (x - 1) * H;
        const int lo_q = colq + (y0 - widen > 0 ? y0 - widen : 0), hi_q = colq + (y1 + widen < H - 1 ? y1 + widen : H - 1);
        int l = 0, r = i;  // the first segment that ends past lo_q: ends ascend as starts do
        while (l < r) {
            const int m = (l + r) >> 1;
            if (Q[m] + L[m] > lo_q) r = m; else l = m + 1;
        }
        for (int j = l; j < i && Q[j] <= hi_q; ++j) ob_union(P, i, j);
    }
    ob_sync();
    // ---- O3: flatten, area and first raster pixel per root, rank ----
    for (int i = tid; i < nseg; i += OB_THREADS) {
        const int r = ob_find(P, i);
        if (r != i) __hip_atomic_store(&P[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // r stays an ancestor for concurrent finds
    }
    ob_sync();
    int roots = 0;
    for (int i = tid; i < nseg; i += OB_THREADS) {
        const int r = ob_load(&P[i]), q = Q[i], x = q / H;
        roots += r == i;
        atomicAdd(&A[r], L[i]);
        atomicMin(&F[r], (q - x * H) * W + x);
    }
    if (tid == 0) sh.ncomp = 0;
    if (tid < OB_MAX_OBJECTS) {
        sh.root[tid] = -1;
        sh.area[tid] = 0;
        sh.first[tid] = 0;
        sh.x0[tid] = sh.y0[tid] = OB_NONE;
        sh.x1[tid] = sh.y1[tid] = -1;
        sh.sum_x[tid] = sh.sum_y[tid] = 0;
    }
    if (tid == OB_MAX_OBJECTS) {
        sh.x0[tid] = sh.y0[tid] = OB_NONE;
        sh.x1[tid] = sh.y1[tid] = -1;
        sh.mask_area = 0;
    }
    ob_sync();
    roots = wave_total(roots);
    if (lane == 0 && roots) atomicAdd(&sh.ncomp, roots);
    // rounds of "largest key below the previous one": key = area << 32 | ~first, unique per component
    unsigned long long prev = ~0ull;
    int kept = 0;
    for (int k = 0; k < a.max_objects; ++k) {
        unsigned long long bk = 0;
        int bi = -1;
        for (int i = tid; i < nseg; i += OB_THREADS) {
            if (ob_load(&P[i]) != i) continue;
            const int ar = ob_load(&A[i]);
            if (ar < a.min_area) continue;
            const unsigned long long key = ((unsigned long long)(unsigned)ar << 32) | (0xffffffffu - (unsigned)ob_load(&F[i]));
            if (key < prev && key > bk) { bk = key; bi = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long ok = __shfl_xor(bk, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ok > bk) { bk = ok; bi = oi; }
        }
        if (lane == 0) { sh.wkey[wv] = bk; sh.widx[wv] = bi; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < OB_WAVES; ++w)
            if (sh.wkey[w] > bk) { bk = sh.wkey[w]; bi = sh.widx[w]; }
        __syncthreads();
        if (bk == 0) break;  // uniform: every thread holds the workgroup's maximum
        if (tid == 0) {
            sh.root[k] = bi;
            sh.area[k] = (int)(bk >> 32);
            sh.first[k] = (int)(0xffffffffu - (unsigned)bk);
        }
        prev = bk;
        kept = k + 1;
    }
    __syncthreads();
    // A becomes the rank of a root (-1: not kept), F the rank of a segment
    for (int i = tid; i < nseg; i += OB_THREADS)
        if (ob_load(&P[i]) == i) A[i] = -1;
    ob_sync();
    if (tid < kept) A[sh.root[tid]] = tid;
    ob_sync();
    // ---- O4: statistics of the kept objects and of the whole mask ----
    int mx0 = OB_NONE, my0 = OB_NONE, mx1 = -1, my1 = -1, marea = 0;
    for (int i = tid; i < nseg; i += OB_THREADS) {
        const int q = Q[i], len = L[i], x = q / H, y0 = q - x * H, y1 = y0 + len - 1;
        const int k = ob_load(&A[ob_load(&P[i])]);
        F[i] = k;
        mx0 = x < mx0 ? x : mx0;
        mx1 = x > mx1 ? x : mx1;
        my0 = y0 < my0 ? y0 : my0;
        my1 = y1 > my1 ? y1 : my1;
        marea += len;
        if (k < 0) continue;
        atomicMin(&sh.x0[k], x);
        atomicMax(&sh.x1[k], x);
        atomicMin(&sh.y0[k], y0);
        atomicMax(&sh.y1[k], y1);
        atomicAdd(&sh.sum_x[k], (unsigned long long)x * (unsigned long long)len);
        atomicAdd(&sh.sum_y[k], (unsigned long long)(y0 + y1) * (unsigned long long)len / 2ull);  // y0 + ... + y1
    }
    if (marea) {
        atomicMin(&sh.x0[OB_MAX_OBJECTS], mx0);
        atomicMax(&sh.x1[OB_MAX_OBJECTS], mx1);
        atomicMin(&sh.y0[OB_MAX_OBJECTS], my0);
        atomicMax(&sh.y1[OB_MAX_OBJECTS], my1);
        atomicAdd(&sh.mask_area, marea);
    }
    ob_sync();
    return nseg;
}

__device__ __forceinline__ int ob_span_flags(int x0, int y0, int x1, int y1, int H, int W) {
    return ((y0 == 0 && y1 == H - 1) ? 1 : 0) | ((x0 == 0 && x1 == W - 1) ? 2 : 0);
}

__global__ __launch_bounds__(OB_THREADS) void objects_components_kernel(sm_objects_args a, int seg_cap) {
    __shared__ int tables[5 * OB_LDS_SEGS];
    __shared__ ObShared sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    const sm_bilateral_image im = a.images[b];
    const int H = im.H, W = im.W;
    int n = a.info[2 * b];
    const int p0 = a.info[2 * b + 1] ? 1 : 0;
    int* ws = (int*)a.workspace + (int64_t)b * 5 * seg_cap;
    int* gQ = ws, *gL = ws + seg_cap, *gF = ws + 4 * (int64_t)seg_cap;
    // a truncated run list (count > cap) and a device table that disagrees with the host's give no objects
    const bool bad = n < 0 || n > a.cap || H <= 0 || W <= 0 || W > a.max_width || (int64_t)H * W > OB_MAX_PIXELS;
    int nseg = -1;
    bool in_lds = false;
    if (!bad) {
        const int bound = (n + 1 + p0) / 2 + W - 1;  // of the segment count
        in_lds = bound <= OB_LDS_SEGS;
        if (in_lds)
            nseg = ob_components(a, sh, b, H, W, n, p0, tables, tables + OB_LDS_SEGS, tables + 2 * OB_LDS_SEGS, tables + 3 * OB_LDS_SEGS,
                                 tables + 4 * OB_LDS_SEGS, OB_LDS_SEGS);
        else if (bound <= seg_cap)
            nseg = ob_components(a, sh, b, H, W, n, p0, gQ, gL, ws + 2 * (int64_t)seg_cap, ws + 3 * (int64_t)seg_cap, gF, seg_cap);
    }
    const bool ok = nseg >= 0;
    const int kept_max = a.max_objects;
    if (tid < kept_max) {
        sm_object o = {};
        if (ok && sh.root[tid] >= 0) {
            o.sum_x = (int64_t)sh.sum_x[tid];
            o.sum_y = (int64_t)sh.sum_y[tid];
            o.area = sh.area[tid];
            o.first = sh.first[tid];
            o.x0 = sh.x0[tid]; o.y0 = sh.y0[tid]; o.x1 = sh.x1[tid]; o.y1 = sh.y1[tid];
            o.flags = ob_span_flags(o.x0, o.y0, o.x1, o.y1, H, W);
        }
        a.objects[(int64_t)b * kept_max + tid] = o;  // every slot is written: mass starts at 0 for the second launch
    }
    if (tid == 0) {
        int* s = a.summary + (int64_t)b * SM_OBJ_SUMMARY_INTS;
        int kept = 0;
        if (ok)
            while (kept < kept_max && sh.root[kept] >= 0) ++kept;
        const bool any = ok && sh.mask_area > 0;
        s[0] = ok ? sh.ncomp : 0;
        s[1] = kept;
        s[2] = ok ? nseg : 0;
        s[3] = ok ? 0 : 1;
        s[4] = any ? sh.x0[OB_MAX_OBJECTS] : 0;
        s[5] = any ? sh.y0[OB_MAX_OBJECTS] : 0;
        s[6] = any ? sh.x1[OB_MAX_OBJECTS] : -1;
        s[7] = any ? sh.y1[OB_MAX_OBJECTS] : -1;
        s[8] = any ? ob_span_flags(s[4], s[5], s[6], s[7], H, W) : 0;
        s[9] = ok ? sh.mask_area : 0;
    }
    // the segment table (q, length, rank) for the mass launch (in the workspace) and for the caller (a.segments)
    const int ns = ok ? nseg : 0;
    const int* Q = in_lds ? tables : gQ;
    const int* L = in_lds ? tables + OB_LDS_SEGS : gL;
    const int* R = in_lds ? tables + 4 * OB_LDS_SEGS : gF;
    if (in_lds && a.masks)
        for (int i = tid; i < ns; i += OB_THREADS) {
            gQ[i] = Q[i];
            gL[i] = L[i];
            gF[i] = R[i];
        }
    if (a.segments) {
        int* out = a.segments + (int64_t)b * seg_cap * 3;
        for (int i = tid; i < ns; i += OB_THREADS) {  // the rows past summary[2] are left as they are
            out[3 * i] = Q[i];
            out[3 * i + 1] = L[i];
            out[3 * i + 2] = R[i];
        }
    }
}

// O5: the soft mass of the kept objects.  One wave per segment, a lane per pixel of its column stretch.
__global__ __launch_bounds__(OB_THREADS) void objects_mass_kernel(sm_objects_args a, int seg_cap) {
    __shared__ unsigned long long acc[OB_MAX_OBJECTS];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int* s = a.summary + (int64_t)b * SM_OBJ_SUMMARY_INTS;
    const int nseg = s[2], kept = s[1];
    if (kept <= 0 || (int)blockIdx.x * OB_WAVES >= nseg) return;
    const sm_bilateral_image im = a.images[b];
    const int H = im.H, W = im.W;
    const int* ws = (const int*)a.workspace + (int64_t)b * 5 * seg_cap;
    const int* __restrict__ Q = ws, *__restrict__ L = ws + seg_cap, *__restrict__ R = ws + 4 * (int64_t)seg_cap;
    const float* __restrict__ m = a.masks + (int64_t)b * a.mask_stride_b + (int64_t)a.best[b] * a.mh * a.mw;
    const auto src = mask_src<const float* __restrict__>(m, a.mh, a.mw, a.scale, H, W);  // the pixels the predictor's finish wrote
    if (tid < OB_MAX_OBJECTS) acc[tid] = 0;
    __syncthreads();
    for (int i = blockIdx.x * OB_WAVES + (tid >> 6); i < nseg; i += gridDim.x * OB_WAVES) {
        const int k = R[i];
        if (k < 0) continue;
        const int q = Q[i], len = L[i], x = q / H, y0 = q - x * H;
        int sum = 0;  // at most 255 * 2^22
        for (int t = lane; t < len; t += 64) sum += (int)up_soft_u8(src.value(y0 + t, x));
        sum = wave_total(sum);
        if (lane == 0 && sum) atomicAdd(&acc[k], (unsigned long long)sum);
    }
    __syncthreads();
    if (tid < kept && acc[tid])
        atomicAdd(reinterpret_cast<unsigned long long*>(&a.objects[(int64_t)b * a.max_objects + tid].mass), acc[tid]);
}

}  // namespace sm

extern "C" int32_t sm_mask_objects_seg_cap(int32_t cap, int32_t max_width) {
    if (cap <= 0 || cap > sm::OB_MAX_PIXELS || max_width <= 0 || max_width > sm::OB_MAX_WIDTH) return 0;
    return sm::ob_seg_cap(cap, max_width);
}

extern "C" size_t sm_mask_objects_workspace_bytes(int32_t B, int32_t cap, int32_t max_width) {
    if (B <= 0 || B > 65535 || cap <= 0 || cap > sm::OB_MAX_PIXELS || max_width <= 0 || max_width > sm::OB_MAX_WIDTH) return 0;
    return ((size_t)B * 5 * sm::ob_seg_cap(cap, max_width) * sizeof(int32_t) + 255) & ~(size_t)255;
}

extern "C" int sm_mask_objects(const sm_objects_args* a, const sm_bilateral_image* images_host, void* stream) {
    SM_REQUIRE(a && images_host, "sm_mask_objects: null pointer (args or the host image table)");
    SM_REQUIRE(a->starts && a->info && a->images && a->objects && a->summary && a->workspace,
               "sm_mask_objects: null pointer (starts, info, images, objects, summary or workspace)");
    SM_REQUIRE(a->connectivity == 4 || a->connectivity == 8, "sm_mask_objects: connectivity=%d (4 or 8)", a->connectivity);
    SM_REQUIRE(a->max_objects >= 1 && a->max_objects <= sm::OB_MAX_OBJECTS, "sm_mask_objects: max_objects=%d (1 .. %d)", a->max_objects,
               sm::OB_MAX_OBJECTS);
    SM_REQUIRE(a->min_area >= 0, "sm_mask_objects: min_area=%d", a->min_area);
    SM_REQUIRE(a->B > 0 && a->B <= 65535 && a->cap > 0 && a->cap <= sm::OB_MAX_PIXELS && a->max_width > 0 && a->max_width <= sm::OB_MAX_WIDTH,
               "sm_mask_objects: bad shape (B=%d cap=%d max_width=%d (<= %d))", a->B, a->cap, a->max_width, sm::OB_MAX_WIDTH);
    if (a->masks)
        SM_REQUIRE(a->best && a->mh > 0 && a->mw > 0 && a->scale >= 0.f, "sm_mask_objects: masks without best, or bad mask %dx%d scale %g", a->mh,
                   a->mw, (double)a->scale);
    for (int b = 0; b < a->B; ++b) {
        const sm_bilateral_image& im = images_host[b];
        SM_REQUIRE(im.H > 0 && im.W > 0 && im.W <= a->max_width && (int64_t)im.H * im.W <= sm::OB_MAX_PIXELS,
                   "sm_mask_objects: image %d is %d x %d (width <= max_width=%d, at most %d pixels)", b, im.H, im.W, a->max_width, sm::OB_MAX_PIXELS);
    }
    SM_REQUIRE(((uintptr_t)a->workspace % 256) == 0 && a->workspace_bytes >= sm_mask_objects_workspace_bytes(a->B, a->cap, a->max_width),
               "sm_mask_objects: workspace too small or misaligned");
    hipStream_t st = (hipStream_t)stream;
    const int seg_cap = sm::ob_seg_cap(a->cap, a->max_width);
    hipLaunchKernelGGL(sm::objects_components_kernel, dim3(a->B), dim3(sm::OB_THREADS), 0, st, *a, seg_cap);
    if (a->masks) {
        int gx = (seg_cap + sm::OB_WAVES - 1) / sm::OB_WAVES;
        gx = gx > sm::OB_MASS_BLOCKS ? sm::OB_MASS_BLOCKS : gx;
        hipLaunchKernelGGL(sm::objects_mass_kernel, dim3(gx, a->B), dim3(sm::OB_THREADS), 0, st, *a, seg_cap);
    }
    return sm::check_launch("sm_mask_objects");
}
