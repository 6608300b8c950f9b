"""The evaluator's edge-case table, shared by test_eval_cases_cpu.py (checks the table) and test_hip_eval_edges.py (checks
the kernels), plus what the CPU check needs to say which branch of eval.hip a case reaches: a NumPy restatement of the band
table and the walk choice, and float64 / float32 restatements of the S-measure that name the ssim branch of every quadrant.

A case is (name, scale, mh, mw, nq, [(H, W), ...], mask kind, gt kind); build_case(i) -> (masks float32 (B, nq, mh, mw),
objectness float32 (B, nq), [gt uint8 (H, W)]), seeded by the case index.  scale = 0 resizes the mask to each GT's size, scale > 0
up-samples by that factor and crops.

Band geometry worth knowing when reading the table (band i = the GT rows whose upper tap is low-res row i; half-pixel centres):
for an up-sampling factor f the interior bands have f rows (f not an integer: floor and ceil of it), band 0 has 1.5 f rows
(its source coordinate is clamped at 0) and the last band 0.5 f.  So H = 56 from mh = 28 gives heights 3, 2 x 26, 1; mh = 4 gives
24, 16, 16, 8 at H = 64, 48, 32, 32, 16 at H = 128 and 50, 34, 33, 17 at H = 134."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

THR = torch.arange(0, 1, 1 / 255).numpy()  # the F-max table of metrics/f_measure.py (float32)
HALF_LO, HALF_HI = np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))

# eval.hip's constants
EV_BAND_MIN, EV_BAND_MAX_H, EV_UPW, EV_NW, EV_CHUNK, EV_LDS_ROWS = 2, 16383, 4, 4, 2048, 8

BOTH = [(70, 65), (40, 63)]  # a band-walk and a raster-walk image for a 28-row mask
CASES = [
    # ---- walk choice and band geometry
    ("h55_raster", 0, 28, 28, 4, [(55, 63), (55, 300)], "noisy", "ellipse"),  # the last height below 2 * mh; the wide one stages its taps
    ("h56_band", 0, 28, 28, 4, [(56, 64)], "noisy", "ellipse"),        # the first band-walk height: interior bands of 2 rows, the last of 1
    ("identity", 0, 28, 28, 4, [(28, 28)], "noisy", "ellipse"),
    ("down_unstaged", 0, 28, 28, 4, [(20, 17)], "noisy", "ellipse"),   # one chunk over all 28 low-res rows: the global-load fallback
    ("x2p5", 0, 28, 28, 4, [(70, 65)], "noisy", "ellipse"),            # band heights 2 and 3
    ("band16", 0, 4, 6, 4, [(64, 130)], "noisy", "ellipse"),           # one whole GT group per band (24 / 16 / 16 / 8)
    ("band32", 0, 4, 6, 4, [(128, 63)], "noisy", "ellipse"),           # the flush exactly at a band's end (48 / 32 / 32 / 16)
    ("band33", 0, 4, 6, 4, [(134, 65)], "noisy", "ellipse"),           # the flush inside a band (50 / 34 / 33 / 17)
    ("crop_h1", 8, 28, 28, 4, [(61, 130)], "noisy", "ellipse"),        # the crop ends one row into band 7: height 1, then empty bands
    ("crop_heavy", 8, 28, 42, 4, [(60, 333)], "noisy", "ellipse"),     # bands 7..27 empty
    ("x8_raster", 8, 28, 42, 4, [(40, 300)], "noisy", "ellipse"),      # scale mode on the raster walk
    ("w1", 0, 28, 28, 4, [(56, 1), (30, 1)], "noisy", "dense"),
    ("mh1", 0, 1, 5, 4, [(9, 70), (1, 9)], "noisy", "dense"),          # both row taps are row 0
    ("mw1", 0, 5, 1, 4, [(40, 9), (7, 3)], "noisy", "dense"),          # both column taps are column 0
    ("tall_band", 0, 1, 2, 4, [(16383, 8)], "ones", "dense"),          # the tallest band the 16-bit counts allow
    ("tall_raster", 0, 1, 2, 4, [(16384, 8)], "ones", "dense"),        # the first height EV_BAND_MAX_H sends to the raster walk
    ("mixed", 0, 28, 28, 4, [(30, 40), (300, 400), (61, 65), (28, 28), (150, 130)], "noisy", "ellipse"),
    # ---- ground truths, each on a band-walk and a raster-walk image
    ("gt_empty", 0, 28, 28, 4, BOTH, "noisy", "empty"),
    ("gt_full", 0, 28, 28, 4, BOTH, "noisy", "full"),
    ("gt_px00", 0, 28, 28, 4, BOTH, "noisy", "px00"),
    ("gt_pxlast", 0, 28, 28, 4, BOTH, "noisy", "pxlast"),
    ("gt_allbut1", 0, 28, 28, 4, BOTH, "noisy", "allbut1"),
    ("gt_col0", 0, 28, 28, 4, BOTH, "noisy", "col0"),
    ("gt_row0", 0, 28, 28, 4, BOTH, "noisy", "row0"),
    ("gt_half_even", 0, 28, 28, 4, BOTH, "noisy", "half_even"),
    ("gt_half_odd", 0, 28, 28, 4, BOTH, "noisy", "half_odd"),
    ("gt_cy_first", 0, 28, 28, 4, [(300, 130), (40, 130)], "noisy", "cy_first"),
    ("gt_cy_inside", 0, 28, 28, 4, [(300, 130), (40, 130)], "noisy", "cy_inside"),
    ("gt_cx64", 0, 28, 28, 4, [(70, 130), (40, 130)], "noisy", "cx64"),
    ("gt_empty_x8", 8, 28, 28, 4, [(224, 220), (40, 100)], "noisy", "empty"),
    # ---- mask values
    ("blocks", 0, 28, 28, 4, [(140, 130), (50, 63)], "blocks", "ellipse"),
    ("blocks_x8", 8, 28, 28, 4, [(224, 220), (50, 200)], "blocks", "ellipse"),
    ("dark", 0, 28, 28, 4, BOTH, "dark", "ellipse"),
    ("sat", 0, 28, 28, 4, BOTH, "sat", "ellipse"),
    # ---- selection
    ("iou_tie", 0, 28, 28, 4, BOTH, "tie", "ellipse"),
    ("nq1", 0, 28, 28, 1, BOTH, "noisy", "ellipse"),
    ("nq21", 0, 28, 28, 21, BOTH, "noisy", "ellipse"),                  # the first count on eval_query_kernel<8>
    ("nq32", 0, 28, 28, 32, BOTH, "noisy", "ellipse"),
    ("nq64", 0, 28, 28, 64, BOTH, "noisy", "ellipse"),                  # two full passes
]
NAMES = [c[0] for c in CASES]
MIXED = NAMES.index("mixed")
RESEED = {"gt_empty_x8": 1}  # case name -> extra seed word, where the first draw broke one of the two input conditions of test_eval_cases_cpu.py


# ---- the band table and the walk choice, restated ------------------------------------------------------------------------
def source_scale(scale, in_size, out_size):
    """sy / sx of the kernels, in float32"""
    return np.float32(1.0) / np.float32(scale) if scale > 0 else np.float32(in_size) / np.float32(out_size)


def upper_taps(s, n, in_size):
    """clamped upper tap of every destination index: the float32 expression of first_dst / up_index"""
    d = np.arange(n, dtype=np.float32)
    src = s * (d + np.float32(0.5)) - np.float32(0.5)
    src = np.maximum(src, np.float32(0))
    return np.minimum(src.astype(np.int64), in_size - 1)


def band_table(scale, mh, H):
    """ytab[i] = first GT row whose upper tap is >= i (a binary search over the monotone tap map), ytab[mh] = H"""
    t = upper_taps(source_scale(scale, mh, H), H, mh)
    assert np.all(np.diff(t) >= 0)
    return np.concatenate([np.searchsorted(t, np.arange(mh), side="left"), [H]]).astype(np.int64)


def band_heights(scale, mh, H):
    return np.diff(band_table(scale, mh, H))


def takes_band_walk(mh, H):
    return EV_BAND_MIN * mh <= H <= EV_BAND_MAX_H


def units_per_wave(mh, W, max_pixels):
    """work units (band, 64 columns) each wave of the band walk takes: slots_of() and the unit loops of eval.hip"""
    units = mh * ((W + 63) // 64)
    nslot = max((max_pixels + EV_CHUNK - 1) // EV_CHUNK, mh)
    slots = min((units + EV_NW * EV_UPW - 1) // (EV_NW * EV_UPW), nslot)
    return [len(range(w, units, slots * EV_NW)) for w in range(slots * EV_NW)]


def raster_chunk_staged(scale, mh, mw, H, W, chunk):
    """whether a raster-walk chunk stages its low-res rows in LDS (lds_rows of sm_evaluate_masks_f32)"""
    lds_rows = min(60 * 1024 // (mw * 32 * 4), EV_LDS_ROWS)
    t = upper_taps(source_scale(scale, mh, H), H, mh)
    y0, y1 = chunk * EV_CHUNK // W, (min((chunk + 1) * EV_CHUNK, H * W) - 1) // W
    r_hi = t[y1] + (1 if t[y1] < mh - 1 else 0)
    return r_hi - t[y0] + 1 <= lds_rows


# ---- builders -------------------------------------------------------------------------------------------------------------
def _gt(kind, H, W, rng, ytab):
    g = np.zeros((H, W), np.uint8)
    if kind == "ellipse":
        yy, xx = np.mgrid[:H, :W]
        cy, ry, cx, rx = H * rng.uniform(.3, .7), H * rng.uniform(.15, .3), W * rng.uniform(.3, .7), W * rng.uniform(.15, .3)
        g = ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1).astype(np.uint8)
    elif kind == "dense":
        g = (rng.random((H, W)) < 0.9).astype(np.uint8)
    elif kind == "full":
        g[:] = 1
    elif kind == "px00":
        g[0, 0] = 1
    elif kind == "pxlast":
        g[H - 1, W - 1] = 1
    elif kind == "allbut1":
        g[:] = 1
        g[H // 2, W // 3] = 0
    elif kind == "col0":
        g[:, 0] = 1
    elif kind == "row0":
        g[0, :] = 1
    elif kind in ("half_even", "half_odd"):  # two pixels, both centroid quotients exactly k + 0.5
        par = 0 if kind == "half_even" else 1
        ky, kx = (H // 2) // 2 * 2 + par, (W // 2) // 2 * 2 + par
        g[ky - 7, kx - 5] = 1
        g[ky + 8, kx + 6] = 1
    elif kind in ("cy_first", "cy_inside"):  # rows symmetric about a band's first row / the row after it
        mh = len(ytab) - 1  # (an image without a band of three rows - the raster walk's - takes the middle band)
        i = next((i for i in range(mh // 2, mh) if ytab[i + 1] - ytab[i] >= 3), mh // 2)
        r = ytab[i] + (0 if kind == "cy_first" else 1)
        g[r - 2: r + 3, W // 4: W - W // 4] = 1
    elif kind == "cx64":
        g[H // 4: H - H // 4, 60: 69] = 1
    else:
        assert kind == "empty", kind
    return g


def _low(gt, scale, mh, mw):
    """the ground truth at the mask's resolution (scale mode: on the uncropped canvas)"""
    if scale > 0:
        canvas = np.zeros((int(mh * scale), int(mw * scale)), np.float32)
        canvas[:gt.shape[0], :gt.shape[1]] = gt
    else:
        canvas = gt.astype(np.float32)
    return F.interpolate(torch.from_numpy(canvas)[None, None], size=(mh, mw), mode="bilinear", align_corners=False)[0, 0].numpy()


def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


def _masks(kind, nq, mh, mw, low, rng):
    def noisy():
        return _sigmoid((low * 8 - 4) * rng.uniform(-0.5, 1.5) + rng.standard_normal((mh, mw)) * rng.uniform(0.5, 3.0))

    if kind == "noisy":  # test_hip_eval.py's scenes
        m = [noisy() for _ in range(nq)]
    elif kind == "blocks":  # 2 x 2 constant blocks on the F-max thresholds, 0.5 and its two neighbours; no two blocks alike
        m = []
        for _ in range(nq):
            bh, bw = (mh + 1) // 2, (mw + 1) // 2  # bh * bw <= 257: every query holds 0.5, both neighbours and distinct thresholds
            v = np.concatenate([[np.float32(0.5), HALF_LO, HALF_HI], rng.permutation(THR[1:])[:bh * bw - 3]]).astype(np.float32)
            v = rng.permutation(v).reshape(bh, bw)
            m.append(np.repeat(np.repeat(v, 2, 0), 2, 1)[:mh, :mw])
    elif kind == "dark":  # mean well below 0.5: the adaptive threshold 2 * mean is below 1
        m = [np.clip(0.02 + 0.05 * rng.random((mh, mw)) + low * rng.uniform(0.5, 0.9) * rng.uniform(0.6, 1.0, (mh, mw)), 0, 1)
             for _ in range(nq)]
    elif kind == "sat":  # exact 0.0 and 1.0 regions with a noisy ramp between
        m = [np.clip(low * 2 - 0.5 + rng.standard_normal((mh, mw)) * 0.2, 0, 1) for _ in range(nq)]
    elif kind == "ones":  # query 0 all ones (the largest per-lane counts); the others ramps
        m = [np.ones((mh, mw)), np.linspace(1, 0, mh * mw).reshape(mh, mw), np.linspace(0.25, 0.75, mh * mw).reshape(mh, mw)]
        m += [rng.random((mh, mw)) for _ in range(nq - 3)]
    else:
        assert kind == "tie" and nq == 4, kind  # queries 1 and 3 identical and the best
        good = _sigmoid((low * 8 - 4) * 1.5 + rng.standard_normal((mh, mw)) * 0.3)
        m = [noisy() * 0.6, good, noisy() * 0.6, good.copy()]
    return np.stack(m).astype(np.float32)


def build_case(i):
    name, scale, mh, mw, nq, sizes, mkind, gkind = CASES[i]
    rng = np.random.Generator(np.random.PCG64([i, 20251] + ([RESEED[name]] if name in RESEED else [])))
    masks, objs, gts = [], [], []
    for (H, W) in sizes:
        gt = _gt(gkind, H, W, rng, band_table(scale, mh, H))
        masks.append(_masks(mkind, nq, mh, mw, _low(gt, scale, mh, mw), rng))
        o = ((rng.permutation(nq) + 1) / (nq + 1)).astype(np.float32)  # distinct: argsort has no tie order to test against
        if mkind == "ones":
            o = np.array([0.5, 0.25, 0.75, 0.125][:nq] + [0.0625] * (nq - 4), np.float32) + np.arange(nq, dtype=np.float32) / 1024
        objs.append(o)
        gts.append(gt)
    return np.stack(masks), np.stack(objs), gts


# ---- oracle rows, computed once per case and process ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_case(i):
    """[(pred (nq, H, W) float32 tensor, q_star, ub, ious, [7 metrics of q_star, 7 of ub]) per image] from the CPU oracle"""
    from oracle import evaluator_oracle as E
    scale = CASES[i][1]
    masks, objs, gts = build_case(i)
    out = []
    for b, gt in enumerate(gts):
        gt_t = torch.from_numpy(gt.astype(np.int64))
        pm, q_star, ub, ious = E.postprocess(torch.from_numpy(masks[b]), torch.from_numpy(objs[b]), gt_t,
                                             scale_factor=scale if scale else None)
        out.append((pm, q_star, ub, ious.numpy(), [E.all_metrics(pm[q], gt_t) for q in (q_star, ub)]))
    return out


# ---- the S-measure in float64, and which ssim branch each quadrant takes ------------------------------------------------
def centroid(gt):
    """(X, Y) as the kernel forms them: exact integer sums, float32 quotient, round half to even"""
    ys, xs = np.nonzero(gt)
    n = np.float32(len(ys))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.rint(np.float32(xs.sum()) / n), np.rint(np.float32(ys.sum()) / n)


def _branch(a, b):
    return 0 if a != 0 else (1 if b == 0 else 2)  # alpha != 0 (NaN included); alpha == 0 and beta == 0; otherwise


def s_measure_f64(pred, gt, force=None):
    """metrics/s_measure.py evaluated in float64 with two-pass moments -> (value, [ssim branch of the four quadrants], or
    None where the ground truth is empty or full).  force = {quadrant: ssim value} replaces the ssim of those quadrants."""
    p, g = np.asarray(pred, np.float64), (np.asarray(gt) != 0).astype(np.float64)
    H, W = g.shape
    if g.sum() == 0:
        return 1.0 - p.mean(), None
    if g.sum() == g.size:
        return p.mean(), None

    def ssim(pq, gq):
        n = pq.size
        if n == 0:
            return np.nan, 0
        x, y = pq.mean(), gq.mean()
        den = n - 1 + 1e-20
        sx2, sy2, sxy = ((pq - x) ** 2).sum() / den, ((gq - y) ** 2).sum() / den, ((pq - x) * (gq - y)).sum() / den
        a, b = 4 * x * y * sxy, (x * x + y * y) * (sx2 + sy2)
        br = _branch(a, b)
        return (a / (b + 1e-20), 1.0, 0.0)[br], br

    def obj(t):
        x = t.mean()
        s = t.std(ddof=1) if t.size > 1 else np.nan  # the unbiased std of one value
        return 2.0 * x / (x * x + 1.0 + s + 1e-20)

    u = g.mean()
    s_obj = u * obj(p[g == 1]) + (1 - u) * obj(1 - p[g == 0])
    X, Y = (int(v) for v in centroid(gt))
    w = [X * Y, (W - X) * Y, X * (H - Y)]
    w = [v / (H * W) for v in w]
    w.append(1 - sum(w))
    quads = [ssim(p[:Y, :X], g[:Y, :X]), ssim(p[:Y, X:], g[:Y, X:]), ssim(p[Y:, :X], g[Y:, :X]), ssim(p[Y:, X:], g[Y:, X:])]
    quads = [((force or {}).get(k, s), br) for k, (s, br) in enumerate(quads)]
    q = 0.5 * s_obj + 0.5 * sum(wk * s for wk, (s, _) in zip(w, quads))
    return (0.0 if q < 0 else q), [br for _, br in quads]


def ssim_branches_f32(pred, gt):
    """the oracle's own float32 arithmetic (torch mean / sum, as oracle/evaluator_oracle.py s_measure) -> (X, Y, [branch of the
    four quadrants]); None where the ground truth is empty or full"""
    p, g = torch.as_tensor(pred, dtype=torch.float32), (torch.as_tensor(gt) != 0).to(torch.float32)
    if g.mean() == 0 or g.mean() == 1:
        return None
    rows, cols = g.shape
    X = int(torch.round((g.sum(dim=0) * torch.arange(cols).float()).sum() / g.sum()))
    Y = int(torch.round((g.sum(dim=1) * torch.arange(rows).float()).sum() / g.sum()))

    def branch(pq, gq):
        n = pq.shape[0] * pq.shape[1]
        x, y = pq.mean(), gq.mean()
        sx2 = ((pq - x) * (pq - x)).sum() / (n - 1 + 1e-20)
        sy2 = ((gq - y) * (gq - y)).sum() / (n - 1 + 1e-20)
        sxy = ((pq - x) * (gq - y)).sum() / (n - 1 + 1e-20)
        return _branch(4 * x * y * sxy, (x * x + y * y) * (sx2 + sy2))

    return X, Y, [branch(p[:Y, :X], g[:Y, :X]), branch(p[:Y, X:], g[:Y, X:]), branch(p[Y:, :X], g[Y:, :X]), branch(p[Y:, X:], g[Y:, X:])]


PLATEAU_FREE = (1, 2)  # the quadrants of plateau_case() without ground truth: upper right, lower left
PLATEAU_OTHERS = (0.3, 0.9, 0.6, 0.55, 0.45, 0.8, 0.2)


def plateau_case(c=0.7):
    """The documented deviation (evaluator): a constant prediction c not in {0, 1} over quadrants without ground truth.
    A 28 x 28 mask of 0.7 resized to 300 x 400 is one distinct value; the GT is two blocks on a diagonal, so the upper right and
    the lower left quadrant hold none of it."""
    mask = np.full((1, 1, 28, 28), c, np.float32)
    gt = np.zeros((300, 400), np.uint8)
    gt[20:60, 30:90] = 1
    gt[220:280, 300:380] = 1
    return mask, np.zeros((1, 1), np.float32), [gt]
