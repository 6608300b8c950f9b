"""E-measure (Fan et al. 2018) and weighted F-measure (Margolin et al. 2014) of an 8-bit saliency map against a binary ground
truth, restated in numpy: the definition ``csrc/sod_metrics.hip`` is held to.

Both metrics are defined on the 8-bit plane ``p8`` of a prediction - the prediction at the ground truth's size, clipped to [0, 1],
times 255, truncated (``up_soft_u8`` of csrc/upsample.h: the predictor's ``soft`` output, the bytes a saved map holds) - so the
number is what a toolkit computes from the saved map.  The ground truth is ``gt > 0``; n = H W, G = its foreground count,
eps = 2^-52.  The prediction is NOT min-max normalised: the original MATLAB code does not, PySODMetrics does.

Quantities that are integers stay integers (histograms, counts, squared distances, nearest-pixel indices); everything else is
fp64 with the operations in the order written here.

E-measure.  Threshold t in 0 .. 255 gives the map ``p8 >= t``; a = #(map and gt), b = #(map and not gt) are the two 256-bin
histograms of ``p8`` over foreground and background summed from the top.  ``e_value`` turns (a, b, G, n) into E(t); ``e_mean`` adds the
256 values in ascending t, ``e_max`` is their maximum, ``e_adp`` the same formula on the adaptive map, which is defined in integers:
foreground where ``p8 n >= min(2 sum(p8), 255 n)`` - the toolkits' ``min(2 mean, 1)`` threshold without a rounding question.

Weighted F.  For every background pixel D is the Euclidean distance to the nearest foreground pixel and src that pixel;
**ties for src go to the lowest raster index** (smallest row, then smallest column).  The rule is part of the definition: SciPy's
and MATLAB's transforms break ties differently from each other, and the choice moves the value in the fourth digit on speckled
ground truths.  ``feature_transform`` returns (D^2, src) exactly; ``weighted_f`` is the rest.

The kernels take planes of up to 2^22 pixels with sides up to 16384 (d^2 < 2^29 then, so the key fits); this module has no side limit.
"""
from typing import Tuple

import numpy as np

EPS = float(np.finfo(np.float64).eps)
MAX_PIXELS = 1 << 22          # H W of one image, as the evaluator's kernels
_IDX_BITS = 22                # the search key is d^2 << 22 | raster index: d^2 < 2^29, index < 2^22
LOG_HALF_OVER_5 = float(np.log(0.5) / 5.0)


def gaussian_7x7() -> np.ndarray:
    """MATLAB's ``fspecial('gaussian', 7, 5)``: (7, 7) fp64, normalised to sum 1."""
    r = np.arange(-3, 4, dtype=np.float64)
    h = np.exp(-(r[:, None] * r[:, None] + r[None, :] * r[None, :]) / (2.0 * 5.0 * 5.0))
    h[h < EPS * h.max()] = 0.0
    return h / h.sum()


def _planes(p8, gt) -> Tuple[np.ndarray, np.ndarray]:
    p8 = np.asarray(p8)
    gt = np.asarray(gt)
    if p8.dtype != np.uint8 or p8.ndim != 2 or gt.shape != p8.shape:
        raise ValueError("p8: a 2-D uint8 plane, gt: a plane of the same shape")
    if p8.size < 1 or p8.size > MAX_PIXELS:
        raise ValueError(f"1 <= H W <= {MAX_PIXELS}")
    return p8, gt > 0


def histograms(p8, gt) -> np.ndarray:
    """(2, 256) int64: the histogram of ``p8`` over the foreground ([0]) and over the background ([1])."""
    p8, g = _planes(p8, gt)
    return np.stack([np.bincount(p8[g], minlength=256), np.bincount(p8[~g], minlength=256)]).astype(np.int64)


def e_value(a, b, G: int, n: int) -> np.ndarray:
    """E of binary maps with a foreground and b background pixels set (integer arrays), ground truth of G of n pixels."""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    if G == 0:
        s = (n - b).astype(np.float64)
    elif G == n:
        s = a.astype(np.float64)
    else:
        mu_f = (a + b).astype(np.float64) / float(n)
        mu_g = float(G) / float(n)
        s = np.zeros(a.shape, np.float64)
        for f, g, cnt in ((1.0, 1.0, a), (1.0, 0.0, b), (0.0, 1.0, G - a), (0.0, 0.0, n - G - b)):
            df = f - mu_f
            dg = g - mu_g
            align = ((2.0 * df) * dg) / ((df * df + dg * dg) + EPS)
            s = s + cnt.astype(np.float64) * (((align + 1.0) * (align + 1.0)) / 4.0)
    return s / ((float(n) - 1.0) + EPS)


def adaptive_threshold(hist: np.ndarray) -> int:
    """The smallest byte v with ``v n >= min(2 sum(p8), 255 n)`` (at most 255: the right side never exceeds 255 n)."""
    hist = np.asarray(hist, np.int64)
    n = int(hist.sum())
    total = int((hist.sum(axis=0) * np.arange(256, dtype=np.int64)).sum())
    bound = min(2 * total, 255 * n)
    return int(-(-bound // n))


def e_curve(hist: np.ndarray) -> np.ndarray:
    """The 256 values E(t) from the two histograms."""
    hist = np.asarray(hist, np.int64)
    a = np.cumsum(hist[0][::-1])[::-1]
    b = np.cumsum(hist[1][::-1])[::-1]
    return e_value(a, b, int(hist[0].sum()), int(hist.sum()))


def e_measure(p8, gt) -> Tuple[float, float, float]:
    """(e_adp, e_mean, e_max)."""
    hist = histograms(p8, gt)
    curve = e_curve(hist)
    mean = 0.0
    for v in curve:  # ascending t
        mean += float(v)
    mean /= 256.0
    t = adaptive_threshold(hist)
    e_adp = float(e_value(hist[0][t:].sum(), hist[1][t:].sum(), int(hist[0].sum()), int(hist.sum())))
    return e_adp, mean, float(curve.max())


def nearest_in_column(g: np.ndarray) -> np.ndarray:
    """(H, W) int64: for every pixel the row of the nearest foreground pixel of its own column, the upper one on a tie, -1 where
    the column has none (the column pass)."""
    H, W = g.shape
    rows = np.arange(H, dtype=np.int64)[:, None]
    far = np.int64(1) << 40
    up = np.maximum.accumulate(np.where(g, rows, -far), axis=0)
    down = np.minimum.accumulate(np.where(g, rows, far)[::-1], axis=0)[::-1]
    near = np.where(rows - up <= down - rows, up, down)
    return np.where(g.any(axis=0)[None, :], near, -1)


def feature_transform(gt) -> Tuple[np.ndarray, np.ndarray]:
    """Exact Euclidean feature transform: (d2, src), both (H, W) int64.  d2 = the squared distance to the nearest foreground pixel
    (0 on the foreground), src = that pixel's raster index, the lowest one among equally near pixels (the pixel itself on the
    foreground).  Without any foreground both are -1.

    The row pass minimises the key ``d2 << 22 | index`` over the columns' candidates as one integer, searching outward from the
    pixel's own column until dx^2 exceeds every pixel's best d2."""
    g = np.asarray(gt) > 0
    if g.ndim != 2 or g.size < 1 or g.size > MAX_PIXELS:
        raise ValueError(f"gt: a 2-D plane, 1 <= H W <= {MAX_PIXELS}")
    H, W = g.shape
    if not g.any():
        none = np.full((H, W), -1, np.int64)
        return none, none.copy()
    near = nearest_in_column(g)
    rows = np.arange(H, dtype=np.int64)[:, None]
    cols = np.arange(W, dtype=np.int64)[None, :]
    none = np.int64(1) << 62
    dy = rows - near
    col_key = np.where(near >= 0, ((dy * dy) << _IDX_BITS) | (near * W + cols), none)  # a candidate's key at dx = 0
    best = col_key.copy()
    for dx in range(1, W):
        if dx * dx > int(best.max() >> _IDX_BITS):
            break
        shift = np.int64(dx * dx) << _IDX_BITS
        cand = np.where(col_key[:, :-dx] < none, col_key[:, :-dx] + shift, none)   # the column dx to the left
        best[:, dx:] = np.minimum(best[:, dx:], cand)
        cand = np.where(col_key[:, dx:] < none, col_key[:, dx:] + shift, none)     # the column dx to the right
        best[:, :-dx] = np.minimum(best[:, :-dx], cand)
    return best >> _IDX_BITS, best & ((1 << _IDX_BITS) - 1)


def transferred_error_u8(p8, gt, src: np.ndarray) -> np.ndarray:
    """255 Et as bytes: ``255 - p8`` of the pixel itself on the foreground and of ``src`` on the background."""
    p8, g = _planes(p8, gt)
    return (255 - p8.reshape(-1)[src.reshape(-1)].astype(np.int64)).reshape(p8.shape).astype(np.uint8)


def smoothed_error(et8: np.ndarray) -> np.ndarray:
    """EA: Et = et8 / 255 filtered with the 7 x 7 Gaussian, zero padding, the 49 taps added in raster order of the window."""
    H, W = et8.shape
    pad = np.zeros((H + 6, W + 6), np.float64)
    pad[3:3 + H, 3:3 + W] = et8.astype(np.float64) / 255.0
    k = gaussian_7x7()
    acc = np.zeros((H, W), np.float64)
    for i in range(7):
        for j in range(7):
            acc = acc + k[i, j] * pad[i:i + H, j:j + W]
    return acc


def weighted_f(p8, gt, parts: bool = False):
    """F^w_beta with beta^2 = 1.  ``parts=True`` also returns (d2, src, sum of Ew over the foreground, over the background)."""
    p8, g = _planes(p8, gt)
    G = int(g.sum())
    if G == 0:
        return (0.0, None, None, 0.0, 0.0) if parts else 0.0
    d2, src = feature_transform(g)
    e = np.where(g, 255 - p8.astype(np.int64), p8.astype(np.int64)).astype(np.float64) / 255.0
    ea = smoothed_error(transferred_error_u8(p8, g, src))
    m = np.where(g & (ea < e), ea, e)
    w = np.where(g, 1.0, 2.0 - np.exp(LOG_HALF_OVER_5 * np.sqrt(d2.astype(np.float64))))
    ew = m * w
    s_fg = float(ew[g].sum())
    s_bg = float(ew[~g].sum())
    tpw = float(G) - s_fg
    fpw = s_bg
    r = 1.0 - s_fg / float(G)
    p = tpw / ((tpw + fpw) + EPS)
    q = ((2.0 * r) * p) / ((r + p) + EPS)
    return (q, d2, src, s_fg, s_bg) if parts else q


def sod_metrics(p8, gt) -> np.ndarray:
    """(4,) fp64: e_adp, e_mean, e_max, wfm - one row of ``ops.sod_metrics``."""
    e_adp, e_mean, e_max = e_measure(p8, gt)
    return np.array([e_adp, e_mean, e_max, weighted_f(p8, gt)], np.float64)


NAMES = ("e_adp", "e_mean", "e_max", "wfm")
