"""Brute-force restatements of E-measure and weighted F-measure, per pixel and without any of the shortcuts of
``selfmask_amd/sod_metrics.py`` (histograms, separable transform, outward search), plus the inputs both test files share."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)


def e_per_pixel(fm: np.ndarray, g: np.ndarray) -> float:
    """E of ONE binary map ``fm`` against the binary ground truth ``g``: the alignment matrix evaluated pixel by pixel."""
    n = g.size
    G = int(g.sum())
    if G == 0:
        s = float((~fm).sum())
    elif G == n:
        s = float(fm.sum())
    else:
        f = fm.astype(np.float64)
        t = g.astype(np.float64)
        df = f - f.mean()
        dg = t - t.mean()
        align = 2.0 * df * dg / (df * df + dg * dg + EPS)
        s = float((((align + 1.0) ** 2) / 4.0).sum())
    return s / (n - 1 + EPS)


def e_measure_brute(p8: np.ndarray, gt: np.ndarray):
    """(e_adp, e_mean, e_max) from the 256 binary maps directly; the adaptive map by the toolkits' fp64 rule."""
    g = gt > 0
    curve = np.array([e_per_pixel(p8 >= t, g) for t in range(256)])
    return e_per_pixel(adaptive_map_float(p8), g), float(curve.mean()), float(curve.max()), curve


def adaptive_map_float(p8: np.ndarray) -> np.ndarray:
    """``pred >= min(2 mean(pred), 1)`` on pred = p8 / 255 in fp64"""
    pred = p8.astype(np.float64) / 255.0
    return pred >= min(2.0 * pred.mean(), 1.0)


def adaptive_map_int(p8: np.ndarray) -> np.ndarray:
    """the definition's integer rule: p8 n >= min(2 sum(p8), 255 n)"""
    n = p8.size
    return p8.astype(np.int64) * n >= min(2 * int(p8.astype(np.int64).sum()), 255 * n)


def feature_transform_brute(gt: np.ndarray):
    """(d2, src) by an argmin over ALL foreground pixels in raster order (argmin returns the first minimum: the lowest raster
    index among equally near pixels)."""
    g = gt > 0
    H, W = g.shape
    fy, fx = np.nonzero(g)  # raster order
    if fy.size == 0:
        return np.full((H, W), -1, np.int64), np.full((H, W), -1, np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    d2 = np.empty((H, W), np.int64)
    src = np.empty((H, W), np.int64)
    for y in range(H):
        d = (fy[None, :] - yy[y][:, None]) ** 2 + (fx[None, :] - xx[y][:, None]) ** 2  # (W, nfg)
        k = d.argmin(axis=1)
        d2[y] = d[np.arange(W), k]
        src[y] = fy[k] * W + fx[k]
    return d2, src


def gaussian_brute() -> np.ndarray:
    k = np.array([[np.exp(-((i - 3) ** 2 + (j - 3) ** 2) / 50.0) for j in range(7)] for i in range(7)])
    return k / k.sum()


def weighted_f_brute(p8: np.ndarray, gt: np.ndarray, d2: np.ndarray, src: np.ndarray) -> float:
    """F^w from a given feature transform, every pixel's 7 x 7 window gathered one by one."""
    g = gt > 0
    H, W = g.shape
    G = int(g.sum())
    if G == 0:
        return 0.0
    pred = p8.astype(np.float64) / 255.0
    e = np.abs(pred - g.astype(np.float64))
    et = np.where(g, e, e.reshape(-1)[src.reshape(-1)].reshape(H, W))
    k = gaussian_brute()
    ea = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            acc = 0.0
            for i in range(7):
                for j in range(7):
                    yy, xx = y + i - 3, x + j - 3
                    if 0 <= yy < H and 0 <= xx < W:
                        acc += k[i, j] * et[yy, xx]
            ea[y, x] = acc
    m = np.where(g & (ea < e), ea, e)
    b = np.where(g, 1.0, 2.0 - np.exp(np.log(0.5) / 5.0 * np.sqrt(d2.astype(np.float64))))
    ew = m * b
    tpw = G - ew[g].sum()
    fpw = ew[~g].sum()
    r = 1.0 - ew[g].mean()
    p = tpw / (tpw + fpw + EPS)
    return float(2.0 * r * p / (r + p + EPS))


def weighted_f_scipy(p8: np.ndarray, gt: np.ndarray):
    """The toolkits' chain on SciPy (PySODMetrics' WeightedFmeasure without its min-max normalisation): returns (wfm, D^2 as
    integers)."""
    from scipy.ndimage import convolve, distance_transform_edt
    g = gt > 0
    G = int(g.sum())
    pred = p8.astype(np.float64) / 255.0
    if G == 0:
        return 0.0, None
    dst, idx = distance_transform_edt(~g, return_indices=True)
    d2 = np.rint(dst * dst).astype(np.int64)
    e = np.abs(pred - g)
    et = e.copy()
    et[~g] = e[idx[0][~g], idx[1][~g]]
    ea = convolve(et, weights=gaussian_brute(), mode="constant", cval=0)
    m = np.where(g & (ea < e), ea, e)
    b = np.where(g, 1.0, 2.0 - np.exp(np.log(0.5) / 5.0 * dst))
    ew = m * b
    tpw = G - ew[g].sum()
    fpw = ew[~g].sum()
    r = 1.0 - ew[g].mean()
    p = tpw / (tpw + fpw + EPS)
    return float(2.0 * r * p / (r + p + EPS)), d2


# ---- inputs -----------------------------------------------------------------------------------------------------------
GT_KINDS = ("speckle", "checker", "empty", "full", "corner", "rect")
SMALL_SIZES = ((1, 1), (1, 9), (9, 1), (5, 3), (37, 53))


def make_gt(kind: str, H: int, W: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(1000 + seed)
    g = np.zeros((H, W), np.uint8)
    if kind == "speckle":      # isolated pixels on a lattice-like scatter: many equally near sources
        g[rng.random((H, W)) < 0.08] = 1
    elif kind == "checker":    # every background pixel tied four ways (two or three at the borders)
        g[(np.add.outer(np.arange(H), np.arange(W)) % 2) == 0] = 1
    elif kind == "full":
        g[:] = 1
    elif kind == "corner":
        g[H - 1, W - 1] = 1
    elif kind == "rect":
        g[H // 4:max(H // 4 + 1, 3 * H // 4), W // 3:max(W // 3 + 1, 2 * W // 3)] = 1
    elif kind == "row":
        g[H // 2, :] = 1
    elif kind == "blob":       # an ellipse covering about a fifth of the plane
        yy, xx = np.mgrid[0:H, 0:W]
        g[((yy - 0.45 * H) / (0.25 * H + 1)) ** 2 + ((xx - 0.55 * W) / (0.26 * W + 1)) ** 2 <= 1.0] = 1
    elif kind != "empty":
        raise ValueError(kind)
    return g * np.uint8(255 if seed % 2 else 1)  # the ground truth is gt > 0 whatever the non-zero byte


def make_pred(gt: np.ndarray, seed: int = 0) -> np.ndarray:
    """an 8-bit map that resembles the ground truth: smooth-ish noise around it, every byte value reachable, saturated areas"""
    rng = np.random.default_rng(2000 + seed)
    H, W = gt.shape
    base = np.where(gt > 0, 0.8, 0.15) + 0.35 * rng.standard_normal((H, W))
    if H > 2 and W > 2:
        base[1:-1, 1:-1] = 0.5 * base[1:-1, 1:-1] + 0.125 * (base[:-2, 1:-1] + base[2:, 1:-1] + base[1:-1, :-2] + base[1:-1, 2:])
    return (np.clip(base, 0.0, 1.0) * 255.0).astype(np.uint8)


def small_cases():
    """(name, p8, gt) over SMALL_SIZES x GT_KINDS"""
    out = []
    for si, (H, W) in enumerate(SMALL_SIZES):
        for ki, kind in enumerate(GT_KINDS):
            gt = make_gt(kind, H, W, seed=si * 7 + ki)
            out.append((f"{kind}_{H}x{W}", make_pred(gt, seed=si * 7 + ki), gt))
    return out
