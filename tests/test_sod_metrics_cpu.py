"""E-measure and weighted F-measure: the numpy definition (selfmask_amd/sod_metrics.py) against brute-force per-pixel
restatements and against the SciPy chain the toolkits use, and the C ABI of sm_sod_metrics_u8 as far as it goes without a GPU."""
import ctypes as C

import numpy as np
import pytest

import _sod_metrics_ref as R
from selfmask_amd import _native as N
from selfmask_amd import sod_metrics as S

SMALL = R.small_cases()


def test_gaussian_is_fspecial_7_5():
    k = S.gaussian_7x7()
    assert k.shape == (7, 7) and abs(k.sum() - 1.0) < 1e-15 and np.array_equal(k, k.T) and np.array_equal(k, k[::-1, ::-1])
    assert np.abs(k - R.gaussian_brute()).max() < 1e-17
    assert abs(k[3, 3] / k[0, 0] - np.exp(18.0 / 50.0)) < 1e-14


@pytest.mark.parametrize("name,p8,gt", SMALL, ids=[c[0] for c in SMALL])
def test_e_measure_equals_the_per_pixel_form(name, p8, gt):
    e_adp, e_mean, e_max = S.e_measure(p8, gt)
    b_adp, b_mean, b_max, curve = R.e_measure_brute(p8, gt)
    got = S.e_curve(S.histograms(p8, gt))
    print(name, "max |E(t) - per-pixel|", np.abs(got - curve).max(), "adp", abs(e_adp - b_adp), "mean", abs(e_mean - b_mean))
    assert np.abs(got - curve).max() <= 1e-12
    assert abs(e_mean - b_mean) <= 1e-12 and abs(e_max - b_max) <= 1e-12 and abs(e_adp - b_adp) <= 1e-12


@pytest.mark.parametrize("name,p8,gt", SMALL, ids=[c[0] for c in SMALL])
def test_feature_transform_and_wfm_equal_brute_force(name, p8, gt):
    d2, src = S.feature_transform(gt)
    bd2, bsrc = R.feature_transform_brute(gt)
    assert d2.dtype == np.int64 and src.dtype == np.int64
    assert np.array_equal(d2, bd2), name
    assert np.array_equal(src, bsrc), name  # ties to the lowest raster index
    if (gt > 0).any():
        assert np.array_equal(src[gt > 0], np.flatnonzero(gt > 0)) and not d2[gt > 0].any()
    got = S.weighted_f(p8, gt)
    want = R.weighted_f_brute(p8, gt, bd2, bsrc)
    print(name, "wfm", got, "|diff|", abs(got - want))
    assert abs(got - want) <= 1e-12
    if not (gt > 0).any():
        assert got == 0.0


def _unique_nearest_cases():
    """ground truths on which every background pixel has ONE nearest foreground pixel (convex foregrounds)"""
    cases = []
    for kind, H, W in (("rect", 300, 400), ("rect", 37, 53), ("corner", 37, 53), ("corner", 1, 9), ("corner", 9, 1), ("row", 37, 53),
                       ("row", 5, 3), ("full", 37, 53), ("full", 5, 3), ("full", 1, 1), ("rect", 64, 61)):
        gt = R.make_gt(kind, H, W, seed=H + W)
        cases.append((f"{kind}_{H}x{W}", R.make_pred(gt, seed=H), gt))
    return cases


UNIQUE = _unique_nearest_cases()


@pytest.mark.parametrize("name,p8,gt", UNIQUE, ids=[c[0] for c in UNIQUE])
def test_wfm_equals_the_scipy_chain_where_the_nearest_pixel_is_unique(name, p8, gt):
    pytest.importorskip("scipy.ndimage")
    want, sd2 = R.weighted_f_scipy(p8, gt)
    got, d2, _, _, _ = S.weighted_f(p8, gt, parts=True)
    print(name, "wfm", got, "scipy", want, "|diff|", abs(got - want))
    assert np.array_equal(d2, sd2)
    assert abs(got - want) <= 1e-12


def test_there_are_enough_witness_cases():
    assert len(UNIQUE) >= 8 and any(gt.shape == (300, 400) for _, _, gt in UNIQUE)


@pytest.mark.parametrize("name,p8,gt", SMALL, ids=[c[0] for c in SMALL])
def test_squared_distances_equal_scipy_ties_or_not(name, p8, gt):
    ndi = pytest.importorskip("scipy.ndimage")
    if not (gt > 0).any():
        return
    dst = ndi.distance_transform_edt(~(gt > 0))
    assert np.array_equal(S.feature_transform(gt)[0], np.rint(dst * dst).astype(np.int64)), name


def test_adaptive_map_integer_rule_equals_the_fp64_rule():
    """p8 n >= min(2 sum p8, 255 n) against p8 / 255 >= min(2 mean(p8 / 255), 1); an input on which they disagree is listed"""
    disagree = []
    planes = [(name, p8) for name, p8, _ in SMALL + UNIQUE]
    rng = np.random.default_rng(5)
    for H, W in R.SMALL_SIZES + ((64, 61),):
        planes.append((f"uniform_{H}x{W}", rng.integers(0, 256, (H, W)).astype(np.uint8)))
        planes.append((f"dark_{H}x{W}", rng.integers(0, 3, (H, W)).astype(np.uint8)))
        planes.append((f"bright_{H}x{W}", rng.integers(120, 256, (H, W)).astype(np.uint8)))
        for v in (0, 1, 127, 128, 254, 255):
            planes.append((f"const{v}_{H}x{W}", np.full((H, W), v, np.uint8)))
    for name, p8 in planes:
        a, b = R.adaptive_map_int(p8), R.adaptive_map_float(p8)
        if not np.array_equal(a, b):
            disagree.append((name, int((a != b).sum())))
        t = S.adaptive_threshold(np.stack([np.bincount(p8.reshape(-1), minlength=256), np.zeros(256, np.int64)]))
        assert np.array_equal(a, p8 >= t), name
    assert disagree == [], disagree


def test_sod_metrics_row_and_argument_checks():
    name, p8, gt = SMALL[-1]
    row = S.sod_metrics(p8, gt)
    assert row.shape == (4,) and row.dtype == np.float64 and S.NAMES == ("e_adp", "e_mean", "e_max", "wfm")
    assert 0.0 <= row[3] <= 1.0 and row[1] <= row[2]
    with pytest.raises(ValueError):
        S.sod_metrics(p8.astype(np.float32), gt)
    with pytest.raises(ValueError):
        S.sod_metrics(p8, gt[:-1])
    # a perfect map: wfm = 1, every pixel fully aligned (the sum is n, the definition divides by n - 1 + eps)
    g = R.make_gt("rect", 20, 30)
    perfect = S.sod_metrics((g > 0).astype(np.uint8) * 255, g)
    assert abs(perfect[3] - 1.0) < 1e-12 and abs(perfect[2] - 600.0 / 599.0) < 1e-12


# ---- ABI (its prototypes and exports: tests/test_abi_cpu.py) ----
def test_workspace_grows_with_batch_and_pixels():
    lib = N.load()
    f = lib.sm_sod_metrics_workspace_bytes
    assert f(1, 1) > 0 and f(1, 1 << 22) >= (1 << 22) * 9
    assert f(2, 120000) > f(1, 120000) > f(1, 60000)
    assert f(8, 120000) >= 8 * 120000 * 9
    for B, mp in ((0, 100), (-1, 100), (65536, 100), (1, 0), (1, (1 << 22) + 1)):
        assert f(B, mp) == 0, (B, mp)
    assert f(3, 1000) % 256 == 0


def test_argument_validation_without_gpu():
    lib = N.load()
    table = (N.EvalImage * 2)()
    table[0].gt_off, table[0].H, table[0].W = 0, 4, 4
    table[1].gt_off, table[1].H, table[1].W = 16, 3, 5
    host = C.addressof(table)
    p = 256  # never dereferenced: every call below is refused on the host
    need = lib.sm_sod_metrics_workspace_bytes(2, 16)

    def call(pred=p, gt=p, images=p, images_host=host, B=2, max_pixels=16, out=p, hist=None, ws=p, wsb=need):
        return lib.sm_sod_metrics_u8(pred, gt, images, images_host, B, max_pixels, out, hist, ws, wsb, None)

    for kw in ({"pred": None}, {"gt": None}, {"images": None}, {"images_host": None}, {"out": None}, {"ws": None}):
        assert call(**kw) == -1 and b"null pointer" in lib.sm_last_error(), kw
    assert call(max_pixels=(1 << 22) + 1) == -1 and b"max_pixels" in lib.sm_last_error()
    assert call(max_pixels=0) == -1 and b"max_pixels" in lib.sm_last_error()
    assert call(B=0) == -1 and b"B=0" in lib.sm_last_error()
    assert call(max_pixels=15) == -1 and b"image 0" in lib.sm_last_error()  # H W above max_pixels
    assert call(wsb=need - 1) == -1 and b"workspace" in lib.sm_last_error()
    assert call(ws=p + 8) == -1 and b"workspace" in lib.sm_last_error()
    table[1].H, table[1].W = 2048, 2049  # H W > 2^22
    assert call(max_pixels=1 << 22, wsb=lib.sm_sod_metrics_workspace_bytes(2, 1 << 22)) == -1 and b"image 1" in lib.sm_last_error()
    table[1].H, table[1].W = 1, 16385  # a side the search key has no room for
    assert call(max_pixels=1 << 22, wsb=lib.sm_sod_metrics_workspace_bytes(2, 1 << 22)) == -1 and b"image 1" in lib.sm_last_error()
    table[1].H, table[1].W = 0, 5
    assert call() == -1 and b"image 1" in lib.sm_last_error()
    # sm_upsample_selected_u8
    u = lib.sm_upsample_selected_u8
    assert u(None, 0, p, 14, p, p, 1, 4, 4, 0.0, 16, None) == -1 and b"sm_upsample_selected_u8" in lib.sm_last_error()
    assert u(p, 0, p, 13, p, p, 1, 4, 4, 0.0, 16, None) == -1
    assert u(p, 0, p, 14, p, p, 1, 4, 4, -1.0, 16, None) == -1
    assert u(p, 0, p, 14, p, p, 1, 4, 4, 0.0, (1 << 22) + 1, None) == -1
    assert u(p, 0, p, 14, None, p, 1, 4, 4, 2.0, 16, None) == -1
