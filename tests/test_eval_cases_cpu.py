"""The evaluator's edge-case table (_eval_cases.py) reaches the branches of eval.hip it is meant to reach, and its inputs
keep clear of the two places where the float32 reference and an exact evaluation may legitimately disagree.  Checks the
table, not the kernels: only the CPU oracle and the restated band table are used (the kernels: test_hip_eval_edges.py)."""
import numpy as np
import pytest

import _eval_cases as C

BY_NAME = {c[0]: i for i, c in enumerate(C.CASES)}


def _images(pred=lambda case: True):
    """(case index, image index, case tuple, H, W) of every image of the table"""
    for i, case in enumerate(C.CASES):
        if pred(case):
            for b, (H, W) in enumerate(case[5]):
                yield i, b, case, H, W


def _band_images():
    return [(i, b, c, H, W) for i, b, c, H, W in _images() if C.takes_band_walk(c[2], H)]


def _heights(name, b=0):
    _, scale, mh, _, _, sizes, _, _ = C.CASES[BY_NAME[name]]
    return C.band_heights(scale, mh, sizes[b][0])


def test_table_is_well_formed():
    assert len(set(C.NAMES)) == len(C.NAMES)
    for i, b, (name, scale, mh, mw, nq, sizes, _, _), H, W in _images():
        assert H * W <= 16384 * 8, name
        if scale > 0:
            assert H <= mh * scale and W <= mw * scale, name
    for i in range(len(C.CASES)):
        name, _, mh, mw, nq, sizes, _, _ = C.CASES[i]
        masks, objs, gts = C.build_case(i)
        assert masks.shape == (len(sizes), nq, mh, mw) and masks.dtype == np.float32 and objs.shape == (len(sizes), nq)
        assert masks.min() >= 0 and masks.max() <= 1
        assert [g.shape for g in gts] == [tuple(s) for s in sizes] and all(g.dtype == np.uint8 and g.max() <= 1 for g in gts)
        assert all(len(set(o.tolist())) == nq for o in objs), name  # argsort has no tie order to test against
        again = C.build_case(i)
        assert np.array_equal(masks, again[0]) and np.array_equal(objs, again[1]) and all(np.array_equal(g, h) for g, h in zip(gts, again[2]))


def test_band_table_restatement():
    """the searched table against the definition: band i = the rows whose clamped upper tap is i"""
    for i, b, (name, scale, mh, _, _, _, _, _), H, W in _images():
        ytab = C.band_table(scale, mh, H)
        taps = C.upper_taps(C.source_scale(scale, mh, H), H, mh)
        assert ytab[0] == 0 and ytab[-1] == H and np.all(np.diff(ytab) >= 0)
        for k in range(mh):
            assert np.all(taps[ytab[k]:ytab[k + 1]] == k), (name, k)


def test_walk_choice_and_band_geometry():
    walk = {n: [C.takes_band_walk(C.CASES[BY_NAME[n]][2], H) for H, _ in C.CASES[BY_NAME[n]][5]] for n in C.NAMES}
    assert walk["h55_raster"] == [False, False] and walk["h56_band"] == [True]
    h = _heights("h56_band")  # band 0 is clamped at the source's top (3 rows), the last band ends with the image (1 row)
    assert h[0] == 3 and h[-1] == 1 and set(h[1:-1]) == {2}
    assert walk["identity"] == [False] and np.array_equal(C.band_table(0, 28, 28), np.arange(29))
    assert walk["down_unstaged"] == [False] and not C.raster_chunk_staged(0, 28, 28, 20, 17, 0)
    assert not C.raster_chunk_staged(0, 28, 28, 55, 63, 0) and all(C.raster_chunk_staged(0, 28, 28, 55, 300, k) for k in range(9))
    assert walk["x2p5"] == [True] and set(_heights("x2p5")[1:-1]) == {2, 3}
    assert walk["band16"] == [True] and _heights("band16").tolist() == [24, 16, 16, 8]
    assert walk["band32"] == [True] and _heights("band32").tolist() == [48, 32, 32, 16]
    assert walk["band33"] == [True] and _heights("band33").tolist() == [50, 34, 33, 17]  # the 32-row flush inside a band
    h = _heights("crop_h1")
    assert walk["crop_h1"] == [True] and h[7] == 1 and np.all(h[8:] == 0) and np.all(h[:7] > 0)
    h = _heights("crop_heavy")
    assert walk["crop_heavy"] == [True] and (h == 0).sum() > len(h) // 2
    assert walk["x8_raster"] == [False] and C.CASES[BY_NAME["x8_raster"]][1] == 8
    assert walk["tall_band"] == [True] and _heights("tall_band").tolist() == [C.EV_BAND_MAX_H]
    assert walk["tall_raster"] == [False] and C.CASES[BY_NAME["tall_raster"]][5] == [(C.EV_BAND_MAX_H + 1, 8)]
    assert walk["mh1"] == [True, False] and walk["mw1"] == [True, False] and walk["w1"] == [True, False]
    assert C.CASES[BY_NAME["mh1"]][2] == 1 and C.CASES[BY_NAME["mw1"]][3] == 1
    # over the band-walk images: every remainder of the 4-row pass, a whole GT group, a whole word, more than a word
    hs = np.concatenate([C.band_heights(c[1], c[2], H) for _, _, c, H, _ in _band_images()])
    assert {int(v) % 4 for v in hs if v > 0} == {0, 1, 2, 3}
    assert {1, 16, 32} <= set(hs.tolist()) and hs.max() > 32 and (hs == 0).any()
    assert {1, 63, 64, 65, 130} <= {W for _, _, _, _, W in _band_images()}


def test_units_per_wave():
    """a case with mh * ceil(W / 64) >= 32 and not a multiple of 16: waves take up to four units and not all the same number"""
    name, scale, mh, mw, nq, sizes, _, _ = C.CASES[BY_NAME["crop_h1"]]
    (H, W), = sizes
    units = mh * ((W + 63) // 64)
    upw = C.units_per_wave(mh, W, H * W)
    assert units >= 32 and units % 16 != 0 and sum(upw) == units
    assert max(upw) == C.EV_UPW and min(upw) >= 2 and upw[-1] < upw[0]
    seen = set()
    for _, _, c, H, W in _band_images():
        seen |= set(C.units_per_wave(c[2], W, max(h * w for h, w in c[5])))
    assert {0, 1, 2, 3, 4} <= seen  # idle waves included (fewer units than waves)


def test_mixed_batch():
    name, scale, mh, mw, nq, sizes, _, _ = C.CASES[C.MIXED]
    assert (30, 40) in sizes and not C.takes_band_walk(mh, 30)
    largest = max(H * W for _, _, c, H, W in _band_images() if c[2] == mh)  # of the band images of 28-row masks
    assert max(h * w for h, w in sizes) == largest and C.takes_band_walk(mh, max(sizes, key=lambda s: s[0] * s[1])[0])


GT_KINDS = ["empty", "full", "px00", "pxlast", "allbut1", "col0", "row0", "half_even", "half_odd", "cy_first", "cy_inside", "cx64"]


@pytest.mark.parametrize("kind", GT_KINDS)
def test_ground_truth_kinds(kind):
    walks = set()
    for i, b, (name, scale, mh, mw, nq, sizes, _, gk), H, W in _images(lambda c: c[7] == kind):
        gt = C.build_case(i)[2][b]
        band = C.takes_band_walk(mh, H)
        walks.add(band)
        ys, xs = np.nonzero(gt)
        n = len(ys)
        X, Y = C.centroid(gt)
        ytab = C.band_table(scale, mh, H)
        if kind == "empty":
            assert n == 0 and nq > 1
            orc = C.oracle_case(i)[b]
            assert orc[2] == 0 and np.all(orc[3] == 0)  # every IoU 0: the upper bound is query 0
        elif kind == "full":
            assert n == H * W
        elif kind == "px00":
            assert n == 1 and (X, Y) == (0, 0)
        elif kind == "pxlast":
            assert n == 1 and (X, Y) == (W - 1, H - 1)
        elif kind == "allbut1":
            assert n == H * W - 1
        elif kind == "col0":
            assert n == H and X == 0
        elif kind == "row0":
            assert n == W and Y == 0
        elif kind in ("half_even", "half_odd"):  # both quotients exactly k + 0.5: round half to even
            assert n == 2 and xs.sum() % 2 == 1 and ys.sum() % 2 == 1
            kx, ky = xs.sum() // 2, ys.sum() // 2
            par = 0 if kind == "half_even" else 1
            assert kx % 2 == par and ky % 2 == par and (X, Y) == (kx + par, ky + par)
        elif kind == "cy_first" and band:
            assert ys.sum() % n == 0 and Y == ys.sum() // n and Y in ytab[:-1] and 0 < Y
        elif kind == "cy_inside" and band:
            k = np.searchsorted(ytab, Y, side="right") - 1
            assert ys.sum() % n == 0 and ytab[k] < Y < ytab[k + 1] - 1
        elif kind == "cx64":
            assert xs.sum() % n == 0 and X == 64
    assert walks == {True, False}, kind  # each on a band-walk and a raster-walk image


def test_threshold_valued_masks():
    below, above = np.nextafter(C.THR, np.float32(-1)), np.nextafter(C.THR, np.float32(2))
    for name, images in (("blocks", (0, 1)), ("blocks_x8", (0,))):
        i = BY_NAME[name]
        masks = C.build_case(i)[0]
        for m in masks.reshape(-1, *masks.shape[2:]):  # no two blocks of a query alike: no constant plateau beyond a block
            v = m[::2, ::2]
            assert len(np.unique(v)) == v.size and np.array_equal(np.repeat(np.repeat(v, 2, 0), 2, 1), m)
            assert np.all(np.isin(v, np.concatenate([C.THR, [0.5, C.HALF_LO, C.HALF_HI]]).astype(np.float32)))
        for b in images:
            pm, q_star, ub = C.oracle_case(i)[b][:3]
            pm = pm.numpy()
            # the query kernel compares every query with 0.5
            assert min((pm == 0.5).sum(), (pm == C.HALF_LO).sum(), (pm == C.HALF_HI).sum()) >= 10, (name, b)
            for q in (q_star, ub):  # the metrics kernel bins the selected masks
                on, lo, hi = np.isin(pm[q], C.THR).sum(), np.isin(pm[q], below).sum(), np.isin(pm[q], above).sum()
                assert on >= 100 and lo >= 10 and hi >= 10, (name, b, q, on, lo, hi)
    assert [C.takes_band_walk(28, H) for H, _ in C.CASES[BY_NAME["blocks"]][5]] == [True, False]


def test_dark_and_saturated_masks():
    i = BY_NAME["dark"]
    for b, (pm, q_star, ub, _, mets) in enumerate(C.oracle_case(i)):
        for k, q in enumerate((q_star, ub)):  # adaptive threshold below 1 and an f_mean that is not trivially 0
            assert 2 * pm[q].double().mean() < 0.9 and mets[k][4] > 0.5, (b, k)
    i = BY_NAME["sat"]
    for b, (pm, q_star, ub, _, _) in enumerate(C.oracle_case(i)):
        for q in (q_star, ub):
            assert (pm[q] == 0).sum() >= 100 and (pm[q] == 1).sum() >= 100, (b, q)
    for name in ("tall_band", "tall_raster"):  # an all-ones query against a dense GT: per-lane counts in the thousands
        (pm, q_star, ub, _, _), = C.oracle_case(BY_NAME[name])
        gt = C.build_case(BY_NAME[name])[2][0]
        assert ub == 0 and q_star != 0 and bool((pm[0] == 1).all()) and gt[:, 0].sum() > 8192


def test_selection_cases():
    i = BY_NAME["iou_tie"]
    masks = C.build_case(i)[0]
    for b, (_, _, ub, ious, _) in enumerate(C.oracle_case(i)):
        assert np.array_equal(masks[b, 1], masks[b, 3]) and ious[1] == ious[3] == ious.max() and ious[0] < ious[1] > ious[2]
        assert ub == 1  # the first maximum, as torch.argmax
    band_nq = {c[4] for _, _, c, _, _ in _band_images()}
    assert {1, 4, 21, 32, 64} <= band_nq


def _selected():
    for i, b, case, H, W in _images():
        pm, q_star, ub, _, mets = C.oracle_case(i)[b]
        gt = C.build_case(i)[2][b]
        for k, q in enumerate((q_star, ub)):
            yield f"{case[0]}[{b}].{'pick' if k == 0 else 'ub'}", pm[q].numpy(), gt, mets[k]


def test_adaptive_threshold_margin():
    """Input condition: no pixel of a selected mask within a relative 1e-5 of 2 * mean.  The kernel rounds an fp64 sum, torch sums in
    fp32: a pixel between the two thresholds would flip f_mean without either side being wrong."""
    for tag, p, _, _ in _selected():
        thr = 2 * p.astype(np.float64).mean()
        assert np.abs(p.astype(np.float64) - thr).min() > 1e-5 * thr, tag


def test_s_measure_branches_are_robust():
    """Input condition: every quadrant takes the same ssim branch in float64 as in the oracle's float32 (alpha != 0; alpha == 0 and
    beta == 0; otherwise), the centroid is the same, and the oracle's own rounding leaves room inside the parity tolerance."""
    seen = set()
    for tag, p, gt, mets in _selected():
        s64, br64 = C.s_measure_f64(p, gt)
        f32 = C.ssim_branches_f32(p, gt)
        assert (br64 is None) == (f32 is None), tag
        if f32 is not None:
            X, Y = C.centroid(gt)
            assert (f32[0], f32[1]) == (X, Y) and f32[2] == br64, (tag, f32, br64, X, Y)
            seen |= set(br64)
        assert (np.isnan(s64) and np.isnan(mets[6])) or abs(s64 - mets[6]) <= 1e-5, (tag, s64, mets[6])
    assert seen == {0, 1, 2}


def test_plateau_is_the_documented_trap():
    """plateau_case() is the input the parity table must not contain: the float32 oracle and the exact formula take different branches"""
    import torch
    from oracle import evaluator_oracle as E
    mask, obj, (gt,) = C.plateau_case()
    pm = E.postprocess(torch.from_numpy(mask[0]), torch.from_numpy(obj[0]), torch.from_numpy(gt.astype(np.int64)))[0][0]
    assert len(torch.unique(pm)) == 1 and 0 < float(pm[0, 0]) < 1
    s64, br64 = C.s_measure_f64(pm.numpy(), gt)
    _, _, br32 = C.ssim_branches_f32(pm.numpy(), gt)
    assert br64[1] == br64[2] == 1 and br32[1] == br32[2] == 2  # the quadrants without ground truth: ssim 1 exactly, 0 in float32
    s32 = E.s_measure(pm, torch.from_numpy(gt).float())
    assert abs(s64 - s32) > 0.1  # up to half the weight of the quadrants without ground truth
