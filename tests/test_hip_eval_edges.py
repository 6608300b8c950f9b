"""The evaluator's metric kernels (eval.hip) on the edge-case table of _eval_cases.py: degenerate ground truths, values on the
thresholds, every band height and both walks, against the CPU oracle with test_hip_eval.py's tolerances unchanged.
test_eval_cases_cpu.py shows which branch each case reaches and that no input sits where the float32 reference and an exact
evaluation may legitimately disagree."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _eval_cases as C  # noqa: E402
from selfmask_amd import ops  # noqa: E402

DEV = "cuda:0"
EXACT = [0, 1, 2, 3]  # iou, pixel_acc, f_score, f_max depend only on integer counts: bit-exact


def _evaluate(masks, objs, gts, scale):
    rows, ious = ops.evaluate_masks(torch.from_numpy(np.ascontiguousarray(masks)).to(DEV), torch.from_numpy(np.ascontiguousarray(objs)).to(DEV),
                                    [torch.from_numpy(g).to(DEV) for g in gts], scale=scale, return_ious=True)
    return rows.cpu().numpy(), ious.cpu().numpy()


@pytest.mark.parametrize("name", C.NAMES)
def test_edge_case_matches_oracle(name):
    i = C.NAMES.index(name)
    masks, objs, gts = C.build_case(i)
    rows, ious = _evaluate(masks, objs, gts, C.CASES[i][1])
    failures = []
    for b, (_, q_star, ub, ref_ious, mets) in enumerate(C.oracle_case(i)):  # as _check_rows of test_hip_eval.py
        ok = int(rows[b, 14]) == q_star and int(rows[b, 15]) == ub and np.array_equal(ious[b], ref_ious)
        for k in range(2):
            ref, got = mets[k], rows[b, 7 * k: 7 * k + 7].astype(np.float64)
            ok = ok and np.array_equal(got[EXACT], ref[EXACT]) and np.allclose(got[[4, 5]], ref[[4, 5]], rtol=1e-6, atol=1e-7)
            ok = ok and np.allclose(got[6], ref[6], rtol=0, atol=2e-5, equal_nan=True)
        if not ok:
            failures.append((b, gts[b].shape, rows[b].tolist(), q_star, ub, [m.tolist() for m in mets], ious[b].tolist(), ref_ious.tolist()))
    assert not failures, failures


def test_a_row_does_not_depend_on_its_neighbours():
    """band_walk(): the walk is chosen per image.  Every image of the mixed batch alone, inside the batch and inside the reversed
    batch: the same 16 floats, bit for bit."""
    masks, objs, gts = C.build_case(C.MIXED)
    scale = C.CASES[C.MIXED][1]
    fwd, _ = _evaluate(masks, objs, gts, scale)
    rev, _ = _evaluate(masks[::-1], objs[::-1], gts[::-1], scale)
    B = len(gts)
    for b in range(B):
        alone, _ = _evaluate(masks[b: b + 1], objs[b: b + 1], gts[b: b + 1], scale)
        assert np.array_equal(alone[0].view(np.uint32), fwd[b].view(np.uint32)), (b, alone[0], fwd[b])
        assert np.array_equal(alone[0].view(np.uint32), rev[B - 1 - b].view(np.uint32)), (b, alone[0], rev[B - 1 - b])


# ---- the constant plateau (evaluator: "constant plateaus in the S-measure") -------------------------------------------
# On a quadrant without ground truth and a prediction of exactly one value c not in {0, 1} the S-measure is ill-conditioned on
# both sides: ssim is 1 if the quadrant's variance comes out exactly 0 and 0 otherwise.  torch's fp32 mean is not c, so the
# reference gives 0.  The kernel's mean is c, and its one-pass variance is sum p^2 - fl(n c^2): 0 only when the rounding of the
# fp64 partial sums of p^2 (c^2 has up to 48 significant bits) lands on the rounded product - which depends on c, the quadrant's
# size and the walk's summation order.  Measured on plateau_case()'s two quadrants without ground truth (ssim upper right, lower
# left):          c =  0.7   0.3   0.9   0.6   0.55  0.45  0.8   0.2
#   band walk          1,1   0,1   0,1   0,1   0,1   0,1   1,1   1,1
#   raster walk        0,0   0,1   0,1   0,1   0,0   0,1   0,0   0,0
def _plateau_expectations(c):
    """(the float64 value of the formula, the four values with ssim 0 or 1 on each quadrant without ground truth) on the oracle's
    up-sample of the constant mask"""
    import itertools
    from oracle import evaluator_oracle as E
    mask, obj, (gt,) = C.plateau_case(c)
    pm = E.postprocess(torch.from_numpy(mask[0]), torch.from_numpy(obj[0]), torch.from_numpy(gt.astype(np.int64)))[0][0].numpy()
    assert len(np.unique(pm)) == 1 and pm[0, 0] == np.float32(c)  # the up-sample is the plateau itself
    s64, branches = C.s_measure_f64(pm, gt)
    assert [branches[k] for k in C.PLATEAU_FREE] == [1, 1]
    return s64, [C.s_measure_f64(pm, gt, force=dict(zip(C.PLATEAU_FREE, v)))[0] for v in itertools.product((0.0, 1.0), repeat=2)]


def test_plateau_at_0p7_gives_the_exact_formula():
    """A 28 x 28 mask of 0.7 at 300 x 400 on the product's walk (the band walk) against the float64 evaluation of the formula,
    not against the float32 oracle.  This pins ONE constant on ONE geometry and walk: here the rounded sum of p^2 equals the rounded
    n c^2 in both quadrants without ground truth, so the variance is exactly 0 and ssim 1.  It is no property of the kernel (see the
    table above: other constants, and the raster walk at this one, take the reference's branch): a change of the fp64 summation
    order may move this value to another entry of test_plateau_takes_one_of_the_two_branches's set, and then this pin moves with it."""
    mask, obj, gts = C.plateau_case()
    rows, _ = _evaluate(mask, obj, gts, 0)
    s64, _ = _plateau_expectations(0.7)
    assert abs(float(rows[0, 6]) - s64) <= 2e-5, (rows[0, 6], s64)


@pytest.mark.parametrize("c", (0.7,) + C.PLATEAU_OTHERS)
def test_plateau_takes_one_of_the_two_branches(c):
    """What does hold on a plateau, for any constant: each quadrant without ground truth contributes ssim 0 (the reference's
    branch) or 1 (the exact one) - the S-measure is one of four values, everything else in it at the usual 2e-5."""
    mask, obj, gts = C.plateau_case(c)
    rows, _ = _evaluate(mask, obj, gts, 0)
    _, allowed = _plateau_expectations(c)
    assert min(abs(float(rows[0, 6]) - v) for v in allowed) <= 2e-5, (c, rows[0, 6], allowed)


_CHILD = r"""
import json, os, sys
import numpy as np, torch
root = sys.argv[1]
sys.path[:0] = [os.path.join(root, "salient-object-detection_amd"), root, os.path.join(root, "tests")]
import _eval_cases as C
from selfmask_amd import ops
out = {}
for i, (name, scale, mh, mw, nq, sizes, _, _) in enumerate(C.CASES):
    keep = [b for b, (H, W) in enumerate(sizes) if C.takes_band_walk(mh, H)]
    if not keep:
        continue
    masks, objs, gts = C.build_case(i)
    rows, ious = ops.evaluate_masks(torch.from_numpy(masks[keep]).cuda(), torch.from_numpy(objs[keep]).cuda(),
                                    [torch.from_numpy(gts[b]).cuda() for b in keep], scale=scale, return_ious=True)
    out[name] = {"rows": rows.cpu().numpy().view(np.uint32).tolist(), "ious": ious.cpu().numpy().view(np.uint32).tolist()}
plateau = {}
for c in (0.7,) + C.PLATEAU_OTHERS:
    mask, obj, gts = C.plateau_case(c)
    rows = ops.evaluate_masks(torch.from_numpy(mask).cuda(), torch.from_numpy(obj).cuda(), [torch.from_numpy(gts[0]).cuda()], scale=0)
    plateau[repr(c)] = rows[0].cpu().numpy().view(np.uint32).tolist()
print("ROWS" + json.dumps({"cases": out, "plateau": plateau}))
"""
_WALKS = {}


def _both_walks():
    """the table's band-walk images and the plateaus through the product library (band walk) and through the tuning library with
    the raster walk forced (SM_EVAL_BAND_MIN=0): one child process per walk, run once for the tests below"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tuning = os.path.join(root, "salient-object-detection_amd", "lib", "libselfmask_hip_tuning.so")
    if not os.path.exists(tuning):
        pytest.skip("tuning library not built (salient-object-detection_amd/build.py --tuning)")
    if not _WALKS:
        for tag, env in (("band", {}), ("raster", {"SM_HIP_LIB": tuning, "SM_EVAL_BAND_MIN": "0"})):
            p = subprocess.run([sys.executable, "-c", _CHILD, root], env={**os.environ, **env}, capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, p.stderr[-2000:]
            _WALKS[tag] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("ROWS")][0][4:])
    return _WALKS


def test_both_walks_agree_on_every_band_case():
    """integer-count metrics, IoUs and selections bit-identical, the fp64-sum metrics to the last fp32 digit"""
    res = {tag: r["cases"] for tag, r in _both_walks().items()}
    assert len(res["band"]) >= 30 and set(res["band"]) == set(res["raster"])
    bad = []
    for name in res["band"]:
        a = np.array(res["band"][name]["rows"], np.uint32).view(np.float32)
        b = np.array(res["raster"][name]["rows"], np.uint32).view(np.float32)
        exact, rest = [0, 1, 2, 3, 7, 8, 9, 10, 14, 15], [4, 5, 6, 11, 12, 13]
        if not (res["band"][name]["ious"] == res["raster"][name]["ious"] and np.array_equal(a[:, exact], b[:, exact]) and
                np.allclose(a[:, rest], b[:, rest], rtol=3e-7, atol=0, equal_nan=True)):
            bad.append((name, a.tolist(), b.tolist()))
    assert not bad, bad


def test_plateau_on_both_walks():
    """On a plateau the two walks add p^2 in different orders and need NOT take the same ssim branch (the table above: they differ
    at 0.7, 0.55, 0.8 and 0.2).  What holds: each walk's S-measure is one of the four allowed values, and everything but the
    S-measure agrees as on any other input."""
    res = {tag: r["plateau"] for tag, r in _both_walks().items()}
    for c in (0.7,) + C.PLATEAU_OTHERS:
        a = np.array(res["band"][repr(c)], np.uint32).view(np.float32)
        b = np.array(res["raster"][repr(c)], np.uint32).view(np.float32)
        _, allowed = _plateau_expectations(c)
        for tag, row in (("band", a), ("raster", b)):
            assert min(abs(float(row[6]) - v) for v in allowed) <= 2e-5, (c, tag, row[6], allowed)
        assert np.array_equal(a[[0, 1, 2, 3, 14, 15]], b[[0, 1, 2, 3, 14, 15]]) and np.allclose(a[[4, 5]], b[[4, 5]], rtol=3e-7, atol=0), (c, a, b)
