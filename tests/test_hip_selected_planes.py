"""The selected query's mask up-sampled to each image's own size (csrc/selected.hip behind ``ops.upsample_selected``,
``ops.upsample_selected_native`` and ``ops.upsample_selected_u8``): one plane kernel in three layouts and two stores, at the edges
of its walk - tails, the 256-pixel workgroup, a second trip round the grid-stride loop, workgroups past a small image's extent.

Bounds.  The fp64 planes against torch on the CPU: rtol 1e-6, atol 1e-7, as test_upsample_selected_native (test_hip_bilateral_mixed.py).
A crop moves no source index: equal.  The 8-bit planes against the fp64 planes: ``_compare_planes`` - at most one step, and only
where the value times 255 lies within 1e-4 of an integer; its share cap is met by the reference alone for these seeds (counted on
the CPU against F.interpolate, within 2e-4: 0 of 2764 pixels (A), 0 of 14208 (B), 49 of 139422 (C), 1 of 13130 (R)), so the
seeds stay.  The predictor's soft and binary planes: equal."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _mask_planes import _compare_planes, _masks  # noqa: E402
from selfmask_amd import ops  # noqa: E402
from selfmask_amd.bilateral_solver import MixedBatch  # noqa: E402

DEV = "cuda:0"
NQ = 3
# name: (seed, k (0: resize mode), (mh, mw), sizes)
CASES = {
    "A": (301, 4, (5, 7), [(20, 28), (1, 1), (20, 1), (1, 28), (13, 20), (19, 27)]),  # tails
    "B": (303, 8, (3, 33), [(1, 255), (1, 256), (1, 257), (24, 264)]),                 # edges of the 256-pixel workgroup
    "C": (303, 8, (33, 33), [(264, 264), (3, 5)]),  # 69696 pixels > 256 x 256: a second trip; workgroups past the small image
    "R": (303, 0, (7, 5), [(3, 4), (1, 1), (97, 61), (3, 200), (7, 5)]),               # down-sample, identity, up-sample
}
WHICH = ("pick", "ub")


def _col(which):
    return 14 if which == "pick" else 15


@functools.lru_cache(maxsize=None)
def _inputs(name, spread=1.0):
    """host arrays and device tensors of a case, drawn once (the second draw, spread 1.3, from the next seed)"""
    seed, k, (mh, mw), sizes = CASES[name]
    masks, obj, rows = _masks(seed if spread == 1.0 else seed + 1000, len(sizes), NQ, mh, mw, spread)
    return masks, obj, rows, tuple(torch.from_numpy(a).to(DEV) for a in (masks, obj, rows))


@functools.lru_cache(maxsize=None)
def _reference(name, which, spread=1.0):
    """torch on the CPU, per image: F.interpolate(scale_factor=k)[..., :h, :w] (scale mode) or F.interpolate(size=(h, w)), as fp64"""
    _, k, _, sizes = CASES[name]
    masks, _, rows, _ = _inputs(name, spread)
    out = []
    for b, (h, w) in enumerate(sizes):
        m = torch.from_numpy(masks[b, int(rows[b, _col(which)])])[None, None]
        kw = dict(scale_factor=k) if k else dict(size=(h, w))
        out.append(F.interpolate(m, mode="bilinear", align_corners=False, **kw)[0, 0, :h, :w].double().numpy())
    return out


def _f64_planes(name, which, spread=1.0):
    """the device's fp64 plane of every image: the native (packed) planes in scale mode, one size-mode call per size otherwise"""
    _, k, _, sizes = CASES[name]
    mp, _, rw = _inputs(name, spread)[3]
    if k:
        mb = MixedBatch(sizes, DEV)
        return [v.cpu().numpy() for v in mb.views(ops.upsample_selected_native(mp, rw, mb, float(k), which))]
    return [ops.upsample_selected(mp, rw, s, which)[b].cpu().numpy() for b, s in enumerate(sizes)]


def _gt_batch(sizes):
    return ops.GtBatch([torch.zeros(s, dtype=torch.uint8) for s in sizes], torch.device(DEV))


def _close(got, ref, label):
    assert got.dtype == np.float64 and got.shape == ref.shape, label
    print(f"\n{label}: max|device - F.interpolate| = {np.abs(got - ref).max():.2e}")
    assert np.allclose(got, ref, rtol=1e-6, atol=1e-7), label


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("name", list(CASES))
def test_f64_planes_equal_torch(name, which):
    _, k, (mh, mw), sizes = CASES[name]
    planes, ref = _f64_planes(name, which), _reference(name, which)
    for b, (h, w) in enumerate(sizes):
        _close(planes[b], ref[b], f"{name} {which} image {b} {h}x{w}")
    if k:  # size mode at the whole grid: the same source ratio 1 / k; a crop moves no source index
        masks, _, rows, (mp, _, rw) = _inputs(name)
        full = ops.upsample_selected(mp, rw, (k * mh, k * mw), which).cpu().numpy()
        for b, (h, w) in enumerate(sizes):
            q = int(rows[b, _col(which)])
            whole = F.interpolate(torch.from_numpy(masks[b, q])[None, None], scale_factor=k, mode="bilinear", align_corners=False)[0, 0]
            _close(full[b], whole.double().numpy(), f"{name} {which} image {b} whole grid")
            assert np.array_equal(planes[b], full[b, :h, :w]), (name, which, b)


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("name", list(CASES))
def test_u8_planes_follow_the_f64_planes(name, which):
    _, k, _, sizes = CASES[name]
    mp, _, rw = _inputs(name)[3]
    gb = _gt_batch(sizes)
    u8 = ops.upsample_selected_u8(mp, rw, gb, float(k), which).cpu().numpy()
    f64 = np.concatenate([p.reshape(-1) for p in _f64_planes(name, which)])  # GtBatch lays its planes end to end too
    assert u8.dtype == np.uint8 and u8.shape == f64.shape and gb.offsets == list(MixedBatch(sizes, DEV).px_off)
    _compare_planes(u8, f64, f"{name} {which}")


@pytest.mark.parametrize("name", list(CASES))
def test_picked_planes_are_the_predictors(name):
    """a draw that is clipped at both ends: the 8-bit plane is the predictor's soft plane, the predictor's binary plane is f64 > 0.5"""
    _, k, _, sizes = CASES[name]
    mp, ob, rw = _inputs(name, 1.3)[3]
    gb = _gt_batch(sizes)
    res = ops.predict_masks(mp, ob, ops.PackedImages(sizes, DEV), float(k), rle=False, binary=True, soft=True).result()
    assert res["best"] == [int(q) for q in _inputs(name, 1.3)[2][:, 14]]
    u8 = ops.upsample_selected_u8(mp, rw, gb, float(k), "pick").cpu().numpy()
    f64, ref = _f64_planes(name, "pick", 1.3), _reference(name, "pick", 1.3)
    assert (u8 == 0).any() and (u8 == 255).any(), name
    for b, (h, w) in enumerate(sizes):
        _close(f64[b], ref[b], f"{name} spread 1.3 image {b}")
        assert np.array_equal(u8[gb.offsets[b]:gb.offsets[b] + h * w].reshape(h, w), res["soft"][b]), (name, b)
        assert np.array_equal(res["binary"][b], (f64[b] > 0.5).astype(np.uint8)), (name, b)


@pytest.mark.parametrize("which", WHICH)
def test_strided_last_layer_view(which):
    """the masks as ``[:, -1]`` of a (B, L, nq, mh, mw) tensor: the bytes of the contiguous copy, from all three entry points"""
    _, k, (mh, mw), sizes = CASES["A"]
    mp, _, rw = _inputs("A")[3]
    layers = torch.full((len(sizes), 3, NQ, mh, mw), 0.25, device=DEV)
    layers[:, -1] = mp
    view = layers[:, -1]
    assert not view.is_contiguous() and view.stride(0) == 3 * NQ * mh * mw
    mb, gb = MixedBatch(sizes, DEV), _gt_batch(sizes)
    for f in (lambda m: ops.upsample_selected(m, rw, (k * mh, k * mw), which),
              lambda m: ops.upsample_selected_native(m, rw, mb, float(k), which),
              lambda m: ops.upsample_selected_u8(m, rw, gb, float(k), which),
              lambda m: ops.upsample_selected_u8(m, rw, gb, 0.0, which)):
        assert torch.equal(f(view), f(mp))


def test_a_misspelt_which_is_refused():
    _, k, _, sizes = CASES["A"]
    mp, _, rw = _inputs("A")[3]
    with pytest.raises(ValueError):
        ops.upsample_selected(mp, rw, sizes[0], "best")
    with pytest.raises(ValueError):
        ops.upsample_selected_native(mp, rw, MixedBatch(sizes, DEV), float(k), "best")
    with pytest.raises(ValueError):
        ops.upsample_selected_u8(mp, rw, _gt_batch(sizes), float(k), "best")
