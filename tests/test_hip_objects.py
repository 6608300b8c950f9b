"""Objects of a mask on the device (csrc/objects.hip: sm_mask_objects behind ``ops.predict_masks(objects=)`` and
``ops.rle_runs_packed_async(objects=)``) against the host restatement (tests/_objects_ref.py) applied to the device's own binary and
soft planes of the same call.  Everything compared is an integer (or a quotient of two), so every comparison is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _objects_ref as R  # noqa: E402
from selfmask_amd import ops  # noqa: E402

DEV = "cuda:0"
LDS_SEGS = 3072  # OB_LDS_SEGS: images whose segment bound is larger work in the global workspace


def _as_masks(planes, seed=0):
    """0/1 planes of any sizes -> (B, 1, Hmax, Wmax) probabilities for scale = 1: > 0.5 exactly where the plane is set, the soft values
    varied so that a wrong pixel in ``mass`` shows"""
    rng = np.random.Generator(np.random.PCG64(seed))
    Hm, Wm = max(p.shape[0] for p in planes), max(p.shape[1] for p in planes)
    m = np.zeros((len(planes), 1, Hm, Wm), np.float32)
    for b, p in enumerate(planes):
        r = rng.random(p.shape).astype(np.float32)
        m[b, 0, :p.shape[0], :p.shape[1]] = np.where(p != 0, 0.55 + 0.45 * r, 0.45 * r)
    return torch.from_numpy(m)


def _run(planes, cap=8192, **opts):
    """-> (result of the call with binary and soft planes, the reference's objects of those planes)"""
    planes = [np.asarray(p, np.uint8) for p in planes]
    masks = _as_masks(planes).to(DEV)
    obj = torch.ones((len(planes), 1), device=DEV)
    table = ops.PackedImages([p.shape for p in planes], DEV)
    res = ops.predict_masks(masks, obj, table, 1.0, rle=True, binary=True, soft=True, cap=cap, objects=opts).result()
    for b, p in enumerate(planes):
        assert np.array_equal(res["binary"][b], p), b  # the case is the one the test names
    return res, [R.objects(res["binary"][b], res["soft"][b], **opts) for b in range(len(planes))]


def _check(planes, cap=8192, **opts):
    res, ref = _run(planes, cap, **opts)
    for b, want in enumerate(ref):
        got = res["objects"][b]
        assert got == want, (b, {k: (got[k], want[k]) for k in want if k != "objects" and got[k] != want[k]},
                             [(g, w) for g, w in zip(got["objects"], want["objects"]) if g != w][:2])
    return res["objects"]


def _seam_planes():
    two = np.zeros((5, 3), np.uint8)
    two[4, 0] = two[0, 1] = 1  # the end of column 0 and the start of column 1: adjacent positions, not neighbours
    return [two, np.ones((6, 9), np.uint8), np.zeros((7, 5), np.uint8), np.ones((1, 1), np.uint8), np.zeros((1, 1), np.uint8),
            np.tile(np.array([1, 1, 0], np.uint8), 24)[None, :70], np.tile(np.array([1, 0, 1, 1], np.uint8), 18)[:70, None],
            np.ones((3, 150), np.uint8), _long_runs()]


def _long_runs():
    """runs that cross many columns and start and end inside one: emitted by a whole wave, beside short runs emitted by one lane"""
    p = np.ones((4, 90), np.uint8)
    p[2, 3] = p[1, 40] = p[3, 41] = p[0, 89] = 0
    p[:, 60] = 0
    p[1, 60] = 1
    return p


@pytest.mark.parametrize("connectivity", [4, 8])
def test_column_seams_and_degenerate_planes(connectivity):
    got = _check(_seam_planes(), connectivity=connectivity, max_objects=64)
    assert got[0]["n_components"] == 2 and [o["area"] for o in got[0]["objects"]] == [1, 1]
    assert got[1]["n_components"] == 1 and got[1]["objects"][0]["area"] == 54 and got[1]["bbox"] == [0, 0, 9, 6]
    assert got[1]["spans"] == {"top_bottom": True, "left_right": True}
    assert got[2]["n_components"] == 0 and got[2]["bbox"] is None and got[2]["objects"] == []
    assert got[3]["n_components"] == 1 and got[4]["n_components"] == 0
    assert got[5]["n_components"] == 24 and got[6]["n_components"] == 18  # one row, one column
    assert got[7]["n_components"] == 1 and got[7]["objects"][0]["area"] == 450  # ONE run of 150 segments
    assert got[8]["n_components"] == 1 and got[8]["objects"][0]["area"] == 353


def test_connectivity_on_a_diagonal_staircase():
    p = np.eye(23, dtype=np.uint8)
    assert _check([p, p[::-1]], connectivity=4, max_objects=64)[0]["n_components"] == 23
    got = _check([p, p[::-1]], connectivity=8, max_objects=64)
    assert got[0]["n_components"] == 1 and got[1]["n_components"] == 1 and got[1]["objects"][0]["area"] == 23


def _spiral(n):
    """a one-pixel path that winds inwards with a one-pixel gap between its turns"""
    p = np.zeros((n, n), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    p[0, 0] = 1
    while True:
        for _ in range(2):  # straight on, or one turn to the right
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and not p[ny, nx] and not (0 <= fy < n and 0 <= fx < n and p[fy, fx]):
                break
            dy, dx = dx, -dy
        else:
            return p
        y, x = ny, nx
        p[y, x] = 1


@pytest.mark.parametrize("connectivity", [4, 8])
def test_late_merges_comb_and_spiral(connectivity):
    comb = np.zeros((41, 37), np.uint8)
    comb[::2, :] = 1
    comb[:, -1] = 1  # 21 teeth that meet in the last column only
    spiral = _spiral(33)
    got = _check([comb, comb[:, ::-1], spiral, spiral.T[::-1]], connectivity=connectivity, max_objects=64)
    assert [g["n_components"] for g in got] == [1, 1, 1, 1]
    assert got[0]["objects"][0]["area"] == int(comb.sum()) and got[2]["objects"][0]["area"] == int(spiral.sum())


def _ranking_plane():
    p = np.zeros((24, 31), np.uint8)
    for (y, x) in ((14, 2), (3, 9), (9, 20), (1, 27)):  # equal areas whose raster order is not their column order
        p[y:y + 2, x:x + 2] = 1
    p[18:21, 12:15] = 1  # the largest
    for (y, x) in ((0, 0), (23, 30), (7, 15), (22, 3)):  # specks
        p[y, x] = 1
    return p


def test_ranking_min_area_and_max_objects():
    p = _ranking_plane()
    every = _check([p], connectivity=4, max_objects=64)[0]
    assert every["n_components"] == 9 and [o["area"] for o in every["objects"]] == [9, 4, 4, 4, 4, 1, 1, 1, 1]
    firsts = [o["first"] for o in every["objects"]]
    assert firsts[1:5] == sorted(firsts[1:5]) and firsts[5:] == sorted(firsts[5:])
    assert [o["bbox"][0] for o in every["objects"][1:5]] == [27, 9, 20, 2]  # by first raster pixel, not by column
    big = _check([p], connectivity=4, min_area=2, max_objects=64)[0]
    assert big["n_components"] == 9 and [o["area"] for o in big["objects"]] == [9, 4, 4, 4, 4]
    top = _check([p], connectivity=4, max_objects=3)[0]
    assert top["n_components"] == 9 and top["objects"] == every["objects"][:3]
    assert _check([p], connectivity=8, min_area=10, max_objects=1)[0]["objects"] == []


def test_positions_across_the_run_kernels_wave_and_workgroup_ranges():
    rng = np.random.Generator(np.random.PCG64(3))
    p = np.kron(rng.random((26, 26)) < 0.45, np.ones((5, 5))).astype(np.uint8)  # 130 x 130 = 16 900 positions: five wave ranges, two workgroups
    assert p.size > 16384
    for connectivity in (4, 8):
        got = _check([p], connectivity=connectivity, max_objects=64)[0]
        assert got["n_components"] > 5


@pytest.mark.parametrize("connectivity", [4, 8])
def test_lds_path_and_global_path_in_one_launch(connectivity):
    yy, xx = np.mgrid[:160, :160]
    big = ((yy + xx) % 2).astype(np.uint8)       # 12 800 segments: the global workspace
    small = big[:64, :64].copy()                 # 2 048 segments (bound 2 111): LDS
    assert big.sum() > LDS_SEGS and small.sum() + 64 <= LDS_SEGS
    got = _check([big, small, big[1:, :]], cap=1 << 15, connectivity=connectivity, max_objects=64)
    want = [12800, 2048, 12720] if connectivity == 4 else [1, 1, 1]
    assert [g["n_components"] for g in got] == want
    if connectivity == 4:
        assert [o["first"] for o in got[0]["objects"]] == list(range(1, 128, 2))  # all of area 1: the first 64 in raster order


def test_cap_retry_covers_the_objects():
    rng = np.random.Generator(np.random.PCG64(11))
    planes = [(rng.random(s) < 0.5).astype(np.uint8) for s in ((40, 50), (33, 47))]
    res, ref = _run(planes, cap=64, connectivity=8, min_area=3, max_objects=32)
    assert min(len(r["counts"]) for r in res["rle"]) > 64  # the run list was truncated at first
    assert res["objects"] == ref
    assert _run(planes, connectivity=8, min_area=3, max_objects=32)[0]["objects"] == ref


def _blobs(rng, n, mh, mw):
    yy, xx = np.mgrid[:mh, :mw].astype(np.float32)
    out = np.zeros((mh, mw), np.float32)
    for _ in range(n):
        cy, cx, ry, rx = rng.uniform(.1, .9) * mh, rng.uniform(.1, .9) * mw, rng.uniform(.08, .2) * mh, rng.uniform(.08, .2) * mw
        out = np.maximum(out, 1 / (1 + np.exp(4 * (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 - 1))))
    return out.astype(np.float32)


@pytest.fixture(scope="module")
def native_batch():
    """three sizes of one 13 x 19 mask at scale 8, widths no multiple of 64; four queries of a few blobs each"""
    rng = np.random.Generator(np.random.PCG64(17))
    sizes = [(100, 150), (97, 141), (90, 130)]
    masks = torch.from_numpy(np.stack([np.stack([_blobs(rng, 4, 13, 19) for _ in range(4)]) for _ in sizes]))
    obj = torch.from_numpy(rng.random((3, 4)).astype(np.float32))
    return sizes, masks.to(DEV), obj.to(DEV)


def test_mixed_batch_in_native_mode(native_batch):
    sizes, masks, obj = native_batch
    opts = dict(connectivity=8, min_area=0, max_objects=16)
    res = ops.predict_masks(masks, obj, ops.PackedImages(sizes, DEV), 8.0, rle=True, binary=True, soft=True, objects=opts).result()
    ref = [R.objects(res["binary"][b], res["soft"][b], **opts) for b in range(3)]
    assert res["objects"] == ref
    assert sum(r["n_components"] for r in ref) >= 4
    assert all(127 / 255 <= o["score"] <= 1 for r in ref for o in r["objects"])  # every pixel of an object is above the threshold
    # the objects alone: no "rle" key, the same objects
    alone = ops.predict_masks(masks, obj, ops.PackedImages(sizes, DEV), 8.0, rle=False, objects=ops.ObjectOptions(**opts)).result()
    assert set(alone) == {"best", "objects"} and alone["objects"] == ref
    # without per-object masks
    bare = ops.predict_masks(masks, obj, ops.PackedImages(sizes, DEV), 8.0, objects=dict(opts, masks=False)).result()
    assert bare["objects"] == [R.objects(res["binary"][b], res["soft"][b], masks=False, **opts) for b in range(3)]
    # and nothing changes for a caller that does not ask
    plain = ops.predict_masks(masks, obj, ops.PackedImages(sizes, DEV), 8.0, rle=True, binary=True, soft=True).result()
    assert set(plain) == {"best", "rle", "binary", "soft"} and plain["rle"] == res["rle"] and plain["best"] == res["best"]


def test_packed_plane_input(native_batch):
    sizes, masks, obj = native_batch
    opts = dict(connectivity=4, min_area=2, max_objects=8)
    table = ops.PackedImages(sizes, DEV)
    pend = ops.predict_masks(masks, obj, table, 8.0, rle=True, binary=True, objects=opts)
    res = pend.result()
    rles, objs = ops.rle_runs_packed_async(pend.binary, table, objects=opts).result()
    assert rles == res["rle"]
    assert objs == [R.objects(res["binary"][b], None, **opts) for b in range(3)]
    for a, b in zip(objs, res["objects"]):
        assert all(o["score"] is None for o in a["objects"])
        assert [{**o, "score": None} for o in b["objects"]] == a["objects"] and {**b, "objects": 0} == {**a, "objects": 0}
    # overflow + retry on the packed path
    assert ops.rle_runs_packed_async(pend.binary, table, cap=8, objects=opts).result() == (rles, objs)
    assert ops.rle_runs_packed_async(pend.binary, table).result() == rles  # unchanged without the option


def test_the_same_call_twice_gives_identical_bytes():
    planes = [_ranking_plane(), _spiral(33), (np.mgrid[:80, :80].sum(0) % 2).astype(np.uint8)]  # the last one: 3 200 segments, the global path
    masks = _as_masks(planes).to(DEV)
    obj = torch.ones((3, 1), device=DEV)
    table = ops.PackedImages([p.shape for p in planes], DEV)
    outs = []
    for _ in range(2):
        pend = ops.predict_masks(masks, obj, table, 1.0, objects=dict(connectivity=4, max_objects=64))
        pend.result()
        o = pend._objects
        torch.cuda.synchronize()
        nseg = o._summary[:, 2].cpu().tolist()
        assert min(nseg) > 0
        # every output buffer: the records, the summaries and the rows of the segment tables that the call defines
        outs.append([o._objects.cpu().numpy().tobytes(), o._summary.cpu().numpy().tobytes()] +
                    [o._segments[b, :n].cpu().numpy().tobytes() for b, n in enumerate(nseg)])
    assert outs[0] == outs[1]
