"""The objects of a mask without a GPU: the host restatement (tests/_objects_ref.py) against itself (flood route vs run / segment
route), against scipy.ndimage.label and against the reference's mask_to_bbox / filter_masks; the segment bound; the host step from
the kernel's segment table to per-object RLE; the argument checks of sm_mask_objects."""
import ctypes as C

import numpy as np
import pytest
import torch

import _objects_ref as R
from selfmask_amd import _native as N, ops
from selfmask_amd.mask_generator import rle_decode


def _planes(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    for i in range(n):
        h, w = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        yield (rng.random((h, w)) < (0.1 + 0.1 * (i % 10))).astype(np.uint8)  # densities 0.1 .. 1.0


@pytest.mark.parametrize("connectivity", [4, 8])
def test_flood_route_equals_segment_route(connectivity):
    for p in _planes(300, 1):
        a, na = R.label_flood(p, connectivity)
        b, nb = R.label_runs(p, connectivity)
        assert na == nb and np.array_equal(a, b), p.shape
        # and the product's host step on the segment route's table gives the flood route's objects back
        table, res, lab = _table(p, connectivity)
        assert ops.segments_to_rles(table, len(res["objects"]), p.shape) == [R.rle_encode(lab == lab.flat[o["first"]]) for o in res["objects"]]
        assert R.objects(p, connectivity=connectivity, route="flood") == R.objects(p, connectivity=connectivity, route="runs")


@pytest.mark.parametrize("connectivity", [4, 8])
def test_labels_equal_scipy(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    for p in _planes(300, 2):
        want, n = ndi.label(p, structure=structure)
        for route in (R.label_flood, R.label_runs):
            got, m = route(p, connectivity)
            assert m == n and np.array_equal(got, want), (route.__name__, p.shape)
        res = R.objects(p, connectivity=connectivity, max_objects=64)
        boxes = ndi.find_objects(want)
        for o in res["objects"]:
            k = want.flat[o["first"]]  # the label that owns the object's first pixel
            sl = boxes[k - 1]
            assert o["bbox"] == [sl[1].start, sl[0].start, sl[1].stop - sl[1].start, sl[0].stop - sl[0].start]
            assert o["area"] == int((want == k).sum()) and np.array_equal(rle_decode(o["rle"]), want == k)


def test_whole_mask_box_and_spans_equal_the_reference_filter():
    from oracle.voting_oracle import filter_masks, mask_to_bbox
    cases = list(_planes(200, 3)) + [np.ones((5, 7), np.uint8), np.zeros((4, 4), np.uint8), np.eye(6, dtype=np.uint8)]
    for p in cases:
        res = R.objects(p)
        box = mask_to_bbox(p)
        if not box:
            assert res["bbox"] is None and res["spans"] == {"top_bottom": False, "left_right": False}
            continue
        y0, y1, x0, x1 = box[0]
        assert res["bbox"] == [x0, y0, x1 - x0 + 1, y1 - y0 + 1]
        # filter_masks(remove_long_masks=True) drops a mask that spans the rows or the columns; with one mask in, "all filtered"
        # hands it back with the identity map, so the test is on the two conditions themselves
        h, w = p.shape
        assert res["spans"] == {"top_bottom": y0 == 0 and y1 + 1 == h, "left_right": x0 == 0 and x1 + 1 == w}
        two = torch.from_numpy(np.stack([p, np.zeros_like(p)]))
        two[1, h // 2, w // 2] = 1  # a second mask that is kept unless the plane is one pixel
        if h > 1 and w > 1:
            kept, index = filter_masks(two, remove_long_masks=True)
            assert (0 in index.values()) == (not (res["spans"]["top_bottom"] or res["spans"]["left_right"]))


def test_segment_bound():
    met = False
    for p in list(_planes(300, 4)) + [np.ones((3, 9), np.uint8)]:
        h, w = p.shape
        starts, p0 = R.run_boundaries(p)
        n = len(R.segments(starts, p0, h, w))
        assert n <= -(-len(starts) // 2) + w
        met |= n == -(-len(starts) // 2) + w
        # the library sizes its segment tables by that bound at count = cap
        assert N.load().sm_mask_objects_seg_cap(max(len(starts), 1), w) >= n
    assert met  # the bound is tight: nothing smaller would do


def _table(p, connectivity=8, max_objects=64):
    """the kernel's segment table (q, length, rank) of a plane, from the reference"""
    h, w = p.shape
    seg = R.segments(*R.run_boundaries(p), h, w)
    lab, _ = R.label_flood(p, connectivity)
    res = R.objects(p, connectivity=connectivity, max_objects=max_objects)
    rank_of = {lab.flat[o["first"]]: k for k, o in enumerate(res["objects"])}
    rank = [rank_of.get(lab[int(q) % h, int(q) // h], -1) for q, _ in seg]
    return np.column_stack([seg, rank]).astype(np.int32).reshape(-1, 3), res, lab


def test_segment_table_to_object_rles():
    for p in _planes(100, 5):
        table, res, lab = _table(p, max_objects=5)
        rles = ops.segments_to_rles(table, len(res["objects"]), p.shape)
        assert rles == [o["rle"] for o in res["objects"]]
        for o, r in zip(res["objects"], rles):
            assert np.array_equal(rle_decode(r), lab == lab.flat[o["first"]])


def test_segment_tables_of_a_batch_in_one_pass():
    planes = list(_planes(40, 6)) + [np.zeros((3, 3), np.uint8), np.ones((2, 5), np.uint8)]
    tables = [_table(p, max_objects=4) for p in planes]
    most = max(len(t[0]) for t in tables)
    seg = np.full((len(planes), most + 2, 3), 7, np.int32)  # rows past an image's count are not read
    for b, (t, _, _) in enumerate(tables):
        seg[b, :len(t)] = t
    got = ops.batch_segments_to_rles(seg, [len(t[0]) for t in tables], [len(t[1]["objects"]) for t in tables], [p.shape for p in planes])
    assert got == [[o["rle"] for o in t[1]["objects"]] for t in tables]
    assert ops.batch_segments_to_rles(seg[:, :0], [0] * len(planes), [0] * len(planes), [p.shape for p in planes]) == [[] for _ in planes]


def test_abutting_segments_merge_across_a_column_end():
    p = np.zeros((4, 3), np.uint8)
    p[2:, 0] = 1
    p[:, 1] = 1
    p[0, 2] = 1  # column-major: positions 2 .. 8 set, three segments that abut at 4 and 8
    table, res, _ = _table(p)
    assert table.tolist() == [[2, 2, 0], [4, 4, 0], [8, 1, 0]]
    assert ops.segments_to_rles(table, 1, p.shape) == [{"size": [4, 3], "counts": [2, 7, 3]}] == [res["objects"][0]["rle"]]
    full = np.ones((3, 2), np.uint8)
    assert ops.segments_to_rles(_table(full)[0], 1, full.shape) == [{"size": [3, 2], "counts": [0, 6]}]


def test_object_options():
    assert ops.ObjectOptions.of(None) is None
    o = ops.ObjectOptions.of({"min_area": 5})
    assert (o.connectivity, o.min_area, o.max_objects, o.masks) == (8, 5, 16, True)
    for bad in ({"connectivity": 6}, {"max_objects": 0}, {"max_objects": 65}, {"min_area": -1}):
        with pytest.raises(ValueError):
            ops.ObjectOptions.of(bad)


def test_workspace_function_returns_zero_out_of_range():
    lib = N.load()
    assert lib.sm_mask_objects_workspace_bytes(2, 8192, 400) >= 2 * 5 * (4096 + 400) * 4
    for B, cap, width in ((0, 8192, 400), (65536, 8192, 400), (1, 0, 400), (1, (1 << 22) + 1, 400), (1, 8192, 0), (1, 8192, 16385)):
        assert lib.sm_mask_objects_workspace_bytes(B, cap, width) == 0, (B, cap, width)
    assert lib.sm_mask_objects_workspace_bytes(1, 8192, 16384) > 0
    assert lib.sm_mask_objects_seg_cap(8192, 400) == 4096 + 400 and lib.sm_mask_objects_seg_cap(7, 5) == 4 + 5
    assert lib.sm_mask_objects_workspace_bytes(3, 100, 30) >= 3 * 5 * 4 * lib.sm_mask_objects_seg_cap(100, 30)
    for cap, width in ((0, 4), (4, 0), (4, 16385), ((1 << 22) + 1, 4)):
        assert lib.sm_mask_objects_seg_cap(cap, width) == 0


def test_argument_validation_without_gpu():
    """as test_abi_cpu.test_argument_validation_without_gpu: refused on the host before any launch"""
    lib = N.load()
    table = (N.BilateralImage * 1)()
    table[0].H, table[0].W = 4, 4
    host = C.addressof(table)
    assert C.sizeof(N.Object) == 56
    assert lib.sm_mask_objects(None, host, None) == -1 and b"null pointer" in lib.sm_last_error()
    a = N.ObjectsArgs()
    a.B, a.cap, a.max_width, a.connectivity, a.min_area, a.max_objects = 1, 16, 4, 8, 0, 16
    assert lib.sm_mask_objects(a, host, None) == -1 and b"null pointer" in lib.sm_last_error()
    a.starts = a.info = a.images = a.objects = a.summary = a.workspace = 256  # never dereferenced: every case below is refused
    assert lib.sm_mask_objects(a, None, None) == -1 and b"null pointer" in lib.sm_last_error()
    a.connectivity = 6
    assert lib.sm_mask_objects(a, host, None) == -1 and b"connectivity=6" in lib.sm_last_error()
    a.connectivity, a.max_objects = 4, 65
    assert lib.sm_mask_objects(a, host, None) == -1 and b"max_objects=65" in lib.sm_last_error()
    a.max_objects, a.min_area = 64, -1
    assert lib.sm_mask_objects(a, host, None) == -1 and b"min_area=-1" in lib.sm_last_error()
    a.min_area, a.max_width = 0, 16385
    assert lib.sm_mask_objects(a, host, None) == -1 and b"max_width" in lib.sm_last_error()
    a.max_width = 3  # narrower than the table's image
    assert lib.sm_mask_objects(a, host, None) == -1 and b"image 0" in lib.sm_last_error()
    a.max_width, a.workspace_bytes = 4, 0
    assert lib.sm_mask_objects(a, host, None) == -1 and b"workspace" in lib.sm_last_error()


@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (5, 1), (37, 53)])
def test_host_decoder_of_run_boundaries_equals_rle_encode(h, w):
    """the one place that turns {count, pixel 0} + ascending starts into COCO counts, fed the restatement's boundaries (what the device
    walk writes), rows padded as the device's ``starts`` buffer is"""
    from selfmask_amd.mask_generator import rle_encode
    from selfmask_amd.runs import _runs_to_rle
    yy, xx = np.mgrid[:h, :w]
    blob = ((((yy - h * 0.4) / max(1.0, h * 0.3)) ** 2 + ((xx - w * 0.55) / max(1.0, w * 0.25)) ** 2) <= 1).astype(np.uint8)
    first = blob.copy()
    first[0, 0] = 200
    planes = [blob, first, np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)]
    bounds = [R.run_boundaries(p) for p in planes]
    info = np.array([[len(s), p0] for s, p0 in bounds], np.int32)
    starts = np.full((len(planes), max(int(info[:, 0].max()), 1) + 3), -7, np.int32)  # what lies past a row's count is not read
    for b, (s, _) in enumerate(bounds):
        starts[b, :len(s)] = s
    assert _runs_to_rle(info, starts, [(h, w)] * len(planes)) == [rle_encode(p) for p in planes]
