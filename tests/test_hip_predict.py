"""The predictor's fused finish (csrc/predict.hip: sm_predict_masks_f32, sm_rle_runs_packed_u8) against the host restatement
(tests/_predict_ref.py) and against the kernels it replaces.  Equality is exact everywhere: the pixel arithmetic is the evaluator's
(csrc/upsample.h) and everything beyond it is integer."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _predict_ref as R  # noqa: E402
from selfmask_amd import _native as N, ops  # noqa: E402
from selfmask_amd.mask_generator import rle_encode  # noqa: E402
from selfmask_amd.voting import rle_runs_async  # noqa: E402

DEV = "cuda:0"
CHUNK = 16384  # positions per workgroup (PR_CHUNK), 4096 per wave (PR_WAVE_POS)
LDS_FLOATS = 12288  # staging limit (PR_LDS_FLOATS)


def _blobs(rng, nq, mh, mw):
    """smooth masks in [0, 1]"""
    yy, xx = np.mgrid[:mh, :mw].astype(np.float32)
    out = []
    for _ in range(nq):
        cy, cx, ry, rx = rng.uniform(.2, .8) * mh, rng.uniform(.2, .8) * mw, rng.uniform(.15, .4) * mh, rng.uniform(.15, .4) * mw
        d = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2
        out.append(1 / (1 + np.exp(4 * (d - 1))))
    return np.stack(out).astype(np.float32)


def _check(pend_result, ref, what=("best", "rle", "binary", "soft")):
    for b, r in enumerate(ref):
        for k in what:
            got = pend_result[k][b]
            if k in ("binary", "soft"):
                assert np.array_equal(got, r[k]), (b, k, int((got != r[k]).sum()))
            else:
                assert got == r[k], (b, k)


@pytest.fixture(scope="module")
def native_case():
    """P = 16, one 16 x 21 token grid: mask 32 x 42, scale 8, nq 20, five sizes of that grid"""
    rng = np.random.Generator(np.random.PCG64(5))
    sizes = [(250, 333), (241, 330), (256, 336), (243, 321), (249, 335)]
    nq, mh, mw = 20, 32, 42
    masks = np.stack([_blobs(rng, nq, mh, mw) for _ in sizes])
    obj = rng.random((len(sizes), nq)).astype(np.float32) * 0.9
    win = [3, 0, 19, 7, 11]
    for b, q in enumerate(win):
        obj[b, q] = 0.95
    obj[3, 12] = 0.95  # a tie for the top in image 3: query 7, the first, must win
    masks[0, win[0]] = np.clip(masks[0, win[0]], 0, 0.5)        # everywhere <= 0.5: an empty mask
    masks[1, win[1]] = 0.5 + masks[1, win[1]] * 0.5 + 1e-3      # everywhere > 0.5: a full mask
    masks[2, win[2], :4, :4] = 0.9                              # pixel (0, 0) set
    masks_t, obj_t = torch.from_numpy(masks), torch.from_numpy(obj)
    ref = R.finish(masks_t, obj_t, sizes, 8.0)
    assert [r["best"] for r in ref] == win
    assert not ref[0]["binary"].any() and ref[1]["binary"].all() and ref[2]["binary"][0, 0] == 1
    return sizes, masks_t, obj_t, ref


def test_native_bucket_mixed_sizes(native_case):
    sizes, masks, obj, ref = native_case
    m, o = masks.to(DEV), obj.to(DEV)
    table = ops.PackedImages(sizes, DEV)
    pend = ops.predict_masks(m, o, table, 8.0, rle=True, binary=True, soft=True)
    res = pend.result()
    _check(res, ref)
    assert pend.best.cpu().tolist() == [r["best"] for r in ref]
    # the witness: the evaluator's own up-sample kernel, told which query to take through column 14
    rows = torch.zeros((len(sizes), 16), device=DEV)
    rows[:, 14] = pend.best.float()
    from selfmask_amd.bilateral_solver import MixedBatch
    mb = MixedBatch(sizes, DEV)
    up = ops.upsample_selected_native(m, rows, mb, 8.0, "pick")
    for b, v in enumerate(mb.views(up)):
        assert np.array_equal((v > 0.5).cpu().numpy().astype(np.uint8), res["binary"][b]), b
        assert np.array_equal(v.float().cpu().numpy(), ref[b]["value"]), b


def test_resized_mode():
    rng = np.random.Generator(np.random.PCG64(6))
    sizes = [(300, 400), (37, 53), (224, 224)]
    masks = torch.from_numpy(np.stack([_blobs(rng, 20, 28, 28) for _ in sizes]))
    obj = torch.from_numpy(rng.random((3, 20)).astype(np.float32))
    res = ops.predict_masks(masks.to(DEV), obj.to(DEV), ops.PackedImages(sizes, DEV), 0.0, rle=True, binary=True, soft=True).result()
    _check(res, R.finish(masks, obj, sizes, 0.0))


@pytest.mark.parametrize("pattern", ["vertical", "horizontal", "last"])
def test_chunk_seams(pattern):
    """one image of several chunks (six workgroups, 21 wave ranges).  Vertical stripes: every change falls exactly at a column start
    q = x H - at 256 x 336 the changes sit at multiples of 2048, so every second one is the FIRST position of a wave range and every
    eighth the first of a workgroup.  Horizontal stripes (250 x 333): changes inside every column.  Last: a full-resolution mask
    (scale 1) whose only change is at the last position."""
    o = torch.ones((1, 1))
    if pattern == "last":
        sizes, scale = [(250, 333)], 1.0
        mask = np.zeros((1, 1, 250, 333), np.float32)
        mask[0, 0, -1, -1] = 1.0
    else:
        sizes, scale = ([(256, 336)] if pattern == "vertical" else [(250, 333)]), 8.0
        mask = np.zeros((1, 1, 32, 42), np.float32)
        if pattern == "vertical":
            mask[0, 0, :, ::2] = 1.0
        else:
            mask[0, 0, ::2, :] = 1.0
    assert sizes[0][0] * sizes[0][1] > 4 * CHUNK
    m = torch.from_numpy(mask)
    ref = R.finish(m, o, sizes, scale)
    counts = ref[0]["rle"]["counts"]
    if pattern == "vertical":
        bounds = np.cumsum(counts)[:-1]
        bounds = bounds[bounds > 0]  # pixel 0 is set: the code starts with an empty run of zeros
        assert len(bounds) == 41 and (bounds % 256 == 0).all() and (bounds % 4096 == 0).sum() >= 20 and (bounds % CHUNK == 0).sum() >= 5
    elif pattern == "horizontal":
        assert len(counts) > 30 * 333
    else:
        assert counts == [250 * 333 - 1, 1]
    res = ops.predict_masks(m.to(DEV), o.to(DEV), ops.PackedImages(sizes, DEV), scale, rle=True, binary=True).result()
    _check(res, ref, ("best", "rle", "binary"))


def test_cap_overflow_and_retry():
    rng = np.random.Generator(np.random.PCG64(8))
    sizes = [(64, 80), (61, 77), (64, 75)]
    B, cap = len(sizes), 16
    masks = torch.from_numpy(rng.random((B, 2, 64, 80)).astype(np.float32))  # noise at full resolution (scale 1)
    obj = torch.from_numpy(rng.random((B, 2)).astype(np.float32))
    ref = R.finish(masks, obj, sizes, 1.0)
    m, o = masks.to(DEV), obj.to(DEV)
    table = ops.PackedImages(sizes, DEV)
    lib = N.load()
    SENT = -7
    starts = torch.full((B + 2, cap), SENT, dtype=torch.int32, device=DEV)  # guard rows before and after
    info = torch.full((B + 2, 2), SENT, dtype=torch.int32, device=DEV)
    best = torch.empty(B, dtype=torch.int32, device=DEV)
    wsb = lib.sm_predict_workspace_bytes(B, table.max_pixels)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    a = N.PredictArgs()
    a.masks, a.mask_stride_b, a.objectness, a.obj_stride_b = m.data_ptr(), m.stride(0), o.data_ptr(), o.stride(0)
    a.images, a.best, a.starts, a.info, a.cap = table.dev.data_ptr(), best.data_ptr(), starts[1].data_ptr(), info[1].data_ptr(), cap
    a.workspace, a.workspace_bytes = ws.data_ptr(), wsb
    a.B, a.nq, a.mh, a.mw, a.max_pixels, a.scale = B, 2, 64, 80, table.max_pixels, 1.0
    N.check(lib.sm_predict_masks_f32(a, C.addressof(table.host), torch.cuda.current_stream().cuda_stream), "sm_predict_masks_f32")
    torch.cuda.synchronize()
    st, inf = starts.cpu().numpy(), info.cpu().numpy()
    assert (st[0] == SENT).all() and (st[-1] == SENT).all() and (inf[0] == SENT).all() and (inf[-1] == SENT).all()
    for b, r in enumerate(ref):
        flat = r["binary"].flatten(order="F")
        change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
        assert change.size > cap and inf[1 + b, 0] == change.size and inf[1 + b, 1] == int(flat[0])
        assert np.array_equal(st[1 + b], change[:cap])  # the first cap positions; the row after it is the next image's or the guard
    # the wrapper finds the runs again with room for the longest code
    res = ops.predict_masks(m, o, table, 1.0, rle=True, cap=cap).result()
    _check(res, ref, ("best", "rle"))


def test_mask_above_the_lds_limit_reads_through_l2():
    """one 1080 x 1920 image from a 270 x 480 mask (129 600 floats > the 12 288 staged in LDS): 127 workgroups, the global-memory path"""
    rng = np.random.Generator(np.random.PCG64(9))
    mh, mw = 270, 480
    assert mh * mw > LDS_FLOATS
    masks = torch.from_numpy(_blobs(rng, 3, mh, mw)[None])
    obj = torch.tensor([[0.2, 0.7, 0.1]])
    sizes = [(1080, 1920)]
    ref = R.finish(masks, obj, sizes, 4.0)
    assert 0 < ref[0]["binary"].mean() < 1
    res = ops.predict_masks(masks.to(DEV), obj.to(DEV), ops.PackedImages(sizes, DEV), 4.0, rle=True, binary=True, soft=True).result()
    _check(res, ref)


def test_rle_runs_packed_equals_host_and_padded_kernel():
    rng = np.random.Generator(np.random.PCG64(10))
    sizes = [(250, 333), (1, 1), (7, 300), (129, 64), (64, 257)]
    planes = [(rng.random(s) > 0.7).astype(np.uint8) * rng.integers(1, 255, s).astype(np.uint8) for s in sizes]  # any non-zero byte = 1
    planes[2][:] = 0
    planes[3][:] = 9
    table = ops.PackedImages(sizes, DEV)
    packed = torch.from_numpy(np.concatenate([p.reshape(-1) for p in planes])).to(DEV)
    got = ops.rle_runs_packed_async(packed, table).result()
    assert got == [rle_encode(p) for p in planes]
    assert ops.rle_runs_packed_async(packed, table, cap=16).result() == got  # overflow + retry
    Hm, Wm = max(h for h, _ in sizes), max(w for _, w in sizes)
    padded = torch.zeros((len(sizes), Hm, Wm), dtype=torch.uint8)
    for b, p in enumerate(planes):
        padded[b, :p.shape[0], :p.shape[1]] = torch.from_numpy(p)
    assert rle_runs_async(padded.to(DEV), cap=1 << 20, sizes=sizes).result() == got


@pytest.mark.parametrize("subset", [("rle",), ("binary",), ("soft",), ("rle", "soft"), ("binary", "soft"), ()])
def test_outputs_are_optional(native_case, subset):
    sizes, masks, obj, ref = native_case
    res = ops.predict_masks(masks.to(DEV), obj.to(DEV), ops.PackedImages(sizes, DEV), 8.0, rle="rle" in subset, binary="binary" in subset,
                            soft="soft" in subset).result()
    assert set(res) == {"best", *subset}
    _check(res, ref, ("best",) + subset)


@pytest.mark.parametrize("nq", [20, 130])
def test_argmax_order_is_the_serving_kernels_with_ties_and_nans(nq):
    """``best`` against sm_pick_mask_f32's scan on the same objectness: first maximum; a NaN never wins, except at q = 0"""
    rng = np.random.Generator(np.random.PCG64(nq))
    B = 12
    obj = rng.integers(0, 4, (B, nq)).astype(np.float32)      # many ties
    obj[1, 0] = np.nan                                        # NaN first: it stays
    obj[2, 3] = obj[2, 3 + 64 if nq > 67 else 5] = np.nan     # NaNs elsewhere (a lane's first query among them): ignored
    obj[3, 1:] = np.nan
    obj[4, :] = np.nan
    obj[5, rng.random(nq) < 0.5] = np.nan
    o = torch.from_numpy(obj).to(DEV)
    m = torch.zeros((B, nq, 2, 2), device=DEV)
    best = ops.predict_masks(m, o, ops.PackedImages([(2, 2)] * B, DEV), 0.0, rle=False).result()["best"]
    out, want = torch.empty((B, 4), device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
    N.check(N.load().sm_pick_mask_f32(m.data_ptr(), m.stride(0), o.data_ptr(), o.stride(0), out.data_ptr(), want.data_ptr(), B, nq, 4,
                                      torch.cuda.current_stream().cuda_stream), "sm_pick_mask_f32")
    assert best == want.cpu().tolist()
    assert best[0] == int(np.flatnonzero(obj[0] == obj[0].max())[0]) and best[1] == 0 and best[3] == 0 and best[4] == 0
