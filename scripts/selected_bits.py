"""Digests of everything that is computed from "the selected query's mask, up-sampled to image b's size", for A/B runs of two builds of
the library that must agree bit for bit (a change of csrc/upsample.h, selected.hip, predict.hip or objects.hip that moves no arithmetic).

Runs a fixed, seeded case list on the library that SM_HIP_LIB names (default: lib/libselfmask_hip.so) and prints ONE JSON object
{case: sha256}: the three sm_upsample_selected_* entry points (both selection columns; scale mode k = 4, 8 and resize mode; the
shapes of tests/test_hip_selected_planes.py; one case with the masks as a strided last-layer view), the two byte-to-float copies, and
predict_masks (best, run codes, binary, soft; a mask under the LDS staging limit and one over it; both modes) with its objects.  The
entry points are called on zeroed outputs, so a byte that is not written shows.  ``--time``: device-event timings of the five entry
points of selected.hip, of sm_predict_masks_f32 and of it followed by sm_mask_objects on the evaluator's workload (B = 64, nq = 20,
28 x 28 masks, the 300-400 px images of scripts/eval_bench.py; size mode: 64 planes of 384 x 384).  Run it once per library, each in
a fresh process, and compare:

    SM_HIP_LIB=$PWD/salient-object-detection_amd/lib/libselfmask_hip_prev.so python scripts/selected_bits.py --out prev.json
    python scripts/selected_bits.py --out new.json
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [os.path.join(ROOT, "salient-object-detection_amd"), ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
# name: (seed, k (0: resize mode), (mh, mw), sizes): tests/test_hip_selected_planes.py
PLANE_CASES = {
    "A": (301, 4, (5, 7), [(20, 28), (1, 1), (20, 1), (1, 28), (13, 20), (19, 27)]),
    "B": (303, 8, (3, 33), [(1, 255), (1, 256), (1, 257), (24, 264)]),
    "C": (303, 8, (33, 33), [(264, 264), (3, 5)]),
    "R": (303, 0, (7, 5), [(3, 4), (1, 1), (97, 61), (3, 200), (7, 5)]),
}
# name: (seed, scale, (mh, mw), sizes): 112 x 112 = 12544 values is over the predictor's LDS staging limit of 12288
PREDICT_CASES = {
    "lds|x8": (11, 8.0, (28, 42), [(224, 336), (199, 300), (217, 333), (1, 1)]),
    "lds|resize": (12, 0.0, (14, 14), [(97, 61), (40, 200), (1, 9), (300, 400)]),
    "l2|x2": (13, 2.0, (112, 112), [(224, 224), (150, 223), (3, 5)]),
    "l2|resize": (14, 0.0, (112, 112), [(97, 61), (300, 400), (112, 112)]),
}
COLS = {"pick": 14, "ub": 15}


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes())
    return h.hexdigest()


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


class Planes:
    """the three up-samples through the C entry points, on zeroed outputs"""

    def __init__(self, mp, rows, sizes):
        from selfmask_amd import _native as N, ops
        from selfmask_amd.bilateral_solver import MixedBatch
        self.N, self.lib, self.mp, self.rows, self.sizes = N, N.load(), mp, rows, sizes
        (self.B, _, self.mh, self.mw), self.mb = mp.shape, MixedBatch(sizes, DEV)
        self.gb = ops.GtBatch([torch.zeros(s, dtype=torch.uint8) for s in sizes], torch.device(DEV))
        self.max_pixels = max(h * w for h, w in sizes)

    def _head(self, col):
        return self.mp.data_ptr(), self.mp.stride(0), self.rows.data_ptr(), col

    def size_mode(self, col, size, out=None):
        out = torch.zeros((self.B,) + tuple(size), dtype=torch.float64, device=DEV) if out is None else out
        self.N.check(self.lib.sm_upsample_selected_f64(*self._head(col), out.data_ptr(), self.B, self.mh, self.mw, size[0], size[1], _stream()),
                     "sm_upsample_selected_f64")
        return out

    def native(self, col, scale, out=None):
        out = torch.zeros(self.mb.n_pixels, dtype=torch.float64, device=DEV) if out is None else out
        self.N.check(self.lib.sm_upsample_selected_native_f64(*self._head(col), self.mb.dev.data_ptr(), out.data_ptr(), self.B, self.mh, self.mw,
                                                              float(scale), self.max_pixels, _stream()), "sm_upsample_selected_native_f64")
        return out

    def u8(self, col, scale, out=None):
        out = torch.zeros(self.mb.n_pixels, dtype=torch.uint8, device=DEV) if out is None else out
        self.N.check(self.lib.sm_upsample_selected_u8(*self._head(col), self.gb.images.data_ptr(), out.data_ptr(), self.B, self.mh, self.mw,
                                                      float(scale), self.max_pixels, _stream()), "sm_upsample_selected_u8")
        return out


def _plane_digests(res, tag, p, k, mh, mw):
    for which, col in COLS.items():
        if k:
            res[f"f64|{tag}|{which}"] = _sha(p.size_mode(col, (k * mh, k * mw)))
            res[f"native|{tag}|{which}"] = _sha(p.native(col, k))
        else:
            res[f"f64|{tag}|{which}"] = _sha(*[p.size_mode(col, s) for s in p.sizes])
        res[f"u8|{tag}|{which}"] = _sha(p.u8(col, k))


def bits():
    from _mask_planes import _masks
    from selfmask_amd import _native as N, ops
    lib, res = N.load(), {}
    for name, (seed, k, (mh, mw), sizes) in PLANE_CASES.items():
        for spread in (1.0, 1.3):
            masks, _, rows = _masks(seed if spread == 1.0 else seed + 1000, len(sizes), 3, mh, mw, spread)
            mp, rw = torch.from_numpy(masks).to(DEV), torch.from_numpy(rows).to(DEV)
            _plane_digests(res, f"{name}|{spread}", Planes(mp, rw, sizes), k, mh, mw)
            if name == "A" and spread == 1.0:  # the masks as [:, -1] of (B, L, nq, mh, mw)
                layers = torch.full((len(sizes), 3, 3, mh, mw), 0.25, device=DEV)
                layers[:, -1] = mp
                _plane_digests(res, "A|strided", Planes(layers[:, -1], rw, sizes), k, mh, mw)
    # the byte-to-float copies
    rng = np.random.Generator(np.random.PCG64(5))
    sizes = [(97, 61), (1, 1), (40, 200), (3, 5)]
    table = ops.PackedImages(sizes, DEV)
    src = torch.from_numpy(rng.integers(0, 256, table.n_pixels, dtype=np.uint8)).to(DEV)
    dst = torch.zeros(table.n_pixels, dtype=torch.float32, device=DEV)
    N.check(lib.sm_mask_u8_to_f32(src.data_ptr(), dst.data_ptr(), src.numel(), _stream()), "sm_mask_u8_to_f32")
    res["mask_u8_to_f32"] = _sha(dst)
    dst = torch.zeros((len(sizes), 1, 97, 200), dtype=torch.float32, device=DEV)
    N.check(lib.sm_mask_planes_u8_to_f32(src.data_ptr(), table.dev.data_ptr(), dst.data_ptr(), len(sizes), 97, 200, table.max_pixels, _stream()),
            "sm_mask_planes_u8_to_f32")
    res["mask_planes_u8_to_f32"] = _sha(dst)
    # the predictor's finish and the objects on it
    for name, (seed, scale, (mh, mw), sizes) in PREDICT_CASES.items():
        masks, obj, _ = _masks(seed, len(sizes), 5, mh, mw, spread=1.3)
        mp, ob = torch.from_numpy(masks).to(DEV), torch.from_numpy(obj).to(DEV)
        out = ops.predict_masks(mp, ob, ops.PackedImages(sizes, DEV), scale, rle=True, binary=True, soft=True,
                                objects={"max_objects": 8, "min_area": 2}).result()
        res[f"predict|{name}"] = hashlib.sha256(json.dumps([out["best"], out["rle"]]).encode() +
                                                b"".join(p.tobytes() for p in out["binary"] + out["soft"])).hexdigest()
        res[f"objects|{name}"] = hashlib.sha256(json.dumps(out["objects"], sort_keys=True).encode()).hexdigest()
    return res


def _timed(name, fn, warmup=5, reps=40):
    ms = []
    for rep in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if rep >= warmup:
            ms.append(e0.elapsed_time(e1) * 1e3)
    print(f"{name:36s} mean {np.mean(ms):9.1f}  min {np.min(ms):9.1f}  max {np.max(ms):9.1f} us ({reps} calls)", flush=True)


def timings():
    from eval_bits import _bench_gts
    from selfmask_amd import _native as N, ops
    lib = N.load()
    B, nq, side, cap = 64, 20, 28, 32768
    sizes = [tuple(g.shape) for g in _bench_gts(B)]
    torch.manual_seed(side)
    mp = torch.sigmoid(torch.randn(B, nq, side, side, device=DEV) * 3)
    ob = torch.rand(B, nq, device=DEV)
    rows = torch.zeros((B, 16), device=DEV)
    rows[:, 14], rows[:, 15] = ob.argmax(1), torch.randint(0, nq, (B,), device=DEV)
    p = Planes(mp, rows, sizes)
    f64, nat, u8 = p.size_mode(14, (384, 384)), p.native(14, 16.0), p.u8(14, 0.0)
    _timed("sm_upsample_selected_f64", lambda: p.size_mode(14, (384, 384), f64))
    _timed("sm_upsample_selected_native_f64", lambda: p.native(14, 16.0, nat))
    _timed("sm_upsample_selected_u8", lambda: p.u8(14, 0.0, u8))
    planes = torch.zeros((B, 384, 384), dtype=torch.uint8, device=DEV)
    as_f32 = torch.zeros((B, 384, 384), dtype=torch.float32, device=DEV)
    _timed("sm_mask_u8_to_f32", lambda: N.check(lib.sm_mask_u8_to_f32(planes.data_ptr(), as_f32.data_ptr(), planes.numel(), _stream()), "u8_to_f32"))
    Hm, Wm = max(h for h, _ in sizes), max(w for _, w in sizes)
    padded = torch.zeros((B, 1, Hm, Wm), dtype=torch.float32, device=DEV)
    _timed("sm_mask_planes_u8_to_f32", lambda: N.check(lib.sm_mask_planes_u8_to_f32(u8.data_ptr(), p.mb.dev.data_ptr(), padded.data_ptr(), B, Hm, Wm,
                                                                                  p.max_pixels, _stream()), "planes_u8_to_f32"))
    # the predictor's finish (runs, binary and soft planes), alone and with the objects behind it; every buffer allocated beforehand
    table, i32 = p.mb, dict(dtype=torch.int32, device=DEV)
    best, starts, info = torch.zeros(B, **i32), torch.zeros((B, cap), **i32), torch.zeros((B, 2), **i32)
    binary, soft = torch.zeros(table.n_pixels, dtype=torch.uint8, device=DEV), torch.zeros(table.n_pixels, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(lib.sm_predict_workspace_bytes(B, table.max_pixels), dtype=torch.uint8, device=DEV)
    a = N.PredictArgs()
    a.masks, a.mask_stride_b, a.objectness, a.obj_stride_b = mp.data_ptr(), mp.stride(0), ob.data_ptr(), ob.stride(0)
    a.images, a.best, a.starts, a.info, a.cap = table.dev.data_ptr(), best.data_ptr(), starts.data_ptr(), info.data_ptr(), cap
    a.binary, a.soft, a.workspace, a.workspace_bytes = binary.data_ptr(), soft.data_ptr(), ws.data_ptr(), ws.numel()
    a.B, a.nq, a.mh, a.mw, a.max_pixels, a.scale = B, nq, side, side, table.max_pixels, 0.0
    K, max_width = 16, max(w for _, w in sizes)
    ows = torch.zeros(lib.sm_mask_objects_workspace_bytes(B, cap, max_width), dtype=torch.uint8, device=DEV)
    objects = torch.zeros(B * K * ctypes.sizeof(N.Object), dtype=torch.uint8, device=DEV)
    summary = torch.zeros((B, N.OBJ_SUMMARY_INTS), **i32)
    o = N.ObjectsArgs()
    o.starts, o.info, o.cap, o.images = starts.data_ptr(), info.data_ptr(), cap, table.dev.data_ptr()
    o.masks, o.mask_stride_b, o.best, o.mh, o.mw, o.scale = mp.data_ptr(), mp.stride(0), best.data_ptr(), side, side, 0.0
    o.objects, o.summary, o.segments, o.workspace, o.workspace_bytes = objects.data_ptr(), summary.data_ptr(), None, ows.data_ptr(), ows.numel()
    o.B, o.max_width, o.connectivity, o.min_area, o.max_objects = B, max_width, 8, 0, K

    def finish():
        N.check(lib.sm_predict_masks_f32(a, ctypes.addressof(table.host), _stream()), "sm_predict_masks_f32")

    def finish_objects():
        finish()
        N.check(lib.sm_mask_objects(o, ctypes.addressof(table.host), _stream()), "sm_mask_objects")

    _timed("predict_masks", finish)
    _timed("predict_masks + objects", finish_objects)
    torch.cuda.synchronize()
    assert int(info[:, 0].max()) <= cap and not bool(summary[:, 3].any()), "a run list longer than cap: the objects were not found"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the JSON object to this file")
    ap.add_argument("--time", action="store_true", help="print device-event timings instead of digests")
    a = ap.parse_args()
    if a.time:
        timings()
        sys.exit(0)
    res = bits()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1, sort_keys=True) + "\n")
    print(json.dumps(res, sort_keys=True))
