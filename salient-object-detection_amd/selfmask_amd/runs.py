"""Run-length codes from the run boundaries the device finds.

Every entry point that ends in a COCO run-length code - ``voting.rle_runs_async`` (padded planes), ``ops.rle_runs_packed_async``
(packed planes) and ``ops.predict_masks`` (the selected query's mask) - launches the same chunked walk (csrc/predict.hip) with its
own pixel source and gets back ``starts`` (B, cap) and ``info`` (B, 2) = {count, pixel 0}.  What follows is the same for all of
them and is written here once: ``PendingRuns`` (the buffers, the copy of ``info`` into page-locked memory, the second walk when a code
is longer than ``cap``, the host's differences) and, on request, the objects of the masks found on those runs (``_PendingObjects``).
"""
import torch

from . import _native as N


def workspace_bytes(n_images: int, max_pixels: int) -> int:
    """bytes of the walk's per-wave counts for ``n_images`` images of at most ``max_pixels`` pixels; raises on what no run entry
    point of the library takes"""
    n = N.load().sm_predict_workspace_bytes(n_images, max_pixels)
    if n == 0:
        raise ValueError(f"run-length codes of {n_images} images of up to {max_pixels} pixels: at most 65535 images of 2^22 pixels")
    return n


def _used_columns_host(starts: torch.Tensor, n: int):
    """the first ``n`` columns of ``starts`` (device) as a numpy array: one asynchronous copy into page-locked memory on the
    current stream and an event - the only wait is for that copy"""
    host = torch.empty((starts.shape[0], max(n, 1)), dtype=torch.int32, pin_memory=True)
    host.copy_(starts[:, :max(n, 1)], non_blocking=True)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(starts.device))
    done.synchronize()
    return host.numpy()


def _runs_to_rle(info, starts, shapes):
    """info (B, 2) {count, pixel 0}, starts (B, >= count) ascending column-major positions -> COCO uncompressed RLE dicts"""
    import numpy as np
    out = []
    for b, (H, W) in enumerate(shapes):
        n, first = int(info[b, 0]), int(info[b, 1])
        counts = np.diff(np.concatenate([[0], starts[b, :n], [H * W]])).tolist()
        out.append({"size": [H, W], "counts": ([0] + counts) if first else counts})
    return out


class ObjectOptions:
    """what ``predict_masks(..., objects=)`` / ``rle_runs_packed_async(..., objects=)`` take (or a dict of the same keys):
    ``connectivity`` 4 or 8, ``min_area`` drops smaller components, the ``max_objects`` (1 .. 64) largest are returned, ``masks``:
    one COCO uncompressed RLE per returned object"""

    def __init__(self, connectivity: int = 8, min_area: int = 0, max_objects: int = 16, masks: bool = True):
        self.connectivity, self.min_area, self.max_objects, self.masks = int(connectivity), int(min_area), int(max_objects), bool(masks)
        if self.connectivity not in (4, 8):
            raise ValueError(f"objects: connectivity={connectivity!r} (4 or 8)")
        if not 1 <= self.max_objects <= N.OBJ_MAX_OBJECTS:
            raise ValueError(f"objects: max_objects={max_objects!r} (1 .. {N.OBJ_MAX_OBJECTS})")
        if self.min_area < 0:
            raise ValueError(f"objects: min_area={min_area!r}")

    @staticmethod
    def of(o):
        if o is None or isinstance(o, ObjectOptions):
            return o
        return ObjectOptions(**dict(o))


def _spans(flags: int):
    """the two ``remove_long_masks`` tests of the reference's ``filter_masks`` on a box"""
    return {"top_bottom": bool(flags & 1), "left_right": bool(flags & 2)}


def batch_segments_to_rles(seg, n_segments, n_objects, shapes):
    """seg (B, >= max n_segments, 3) rows {start q, length, rank} ascending in q, the first n_segments[b] of image b used -> per image
    one COCO uncompressed RLE per rank 0 .. n_objects[b] - 1; segments of one object that abut (across a column end) merge into one
    run.  One pass over the tables of the whole batch."""
    import numpy as np
    B, K = len(shapes), max(max(n_objects, default=0), 1)
    used = (np.arange(seg.shape[1])[None, :] < np.asarray(n_segments)[:, None]) & (seg[:, :, 2] >= 0)
    image = np.nonzero(used)[0]
    rows = seg[used]
    key = image * K + rows[:, 2]
    order = np.argsort(key, kind="stable")  # by image and rank, ascending in q inside an object
    rows, key = rows[order], key[order]
    s = rows[:, 0].astype(np.int64)
    e = s + rows[:, 1]
    if not len(rows):
        return [[] for _ in shapes]
    joined = (s[1:] == e[:-1]) & (key[1:] == key[:-1])
    opens, closes = np.concatenate([[True], ~joined]), np.concatenate([~joined, [True]])
    bounds = np.stack([s[opens], e[closes]], axis=1).reshape(-1)  # run starts and ends, interleaved
    counts = np.diff(bounds, prepend=0)
    at = 2 * np.searchsorted(key[opens], np.arange(B * K + 1))  # where each object's bounds begin
    first = at[:-1][at[:-1] < at[1:]]  # (slots without an object are empty)
    counts[first] = bounds[first]  # an object's first count is its first start
    counts, bounds, at = counts.tolist(), bounds.tolist(), at.tolist()
    out = []
    for b, (H, W) in enumerate(shapes):
        rles = []
        for k in range(n_objects[b]):
            lo, hi = at[b * K + k], at[b * K + k + 1]
            c = counts[lo:hi]
            if bounds[hi - 1] != H * W:  # unless the object holds the last pixel, zeros close the code
                c.append(H * W - bounds[hi - 1])
            rles.append({"size": [int(H), int(W)], "counts": c})
        out.append(rles)
    return out


def segments_to_rles(seg, n_objects: int, size):
    """``batch_segments_to_rles`` for one image: seg (n, 3)"""
    return batch_segments_to_rles(seg[None], [len(seg)], [n_objects], [size])[0]


class _PendingObjects:
    """sm_mask_objects queued behind the kernels that wrote ``starts`` / ``info``, its small outputs on their way into page-locked
    memory; ``result()`` waits for those copies alone"""

    def __init__(self, table, opts, starts, info, cap, mask_src=None):
        import ctypes
        import numpy as np
        self.table, self.opts = table, opts
        dev = starts.device
        lib = N.load()
        B, K = table.B, opts.max_objects
        max_width = max(w for _, w in table.shapes)
        wsb = lib.sm_mask_objects_workspace_bytes(B, cap, max_width)
        if wsb == 0:
            raise ValueError(f"objects: unsupported shape (an image wider than {N.OBJ_MAX_WIDTH} pixels?)")
        self._ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        self._objects = torch.empty(B * K * ctypes.sizeof(N.Object), dtype=torch.uint8, device=dev)
        self._summary = torch.empty((B, N.OBJ_SUMMARY_INTS), dtype=torch.int32, device=dev)
        self._segments = torch.empty((B, lib.sm_mask_objects_seg_cap(cap, max_width), 3), dtype=torch.int32, device=dev) if opts.masks else None
        a = N.ObjectsArgs()
        a.starts, a.info, a.cap, a.images = starts.data_ptr(), info.data_ptr(), cap, table.dev.data_ptr()
        self.scored = mask_src is not None
        if self.scored:
            masks, best, scale = mask_src
            a.masks, a.mask_stride_b, a.best = masks.data_ptr(), masks.stride(0), best.data_ptr()
            a.mh, a.mw, a.scale = masks.shape[2], masks.shape[3], scale
        a.objects, a.summary = self._objects.data_ptr(), self._summary.data_ptr()
        a.segments = self._segments.data_ptr() if opts.masks else None
        a.workspace, a.workspace_bytes = self._ws.data_ptr(), wsb
        a.B, a.max_width = B, max_width
        a.connectivity, a.min_area, a.max_objects = opts.connectivity, opts.min_area, K
        N.check(lib.sm_mask_objects(a, ctypes.addressof(table.host), torch.cuda.current_stream(dev).cuda_stream), "sm_mask_objects")
        self._objects_h = torch.empty(self._objects.shape, dtype=torch.uint8, pin_memory=True)
        self._objects_h.copy_(self._objects, non_blocking=True)
        self._summary_h = torch.empty(self._summary.shape, dtype=torch.int32, pin_memory=True)
        self._summary_h.copy_(self._summary, non_blocking=True)
        self._done = torch.cuda.Event()
        self._done.record(torch.cuda.current_stream(dev))
        self._dtype = np.dtype([(n, np.int64 if t is ctypes.c_int64 else np.int32) for n, t in N.Object._fields_])

    def result(self):
        """-> per image {"size", "n_components", "bbox", "spans", "objects": [...]} (boxes [x, y, w, h])"""
        self._done.synchronize()
        K = self.opts.max_objects
        objs = self._objects_h.numpy().view(self._dtype).reshape(self.table.B, K)
        f = {n: objs[n].tolist() for n in self._dtype.names}  # plain ints from here on
        summ = self._summary_h.numpy()
        assert not summ[:, 3].any(), "objects of a truncated run list (the caller finds the runs again first)"
        all_rles, most = None, int(summ[:, 2].max(initial=0))
        if self._segments is not None and most:
            seg = _used_columns_host(self._segments.view(self.table.B, -1), 3 * most)
            all_rles = batch_segments_to_rles(seg.reshape(self.table.B, most, 3), summ[:, 2], summ[:, 1].tolist(), self.table.shapes)
        out = []
        for b, ((H, W), row) in enumerate(zip(self.table.shapes, summ.tolist())):
            ncomp, kept, nseg, _, x0, y0, x1, y1, flags, _area = row
            rles = all_rles[b] if all_rles else [None] * kept
            items = []
            for k in range(kept):
                area = f["area"][b][k]
                items.append({"bbox": [f["x0"][b][k], f["y0"][b][k], f["x1"][b][k] - f["x0"][b][k] + 1, f["y1"][b][k] - f["y0"][b][k] + 1],
                              "area": area, "centroid": (f["sum_x"][b][k] / area, f["sum_y"][b][k] / area),
                              "score": f["mass"][b][k] / (255 * area) if self.scored else None,
                              "first": f["first"][b][k], "spans": _spans(f["flags"][b][k]), "rle": rles[k]})
            out.append({"size": [H, W], "n_components": ncomp, "bbox": [x0, y0, x1 - x0 + 1, y1 - y0 + 1] if x1 >= 0 else None,
                        "spans": _spans(flags), "objects": items})
        return out


class PendingRuns:
    """The run boundaries of one batch, queued on the current stream; ``result()`` waits for the copy of ``info`` alone.
    ``launch(starts, info, cap, workspace, first)`` queues the caller's walk: ``first`` is False when it runs again because a code
    was longer than ``cap`` (noise-like masks) - whatever else the caller's launch produces is wanted the first time only.  The
    closure keeps its inputs alive until ``result()``, so the stream must not overwrite them before.  ``shapes``: (H_b, W_b) per
    image; ``max_pixels``: the largest size an image can have (sizes the workspace, which is kept for the second walk);
    ``objects``: (table, ObjectOptions, mask_src or None) - sm_mask_objects is queued behind every walk."""

    def __init__(self, launch, shapes, cap: int, max_pixels: int, device, objects=None):
        self._launch, self.shapes, self.cap, self._want_objects = launch, shapes, int(cap), objects
        self._ws = torch.empty(workspace_bytes(len(shapes), max_pixels), dtype=torch.uint8, device=device)
        self._info = torch.empty((len(shapes), 2), dtype=torch.int32, device=device)
        self._objects = None
        self._starts = self._walk(self.cap, True)
        self._info_h = torch.empty(self._info.shape, dtype=torch.int32, pin_memory=True)
        self._info_h.copy_(self._info, non_blocking=True)
        self._done = torch.cuda.Event()
        self._done.record(torch.cuda.current_stream(device))

    def _walk(self, cap, first):
        starts = torch.empty((len(self.shapes), cap), dtype=torch.int32, device=self._info.device)
        self._launch(starts, self._info, cap, self._ws, first)
        if self._want_objects is not None:  # the objects are found on the runs
            table, opts, mask_src = self._want_objects
            self._objects = _PendingObjects(table, opts, starts, self._info, cap, mask_src)
        return starts

    def result(self, rle: bool = True):
        """-> (one COCO uncompressed RLE dict per image, or None without ``rle``; ``_PendingObjects.result()``, or None)"""
        self._done.synchronize()
        info = self._info_h.numpy()
        longest = int(info[:, 0].max(initial=0))
        starts = self._starts
        if longest > self.cap:  # once more, with room for the longest code (and the objects with it)
            starts = self._walk(longest, False)
        rles = _runs_to_rle(info, _used_columns_host(starts, longest), self.shapes) if rle else None
        return rles, None if self._objects is None else self._objects.result()
