"""Plain-numpy restatement of the objects of a mask (csrc/objects.hip, ``ops.predict_masks(objects=)``): connected components of a
0/1 plane with box, area, centroid, score, first raster pixel and per-object RLE.  Two routes that must agree: pixel flood labelling
and the kernel's own route, run boundaries -> vertical segments -> union of overlapping segments of neighbouring columns."""
import numpy as np


# ---- route 1: pixel flood ---------------------------------------------------------------------------------------------------------
def label_flood(plane, connectivity=8):
    """-> (labels int32 (H, W), n): 0 = background, labels 1 .. n numbered by the first pixel in row-major raster order"""
    m = np.asarray(plane) != 0
    H, W = m.shape
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    lab = np.zeros((H, W), np.int32)
    n = 0
    for y, x in zip(*np.nonzero(m)):  # raster order
        if lab[y, x]:
            continue
        n += 1
        lab[y, x] = n
        stack = [(y, x)]
        while stack:
            cy, cx = stack.pop()
            for dy, dx in nb:
                yy, xx = cy + dy, cx + dx
                if 0 <= yy < H and 0 <= xx < W and m[yy, xx] and not lab[yy, xx]:
                    lab[yy, xx] = n
                    stack.append((yy, xx))
    return lab, n


# ---- route 2: runs -> segments -> union ---------------------------------------------------------------------------------------------
def run_boundaries(plane):
    """-> (starts, pixel 0): the ascending column-major positions q = x H + y that differ from the one before (sm_rle_runs_u8)"""
    flat = (np.asarray(plane) != 0).flatten(order="F")
    return np.flatnonzero(flat[1:] != flat[:-1]) + 1, int(flat[0]) if flat.size else 0


def segments(starts, p0, H, W):
    """foreground runs cut at the column ends they cross -> (n, 2) int64 rows (q, length), ascending"""
    bounds = np.concatenate([[0], starts, [H * W]]).astype(np.int64)
    out = []
    for j in range(1 - p0, len(bounds) - 1, 2):  # runs alternate, starting with pixel 0's value
        s, e = int(bounds[j]), int(bounds[j + 1])
        for x in range(s // H, (e - 1) // H + 1):
            q = max(s, x * H)
            out.append((q, min(e, (x + 1) * H) - q))
    return np.array(out, np.int64).reshape(-1, 2)


def label_runs(plane, connectivity=8):
    """the same (labels, n) as ``label_flood`` by the segment route"""
    H, W = np.asarray(plane).shape
    seg = segments(*run_boundaries(plane), H, W)
    parent = list(range(len(seg)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    widen = 1 if connectivity == 8 else 0
    by_col = {}
    for i, (q, ln) in enumerate(seg):
        by_col.setdefault(int(q) // H, []).append(i)
    for i, (q, ln) in enumerate(seg):
        x, y0 = int(q) // H, int(q) % H
        for j in by_col.get(x - 1, ()):
            z0 = int(seg[j, 0]) % H
            if z0 + int(seg[j, 1]) - 1 >= y0 - widen and z0 <= y0 + int(ln) - 1 + widen:
                a, b = find(i), find(j)
                parent[max(a, b)] = min(a, b)
    roots = [find(i) for i in range(len(seg))]
    first = {}
    for i, (q, ln) in enumerate(seg):
        key = (int(q) % H) * W + int(q) // H
        first[roots[i]] = min(first.get(roots[i], key), key)
    number = {r: k + 1 for k, r in enumerate(sorted(first, key=first.get))}
    lab = np.zeros((H, W), np.int32)
    for i, (q, ln) in enumerate(seg):
        lab[int(q) % H:int(q) % H + int(ln), int(q) // H] = number[roots[i]]
    return lab, len(number)


# ---- the result of ops.predict_masks(objects=) ------------------------------------------------------------------------------------
def rle_encode(mask):
    flat = (np.asarray(mask) != 0).flatten(order="F")
    counts = np.diff(np.concatenate([[0], np.flatnonzero(flat[1:] != flat[:-1]) + 1, [flat.size]])).tolist()
    return {"size": [int(mask.shape[0]), int(mask.shape[1])], "counts": ([0] + counts) if flat.size and flat[0] else counts}


def _box(ys, xs):
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]


def _spans(box, H, W):
    return {"top_bottom": box[1] == 0 and box[3] == H, "left_right": box[0] == 0 and box[2] == W}


def objects(plane, soft=None, connectivity=8, min_area=0, max_objects=16, masks=True, route="flood"):
    """plane (H, W) 0/1, soft (H, W) uint8 or None -> the per-image dict of ``ops.predict_masks(...).result()["objects"]``"""
    plane = np.asarray(plane)
    H, W = plane.shape
    lab, n = (label_flood if route == "flood" else label_runs)(plane, connectivity)
    ys, xs = np.nonzero(lab)
    ids = lab[ys, xs] - 1
    area = np.bincount(ids, minlength=n)
    sum_x, sum_y = np.bincount(ids, xs, minlength=n), np.bincount(ids, ys, minlength=n)
    mass = np.bincount(ids, soft[ys, xs], minlength=n) if soft is not None else None
    order = [k for k in sorted(range(n), key=lambda k: (-int(area[k]), k)) if area[k] >= min_area][:max_objects]  # labels ascend with `first`
    items = []
    for k in order:
        oy, ox = ys[ids == k], xs[ids == k]
        box, a = _box(oy, ox), int(area[k])
        items.append({"bbox": box, "area": a, "centroid": (int(round(sum_x[k])) / a, int(round(sum_y[k])) / a),
                      "score": int(round(mass[k])) / (255 * a) if mass is not None else None, "first": int((oy * W + ox).min()),
                      "spans": _spans(box, H, W), "rle": rle_encode(lab == k + 1) if masks else None})
    whole = _box(ys, xs) if ys.size else None
    return {"size": [H, W], "n_components": n, "bbox": whole,
            "spans": _spans(whole, H, W) if whole else {"top_bottom": False, "left_right": False}, "objects": items}
