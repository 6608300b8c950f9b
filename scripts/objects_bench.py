"""Objects of the predicted masks on the device against the host route -> profiles/objects_bench.log.

Steps, each a child process of its own under its own time limit (a step that fails or runs out of time ends the run):
  finish   128 images of 300 x 400 and 8 images of 1080 x 1920 at P = 16 (masks 38 x 50 and 136 x 240, scale 8; the shapes of
           scripts/predict_bench.py), three blobs per query.  Three sides alternating in one process, wall clock from the call to the
           host-side result (3 warm-up, 20 timed repetitions, min / median / max):
             rle            ops.predict_masks(rle=True).result()
             rle + objects  ops.predict_masks(rle=True, objects=...).result()
             host route     ops.predict_masks(rle=False, binary=True).result(), then scipy.ndimage.label + find_objects per image
           and sm_mask_objects alone between device events, with and without the mass launch.
  e2e      images/s of SaliencyPredictor on the 1 024-file corpus of scripts/predict_bench.py, output="rle" against "objects" (with
           and without a per-object RLE).

    python scripts/objects_bench.py            # all steps, tee'd into profiles/objects_bench.log
"""
import argparse
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "salient-object-detection_amd"))
STEPS = {"finish": 300, "e2e": 420}  # seconds
WARMUP, REPS = 3, 20
OPTS = dict(connectivity=8, min_area=16, max_objects=16)


def _stats(ms):
    import numpy as np
    ms = np.asarray(ms)
    return f"min {ms.min():8.3f}  median {np.median(ms):8.3f}  max {ms.max():8.3f} ms ({len(ms)} reps)"


def step_finish():
    import numpy as np
    import torch
    from scipy import ndimage
    from selfmask_amd import _native as N, ops
    dev = torch.device("cuda:0")
    lib = N.load()
    eight = np.ones((3, 3), int)
    for B, (H, W) in ((128, (300, 400)), (8, (1080, 1920))):
        gh, gw = -(-H // 16), -(-W // 16)
        nq, mh, mw, scale = 20, 2 * gh, 2 * gw, 8.0
        rng = np.random.Generator(np.random.PCG64(B))
        yy, xx = np.mgrid[:mh, :mw].astype(np.float32)
        masks = np.zeros((B, nq, mh, mw), np.float32)
        for b in range(B):
            for q in range(nq):
                for _ in range(3):
                    cy, cx, r = rng.uniform(.1, .9) * mh, rng.uniform(.1, .9) * mw, rng.uniform(.06, .2) * min(mh, mw)
                    masks[b, q] = np.maximum(masks[b, q], 1 / (1 + np.exp(np.minimum(((yy - cy) ** 2 + (xx - cx) ** 2) / (r * r) * 4 - 4, 60))))
        m = torch.from_numpy(masks).to(dev)
        o = torch.from_numpy(rng.random((B, nq)).astype(np.float32)).to(dev)
        table = ops.PackedImages([(H, W)] * B, dev)

        def rle():
            return ops.predict_masks(m, o, table, scale, rle=True).result()

        def rle_objects():
            return ops.predict_masks(m, o, table, scale, rle=True, objects=OPTS).result()

        def host_route():
            out = []
            for plane in ops.predict_masks(m, o, table, scale, rle=False, binary=True).result()["binary"]:
                lab, n = ndimage.label(plane, structure=eight)
                out.append((n, ndimage.find_objects(lab)))
            return out

        sides = {"rle": rle, "rle + objects": rle_objects, "host route": host_route}
        ms = {k: [] for k in sides}
        last = {}
        for rep in range(WARMUP + REPS):
            for name, fn in sides.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                last[name] = fn()
                if rep >= WARMUP:
                    ms[name].append((time.perf_counter() - t) * 1e3)
        objs = last["rle + objects"]["objects"]
        same = all(ob["n_components"] == n for ob, (n, _) in zip(objs, last["host route"]))
        print(f"{B} images of {H} x {W} (mask {mh} x {mw}): {sum(ob['n_components'] for ob in objs)} components, longest code "
              f"{max(len(r['counts']) for r in last['rle']['rle'])} runs; component counts equal scipy's: {same}")
        for name in sides:
            print(f"  {name:14s} call -> host result   {_stats(ms[name])}")
        print(f"  host route / (rle + objects) (medians) = {np.median(ms['host route']) / np.median(ms['rle + objects']):.2f}x; "
              f"objects add {np.median(ms['rle + objects']) - np.median(ms['rle']):.3f} ms to rle", flush=True)
        # the kernels alone, on the runs of one finish
        pend = ops.predict_masks(m, o, table, scale, rle=True)
        pend.result()
        cap, K = pend.cap, OPTS["max_objects"]
        wsb = lib.sm_mask_objects_workspace_bytes(B, cap, W)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        objects = torch.empty(B * K * C.sizeof(N.Object), dtype=torch.uint8, device=dev)
        summary = torch.empty((B, N.OBJ_SUMMARY_INTS), dtype=torch.int32, device=dev)
        segments = torch.empty((B, lib.sm_mask_objects_seg_cap(cap, W), 3), dtype=torch.int32, device=dev)
        a = N.ObjectsArgs()
        a.starts, a.info, a.cap, a.images = pend._starts.data_ptr(), pend._info.data_ptr(), cap, table.dev.data_ptr()
        a.mask_stride_b, a.best, a.mh, a.mw, a.scale = m.stride(0), pend.best.data_ptr(), mh, mw, scale
        a.objects, a.summary, a.segments = objects.data_ptr(), summary.data_ptr(), segments.data_ptr()
        a.workspace, a.workspace_bytes, a.B, a.max_width = ws.data_ptr(), wsb, B, W
        a.connectivity, a.min_area, a.max_objects = OPTS["connectivity"], OPTS["min_area"], K
        for label, ptr in (("components + mass", m.data_ptr()), ("components alone ", None)):
            a.masks = ptr
            dt = []
            for rep in range(WARMUP + REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                N.check(lib.sm_mask_objects(a, C.addressof(table.host), torch.cuda.current_stream(dev).cuda_stream), "sm_mask_objects")
                e1.record()
                e1.synchronize()
                if rep >= WARMUP:
                    dt.append(e0.elapsed_time(e1))
            print(f"  sm_mask_objects, {label} (device events)  {_stats(dt)}", flush=True)


def step_e2e():
    import torch
    from selfmask_amd import MaskFormer, synthetic_state_dict
    from selfmask_amd import datasets as DS
    from selfmask_amd.predictor import SaliencyPredictor
    dev = torch.device("cuda:0")
    n_images, batch = 1024, 64
    model = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    model.load_state_dict(synthetic_state_dict(24, "calib", patch_size=16), strict=True)
    model = model.to(dev).eval()
    root = tempfile.mkdtemp(prefix="sm_objects_bench_")
    try:
        DS.write_synthetic_dataset(root, "duts", n_images, seed=7, size_range=(300, 400))
        ds = DS.get_dataset(root, "duts")
        pred = SaliencyPredictor(model, device=dev, batch_size=batch)
        sides = {"output='rle'": lambda: pred(ds.p_imgs), "output='objects'": lambda: pred(ds.p_imgs, output="objects", objects=OPTS),
                 "objects, masks=False": lambda: pred(ds.p_imgs, output="objects", objects=dict(OPTS, masks=False))}
        secs = {k: [] for k in sides}
        for rep in range(1 + 5):  # one warm-up round (decode workers, graphs, page-locked pools), five timed
            for k, fn in sides.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep:
                    secs[k].append(time.perf_counter() - t)
        print(f"SaliencyPredictor end to end from {n_images} files of 300-400 px (P = 16, batch {batch}, 3 streams), wall clock:")
        for k, v in secs.items():
            r = sorted(n_images / s for s in v)
            print(f"  {k:22s} images/s  min {r[0]:7.0f}  median {r[len(r) // 2]:7.0f}  max {r[-1]:7.0f} ({len(r)} runs)", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "objects_bench.log"))
    args = ap.parse_args()
    if args.step:
        {"finish": step_finish, "e2e": step_e2e}[args.step]()
        return 0
    with open(args.log, "w") as log:
        for step, limit in STEPS.items():
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], timeout=limit, capture_output=True, text=True)
            except subprocess.TimeoutExpired:
                log.write(f"[{step}] ran out of its {limit} s\n")
                print(f"[{step}] ran out of its {limit} s")
                return 124
            log.write(p.stdout)
            print(p.stdout, end="")
            if p.returncode != 0:
                log.write(f"[{step}] failed with status {p.returncode}\n{p.stderr[-2000:]}\n")
                print(p.stderr[-2000:])
                return p.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
