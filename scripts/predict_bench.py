"""The bulk predictor's finish and the predictor end to end -> profiles/predict_bench.log.

Steps, each a child process of its own under its own time limit (a step that fails or runs out of time ends the run):
  finish   the fused finish (sm_predict_masks_f32: run boundaries only) against the composition of the kernels it replaces, in one
           process, the two sides alternating: sm_pick_mask_f32 -> sm_upsample_selected_native_f64 -> threshold into uint8 planes ->
           sm_rle_runs_u8 (its run step is by now the fused side's own chunked walk over a byte source: what is compared is the
           composition).  128 images of 300 x 400 and 8 images of 1080 x 1920 at P = 16 (masks 38 x 50 and 136 x 240, scale 8).
           Device events around one call, 3 warm-up and 30 timed repetitions: min / median / max.  All buffers are allocated beforehand.
  rle      voting.rle_runs_async on padded planes of blob masks, the same two shapes: wall clock from the call to .result(), and
           device events around the call alone (the walk and the copy of its 8 bytes per image).
  e2e      images/s of SaliencyPredictor from files (synthetic 300-400 px set) beside the evaluator's bucketed native rate on the
           same files in the same process, wall clock.  Both are bound by the host's decode above a few thousand images/s.

    python scripts/predict_bench.py            # all steps, tee'd into profiles/predict_bench.log
    python scripts/predict_bench.py --step finish
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
STEPS = {"finish": 240, "rle": 120, "e2e": 420}  # seconds
WARMUP, REPS = 3, 30


def _stats(ms):
    import numpy as np
    ms = np.asarray(ms)
    return f"min {ms.min():8.3f}  median {np.median(ms):8.3f}  max {ms.max():8.3f} ms ({len(ms)} reps)"


def step_finish():
    import numpy as np
    import torch
    from selfmask_amd import _native as N, ops
    dev = torch.device("cuda:0")
    lib = N.load()
    st = lambda: torch.cuda.current_stream(dev).cuda_stream  # noqa: E731
    for B, (H, W) in ((128, (300, 400)), (8, (1080, 1920))):
        gh, gw = -(-H // 16), -(-W // 16)
        nq, mh, mw, scale, cap = 20, 2 * gh, 2 * gw, 8.0, 8192
        rng = np.random.Generator(np.random.PCG64(B))
        yy, xx = np.mgrid[:mh, :mw].astype(np.float32)
        masks = np.empty((B, nq, mh, mw), np.float32)
        for b in range(B):  # smooth blobs, a different one per query
            for q in range(nq):
                cy, cx, r = rng.uniform(.2, .8) * mh, rng.uniform(.2, .8) * mw, rng.uniform(.15, .35) * min(mh, mw)
                masks[b, q] = 1 / (1 + np.exp(((yy - cy) ** 2 + (xx - cx) ** 2) / (r * r) * 4 - 4))
        m = torch.from_numpy(masks).to(dev)
        o = torch.from_numpy(rng.random((B, nq)).astype(np.float32)).to(dev)
        table = ops.PackedImages([(H, W)] * B, dev)
        # fused side
        best = torch.empty(B, dtype=torch.int32, device=dev)
        starts, info = torch.empty((B, cap), dtype=torch.int32, device=dev), torch.empty((B, 2), dtype=torch.int32, device=dev)
        wsb = lib.sm_predict_workspace_bytes(B, H * W)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        a = N.PredictArgs()
        a.masks, a.mask_stride_b, a.objectness, a.obj_stride_b = m.data_ptr(), m.stride(0), o.data_ptr(), o.stride(0)
        a.images, a.best, a.starts, a.info, a.cap = table.dev.data_ptr(), best.data_ptr(), starts.data_ptr(), info.data_ptr(), cap
        a.workspace, a.workspace_bytes = ws.data_ptr(), wsb
        a.B, a.nq, a.mh, a.mw, a.max_pixels, a.scale = B, nq, mh, mw, H * W, scale

        def fused():
            N.check(lib.sm_predict_masks_f32(a, C.addressof(table.host), st()), "sm_predict_masks_f32")

        # composed side: the parent commit's kernels
        picked = torch.empty((B, mh * mw), dtype=torch.float32, device=dev)
        best2 = torch.empty(B, dtype=torch.int32, device=dev)
        rows = torch.zeros((B, 16), dtype=torch.float32, device=dev)
        target = torch.empty(B * H * W, dtype=torch.float64, device=dev)
        planes = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        starts2, info2, ws2 = torch.empty_like(starts), torch.empty_like(info), torch.empty_like(ws)

        def composed():
            N.check(lib.sm_pick_mask_f32(m.data_ptr(), m.stride(0), o.data_ptr(), o.stride(0), picked.data_ptr(), best2.data_ptr(), B, nq,
                                         mh * mw, st()), "sm_pick_mask_f32")
            rows[:, 14] = best2
            N.check(lib.sm_upsample_selected_native_f64(m.data_ptr(), m.stride(0), rows.data_ptr(), 14, table.dev.data_ptr(), target.data_ptr(),
                                                        B, mh, mw, scale, H * W, st()), "sm_upsample_selected_native_f64")
            torch.gt(target.view(B, H, W), 0.5, out=planes.view(torch.bool))
            N.check(lib.sm_rle_runs_u8(planes.data_ptr(), B, H, W, None, starts2.data_ptr(), cap, info2.data_ptr(), ws2.data_ptr(), wsb,
                                       st()), "sm_rle_runs_u8")

        ms = {"fused": [], "composed": []}
        for rep in range(WARMUP + REPS):
            for name, fn in (("fused", fused), ("composed", composed)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rep >= WARMUP:
                    ms[name].append(e0.elapsed_time(e1))
        same = torch.equal(info, info2) and torch.equal(best, best2) and all(
            torch.equal(starts[b, :int(info[b, 0])], starts2[b, :int(info[b, 0])]) for b in range(B) if int(info[b, 0]) <= cap)
        print(f"finish alone, {B} images of {H} x {W} (mask {mh} x {mw}, {'LDS' if mh * mw <= 12288 else 'L2'} path), "
              f"longest code {int(info[:, 0].max())} boundaries, outputs identical: {same}")
        print(f"  fused    (sm_predict_masks_f32)                      {_stats(ms['fused'])}")
        print(f"  composed (pick -> upsample f64 -> threshold -> rle)  {_stats(ms['composed'])}")
        print(f"  composed / fused (medians) = {np.median(ms['composed']) / np.median(ms['fused']):.2f}x", flush=True)


def step_rle():
    import numpy as np
    import torch
    from selfmask_amd.voting import rle_runs_async
    dev = torch.device("cuda:0")
    for B, (H, W) in ((128, (300, 400)), (8, (1080, 1920))):
        rng = np.random.Generator(np.random.PCG64(B))
        yy, xx = np.mgrid[:H, :W].astype(np.float32)
        planes = np.zeros((B, H, W), np.uint8)
        for b in range(B):  # three blobs per image
            for _ in range(3):
                cy, cx, r = rng.uniform(.1, .9) * H, rng.uniform(.1, .9) * W, rng.uniform(.06, .2) * min(H, W)
                planes[b] |= ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.uint8)
        p = torch.from_numpy(planes).to(dev)
        wall, device = [], []
        for rep in range(WARMUP + REPS):
            torch.cuda.synchronize()
            t = time.perf_counter()
            codes = rle_runs_async(p).result()
            if rep >= WARMUP:
                wall.append((time.perf_counter() - t) * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pend = rle_runs_async(p)
            e1.record()
            e1.synchronize()
            if rep >= WARMUP:
                device.append(e0.elapsed_time(e1))
            assert pend.result() == codes
        print(f"rle_runs_async, {B} planes of {H} x {W}, longest code {max(len(c['counts']) for c in codes)} runs")
        print(f"  call -> host result          {_stats(wall)}")
        print(f"  the call alone (device events) {_stats(device)}", flush=True)


def step_e2e():
    import torch
    from selfmask_amd import MaskFormer, synthetic_state_dict
    from selfmask_amd import datasets as DS
    from selfmask_amd.evaluator import Evaluator
    from selfmask_amd.predictor import SaliencyPredictor
    dev = torch.device("cuda:0")
    n_images, batch = 1024, 64
    model = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    model.load_state_dict(synthetic_state_dict(24, "calib", patch_size=16), strict=True)
    model = model.to(dev).eval()
    root = tempfile.mkdtemp(prefix="sm_predict_bench_")
    try:
        DS.write_synthetic_dataset(root, "duts", n_images, seed=7, size_range=(300, 400))
        ds = DS.get_dataset(root, "duts")
        pred = SaliencyPredictor(model, device=dev, batch_size=batch)
        ev = Evaluator(network=model, dir_dataset=root)
        ev.device = dev
        sides = {"SaliencyPredictor, output='rle'": lambda: pred(ds.p_imgs),
                 "SaliencyPredictor, output='soft'": lambda: pred(ds.p_imgs, output="soft"),
                 "Evaluator, bucketed native (context)": lambda: ev("duts", dir_ckpt=os.path.join(root, "ck"), batch_size=batch, device=dev)}
        secs = {k: [] for k in sides}
        for rep in range(1 + 5):  # one warm-up round (decode workers, graphs, page-locked pools), five timed
            for k, fn in sides.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep:
                    secs[k].append(time.perf_counter() - t)
        print(f"end to end from {n_images} files of 300-400 px (P = 16, batch {batch}, 3 streams), wall clock, host-decode-bound:")
        for k, v in secs.items():
            r = sorted(n_images / s for s in v)
            print(f"  {k:40s} images/s  min {r[0]:7.0f}  median {r[len(r) // 2]:7.0f}  max {r[-1]:7.0f} ({len(r)} runs)", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "predict_bench.log"))
    args = ap.parse_args()
    if args.step:
        {"finish": step_finish, "rle": step_rle, "e2e": step_e2e}[args.step]()
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
