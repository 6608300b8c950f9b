"""E-measure and weighted F-measure on the device against the host chain -> profiles/sod_metrics_bench.log.

Steps, each a child process of its own under its own time limit (a step that fails or runs out of time ends the run):
  kernels  sm_sod_metrics_u8 on 128 images of 300 x 400 and on 8 images of 1080 x 1920, for two ground truths each: a blob covering
           about a fifth of the plane (typical) and ONE foreground pixel in a corner (the row pass's longest search).  Device events
           around the call (3 warm-up, 30 timed: median, min - max), one call under the library's taps for the share of each launch,
           and sm_evaluate_masks_f32 on the same batch for scale.
  host     the SciPy / numpy chain (distance_transform_edt with indices, ndimage.convolve, the two 256-bin histograms) on the first
           16 images of the same inputs, on one host thread and on a pool of 16 processes; this step never opens the GPU.
  e2e      images/s of one Evaluator pass over 256 files of 300 - 400 px, with and without extra_metrics (P = 16, batch 32).

    python scripts/sod_metrics_bench.py            # all steps, tee'd into profiles/sod_metrics_bench.log
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "salient-object-detection_amd"))
STEPS = {"kernels": 400, "host": 400, "e2e": 300}  # seconds
WARMUP, REPS = 3, 30
HOST_IMAGES = 16  # images the host chain is timed on (per-image cost x the batch)


def _stats(ms):
    import numpy as np
    ms = np.asarray(ms)
    return f"median {np.median(ms):9.3f}  min {ms.min():9.3f}  max {ms.max():9.3f} ms ({len(ms)} reps)"


def _inputs(B, H, W, kind, seed):
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:H, 0:W]
    gts, preds = [], []
    for b in range(B):
        g = np.zeros((H, W), np.uint8)
        if kind == "blob":
            cy, cx = rng.uniform(.35, .65) * H, rng.uniform(.35, .65) * W
            g[((yy - cy) / (0.25 * H)) ** 2 + ((xx - cx) / (0.26 * W)) ** 2 <= 1.0] = 1
        else:
            g[H - 1, W - 1] = 1
        base = np.where(g > 0, 0.8, 0.15) + 0.3 * rng.standard_normal((H, W)).astype(np.float32)
        gts.append(g)
        preds.append((np.clip(base, 0, 1) * 255).astype(np.uint8))
    return preds, gts


def _host_chain(args):
    """the toolkits' route for one image: both metrics from the saved map"""
    import numpy as np
    from scipy.ndimage import convolve, distance_transform_edt
    from selfmask_amd import sod_metrics as S
    p8, gt = args
    g = gt > 0
    e_adp, e_mean, e_max = S.e_measure(p8, gt)
    pred = p8.astype(np.float64) / 255.0
    dst, idx = distance_transform_edt(~g, return_indices=True)
    e = np.abs(pred - g)
    et = e.copy()
    et[~g] = e[idx[0][~g], idx[1][~g]]
    ea = convolve(et, weights=S.gaussian_7x7(), mode="constant", cval=0)
    m = np.where(g & (ea < e), ea, e)
    ew = m * np.where(g, 1.0, 2.0 - np.exp(S.LOG_HALF_OVER_5 * dst))
    G = int(g.sum())
    tpw, fpw = G - ew[g].sum(), ew[~g].sum()
    r, p = 1.0 - ew[g].mean(), tpw / (tpw + fpw + S.EPS)
    return e_adp, e_mean, e_max, 2.0 * r * p / (r + p + S.EPS)


def step_kernels():
    import numpy as np
    import torch
    from selfmask_amd import _native as N, ops
    dev = torch.device("cuda:0")
    lib = N.load()
    for B, (H, W) in ((128, (300, 400)), (8, (1080, 1920))):
        medians = {}
        for kind in ("blob", "corner"):
            preds, gts = _inputs(B, H, W, kind, seed=B)
            gb = ops.GtBatch([torch.from_numpy(g) for g in gts], dev)
            flat = torch.cat([torch.from_numpy(p).reshape(-1) for p in preds]).to(dev)
            dt = []
            for rep in range(WARMUP + REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = ops.sod_metrics(flat, gb)
                e1.record()
                e1.synchronize()
                if rep >= WARMUP:
                    dt.append(e0.elapsed_time(e1))
            medians[kind] = float(np.median(dt))
            print(f"{B} images of {H} x {W}, ground truth = {kind}: sm_sod_metrics_u8 (device events)  {_stats(dt)}")
            N.check(lib.sm_forward_timing(1), "sm_forward_timing")
            try:
                ops.sod_metrics(flat, gb)
                torch.cuda.synchronize()
                buf = (N.KernelTime * 64)()
                n = lib.sm_forward_timing_read(buf, 64)
            finally:
                lib.sm_forward_timing(0)
            for k in range(n):
                print(f"    {buf[k].name.decode():<20s} {buf[k].total_us:10.1f} us")
            print(f"    first image: e_adp, e_mean, e_max, wfm = {[round(float(v), 12) for v in out[0].cpu()]}", flush=True)
        print(f"  corner / blob (medians) = {medians['corner'] / medians['blob']:.1f}x")
        # sm_evaluate_masks_f32 on the same batch
        mh, mw = 2 * (-(-H // 16)), 2 * (-(-W // 16))
        rng = np.random.Generator(np.random.PCG64(1))
        mp = torch.from_numpy(rng.random((B, 20, mh, mw)).astype(np.float32)).to(dev)
        ob = torch.from_numpy(rng.random((B, 20)).astype(np.float32)).to(dev)
        dt = []
        for rep in range(WARMUP + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.evaluate_masks(mp, ob, gb, scale=8.0)
            e1.record()
            e1.synchronize()
            if rep >= WARMUP:
                dt.append(e0.elapsed_time(e1))
        print(f"  sm_evaluate_masks_f32 on the same batch (20 queries, mask {mh} x {mw})      {_stats(dt)}", flush=True)


def step_host():
    from concurrent.futures import ProcessPoolExecutor
    for B, (H, W) in ((128, (300, 400)), (8, (1080, 1920))):
        for kind in ("blob", "corner"):
            preds, gts = _inputs(B, H, W, kind, seed=B)
            sub = list(zip(preds[:HOST_IMAGES], gts[:HOST_IMAGES]))
            _host_chain(sub[0])  # imports and first-call set-up stay out of the timing
            t = time.perf_counter()
            ref = [_host_chain(a) for a in sub]
            one = (time.perf_counter() - t) / len(sub)
            with ProcessPoolExecutor(16) as pool:
                list(pool.map(_host_chain, sub[:2]))  # the workers are up
                t = time.perf_counter()
                list(pool.map(_host_chain, sub))
                many = (time.perf_counter() - t) / len(sub)
            print(f"{B} images of {H} x {W}, ground truth = {kind}: host chain (SciPy / numpy) {one * 1e3:8.2f} ms per image on one thread "
                  f"= {one * B * 1e3:9.1f} ms per batch; on 16 processes {many * 1e3:8.2f} ms per image = {many * B * 1e3:9.1f} ms per batch")
            print(f"    first image: e_adp, e_mean, e_max, wfm = {[round(float(v), 12) for v in ref[0]]}", flush=True)


def step_e2e():
    import torch
    from selfmask_amd import MaskFormer, synthetic_state_dict
    from selfmask_amd import datasets as DS
    from selfmask_amd.evaluator import Evaluator
    dev = torch.device("cuda:0")
    n_images, batch = 256, 32
    model = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    model.load_state_dict(synthetic_state_dict(24, "calib", patch_size=16), strict=True)
    model = model.to(dev).eval()
    root = tempfile.mkdtemp(prefix="sm_sod_bench_")
    try:
        DS.write_synthetic_dataset(root, "duts", n_images, seed=7, size_range=(300, 400))
        ev = Evaluator(network=model, dir_dataset=root)
        ev.device = dev
        secs = {False: [], True: []}
        for rep in range(1 + 3):  # one warm-up round (decode workers, graphs, page-locked pools), three timed
            for extra in (False, True):
                torch.cuda.synchronize()
                t = time.perf_counter()
                ev("duts", dir_ckpt=os.path.join(root, "ckpt"), img_size=224, batch_size=batch, device=dev, extra_metrics=extra)
                torch.cuda.synchronize()
                if rep:
                    secs[extra].append(time.perf_counter() - t)
        print(f"Evaluator end to end, {n_images} files of 300-400 px (P = 16, img_size 224, batch {batch}), wall clock:")
        for extra, v in secs.items():
            r = sorted(n_images / s for s in v)
            print(f"  extra_metrics={str(extra):5s} images/s  min {r[0]:7.0f}  median {r[len(r) // 2]:7.0f}  max {r[-1]:7.0f} ({len(r)} runs)",
                  flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "sod_metrics_bench.log"))
    args = ap.parse_args()
    if args.step:
        {"kernels": step_kernels, "host": step_host, "e2e": step_e2e}[args.step]()
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
