"""Device JPEG decode: images/s of decode_jpeg_batch alone by host thread count, and SaliencyPredictor with decode="device" against
decode="host" (the parent configuration: Pillow in the decode worker processes) in the SAME job over the same files
-> profiles/jpeg_device_bench.log.

The file set is scripts/predict_bench.py's: 1 024 synthetic JPEG files of 300-400 px.  Steps, each a child process of its own under
its own time limit (a step that fails or runs out of time ends the run):
  decode     decode_jpeg_batch over the set in batches of 64 on one stream, threads = 1, 2, 4, 8, 16: wall clock of the whole set
             (one warm-up pass, three timed), plus the host half alone (HostBatch: file read + entropy decode, no device call) and
             the device half alone (device events around to_device of prepared batches), so the bounding side can be read off
  predictor  SaliencyPredictor(output="rle") with both decode settings, alternating, one warm-up round and five timed

    python scripts/jpeg_decode_bench.py            # all steps, tee'd into profiles/jpeg_device_bench.log
    python scripts/jpeg_decode_bench.py --step decode
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
STEPS = {"decode": 300, "predictor": 420}  # seconds
N_IMAGES, BATCH = 1024, 64


def _files(root):
    from selfmask_amd import datasets as DS
    DS.write_synthetic_dataset(root, "duts", N_IMAGES, seed=7, size_range=(300, 400))
    return DS.get_dataset(root, "duts").p_imgs


def _rates(secs):
    r = sorted(N_IMAGES / s for s in secs)
    return f"images/s  min {r[0]:7.0f}  median {r[len(r) // 2]:7.0f}  max {r[-1]:7.0f} ({len(r)} runs)"


def step_decode():
    import numpy as np
    import torch
    from selfmask_amd.jpeg import HostBatch, decode_jpeg_batch, probe_jpeg
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="sm_jpeg_bench_")
    try:
        files = _files(root)
        batches = [files[s:s + BATCH] for s in range(0, len(files), BATCH)]
        heads = [probe_jpeg(p) for p in files]
        nbytes = sum(os.path.getsize(p) for p in files)
        print(f"{len(files)} files of 300-400 px, {nbytes / len(files) / 1024:.1f} KiB each on average, "
              f"{sum(h.supported for h in heads)} taken by the device path, {sum(h.coef_bytes for h in heads) / len(files) / 1024:.0f} KiB of "
              f"coefficients per image; batches of {BATCH}, one stream, wall clock of the whole set")
        _, _, _, flags = decode_jpeg_batch(batches[0], dev, return_info=True)
        print(f"  first batch: {flags.count('device')} device, {flags.count('fallback')} fallback")
        for threads in (1, 2, 4, 8, 16):
            both, host = [], []
            for rep in range(1 + 3):
                torch.cuda.synchronize()
                t = time.perf_counter()
                for b in batches:
                    decode_jpeg_batch(b, dev, threads=threads)
                torch.cuda.synchronize()
                if rep:
                    both.append(time.perf_counter() - t)
                t = time.perf_counter()
                hbs = [HostBatch(b, threads) for b in batches]
                if rep:
                    host.append(time.perf_counter() - t)
                for hb in hbs:  # hand the page-locked buffers back
                    hb.to_device(dev)
                torch.cuda.synchronize()
            print(f"  threads {threads:2d}: decode_jpeg_batch {_rates(both)}   host half alone {_rates(host)}", flush=True)
        hbs = [HostBatch(b, 16) for b in batches]
        ms = []
        for hb in hbs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hb.to_device(dev)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = np.asarray(ms[1:])
        mb = sum(hb.staging.numel() for hb in hbs[1:]) / len(ms) / 1e6
        print(f"  device half alone (one copy of {mb:.1f} MB + two launches per batch of {BATCH}, device events): min {ms.min():.3f}  median "
              f"{np.median(ms):.3f}  max {ms.max():.3f} ms = {BATCH / np.median(ms) * 1e3:.0f} images/s", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def step_predictor():
    import torch
    from selfmask_amd import MaskFormer, synthetic_state_dict
    from selfmask_amd.predictor import SaliencyPredictor
    dev = torch.device("cuda:0")
    model = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    model.load_state_dict(synthetic_state_dict(24, "calib", patch_size=16), strict=True)
    model = model.to(dev).eval()
    root = tempfile.mkdtemp(prefix="sm_jpeg_bench_")
    try:
        files = _files(root)
        sides = {d: SaliencyPredictor(model, device=dev, batch_size=BATCH, decode=d) for d in ("host", "device")}
        secs, res = {k: [] for k in sides}, {}
        for rep in range(1 + 5):  # one warm-up round (decode workers, threads, graphs, page-locked pools), five timed
            for k, pred in sides.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                res[k] = pred(files)
                torch.cuda.synchronize()
                if rep:
                    secs[k].append(time.perf_counter() - t)
        print(f"SaliencyPredictor(output='rle') from {N_IMAGES} files of 300-400 px (P = 16, batch {BATCH}, 3 streams), wall clock; results of "
              f"the two settings identical: {res['host'] == res['device']}")
        for k, v in secs.items():
            print(f"  decode={k!r:9s} {_rates(v)}", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "jpeg_device_bench.log"))
    args = ap.parse_args()
    if args.step:
        {"decode": step_decode, "predictor": step_predictor}[args.step]()
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
