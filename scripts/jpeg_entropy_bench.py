"""Device entropy decode: decode_jpeg_batch(entropy="device") against entropy="host" in the SAME job over the same files, the host
half alone, the entropy launch alone (with its synchronisation rounds), bytes copied per batch, and SaliencyPredictor end to end with
decode="host", decode="device" and decode="device" + entropy="device" -> profiles/jpeg_entropy_bench.log.

The protocol is scripts/jpeg_decode_bench.py's: 1 024 synthetic JPEG files of 300-400 px, batches of 64, the settings alternating
inside one process, medians with min - max.  Steps, each a child process of its own under its own time limit (a step that fails or
runs out of time ends the run):
  decode     decode_jpeg_batch over the set on one stream, threads = 1, 4, 16, both settings alternating (one warm-up pass, three
             timed), the host half alone of each (HostBatch, no device call), the bytes of the one copy per batch, and the entropy
             launch alone (device events around sm_jpeg_entropy_decode_batch on uploaded records, rounds and chunks from its
             workspace)
  predictor  SaliencyPredictor(output="rle") with the three settings, alternating, one warm-up round and five timed

    python scripts/jpeg_entropy_bench.py            # all steps, tee'd into profiles/jpeg_entropy_bench.log
    python scripts/jpeg_entropy_bench.py --step decode
"""
import argparse
import ctypes
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
ENTROPIES = ("host", "device")


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
    from selfmask_amd import _native as N
    from selfmask_amd.jpeg import HostBatch, decode_jpeg_batch
    dev = torch.device("cuda:0")
    lib = N.load()
    root = tempfile.mkdtemp(prefix="sm_jpeg_bench_")
    try:
        files = _files(root)
        batches = [files[s:s + BATCH] for s in range(0, len(files), BATCH)]
        nbytes = sum(os.path.getsize(p) for p in files)
        print(f"{len(files)} files of 300-400 px, {nbytes / len(files) / 1024:.1f} KiB each on average; batches of {BATCH}, one stream, wall "
              f"clock of the whole set")
        same = True
        for e in ENTROPIES:
            _, _, _, flags = decode_jpeg_batch(batches[0], dev, return_info=True, entropy=e)
            print(f"  first batch, entropy={e!r}: {flags.count('device')} device, {flags.count('fallback')} fallback")
        a, b = (decode_jpeg_batch(batches[0], dev, return_info=True, entropy=e) for e in ENTROPIES)
        for k, (h, w) in enumerate(a[1]):
            o = a[2][k]
            same = same and bool(torch.equal(a[0][o:o + h * w * 3], b[0][o:o + h * w * 3]))
        print(f"  pixels of the two settings identical on the first batch: {same}")
        for threads in (1, 4, 16):
            both, host = {e: [] for e in ENTROPIES}, {e: [] for e in ENTROPIES}
            for rep in range(1 + 3):
                for e in ENTROPIES:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for bt in batches:
                        decode_jpeg_batch(bt, dev, threads=threads, entropy=e)
                    torch.cuda.synchronize()
                    if rep:
                        both[e].append(time.perf_counter() - t)
                    t = time.perf_counter()
                    hbs = [HostBatch(bt, threads, entropy=e) for bt in batches]
                    if rep:
                        host[e].append(time.perf_counter() - t)
                    for hb in hbs:  # hand the page-locked buffers back
                        hb.to_device(dev)
                    torch.cuda.synchronize()
            for e in ENTROPIES:
                print(f"  threads {threads:2d} entropy={e!r:9s}: decode_jpeg_batch {_rates(both[e])}   host half alone {_rates(host[e])}", flush=True)
        for e in ENTROPIES:
            hbs = [HostBatch(bt, 16, entropy=e) for bt in batches]
            mb = sum(hb.copy_bytes for hb in hbs) / len(hbs) / 1e6
            extra = f" + {4 * BATCH} status bytes back" if e == "device" else ""
            print(f"  entropy={e!r:9s}: one copy of {mb:.2f} MB per batch of {BATCH} ({mb * 1e3 / BATCH:.0f} kB per image){extra}")
            for hb in hbs:
                hb.to_device(dev)
            torch.cuda.synchronize()
        # the entropy launch alone, on records that are on the device already
        ms, rounds, chunks = [], [], []
        for bt in batches:
            hb = HostBatch(bt, 16, entropy="device")
            n = hb.n_device
            d = hb.staging.to(dev)
            coef = torch.empty(hb.coef_bytes, dtype=torch.uint8, device=dev)
            status = torch.empty(n, dtype=torch.int32, device=dev)
            ws = int(lib.sm_jpeg_entropy_workspace_bytes(ctypes.addressof(hb.scans), n, 0, 0))
            stats = torch.zeros(ws // 4, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            for rep in range(2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                N.check(lib.sm_jpeg_entropy_decode_batch(ctypes.addressof(hb.scans), d.data_ptr() + hb.scan_at, n, d.data_ptr(), coef.data_ptr(),
                                                         status.data_ptr(), stats.data_ptr(), ws, 0, 0, torch.cuda.current_stream().cuda_stream),
                        "sm_jpeg_entropy_decode_batch")
                e1.record()
                e1.synchronize()
            ms.append(e0.elapsed_time(e1))
            assert not status.any().item()
            st = stats.cpu().numpy()[:2 * n].reshape(n, 2)
            rounds += st[:, 0].tolist()
            chunks += st[:, 1].tolist()
            hb.discard()
        ms = np.asarray(ms)
        print(f"  entropy launch alone (one launch per batch of {BATCH}, records on the device, device events, second of two runs): min "
              f"{ms.min():.3f}  median {np.median(ms):.3f}  max {ms.max():.3f} ms = {BATCH / np.median(ms) * 1e3:.0f} images/s; "
              f"synchronisation rounds per image: min {min(rounds)}  median {int(np.median(rounds))}  max {max(rounds)}, chunks per image: "
              f"max {max(chunks)} (1024-bit sub-sequences, 1024 per chunk)", flush=True)
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
        sides = {"decode='host'": SaliencyPredictor(model, device=dev, batch_size=BATCH, decode="host"),
                 "decode='device', entropy='host'": SaliencyPredictor(model, device=dev, batch_size=BATCH, decode="device"),
                 "decode='device', entropy='device'": SaliencyPredictor(model, device=dev, batch_size=BATCH, decode="device", entropy="device")}
        secs, res = {k: [] for k in sides}, {}
        for rep in range(1 + 5):  # one warm-up round (decode workers, threads, graphs, page-locked pools), five timed
            for k, pred in sides.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                res[k] = pred(files)
                torch.cuda.synchronize()
                if rep:
                    secs[k].append(time.perf_counter() - t)
        first = res["decode='host'"]
        print(f"SaliencyPredictor(output='rle') from {N_IMAGES} files of 300-400 px (P = 16, batch {BATCH}, 3 streams), wall clock; results of "
              f"the three settings identical: {all(r == first for r in res.values())}")
        for k, v in secs.items():
            print(f"  {k:34s} {_rates(v)}", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "jpeg_entropy_bench.log"))
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
