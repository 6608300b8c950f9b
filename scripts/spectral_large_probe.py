#!/usr/bin/env python3
"""Phase times of the spectral clusterer (k-NN, graph, eigen-solve, k-means) at chosen n and B, through the library's own taps
(sm_forward_timing): image-like features (tests/test_oracle_spectral.py scene(), g x g points, cropped to n), one warm-up call, then
`reps` timed calls.  Prints one line per phase with ms per call and ms per image; the streaming k-NN's line adds its TFLOP/s
(three f16 products per multiply-add counted as one, as for gemm_f16x2).  Run it under `rocprofv3 --kernel-trace --stats -- python ...`
for the per-kernel split.  usage: spectral_large_probe.py [n,n,...] [B,B,...] [reps]"""
import ctypes as C
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "salient-object-detection_amd"), REPO, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from selfmask_amd import _native as N  # noqa: E402
from selfmask_amd import voting as VT  # noqa: E402
from test_oracle_spectral import scene  # noqa: E402

ns = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "9216,16384,32400").split(",")]
Bs = [int(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "1,32").split(",")]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
dev = torch.device("cuda:0")
lib = N.load()
for n in ns:
    g = int(np.ceil(np.sqrt(n)))
    one = scene(g, 3, 1)[0][:n]
    for B in Bs:
        x = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(one, (B, n, 384)))).to(dev)
        labels, det = VT.spectral_cluster(x, (2, 3, 4), return_details=True)  # warm-up (and the iteration counts)
        torch.cuda.synchronize()
        info = det["info"].cpu().numpy()
        lib.sm_forward_timing(1)
        t0 = time.perf_counter()
        for _ in range(reps):
            VT.spectral_cluster(x, (2, 3, 4))
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / reps * 1e3
        out = (N.KernelTime * 64)()
        k = lib.sm_forward_timing_read(out, 64)
        lib.sm_forward_timing(0)
        print(f"n {n} B {B}: {wall:.2f} ms per call, {wall / B:.2f} ms per image; outer iterations {info[:, 0].min()}..{info[:, 0].max()}, "
              f"mat-vecs {info[:, 1].min()}..{info[:, 1].max()}, converged {int(info[:, 2].sum())}/{B}")
        for e in out[:k]:
            if e.launches == 0:
                continue
            ms = e.total_us / reps * 1e-3
            line = f"    {e.name.decode():48s} {ms:9.3f} ms per call {ms / B:8.3f} ms per image"
            if e.flops > 0 and "knn_stream" in e.name.decode():
                line += f"  {e.flops / (e.total_us * 1e-6) / 1e12:7.1f} TFLOP/s (f16 MFMA peak ~2500 dense, x3 products)"
            print(line)
        sys.stdout.flush()
