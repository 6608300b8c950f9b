"""Digests of the spectral clusterer's outputs, for A/B runs of two builds of the library that must agree bit for bit (a change of
csrc/spectral.hip that moves no arithmetic).

Runs a fixed, seeded case list (features from tests/test_oracle_spectral.scene) on the library that SM_HIP_LIB names (default:
lib/libselfmask_hip.so) and prints ONE JSON object {case: {output: sha256 of the tensor's bytes}}: the lists of voting.knn for
every method, and knn / eigenvalues / embedding / residuals / info / labels of voting.spectral_cluster(..., return_details=True).
Between them the cases reach the three k-NN paths at both feature widths and both list capacities, and every instantiation of the
eigen-solver; each clusterer case carries the plan the host chooses for it ("plan": sp_plan's arithmetic restated below) and whether
the lists, as the device counts them, fit the LDS of a MODE 3 launch ("lds_graph": false = the kernel fell back to MODE 0's steps).
``--tuning`` adds the plans and the k-NN path only the tuning library can force (SM_SPECTRAL_PLAN, SM_SPECTRAL_KNN).  Run it once
per library, each in a fresh process, and compare the objects:

    SM_HIP_LIB=$PWD/salient-object-detection_amd/lib/libselfmask_hip_prev.so python scripts/spectral_bits.py --out prev.json
    python scripts/spectral_bits.py --out new.json
    python scripts/spectral_bits.py --plans        # no GPU: the case list with its plans
"""
import argparse
import hashlib
import json
import math
import os
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [os.path.join(ROOT, "salient-object-detection_amd"), ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
from test_oracle_spectral import scene  # noqa: E402

DEV = "cuda:0"
LDS_MAX, STAGED_MAX = 159744, 153600  # SP_LDS_MAX and the staged block's limit in sp_plan


def ent_offset(n, w):
    return (2 * (n + 1) * w * 8 + ((n + 1) * 8 if w == 8 else 0) + (2 * n + 1) * 2 + 15) & ~15


def plan(n, m, forced=None):
    """(mode, cg) as sp_plan(n, m) decides; forced: a value of the tuning library's SM_SPECTRAL_PLAN"""
    p = (0, 0)
    if ((ent_offset(n, 8) + (((2 * m + 3) * n + 7) & ~7) * 2 + 15) & ~15) <= LDS_MAX and n * 64 <= 65535:
        p = (2, 8)
    for c in (4, 2, 1):
        if not p[1] and ent_offset(n, c) + (2 * m + 1) * n * 2 <= LDS_MAX and n * c * 8 <= 65535:
            p = (3, c)
    if forced is not None:
        p = {"cg1": (0, 1), "gather": (1, 8), "0": (0, 0)}[forced]
    if not p[1]:
        fit = [c for c in (8, 4, 2, 1) if (n + 1) * c * 8 <= STAGED_MAX]
        p = (0, fit[0]) if fit else (1, 8)
    return p


def lists_fit(knn, cg):
    """does the graph of these lists (m own + in-degree entries per row, every list padded to four) fit a MODE 3 launch with cg columns"""
    n, m = knn.shape
    first = np.ones(n * m, bool)  # a point that lists another twice counts once
    for r in range(1, m):
        first[r::m] = ~(knn[:, :r] == knn[:, r:r + 1]).any(1)
    indeg = np.bincount(knn.reshape(-1)[first], minlength=n)
    total4 = int(((m + indeg + 3) // 4).sum())
    return total4 <= (LDS_MAX - ent_offset(n, cg)) // 8 and total4 <= 0xffff


def points(n, dim=384, seed=0, k=3):
    g = math.isqrt(n - 1) + 1
    return scene(g, k, 100 + seed, dim=dim)[0][:n]


def with_nan(x):
    x = x.copy()
    x[5] = np.nan
    x[77, 3] = np.inf
    return x


# name: (features (B, n, D), n_neighbors)
def knn_cases():
    c = {}
    for d in (384, 2048):
        c[f"knn|d{d}|n784|nn10"] = (points(784, d)[None], 10)      # CAP 16
        c[f"knn|d{d}|n784|nn20"] = (points(784, d, 1)[None], 20)   # CAP 32
        c[f"knn|d{d}|n100|nn10"] = (points(100, d, 2)[None], 10)   # tails in every tile
        c[f"knn|d{d}|n100|nn20|b2"] = (np.stack([points(100, d, 3), points(100, d, 4)]), 20)
        c[f"knn|d{d}|n784|nn10|nan"] = (with_nan(points(784, d, 5))[None], 10)  # the fallback index
    c["knn|d384|n784|nn10|b2"] = (np.stack([points(784, 384, 6), points(784, 384, 7)]), 10)
    c["knn|d2048|n8448|nn10"] = (points(8448, 2048, 8)[None], 10)  # slabs: 4 whole and one of 256 rows
    c["knn|d384|n8448|nn10"] = (points(8448, 384, 9)[None], 10)
    return c


# name: (n, D, n_neighbors, B, nan); the expected plan is asserted
CLUSTER = {
    "n784": (784, 384, 10, 1, False, (2, 8)),
    "n784|b2": (784, 384, 10, 2, False, (2, 8)),
    "n784|nan": (784, 384, 10, 1, True, (2, 8)),
    "n784|d2048": (784, 2048, 10, 1, False, (2, 8)),
    "n1024": (1024, 384, 10, 1, False, (3, 4)),
    "n1936": (1936, 384, 10, 1, False, (3, 2)),
    "n2156": (2156, 384, 10, 1, False, (3, 2)),   # the most points of the two-column plan: padded, the lists do not fit
    "n2500": (2500, 384, 10, 1, False, (3, 1)),
    "n1936|nn20": (1936, 384, 20, 1, False, (0, 8)),
    "n3136": (3136, 384, 10, 1, False, (0, 4)),
    "n6400": (6400, 384, 10, 1, False, (0, 2)),
    "n8448|d2048": (8448, 2048, 10, 1, False, (0, 2)),  # the slab path inside the clusterer
    "n16384": (16384, 384, 10, 1, False, (0, 1)),
    "n32768": (32768, 384, 10, 1, False, (1, 8)),
}
FORCED = (("SM_SPECTRAL_PLAN", "0"), ("SM_SPECTRAL_PLAN", "cg1"), ("SM_SPECTRAL_PLAN", "gather"), ("SM_SPECTRAL_KNN", "stream"))


def cluster_features(name):
    n, d, nn, B, nan, want = CLUSTER[name]
    seed = sorted(CLUSTER).index(name)
    x = np.stack([points(n, d, 20 + seed + 50 * b) for b in range(B)])
    return (with_nan(x[0])[None] if nan else x), nn


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def bits(tuning):
    import torch
    from selfmask_amd import voting as VT
    res, t0 = {}, time.perf_counter()

    def progress(key):  # (to stderr: stdout carries the JSON object alone)
        print(f"[{time.perf_counter() - t0:7.1f} s] {key}", file=sys.stderr, flush=True)

    for name, (x, nn) in knn_cases().items():
        xd = torch.from_numpy(x).to(DEV)
        res[name] = {method: sha(VT.knn(xd, nn, method)) for method in ("auto", "gram", "stream")}
        del xd
        VT.release_scratch()
        progress(name)

    def cluster(name, key, forced=None):
        n, d, nn, B, nan, want = CLUSTER[name]
        x, nn = cluster_features(name)
        labels, det = VT.spectral_cluster(torch.from_numpy(x).to(DEV), (2, 3, 4), nn, return_details=True)
        torch.cuda.synchronize()
        p = plan(n, min(nn - 1, n - 1), forced)
        out = {k: sha(v) for k, v in sorted(det.items())}
        out["labels"] = sha(labels)
        out["plan"] = f"MODE {p[0]}, CG {p[1]}"
        if p[0] == 3:
            out["lds_graph"] = all(lists_fit(det["knn"][b].cpu().numpy(), p[1]) for b in range(B))
        out["info_rows"] = det["info"].cpu().numpy().tolist()
        res[key] = out
        VT.release_scratch()
        progress(f"{key}: {out['plan']}")

    for name in CLUSTER:
        cluster(name, f"cluster|{name}")
    if tuning:
        for var, val in FORCED:
            os.environ[var] = val
            cluster("n784", f"cluster|n784|{var}={val}", val if var == "SM_SPECTRAL_PLAN" else None)
            del os.environ[var]
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the JSON object to this file")
    ap.add_argument("--tuning", action="store_true", help="SM_HIP_LIB names a tuning library: add its forced plans and k-NN path at n = 784")
    ap.add_argument("--plans", action="store_true", help="print the clusterer cases with their plans and exit (no GPU)")
    a = ap.parse_args()
    for name, (n, d, nn, B, nan, want) in CLUSTER.items():
        assert plan(n, min(nn - 1, n - 1)) == want, (name, plan(n, min(nn - 1, n - 1)), want)
    if a.plans:
        for name, (n, d, nn, B, nan, want) in CLUSTER.items():
            print(f"{name:14s} n={n:6d} D={d:5d} n_neighbors={nn:3d} B={B}: MODE {want[0]}, CG {want[1]}")
        sys.exit(0)
    res = bits(a.tuning)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")
    print(json.dumps(res, sort_keys=True))
