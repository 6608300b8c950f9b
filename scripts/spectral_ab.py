#!/usr/bin/env python3
"""A/B of two builds of the library on the spectral clusterer and its k-NN, in ONE job: child processes alternate between the
libraries (the SM_HIP_LIB switch, as scripts/ab_libs.sh does for bench.py), and the first library runs twice per round - its two
series against each other give the spread of every line, which the other library's median is then judged against.

Per child: scripts/knn_dim_bench.py --skip-generator (the three k-NN paths) and, in a process of its own, voting.spectral_cluster
(feats, (2, 3, 4)) under device events on scene features, one n per eigen-solver mode: n = 784 at bench.py's batch of 128, and
n = 1900, 3136, 16384 at B = 8.  --bench adds bench.py's own clustering figure (--only-leg pseudo_masks), once per library.

    python scripts/spectral_ab.py --prev salient-object-detection_amd/lib/libselfmask_hip_prev.so [--rounds 3] [--out FILE]

A child that fails or runs out of time ends the job: nothing more is started."""
import argparse
import json
import math
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [os.path.join(ROOT, "salient-object-detection_amd"), ROOT, os.path.join(ROOT, "tests")]
CLUSTER_CASES = ((784, 128, 7), (1900, 8, 5), (3136, 8, 5), (16384, 8, 3))  # (points, batch, timed calls)


def child():
    import numpy as np
    import torch
    from selfmask_amd import voting as VT
    from test_oracle_spectral import scene
    out = {}
    for n, B, reps in CLUSTER_CASES:
        g = math.isqrt(n - 1) + 1
        x = torch.from_numpy(np.stack([scene(g, 3, 300 + b)[0][:n] for b in range(B)])).to("cuda:0")
        VT.spectral_cluster(x, (2, 3, 4))
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            VT.spectral_cluster(x, (2, 3, 4))
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        out[f"spectral_cluster n={n} B={B}"] = float(np.median(ms))
        del x
        VT.release_scratch()
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out), flush=True)


def run(cmd, lib, limit, log):
    env = dict(os.environ)
    if lib:
        env["SM_HIP_LIB"] = os.path.abspath(lib)
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        log(f"FAILED ({r.returncode}): {' '.join(cmd)}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        sys.exit(1)
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--prev", help="the library to compare lib/libselfmask_hip.so against")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--knn-reps", type=int, default=5)
    ap.add_argument("--budget", type=float, default=0.0, help="seconds after which no further round is started (0: none)")
    ap.add_argument("--bench", action="store_true", help="also bench.py --only-leg pseudo_masks, once per library")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_ab.log"))
    a = ap.parse_args()
    if a.child:
        return child()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "w")

    def log(line=""):
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    libs = (("prev", a.prev), ("prev again", a.prev), ("new", None))
    series = {name: {} for name, _ in libs}  # name -> line -> one median per round
    tmp = os.path.join(tempfile.mkdtemp(prefix="spectral_ab_"), "knn.log")
    log(f"# spectral_ab.py: prev = {a.prev}, new = lib/libselfmask_hip.so; {a.rounds} rounds of (prev, prev again, new), a fresh process each; ms")
    t0 = time.perf_counter()
    for rnd in range(a.rounds):
        if rnd and a.budget and time.perf_counter() - t0 > a.budget * rnd / (rnd + 1):  # (the next round would not fit)
            log(f"# {rnd} rounds in {time.perf_counter() - t0:.0f} s: the budget of {a.budget:.0f} s leaves no room for another")
            break
        for name, lib in libs:
            run([sys.executable, "scripts/knn_dim_bench.py", "--skip-generator", "--reps", str(a.knn_reps), "--out", tmp], lib, 400, log)
            got = {}
            for line in open(tmp):
                m = re.match(r"(knn .*?):\s+([0-9.]+) ms", line)
                if m:
                    got[re.sub(r"\s+", " ", m.group(1))] = float(m.group(2))
            text = run([sys.executable, "scripts/spectral_ab.py", "--child"], lib, 400, log)
            got.update(json.loads([ln for ln in text.splitlines() if ln.startswith("RESULT ")][-1][7:]))
            for k, v in got.items():
                series[name].setdefault(k, []).append(v)
            log(f"round {rnd} {name:10s}: " + ", ".join(f"{v:.3f}" for v in got.values()))
    log()
    log(f"{'line':44s} {'prev: median (min - max of both series)':>42s} {'prev again':>11s} {'new':>11s}  new within prev's spread")
    worst = True
    for k in series["prev"]:
        both = sorted(series["prev"][k] + series["prev again"][k])
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        new = med(series["new"][k])
        ok = both[0] <= new <= both[-1]
        faster = new < both[0]
        worst &= ok or faster
        log(f"{k:44s} {med(series['prev'][k]):14.3f} ({both[0]:.3f} - {both[-1]:.3f})".ljust(88) +
            f"{med(series['prev again'][k]):11.3f} {new:11.3f}  {'yes' if ok else 'below it (faster)' if faster else 'NO: above it'}")
    log(f"# every line of the new library within, or below, the spread of prev: {worst}")
    if a.bench:
        for name, lib in (("prev", a.prev), ("new", None)):
            log(f"# bench.py --only-leg pseudo_masks on {name} ...")
            text = run([sys.executable, "bench.py", "--only-leg", "pseudo_masks", "--no-cpu-baseline"], lib, 900, log)
            r = json.loads(text.strip().splitlines()[-1])["pseudo_masks"]
            log(f"bench.py pseudo_masks {name:5s}: {r['value']} images/s, spectral_cluster_ms_per_batch {r['spectral_cluster_ms_per_batch']}, "
                f"native 300x400: {r['native_300x400']['value']} images/s, spectral_cluster_ms_per_batch {r['native_300x400']['spectral_cluster_ms_per_batch']}")
    f.close()


if __name__ == "__main__":
    main()
