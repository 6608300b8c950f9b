#!/usr/bin/env python3
"""Generate tests/golden/attention_*.npz: the last block's self-attention of the REAL reference encoder on the CPU.

Usage (from the repository root, on the build machine that has the reference checkout):
    python scripts/gen_attention_golden.py

The reference is imported through oracle.gen_golden (_import_reference / build_reference_model, used as they are); this
script holds none of its text.  Inputs are the synthetic checkpoints and images of the forward fixtures (the seeds and styles of
oracle.gen_golden.FORWARD_CASES), so the tests re-generate them from the seeds.  Stored, in fp32 and fp64, from
``model.encoder.get_last_selfattention(x)`` (vision_transformer.py:307-314):
  cls_f32 / cls_f64          (B, 6, N)         row 0: the CLS token's attention
  rows, rows_f32 / rows_f64  (R,), (B, 6, R, N) a few whole query rows
  f32_vs_f64_maxabs          max |fp32 - fp64| over exactly the entries the fixture stores
The peaky 224^2 case also stores image 0's whole fp64 matrix, two heads per file (attention_<name>_full_h<k>.npz: full_f64
(2, N, N)), to keep every file small.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import gen_golden as G  # noqa: E402

# name -> (query rows stored besides the CLS row, store image 0 in full)
CASES = {
    "p16_224_peaky": ((), True),
    "p16_224_soft": ((0, 1, 98, 196), False),
    "p16_250x333_peaky": ((0, 1, 168, 336), False),
    "p8_200x168_calib": ((0, 1, 263, 525), False),
}


@torch.no_grad()
def main():
    _vits, mf = G._import_reference()
    torch.set_num_threads(G.N_THREADS)
    forward = {c[0]: c for c in G.FORWARD_CASES}
    for name, (rows, full) in CASES.items():
        _, patch, (B, Hh, Ww), wseed, style, xseed, _ = forward[name]
        sd = G.synthetic_state_dict(wseed, style, patch_size=patch)
        x = torch.from_numpy(G.synthetic_images(xseed, (B, 3, Hh, Ww)))
        a32 = G.build_reference_model(mf, patch, sd).encoder.get_last_selfattention(x).double()
        a64 = G.build_reference_model(mf, patch, sd, torch.float64).encoder.get_last_selfattention(x.double())
        n = a64.shape[-1]
        assert a64.shape == (B, 6, n, n) and a32.shape == a64.shape
        diff = (a32 - a64).abs()
        err = diff[:, :, 0].max().item()
        save = dict(meta=np.array([patch, B, Hh, Ww, wseed, xseed, G.N_THREADS]), style=np.array(style), n_tokens=np.array(n),
                    cls_f32=a32[:, :, 0].float().numpy(), cls_f64=a64[:, :, 0].numpy())
        if rows:
            idx = torch.tensor(rows)
            assert rows[-1] == n - 1
            save.update(rows=np.array(rows), rows_f32=a32[:, :, idx].float().numpy(), rows_f64=a64[:, :, idx].numpy())
            err = max(err, diff[:, :, idx].max().item())
        if full:
            err = max(err, diff[0].max().item())
            for k in range(3):
                fp = os.path.join(G.GOLD, f"attention_{name}_full_h{k}.npz")
                np.savez_compressed(fp, heads=np.array([2 * k, 2 * k + 1]), full_f64=a64[0, 2 * k:2 * k + 2].numpy())
                print(f"  {os.path.basename(fp)}: {os.path.getsize(fp) / 1e6:.2f} MB")
        save["f32_vs_f64_maxabs"] = np.array(err)
        ent = -(a64[:, :, 0] * a64[:, :, 0].clamp_min(1e-300).log()).sum(-1)
        fp = os.path.join(G.GOLD, f"attention_{name}.npz")
        np.savez_compressed(fp, **save)
        print(f"{name}: N={n} max p={a64.max().item():.3f} CLS-row entropy {ent.min().item():.2f}..{ent.max().item():.2f} nats "
              f"(uniform {np.log(n):.2f}) f32-f64={err:.2e} -> {os.path.getsize(fp) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
