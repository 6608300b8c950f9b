#!/usr/bin/env python3
"""Where one workgroup of png_deflate_kernel spends its time (experiment build: build.py --variant=pngstamps -DSM_PNG_STAMPS; chunk 0 of
image 0 then leaves lane 0's cycle counts between marks in the unused tail of the workspace's plan).  usage: png_stamps.py [H W C]"""
import os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("SM_HIP_LIB", os.path.join(REPO, "salient-object-detection_amd", "lib", "libselfmask_hip_pngstamps.so"))
sys.path[:0] = [os.path.join(REPO, "salient-object-detection_amd"), os.path.join(REPO, "scripts")]
import numpy as np, torch
from selfmask_amd import _native as N
from present_bench import _upload
H, W, C = (int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (300, 400, 3)
a = _upload(H, W)
a = a[..., 0].copy() if C == 1 else a if C == 3 else np.concatenate([a, a[..., :1]], 2)
lib, dev = N.load(), torch.device("cuda:0")
t = (N.PngImage * 1)()
t[0].H, t[0].W, t[0].channels, t[0].filter_mode, t[0].out_cap = H, W, C, -1, lib.sm_png_bound(H, W, C)
pixels = torch.from_numpy(a.reshape(-1)).to(dev)
table = torch.from_numpy(np.frombuffer(bytes(t), np.uint8).copy()).to(dev)
out = torch.empty(t[0].out_cap, dtype=torch.uint8, device=dev)
sizes = torch.zeros(1, dtype=torch.int64, device=dev)
wsb = lib.sm_png_workspace_bytes(t, 1)
ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
for _ in range(3):
    N.check(lib.sm_png_encode_batch_u8(pixels.data_ptr(), t, table.data_ptr(), 1, out.data_ptr(), sizes.data_ptr(), ws.data_ptr(), wsb,
                                       torch.cuda.current_stream().cuda_stream), "sm_png_encode_batch_u8")
torch.cuda.synchronize()
marks = ws[64:64 + 96].cpu().numpy().view(np.uint64).astype(np.float64)
names = ["load", "run scans", "histogram walk + Adler", "literal/length lengths", "costs + code-length histogram", "code-length code",
         "choice + canonical codes", "bit-length walk + prefix sum", "deposit walk", "header bits + arrival", "CRC-32", "stores"]
print(f"png_deflate_kernel, chunk 0 of a {H} x {W} x {C} picture ({int(sizes[0])} bytes of file): counter units of lane 0 between marks")
for n, m in zip(names, marks):
    print(f"  {n:32s} {m:10.0f}  {100 * m / marks.sum():5.1f} %")
