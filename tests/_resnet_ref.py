"""CPU witness of the ResNet-50 backbone: our own restatement of the network the reference builds with
``ResNetBackbone("resnet50_dilated8")`` / ``("resnet50")`` (networks/resnet_backbone.py:42-105, resnet_models.py:57-154) as a layer
table driving ``torch.nn.functional`` - pinned against the real reference by the fixtures of scripts/gen_resnet_golden.py
(tests/test_resnet_cpu.py) - plus numpy forms of the device kernels' index arithmetic (tap gather, stem gather, max-pool).
"""
import numpy as np
import torch
import torch.nn.functional as F

from _resnet_cases import STAGES

BN_EPS = 1e-5


def block_table(dilated: bool):
    """One row per bottleneck: (prefix, inplanes, planes, stride of conv2 and of the down-sample, dilation = pad of conv2,
    has_downsample).  The stride sits on conv2 (resnet_models.py:64).  Dilated (resnet_backbone.py:49-55,72-85, multi_grid None):
    layers 3 / 4 lose their stride; the convolution that had it gets dilation d // 2, every other 3 x 3 of the layer d, with
    d = 2 (layer 3) and 4 (layer 4)."""
    rows = []
    inplanes = 64
    for lname, planes, blocks in STAGES:
        lstride = 1 if lname == "layer1" else 2
        d = {"layer3": 2, "layer4": 4}.get(lname, 1) if dilated else 1
        for i in range(blocks):
            stride = lstride if i == 0 else 1
            dil = 1
            if d > 1:
                dil = d // 2 if stride == 2 else d
                stride = 1
            rows.append((f"{lname}.{i}", inplanes, planes, stride, dil, i == 0))
            inplanes = planes * 4
    return rows


def _bn(x, sd, name):
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"],
                        False, 0.0, BN_EPS)


def prepare(sd, device, dtype, prefix: str = "network."):
    """the floating-point entries without the prefix, on ``device`` in ``dtype``"""
    return {k[len(prefix):]: v.to(device=device, dtype=dtype) for k, v in sd.items() if v.dtype.is_floating_point}


@torch.no_grad()
def forward(sd, x, dilated: bool = True, dtype=torch.float64, prefix: str = "network."):
    """The four feature maps (NCHW) in ``dtype`` on x's device.  ``sd``: the 318-entry state_dict, or (``prefix`` None) what
    ``prepare`` made of it."""
    if prefix is not None:
        sd = prepare(sd, x.device, dtype, prefix)
    x = x.to(dtype)
    x = F.relu(_bn(F.conv2d(x, sd["prefix.conv1.weight"], None, 2, 3), sd, "prefix.bn1"))
    x = F.max_pool2d(x, 3, 2, 1)
    outs = []
    table = block_table(dilated)
    for n, (p, _inpl, _planes, stride, dil, down) in enumerate(table):
        r = x
        o = F.relu(_bn(F.conv2d(x, sd[p + ".conv1.weight"]), sd, p + ".bn1"))
        o = F.relu(_bn(F.conv2d(o, sd[p + ".conv2.weight"], None, stride, dil, dil), sd, p + ".bn2"))
        o = _bn(F.conv2d(o, sd[p + ".conv3.weight"]), sd, p + ".bn3")
        if down:
            r = _bn(F.conv2d(x, sd[p + ".downsample.0.weight"], None, stride), sd, p + ".downsample.1")
        x = F.relu(o + r)
        if n + 1 == len(table) or table[n + 1][0].split(".")[0] != p.split(".")[0]:
            outs.append(x)
    return outs


@torch.no_grad()
def features(sd, x, dilated: bool = True, dtype=torch.float64):
    """What mask_generator.pyc@L150-159 hands the clusterer: zero-pad right / bottom to a multiple of 8, last map, bilinear x 2
    (align_corners=True), channels last -> ((B, 2h * 2w, 2048), (h, w))."""
    H, W = x.shape[-2:]
    x = F.pad(x, (0, (8 - W % 8) % 8, 0, (8 - H % 8) % 8), value=0)
    f = forward(sd, x, dilated, dtype)[-1]
    h, w = f.shape[-2:]
    up = F.interpolate(f, scale_factor=2, mode="bilinear", align_corners=True)
    return up.permute(0, 2, 3, 1).reshape(f.shape[0], 4 * h * w, f.shape[1]), (h, w)


def out_size(n: int, k: int, stride: int, dil: int, pad: int) -> int:
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def gather_taps(x: np.ndarray, k: int, stride: int, dil: int, pad: int) -> np.ndarray:
    """x (B, H, W, C) of any dtype -> (B, oh, ow, k * k * C): the taps (i, j) row-major, each a whole input row; zeros outside."""
    B, H, W, C = x.shape
    oh, ow = out_size(H, k, stride, dil, pad), out_size(W, k, stride, dil, pad)
    out = np.zeros((B, oh, ow, k * k, C), x.dtype)
    for oy in range(oh):
        for ox in range(ow):
            for i in range(k):
                for j in range(k):
                    y, xx = oy * stride - pad + i * dil, ox * stride - pad + j * dil
                    if 0 <= y < H and 0 <= xx < W:
                        out[:, oy, ox, i * k + j] = x[:, y, xx]
    return out.reshape(B, oh, ow, k * k * C)


def gather_stem(x: np.ndarray, kpad: int = 160) -> np.ndarray:
    """x (B, 3, H, W) -> (B, oh, ow, kpad): column c * 49 + i * 7 + j = x[b, c, 2 oy - 3 + i, 2 ox - 3 + j] (the (Cout, Cin, kh, kw)
    weight flattened as it lies), zeros outside the image and in columns 147...kpad."""
    B, C, H, W = x.shape
    oh, ow = out_size(H, 7, 2, 1, 3), out_size(W, 7, 2, 1, 3)
    xp = np.zeros((B, C, H + 6, W + 6), x.dtype)
    xp[:, :, 3:3 + H, 3:3 + W] = x
    out = np.zeros((B, oh, ow, kpad), x.dtype)
    for c in range(C):
        for i in range(7):
            for j in range(7):
                out[..., c * 49 + i * 7 + j] = xp[:, c, i:i + 2 * oh:2, j:j + 2 * ow:2]
    return out


def maxpool3x3s2(x: np.ndarray) -> np.ndarray:
    """x (B, H, W, C) -> (B, oh, ow, C); padding never wins (it is -inf, as in F.max_pool2d)."""
    B, H, W, C = x.shape
    oh, ow = out_size(H, 3, 2, 1, 1), out_size(W, 3, 2, 1, 1)
    xp = np.full((B, H + 2, W + 2, C), -np.inf, x.dtype)
    xp[:, 1:1 + H, 1:1 + W] = x
    out = np.full((B, oh, ow, C), -np.inf, x.dtype)
    for i in range(3):
        for j in range(3):
            out = np.maximum(out, xp[:, i:i + 2 * oh:2, j:j + 2 * ow:2])
    return out
