"""Synthetic ResNet-50 checkpoints and inputs for the backbone fixtures (tests/golden/resnet50_*.npz), from
``numpy.random.RandomState`` only: the 94 MB of weights are re-generated from the seed by the generator script and by every test,
never committed.

Weight style (keeps every feature map at max |x| of a few units through 16 residual blocks, so that the 1e-4 parity gate means
what it says - scripts/gen_resnet_golden.py asserts 1 <= max |x| <= 8 per map):
  convolutions        N(0, 2 / fan_in)
  BN gain             uniform in [0.5, 1], HALVED for every bn3 and downsample.1 (the two summands of a residual add)
  BN bias, run. mean  0.2 N(0, 1)
  running variance    uniform in [0.5, 1.5]
  num_batches_tracked 0 (int64)
"""
import functools
from collections import OrderedDict

import numpy as np
import torch

# (name, planes, blocks): resnet_models.py:218 ([3, 4, 6, 3] bottlenecks), :122-125
STAGES = (("layer1", 64, 3), ("layer2", 128, 4), ("layer3", 256, 6), ("layer4", 512, 3))

# name -> (dilated, input shape, weight seed, input seed)
CASES = OrderedDict([
    ("d8_17x23_b2", (True, (2, 3, 17, 23), 11, 101)),
    ("d8_40x56", (True, (1, 3, 40, 56), 11, 102)),
    ("d8_64x64", (True, (1, 3, 64, 64), 11, 103)),
    ("s32_64x64", (False, (1, 3, 64, 64), 11, 104)),
])
STORE_EVERY = 8  # layers 1-3 are stored on every 8th channel, layer 4 whole


def state_entries():
    """(name without the ``network.`` prefix, shape, dtype name) of the 318 entries, in state_dict order."""
    out = []

    def conv(name, cout, cin, k):
        out.append((name + ".weight", (cout, cin, k, k), "float32"))

    def bn(name, c):
        for f in ("weight", "bias", "running_mean", "running_var"):
            out.append((f"{name}.{f}", (c,), "float32"))
        out.append((name + ".num_batches_tracked", (), "int64"))

    conv("prefix.conv1", 64, 3, 7)
    bn("prefix.bn1", 64)
    inplanes = 64
    for lname, planes, blocks in STAGES:
        for i in range(blocks):
            p = f"{lname}.{i}"
            conv(p + ".conv1", planes, inplanes, 1)
            bn(p + ".bn1", planes)
            conv(p + ".conv2", planes, planes, 3)
            bn(p + ".bn2", planes)
            conv(p + ".conv3", planes * 4, planes, 1)
            bn(p + ".bn3", planes * 4)
            if i == 0:
                conv(p + ".downsample.0", planes * 4, inplanes, 1)
                bn(p + ".downsample.1", planes * 4)
            inplanes = planes * 4
    return out


@functools.lru_cache(maxsize=2)
def _synthetic(seed: int):
    rng = np.random.RandomState(seed)
    sd = OrderedDict()
    for name, shape, dt in state_entries():
        key = "network." + name
        if name.endswith("num_batches_tracked"):
            v = np.zeros((), np.int64)
        elif len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            v = (rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)).astype(np.float32)
        elif name.endswith(".weight"):
            v = rng.uniform(0.5, 1.0, shape)
            if ".bn3." in name or ".downsample.1." in name:
                v = v * 0.5
            v = v.astype(np.float32)
        elif name.endswith("running_var"):
            v = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        else:  # bias, running_mean
            v = (0.2 * rng.standard_normal(shape)).astype(np.float32)
        sd[key] = torch.from_numpy(v)
    return sd


def synthetic_resnet_state_dict(seed: int, dilated: bool = True):
    """The 318-entry ``ResNet50`` state_dict (keys under ``network.``).  ``dilated`` changes strides and dilations only, never a
    shape, so both variants share the tensors of a seed; the returned dict is a fresh one over shared (read-only) tensors."""
    del dilated
    return OrderedDict(_synthetic(seed))


def synthetic_input(seed: int, shape):
    """A normalised-image-like batch: N(0, 1) fp32."""
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))
