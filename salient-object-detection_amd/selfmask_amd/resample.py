"""Pillow's 8-bit two-pass resampler (libImaging/Resample.c: ImagingResample) on the host, written once: the tap tables the
device kernels apply (``csrc/resample.h``), the integer pass the numpy references are made of, and the packer of the tables'
device layout.  numpy and ``math`` only: ``pipeline`` binds it to BILINEAR (the input resize), ``present`` to LANCZOS (the
response's mask).
"""
import math
from functools import lru_cache
from typing import Tuple

import numpy as np

PRECISION_BITS = 32 - 8 - 2  # Pillow, libImaging/Resample.c


def _bilinear(x: float) -> float:
    """Resample.c: bilinear_filter"""
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def _lanczos(x: float) -> float:
    """Resample.c: lanczos_filter, truncated to -3 <= x < 3"""
    def sinc(v):
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    if -3.0 <= x < 3.0:
        return sinc(x) * sinc(x / 3)
    return 0.0


FILTERS = {"bilinear": (1.0, _bilinear), "lanczos": (3.0, _lanczos)}  # name -> (support, function)


@lru_cache(maxsize=8192)
def pil_coeffs(in_size: int, out_size: int, filter: str) -> Tuple[np.ndarray, np.ndarray, int]:
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for one of FILTERS, box = the whole axis.  Returns (bounds int32
    (out, 2) = first input index / tap count, taps int32 (out, ks), ks); ks = 2 ceil(support) + 1 when up-scaling, 2 ceil(support
    in / out) + 1 when the output is the smaller one.  Plain Python floats are IEEE doubles evaluated in the C code's order, so
    the fixed-point taps are Pillow's bit for bit."""
    support, fn = FILTERS[filter]
    scale = in_size / out_size
    filterscale = scale if scale >= 1.0 else 1.0
    support = support * filterscale
    ks = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    taps = np.zeros((out_size, ks), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            wv = fn((x + xmin - center + 0.5) * ss)
            w.append(wv)
            ww += wv
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            taps[xx, x] = int(-0.5 + k * (1 << PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, taps, ks


def resample_pass(a: np.ndarray, n_out: int, filter: str) -> np.ndarray:
    """One pass of ImagingResample along axis 1 in numpy integers: (rows, n_in) or (rows, n_in, C) uint8 -> the same with n_out in
    place of n_in: accumulate from 2^21, shift, clip.  A pass between equal lengths runs like any other (the caller skips it where
    Pillow does)."""
    bounds, taps, _ = pil_coeffs(a.shape[1], n_out, filter)
    out = np.empty(a.shape[:1] + (n_out,) + a.shape[2:], np.uint8)
    for xx in range(n_out):
        x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        k = taps[xx, :n].astype(np.int64).reshape((1, n) + (1,) * (a.ndim - 2))
        acc = (a[:, x0:x0 + n].astype(np.int64) * k).sum(1) + (1 << (PRECISION_BITS - 1))
        out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


class CoefTable:
    """The tap tables of one batch as the kernels read them: per (n_in, n_out) ``[n_out][2] bounds, then [n_out][ks] taps``, int32,
    laid end to end, each pair once."""

    def __init__(self, filter: str):
        self.filter, self._parts, self._index, self._size = filter, [], {}, 0

    def add(self, n_in: int, n_out: int) -> Tuple[int, int]:
        """-> (offset of the pair's table in int32 elements, its ks)"""
        if (n_in, n_out) not in self._index:
            bounds, taps, ks = pil_coeffs(n_in, n_out, self.filter)
            self._index[(n_in, n_out)] = (self._size, ks)
            self._parts += [bounds.reshape(-1), taps.reshape(-1)]
            self._size += bounds.size + taps.size
        return self._index[(n_in, n_out)]

    def array(self) -> np.ndarray:
        """the concatenation; one zero when nothing was added (a pointer the ABI can take)"""
        return np.concatenate(self._parts) if self._parts else np.zeros(1, np.int32)
