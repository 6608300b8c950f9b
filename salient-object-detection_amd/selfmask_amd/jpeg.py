"""Baseline JPEG files decoded with the back half on the device, bit-identical to Pillow (csrc/jpeg.hip, csrc/jpeg_host.h).

    pixels, shapes, offsets = decode_jpeg_batch(paths_or_bytes, device)

``pixels`` is ONE uint8 device buffer in the layout of ``pipeline.pack_images``: image b's (H, W, 3) RGB bytes at ``offsets[b]``
(= ``pipeline.packed_pixel_offsets(shapes)``), exactly the bytes ``Image.open(f).convert("RGB")`` gives - so
``preprocess_on_device(shapes, S, device, packed=packed_from_device(...))``, the predictor's finish and the bilateral refinement take
it as they take host-decoded pixels.

The host half (markers + Huffman decode into int16 coefficients) is C++ behind ctypes, which releases the GIL for the whole call: it
runs on a pool of at most 16 THREADS, no worker processes.  The coefficients of a batch travel through one page-locked buffer and
one asynchronous copy on the current stream; two launches (dequantise + IDCT, up-sample + colour conversion) write the pixels.
A file the host half does not take - progressive, CMYK, odd sampling, not a JPEG at all, or anything irregular in the stream - is
decoded by Pillow (``sm_decode_worker.decode_item``) on the same thread and copied into its slot: behaviour on every file is
Pillow's, including which damaged files raise.
"""
import ctypes
import io
import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native as N

MAX_THREADS = 16
MAX_DEVICE_PIXELS = 1 << 24  # larger frames (by their header) go to Pillow, which has its own decompression-bomb check
PROBE_PREFIX = 1 << 16       # bytes read for a header; the whole file only when the scan header lies further in
JpegHeader = namedtuple("JpegHeader", "height width components sampling supported coef_bytes")
Source = Union[str, bytes, os.PathLike]

_POOLS = {}


def default_threads() -> int:
    from .decode_pool import default_workers
    return max(1, min(MAX_THREADS, default_workers()))


def _pool(threads: Optional[int]) -> ThreadPoolExecutor:
    n = default_threads() if threads is None else max(1, min(MAX_THREADS, int(threads)))
    p = _POOLS.get(n)
    if p is None:
        p = _POOLS[n] = ThreadPoolExecutor(max_workers=n, thread_name_prefix="sm_jpeg")
    return p


def _read(source: Source) -> bytes:
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    with open(source, "rb") as f:
        return f.read()


def _header(data: bytes) -> N.JpegInfo:
    info = N.JpegInfo()
    N.check(N.load().sm_jpeg_probe(data, len(data), info), "sm_jpeg_probe")
    if info.supported and info.width * info.height > MAX_DEVICE_PIXELS:
        info.supported = 0  # nothing is sized from such a header here
    return info


def probe_jpeg(source: Source) -> JpegHeader:
    """The header alone: sizes, sampling and whether the device path takes the file (``supported``); an unsupported file reports
    what could be read of its frame header (0 x 0 when it is no JPEG).  Of a file on disk only the first 64 KiB are read, the rest
    only if the scan header was not among them."""
    if isinstance(source, (bytes, bytearray, memoryview)):
        info = _header(bytes(source))
    else:
        with open(source, "rb") as f:
            data = f.read(PROBE_PREFIX)
            info = _header(data)
            if not info.supported and len(data) == PROBE_PREFIX:
                info = _header(data + f.read())
    return JpegHeader(info.height, info.width, info.components, info.sampling, bool(info.supported), int(info.coef_bytes))


def packed_layout(shapes) -> Tuple[List[int], int]:
    """-> (byte offset of every image, bytes in all) of the packed pixel buffer: ``pipeline.pack_images``'s layout"""
    from .pipeline import packed_pixel_offsets
    shapes = list(shapes)
    offs = packed_pixel_offsets(shapes)
    total = offs[-1] + ((shapes[-1][0] * shapes[-1][1] * 3 + 15) & ~15) if shapes else 0
    return offs, max(total, 16)


def _pillow(source: Source, data: bytes) -> np.ndarray:
    from .decode_pool import decode_item
    return decode_item(io.BytesIO(data) if isinstance(source, (bytes, bytearray, memoryview)) else os.fspath(source), None)[0]


class HostBatch:
    """The host half of one batch: per image its header (device path) or its Pillow pixels (fallback), and the page-locked staging
    buffer [coefficients | quantisation tables | descriptor table] ready for its one copy."""

    def __init__(self, sources: Sequence[Source], threads: Optional[int] = None):
        from .pipeline import _POOL
        lib = N.load()
        pool = _pool(threads)
        self.B = B = len(sources)
        self.queued = False  # to_device has handed the staging buffer to its copy
        if B == 0:
            raise ValueError("an empty batch")

        def first(src):  # file read + header; a file that is not ours is decoded right here
            data = _read(src)
            info = _header(data)
            return (data, info, None) if info.supported else (None, None, _pillow(src, data))

        items = list(pool.map(first, sources))
        coef_off, o = [], 0
        for data, info, _ in items:
            coef_off.append(o)
            if info is not None:
                o += int(info.coef_bytes)  # a multiple of 128
        self.coef_bytes = o
        qt_at = o
        descr_at = qt_at + B * 384
        self.staging = _POOL.get(descr_at + B * ctypes.sizeof(N.JpegImage), torch.uint8)
        base = self.staging.data_ptr()

        def second(b):  # Huffman decode straight into the staging buffer; anything irregular -> Pillow
            data, info, rgb = items[b]
            if info is None:
                return None, rgb
            out = N.JpegInfo()
            rc = lib.sm_jpeg_entropy_decode(data, len(data), base + coef_off[b], int(info.coef_bytes), base + qt_at + 384 * b, out)
            if rc == N.JPEG_UNSUPPORTED:
                return None, _pillow(sources[b], data)
            N.check(rc, "sm_jpeg_entropy_decode")
            return out, None

        try:
            done = list(pool.map(second, range(B)))
        except BaseException:
            _POOL.release((self.staging,))  # Pillow raised on a damaged file: the batch never reaches a copy
            raise
        self.fallback = {b: rgb for b, (info, rgb) in enumerate(done) if info is None}
        self.shapes = [(int(rgb.shape[0]), int(rgb.shape[1])) if info is None else (int(info.height), int(info.width)) for info, rgb in done]
        self.offsets, self.out_bytes = packed_layout(self.shapes)
        self.flags = ["fallback" if info is None else "device" for info, _ in done]
        table = (N.JpegImage * B)()
        n = 0
        for b, (info, _) in enumerate(done):
            if info is None:
                continue
            e = table[n]
            e.coef_off, e.out_off, e.qt_off, e.H, e.W, e.sampling = coef_off[b], self.offsets[b], 192 * b, info.height, info.width, info.sampling
            nc = info.components
            for c in range(3):
                e.blocks_w[c], e.blocks_h[c] = (info.blocks_w[c], info.blocks_h[c]) if c < nc else (0, 0)
            n += 1
        self.n_device, self.table = n, table
        self.qt_at, self.descr_at = qt_at, descr_at
        if n:
            self.staging.numpy()[descr_at:descr_at + n * ctypes.sizeof(N.JpegImage)] = np.frombuffer(bytes(table), np.uint8)[:n * ctypes.sizeof(N.JpegImage)]

    def discard(self) -> None:
        """a batch that will never reach ``to_device``: hand its page-locked buffer back"""
        from .pipeline import _POOL
        _POOL.release((self.staging,))

    def to_device(self, device) -> torch.Tensor:
        """the device half on the current stream -> the packed uint8 pixel buffer"""
        from .pipeline import _POOL
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"decode_jpeg_batch's IDCT / colour kernels run on a HIP device (got {device}); there is no CPU fallback")
        stream = torch.cuda.current_stream(device)
        out = torch.empty(self.out_bytes, dtype=torch.uint8, device=device)
        used = [self.staging]
        if self.n_device:
            dev = self.staging.to(device, non_blocking=True)  # coefficients, tables and descriptors: one copy
            p = dev.data_ptr()
            N.check(N.load().sm_jpeg_decode_batch_u8(ctypes.addressof(self.table), p + self.descr_at, self.n_device, p, p + self.qt_at,
                                                    out.data_ptr(), stream.cuda_stream), "sm_jpeg_decode_batch_u8")
        for b, rgb in self.fallback.items():
            n = rgb.size
            h = _POOL.get(n, torch.uint8)
            h.numpy()[:] = rgb.reshape(-1)
            out[self.offsets[b]:self.offsets[b] + n].copy_(h, non_blocking=True)
            used.append(h)
        _POOL.release_after(used, stream)
        self.queued = True
        return out


def decode_jpeg_batch(sources: Sequence[Source], device, threads: Optional[int] = None, return_info: bool = False):
    """``sources``: paths or ``bytes`` objects -> (packed uint8 device buffer, [(H, W)], byte offsets[, ["device" | "fallback"]]).
    For ANY input the buffer holds what ``pipeline.pack_images`` would have built from Pillow's pixels; ``threads``: host threads of
    the entropy decode (default: this rank's share of the cores, at most 16)."""
    hb = HostBatch(sources, threads)
    out = hb.to_device(device)
    return (out, hb.shapes, hb.offsets, hb.flags) if return_info else (out, hb.shapes, hb.offsets)


def packed_from_device(pixels: torch.Tensor, shapes, S: Optional[int]):
    """the ``packed=`` argument of ``pipeline.preprocess_on_device`` for pixels that are on the device already"""
    from .pipeline import pack_tables
    coef, descr, out_elems = pack_tables(shapes, S, pinned=True)
    return pixels, coef, descr, max(h for h, _ in shapes), max(h * w for h, w in shapes), out_elems
