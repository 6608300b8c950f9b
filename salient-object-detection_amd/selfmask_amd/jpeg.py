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

``entropy="device"`` (opt-in) moves the Huffman decode itself to the GPU (csrc/jpeg_entropy.hip): the host threads only parse the
markers and strip the byte stuffing (``sm_jpeg_scan_prepare``), the staging buffer carries [scan records | tables | descriptors]
- about the size of the files instead of 128 bytes per block - and one launch writes the coefficients on the device, the same
ones with the same verdict.  What that launch flags (anything irregular INSIDE the entropy-coded data) is known only once the
batch's status words are back: one small copy and a wait on the batch's stream, then Pillow decodes those files into their slots.
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
DEVICE_ENTROPY_THREADS = 4  # entropy="device": the threads only read files and strip stuffing; more of them cost more than they do
MAX_DEVICE_PIXELS = 1 << 24  # larger frames (by their header) go to Pillow, which has its own decompression-bomb check
PROBE_PREFIX = 1 << 16       # bytes read for a header; the whole file only when the scan header lies further in
JpegHeader = namedtuple("JpegHeader", "height width components sampling supported coef_bytes")
Source = Union[str, bytes, os.PathLike]
ENTROPIES = ("host", "device")

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

    def __init__(self, sources: Sequence[Source], threads: Optional[int] = None, entropy: str = "host", subseq_bits: int = 0,
                 chunk_subseqs: int = 0):
        """``entropy``: "host" = the threads Huffman-decode; "device" = they only prepare the scans and the GPU decodes them
        (``subseq_bits`` / ``chunk_subseqs``: its parameters, 0 = the defaults; see sm_jpeg_entropy_decode_batch)"""
        from .pipeline import _POOL
        if entropy not in ENTROPIES:
            raise ValueError(f"entropy={entropy!r}: one of {ENTROPIES}")
        lib = N.load()
        if entropy == "device" and threads is None:
            threads = min(DEVICE_ENTROPY_THREADS, default_threads())
        pool = _pool(threads)
        self.B = B = len(sources)
        self.entropy, self.subseq_bits, self.chunk_subseqs = entropy, int(subseq_bits), int(chunk_subseqs)
        self.queued = False  # to_device has handed the staging buffer to its copy
        if B == 0:
            raise ValueError("an empty batch")
        self._sources = list(sources) if entropy == "device" else None  # files the device flags are Pillow's, after the batch ran

        def first(src):  # file read + header; a file that is not ours is decoded right here
            data = _read(src)
            info = _header(data)
            return (data, info, None) if info.supported else (None, None, _pillow(src, data))

        items = list(pool.map(first, sources))
        device_entropy = entropy == "device"
        coef_off, rec_off, rec_cap, o, r = [], [], [], 0, 0
        for data, info, _ in items:
            coef_off.append(o)
            rec_off.append(r)
            rec_cap.append(0)
            if info is not None:
                o += int(info.coef_bytes)  # a multiple of 128
                if device_entropy:
                    rec_cap[-1] = int(lib.sm_jpeg_scan_bound(info, len(data)))  # a multiple of 16
                    r += rec_cap[-1]
        self.coef_bytes = o
        # entropy="host": [coefficients | tables | descriptors]; "device": [scan records | tables | descriptors | scan descriptors]
        qt_at = r if device_entropy else o
        descr_at = qt_at + B * 384
        scan_at = descr_at + B * ctypes.sizeof(N.JpegImage)
        self.staging = _POOL.get(scan_at + (B * ctypes.sizeof(N.JpegScan) if device_entropy else 0), torch.uint8)
        base = self.staging.data_ptr()

        scan_of = {}  # entropy="device": the descriptor of every prepared scan

        def second(b):  # Huffman decode straight into the staging buffer; anything irregular -> Pillow
            data, info, rgb = items[b]
            if info is None:
                return None, rgb
            out = N.JpegInfo()
            if device_entropy:  # markers and byte stuffing only: the record the device decodes
                scan = N.JpegScan()
                rc = lib.sm_jpeg_scan_prepare(data, len(data), base + rec_off[b], rec_cap[b], scan, base + qt_at + 384 * b, out)
                if rc == N.JPEG_UNSUPPORTED:
                    return None, _pillow(sources[b], data)
                N.check(rc, "sm_jpeg_scan_prepare")
                scan.rec_off, scan.coef_off = rec_off[b], coef_off[b]
                scan_of[b] = scan
                return out, None
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
        scans = (N.JpegScan * B)() if device_entropy else None
        self.device_slots = []  # batch position of every table entry
        n = 0
        for b, (info, _) in enumerate(done):
            if info is None:
                continue
            self.device_slots.append(b)
            if device_entropy:
                scans[n] = scan_of[b]
            e = table[n]
            e.coef_off, e.out_off, e.qt_off, e.H, e.W, e.sampling = coef_off[b], self.offsets[b], 192 * b, info.height, info.width, info.sampling
            nc = info.components
            for c in range(3):
                e.blocks_w[c], e.blocks_h[c] = (info.blocks_w[c], info.blocks_h[c]) if c < nc else (0, 0)
            n += 1
        self.n_device, self.table, self.scans = n, table, scans
        self.qt_at, self.descr_at, self.scan_at = qt_at, descr_at, scan_at
        self.copy_bytes = self.staging.numel()  # what to_device sends in its one copy
        if n:
            self.staging.numpy()[descr_at:descr_at + n * ctypes.sizeof(N.JpegImage)] = np.frombuffer(bytes(table), np.uint8)[:n * ctypes.sizeof(N.JpegImage)]
            if device_entropy:
                self.staging.numpy()[scan_at:scan_at + n * ctypes.sizeof(N.JpegScan)] = np.frombuffer(bytes(scans), np.uint8)[:n * ctypes.sizeof(N.JpegScan)]

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
        status_h = None
        if self.n_device:
            lib = N.load()
            dev = self.staging.to(device, non_blocking=True)  # coefficients (or scan records), tables and descriptors: one copy
            p = dev.data_ptr()
            coef = p
            if self.entropy == "device":
                n = self.n_device
                coef_t = torch.empty(max(self.coef_bytes, 16), dtype=torch.uint8, device=device)  # the kernel zeroes what it does not write
                ws_bytes = int(lib.sm_jpeg_entropy_workspace_bytes(ctypes.addressof(self.scans), n, self.subseq_bits, self.chunk_subseqs))
                if ws_bytes == 0:
                    raise ValueError("sm_jpeg_entropy_workspace_bytes: " + lib.sm_last_error().decode())
                self.stats = torch.empty(ws_bytes // 4, dtype=torch.int32, device=device)  # [rounds, chunks] per image
                status = torch.empty(n, dtype=torch.int32, device=device)
                N.check(lib.sm_jpeg_entropy_decode_batch(ctypes.addressof(self.scans), p + self.scan_at, n, p, coef_t.data_ptr(), status.data_ptr(),
                                                         self.stats.data_ptr(), ws_bytes, self.subseq_bits, self.chunk_subseqs,
                                                         stream.cuda_stream), "sm_jpeg_entropy_decode_batch")
                coef = coef_t.data_ptr()
                status_h = _POOL.get(n, torch.int32)
                status_h.copy_(status, non_blocking=True)
                verdicts = torch.cuda.Event()
                verdicts.record(stream)  # the back half below is queued behind it and runs while the host reads the verdicts
            N.check(lib.sm_jpeg_decode_batch_u8(ctypes.addressof(self.table), p + self.descr_at, self.n_device, coef, p + self.qt_at,
                                                out.data_ptr(), stream.cuda_stream), "sm_jpeg_decode_batch_u8")
        if status_h is not None:
            # what the device flagged is Pillow's: known only now, so the copy of the verdicts is waited for (the back half is queued already)
            verdicts.synchronize()
            codes = status_h.tolist()
            _POOL.release((status_h,))
            try:
                for k, rc in enumerate(codes):
                    if rc == N.JPEG_UNSUPPORTED:
                        b = self.device_slots[k]
                        rgb = _pillow(self._sources[b], _read(self._sources[b]))
                        if (int(rgb.shape[0]), int(rgb.shape[1])) != tuple(self.shapes[b]):
                            raise ValueError(f"decode_jpeg_batch: file {b}: Pillow decodes {rgb.shape[:2]}, its header says {self.shapes[b]}")
                        self.fallback[b] = rgb
                        self.flags[b] = "fallback"
                    elif rc != 0:
                        raise RuntimeError(f"sm_jpeg_entropy_decode_batch: file {self.device_slots[k]}: status {rc} (a record the prepare step did not write)")
            except BaseException:
                _POOL.release_after(used, stream)  # Pillow raised on a damaged file: the copy has been waited for
                self.queued = True
                raise
        for b, rgb in self.fallback.items():
            n = rgb.size
            h = _POOL.get(n, torch.uint8)
            h.numpy()[:] = rgb.reshape(-1)
            out[self.offsets[b]:self.offsets[b] + n].copy_(h, non_blocking=True)
            used.append(h)
        _POOL.release_after(used, stream)
        self.queued = True
        return out


def decode_jpeg_batch(sources: Sequence[Source], device, threads: Optional[int] = None, return_info: bool = False, entropy: str = "host"):
    """``sources``: paths or ``bytes`` objects -> (packed uint8 device buffer, [(H, W)], byte offsets[, ["device" | "fallback"]]).
    For ANY input the buffer holds what ``pipeline.pack_images`` would have built from Pillow's pixels; ``threads``: host threads of
    the entropy decode (default: this rank's share of the cores, at most 16); ``entropy``: "host" = those threads Huffman-decode,
    "device" = they only prepare the scans and the GPU decodes them - the same pixels, and a wait on the current stream inside the
    call (the verdict on every scan comes back before the files it flags go to Pillow)."""
    hb = HostBatch(sources, threads, entropy)
    out = hb.to_device(device)
    return (out, hb.shapes, hb.offsets, hb.flags) if return_info else (out, hb.shapes, hb.offsets)


def packed_from_device(pixels: torch.Tensor, shapes, S: Optional[int]):
    """the ``packed=`` argument of ``pipeline.preprocess_on_device`` for pixels that are on the device already"""
    from .pipeline import pack_tables
    coef, descr, out_elems = pack_tables(shapes, S, pinned=True)
    return pixels, coef, descr, max(h for h, _ in shapes), max(h * w for h, w in shapes), out_elems
