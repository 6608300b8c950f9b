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

The batch machinery itself - thread-pool passes, staging buffer, copy, verdict loop, fallback copy-in - is ``device_decode.DeviceDecodeBatch``,
shared with png_decode.py; ``HostBatch`` below holds what is JPEG's own.
"""
import ctypes
from collections import namedtuple
from typing import Optional, Sequence

import torch

from . import _native as N
from .device_decode import MAX_THREADS, DeviceDecodeBatch, Source, _pool, _read, default_threads, packed_layout  # noqa: F401 (re-exported)

DEVICE_ENTROPY_THREADS = 4  # entropy="device": the threads only read files and strip stuffing; more of them cost more than they do
MAX_DEVICE_PIXELS = 1 << 24  # larger frames (by their header) go to Pillow, which has its own decompression-bomb check
PROBE_PREFIX = 1 << 16       # bytes read for a header; the whole file only when the scan header lies further in
JpegHeader = namedtuple("JpegHeader", "height width components sampling supported coef_bytes")
ENTROPIES = ("host", "device")


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


class HostBatch(DeviceDecodeBatch):
    """``DeviceDecodeBatch`` for baseline JPEGs: per image its header (device path) or its Pillow pixels (fallback), and the staging
    buffer [coefficients | quantisation tables | descriptor table], or with ``entropy="device"`` [scan records | quantisation tables |
    descriptor table | scan descriptor table]."""
    NAME, KERNELS, LAUNCH = "decode_jpeg_batch", "IDCT / colour", "sm_jpeg_entropy_decode_batch"
    UNSUPPORTED, ENTRY = N.JPEG_UNSUPPORTED, N.JpegImage

    def __init__(self, sources: Sequence[Source], threads: Optional[int] = None, entropy: str = "host", subseq_bits: int = 0,
                 chunk_subseqs: int = 0):
        """``entropy``: "host" = the threads Huffman-decode; "device" = they only prepare the scans and the GPU decodes them
        (``subseq_bits`` / ``chunk_subseqs``: its parameters, 0 = the defaults; see sm_jpeg_entropy_decode_batch)"""
        if entropy not in ENTROPIES:
            raise ValueError(f"entropy={entropy!r}: one of {ENTROPIES}")
        if entropy == "device" and threads is None:
            threads = min(DEVICE_ENTROPY_THREADS, default_threads())
        self.entropy, self.subseq_bits, self.chunk_subseqs = entropy, int(subseq_bits), int(chunk_subseqs)
        super().__init__(sources, threads)
        if self.scans is not None:
            self.blit(self.scans, self.scan_at)

    def probe(self, data):
        info = _header(data)
        return info if info.supported else None

    def capacity(self, data, info):  # the coefficients (a multiple of 128), or the record the device decodes (a multiple of 16)
        return int(self.lib.sm_jpeg_scan_bound(info, len(data))) if self.entropy == "device" else int(info.coef_bytes)

    def layout(self, infos, rec_bytes):
        B, device_entropy = self.B, self.entropy == "device"
        self._coef_off, o = [], 0  # entropy="host": the records ARE the coefficients, o ends as rec_bytes
        for info in infos:
            self._coef_off.append(o)
            o += int(info.coef_bytes) if info is not None else 0
        self.coef_bytes = o
        self.qt_at = rec_bytes
        self.descr_at = self.qt_at + B * 384
        self.scan_at = self.descr_at + B * ctypes.sizeof(N.JpegImage)
        self.scans, self._scan_of = ((N.JpegScan * B)(), {}) if device_entropy else (None, None)
        return self.scan_at + (B * ctypes.sizeof(N.JpegScan) if device_entropy else 0)

    def prepare(self, b, data, info, base, at, cap):
        out = N.JpegInfo()
        if self.entropy == "device":  # markers and byte stuffing only: the record the device decodes
            scan = N.JpegScan()
            if not self.taken(self.lib.sm_jpeg_scan_prepare(data, len(data), base + at, cap, scan, base + self.qt_at + 384 * b, out), "sm_jpeg_scan_prepare"):
                return None
            scan.rec_off, scan.coef_off = at, self._coef_off[b]
            self._scan_of[b] = scan
        elif not self.taken(self.lib.sm_jpeg_entropy_decode(data, len(data), base + at, cap, base + self.qt_at + 384 * b, out), "sm_jpeg_entropy_decode"):
            return None  # Huffman decode straight into the staging buffer; anything irregular -> Pillow
        return out, (out.height, out.width)

    def fill_table(self, n, b, info):
        if self.scans is not None:
            self.scans[n] = self._scan_of[b]
        e = self.table[n]
        e.coef_off, e.out_off, e.qt_off, e.H, e.W, e.sampling = self._coef_off[b], self.offsets[b], 192 * b, info.height, info.width, info.sampling
        nc = info.components
        for c in range(3):
            e.blocks_w[c], e.blocks_h[c] = (info.blocks_w[c], info.blocks_h[c]) if c < nc else (0, 0)

    def launch(self, p, out, stream):
        lib, n, coef, verdicts = self.lib, self.n_device, p, None
        if self.entropy == "device":
            coef_t = torch.empty(max(self.coef_bytes, 16), dtype=torch.uint8, device=out.device)  # the kernel zeroes what it does not write
            ws_bytes = int(lib.sm_jpeg_entropy_workspace_bytes(ctypes.addressof(self.scans), n, self.subseq_bits, self.chunk_subseqs))
            if ws_bytes == 0:
                raise ValueError("sm_jpeg_entropy_workspace_bytes: " + lib.sm_last_error().decode())
            self.stats = torch.empty(ws_bytes // 4, dtype=torch.int32, device=out.device)  # [rounds, chunks] per image
            status = torch.empty(n, dtype=torch.int32, device=out.device)
            N.check(lib.sm_jpeg_entropy_decode_batch(ctypes.addressof(self.scans), p + self.scan_at, n, p, coef_t.data_ptr(), status.data_ptr(),
                                                     self.stats.data_ptr(), ws_bytes, self.subseq_bits, self.chunk_subseqs,
                                                     stream.cuda_stream), "sm_jpeg_entropy_decode_batch")
            coef = coef_t.data_ptr()
            event = torch.cuda.Event()
            verdicts = self.read_back(status), event.synchronize
            event.record(stream)  # the back half below is queued behind it and runs while the host reads the verdicts
        N.check(lib.sm_jpeg_decode_batch_u8(ctypes.addressof(self.table), p + self.descr_at, n, coef, p + self.qt_at, out.data_ptr(),
                                            stream.cuda_stream), "sm_jpeg_decode_batch_u8")
        return verdicts


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
