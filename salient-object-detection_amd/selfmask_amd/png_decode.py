"""PNG files decoded on the device, bit-identical to Pillow (csrc/png_decode.hip, csrc/png_host.h, csrc/png_inflate.h).

    pixels, shapes, offsets = decode_png_batch(paths_or_bytes, device, mode="rgb" | "l" | "gt")

``pixels`` is ONE uint8 device buffer.  ``mode="rgb"``: the layout of ``pipeline.pack_images`` - image b's (H, W, 3) bytes at
``offsets[b]`` (= ``pipeline.packed_pixel_offsets(shapes)``), exactly the bytes of ``Image.open(f).convert("RGB")`` (grey
replicated, alpha dropped).  ``mode="l"``: one byte per pixel as ``.convert("L")``.  ``mode="gt"``: the evaluator's ground truth,
``sm_decode_worker.decode_item``'s rule on top of "l" (an image whose maximum exceeds 1 becomes ``pixel > 0``); ``ops.GtBatch.from_device``
takes that buffer as it is.

The host half only walks the chunks (CRC-32 of each), strips the zlib wrapper and concatenates the IDAT payloads - C++ behind ctypes,
which releases the GIL, on a pool of at most 16 THREADS, no worker processes; it decodes nothing.  The records of a batch travel
through one page-locked buffer and one asynchronous copy; two launches (inflate, unfilter + conversion; one workgroup per image) write
the pixels.  A file the host half does not take - palette, 1 / 2 / 4 / 16-bit, interlaced, tRNS, APNG, a bad CRC, not a PNG at all - is
decoded by Pillow on the same thread.  What the device flags (anything irregular INSIDE the data stream: a code that is not
complete, a distance before the start, a wrong Adler-32, a filter id above 4, ...) is known only once the batch's status words are
back: one small copy and a wait on the batch's stream, then Pillow decodes those files into their slots.  So the pixels of every file
are Pillow's, and a file the device path refuses or flags raises exactly where Pillow raises on it.  One difference remains: the chunk
walk checks an ancillary chunk's CRC and does not look inside it, so a file whose only defect is a malformed ancillary chunk (a pHYs of
the wrong length, say) is decoded here where ``Image.open`` may raise.  Files above ``MAX_DEVICE_FILE_BYTES`` or ``MAX_DEVICE_PIXELS``
go to Pillow as well: the device's time per file grows with the length of its data stream.

Where it pays and where it does not (scripts/png_decode_bench.py, profiles/png_decode_bench.log): one lane walks the symbols of an
image, so the cost follows the number of deflate symbols.  A ground-truth mask is a few thousand of them; a photo stored as PNG has
a few hundred thousand, and there the single-lane walk loses to 16 host threads running Pillow.  The path is opt-in everywhere.

The batch machinery itself - thread-pool passes, staging buffer, copy, verdict loop, fallback copy-in - is ``device_decode.DeviceDecodeBatch``,
shared with jpeg.py (one thread pool for both decoders); ``PngHostBatch`` below holds what is PNG's own.
"""
import ctypes
from collections import namedtuple
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native as N
from .device_decode import DeviceDecodeBatch, Source, _openable, _pool, _read, packed_layout, plane_layout  # noqa: F401 (re-exported)

PngHeader = namedtuple("PngHeader", "height width colour_type bit_depth supported inflated_bytes")
MODES = ("rgb", "l", "gt")
PROBE_PREFIX = 64  # signature + IHDR are the first 33 bytes
# One lane walks a file's whole deflate stream (about 2 us per byte of file on the measured photos: about 450 ms for 225 KiB), so what the
# device takes is capped: a larger file, or one of more pixels, is Pillow's - a launch stays well under two seconds whatever is handed in
MAX_DEVICE_FILE_BYTES = 1 << 19
MAX_DEVICE_PIXELS = 1 << 22


def probe_png(source: Source) -> PngHeader:
    """The header alone: sizes, colour type, bit depth and whether the device path takes such a file (``supported``; the chunks behind
    IHDR may still send it to Pillow).  0 x 0 when it is no PNG."""
    if isinstance(source, (bytes, bytearray, memoryview)):
        data = bytes(source[:PROBE_PREFIX])
    else:
        with open(source, "rb") as f:
            data = f.read(PROBE_PREFIX)
    info = N.PngInfo()
    N.check(N.load().sm_png_probe(data, len(data), info), "sm_png_probe")
    return PngHeader(info.height, info.width, info.colour_type, info.bit_depth, bool(info.supported), int(info.inflated_bytes))


class PngHostBatch(DeviceDecodeBatch):
    """``DeviceDecodeBatch`` for PNG files: per image its record (device path) or its Pillow pixels (fallback), and the staging buffer
    [records | descriptor table].  ``to_device`` waits on the stream for the verdicts."""
    NAME, KERNELS, LAUNCH = "decode_png_batch", "inflate / unfilter", "sm_png_decode_batch_u8"
    UNSUPPORTED, ENTRY = N.PNG_UNSUPPORTED, N.PngStream
    ZEROED = True

    def __init__(self, sources: Sequence[Source], threads: Optional[int] = None, mode: str = "rgb"):
        if mode not in MODES:
            raise ValueError(f"mode={mode!r}: one of {MODES}")
        self.mode = mode
        super().__init__(sources, threads)

    def probe(self, data):
        info = N.PngInfo()
        N.check(self.lib.sm_png_probe(data, len(data), info), "sm_png_probe")
        ours = info.supported and len(data) <= MAX_DEVICE_FILE_BYTES and info.height * info.width <= MAX_DEVICE_PIXELS
        return info if ours else None

    def pillow(self, source, data):
        if self.mode == "rgb":
            return super().pillow(source, data)
        from PIL import Image
        m = np.asarray(Image.open(_openable(source, data)).convert("L"))
        if self.mode == "gt" and m.max() > 1:  # decode_item's ground-truth half
            m = m > 0
        return np.ascontiguousarray(m.astype(np.uint8))

    def capacity(self, data, info):
        return int(self.lib.sm_png_stream_bound(info, len(data)))  # a multiple of 16

    def layout(self, infos, rec_bytes):
        self.descr_at, self.ws_bytes = rec_bytes, 0
        return rec_bytes + self.B * ctypes.sizeof(N.PngStream)

    def prepare(self, b, data, info, base, at, cap):  # chunk walk + concatenation straight into the staging buffer
        st, out = N.PngStream(), N.PngInfo()
        if not self.taken(self.lib.sm_png_stream_prepare(data, len(data), base + at, cap, st, out), "sm_png_stream_prepare"):
            return None
        return st, (st.H, st.W)

    def out_layout(self, shapes):
        return packed_layout(shapes) if self.mode == "rgb" else plane_layout(shapes)

    def fill_table(self, n, b, st):
        st.rec_off, st.ws_off, st.out_off = self._rec_off[b], self.ws_bytes, self.offsets[b]
        self.ws_bytes += (int(st.inflated_bytes) + 15) & ~15
        self.table[n] = st

    def launch(self, p, out, stream):
        lib, n = self.lib, self.n_device
        ws_bytes = int(lib.sm_png_decode_workspace_bytes(ctypes.addressof(self.table), n))
        if ws_bytes == 0:
            raise ValueError("sm_png_decode_workspace_bytes: " + lib.sm_last_error().decode())
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=out.device)
        status = torch.empty(n, dtype=torch.int32, device=out.device)
        N.check(lib.sm_png_decode_batch_u8(ctypes.addressof(self.table), p + self.descr_at, n, p, ws.data_ptr(), ws_bytes, out.data_ptr(),
                                           status.data_ptr(), MODES.index(self.mode), stream.cuda_stream), "sm_png_decode_batch_u8")
        return self.read_back(status), stream.synchronize


def decode_png_batch(sources: Sequence[Source], device, mode: str = "rgb", threads: Optional[int] = None, return_info: bool = False):
    """``sources``: paths or ``bytes`` objects -> (uint8 device buffer, [(H, W)], byte offsets[, ["device" | "fallback"]]).  For ANY file
    Pillow opens (a JPEG is simply a fallback) the buffer holds Pillow's pixels: ``mode="rgb"`` what ``pipeline.pack_images`` would have
    built, "l" / "gt" one byte per pixel with every image at a multiple of 16; ``threads``: host threads of the file reads and the chunk
    walk (default: this rank's share of the cores, at most 16).  The call waits on the current stream once (the device's verdicts)."""
    hb = PngHostBatch(sources, threads, mode)
    out = hb.to_device(device)
    return (out, hb.shapes, hb.offsets, hb.flags) if return_info else (out, hb.shapes, hb.offsets)
