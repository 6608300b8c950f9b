"""The host half that the device decoders share (jpeg.py, png_decode.py): ``DeviceDecodeBatch`` is one batch on its way to the device.

A first pass on the thread pool reads and probes every file (one the device path does not take is decoded by Pillow on the spot), the
records' offsets are summed up, ONE page-locked staging buffer comes from ``pipeline._POOL``, and a second pass prepares every record
straight into it (a file the prepare step refuses is Pillow's too); the descriptor table is blitted behind the records.  ``to_device``
sends the buffer in one copy, lets the decoder launch, reads the status words back, hands what the device flagged to Pillow and copies
every fallback image into its slot.  A decoder supplies what differs: probe, fallback, capacities and layout, prepare, table entry,
launch and how it waits for the verdicts.
"""
import ctypes
import io
import os
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native as N

MAX_THREADS = 16
Source = Union[str, bytes, os.PathLike]

_POOLS = {}


def default_threads() -> int:
    from .decode_pool import default_workers
    return max(1, min(MAX_THREADS, default_workers()))


def _pool(threads: Optional[int]) -> ThreadPoolExecutor:
    """one thread pool per size, for every decoder"""
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


def _openable(source: Source, data: bytes):
    """what Pillow opens: the bytes that were handed in, else the path"""
    return io.BytesIO(data) if isinstance(source, (bytes, bytearray, memoryview)) else os.fspath(source)


def packed_layout(shapes) -> Tuple[List[int], int]:
    """-> (byte offset of every image, bytes in all) of the packed pixel buffer: ``pipeline.pack_images``'s layout"""
    from .pipeline import packed_pixel_offsets
    shapes = list(shapes)
    offs = packed_pixel_offsets(shapes)
    total = offs[-1] + ((shapes[-1][0] * shapes[-1][1] * 3 + 15) & ~15) if shapes else 0
    return offs, max(total, 16)


def plane_layout(shapes) -> Tuple[List[int], int]:
    """-> (byte offset of every image, bytes in all) of a one-byte-per-pixel buffer: planes end to end, each at a multiple of 16"""
    offs, o = [], 0
    for h, w in shapes:
        offs.append(o)
        o += (h * w + 15) & ~15
    return offs, max(o, 16)


class DeviceDecodeBatch:
    """The host half of one batch: per image its prepared record (device path) or its Pillow pixels (fallback), and the page-locked
    staging buffer [records | ... | descriptor table] ready for its one copy.  A decoder sets the names below and supplies
      probe(data) -> the file's header if the device path takes it, else None
      capacity(data, info) -> staging bytes of the file's record
      layout(infos, rec_bytes) -> bytes of the staging buffer; places what follows the records (``self.descr_at`` at least)
      prepare(b, data, info, base, at, cap): writes file b's record to staging[at:at + cap], which lies at address base + at
        -> (item, (H, W)), or None: the file is Pillow's
      fill_table(n, b, item): table entry n is file b
      launch(p, out, stream): the launches on the staged buffer at device address p -> None, or (``read_back(status)``, wait): the
        verdicts' host buffer and the call that waits for its copy - an event's or the stream's, each decoder's own"""
    NAME = KERNELS = LAUNCH = ""  # the entry point, its kernels and the launch that writes the status words: for the messages
    UNSUPPORTED = None            # the status that sends a file to Pillow
    ENTRY = None                  # ctypes type of a descriptor table entry
    ZEROED = False                # the output buffer starts as zeros (its padding is part of what is returned), not uninitialised
    out_layout = staticmethod(packed_layout)

    def pillow(self, source: Source, data: bytes) -> np.ndarray:
        from .decode_pool import decode_item
        return decode_item(_openable(source, data), None)[0]

    def __init__(self, sources: Sequence[Source], threads: Optional[int] = None):
        from .pipeline import _POOL
        self.lib = N.load()
        pool = _pool(threads)
        self.B = B = len(sources)
        self.queued = False  # to_device has handed the staging buffer to its copy
        if B == 0:
            raise ValueError("an empty batch")
        self._sources = list(sources)  # files the device flags are Pillow's, after the batch ran

        def first(src):  # file read + header; a file that is not ours is decoded right here
            data = _read(src)
            info = self.probe(data)
            return (data, info, None) if info is not None else (None, None, self.pillow(src, data))

        items = list(pool.map(first, sources))
        self._rec_off, rec_cap, r = [], [], 0
        for data, info, _ in items:
            self._rec_off.append(r)
            rec_cap.append(self.capacity(data, info) if info is not None else 0)
            r += rec_cap[-1]
        self.staging = _POOL.get(self.layout([info for _, info, _ in items], r), torch.uint8)
        base = self.staging.data_ptr()

        def second(b):  # the record straight into the staging buffer; anything irregular -> Pillow
            data, info, px = items[b]
            if info is not None:
                done = self.prepare(b, data, info, base, self._rec_off[b], rec_cap[b])
                if done is not None:
                    return done
                px = self.pillow(sources[b], data)
            return None, px

        try:
            done = list(pool.map(second, range(B)))
        except BaseException:
            _POOL.release((self.staging,))  # Pillow raised on a damaged file: the batch never reaches a copy
            raise
        self.fallback = {b: px for b, (item, px) in enumerate(done) if item is None}
        self.shapes = [(int(x.shape[0]), int(x.shape[1])) if item is None else (int(x[0]), int(x[1])) for item, x in done]  # pixels | (H, W)
        self.offsets, self.out_bytes = self.out_layout(self.shapes)
        self.flags = ["fallback" if item is None else "device" for item, _ in done]
        self.table = (self.ENTRY * B)()
        self.device_slots = []  # batch position of every table entry
        for b, (item, _) in enumerate(done):
            if item is not None:
                self.fill_table(len(self.device_slots), b, item)
                self.device_slots.append(b)
        self.n_device = len(self.device_slots)
        self.copy_bytes = self.staging.numel()  # what to_device sends in its one copy
        self.blit(self.table, self.descr_at)

    def taken(self, rc: int, what: str) -> bool:
        """a prepare call's status: False = the file is Pillow's; any other failure raises"""
        if rc == self.UNSUPPORTED:
            return False
        N.check(rc, what)
        return True

    def blit(self, table, at: int) -> None:
        """the first n_device entries of a descriptor table into the staging buffer"""
        n = self.n_device * ctypes.sizeof(table._type_)
        if n:
            self.staging.numpy()[at:at + n] = np.frombuffer(bytes(table), np.uint8)[:n]

    def read_back(self, status: torch.Tensor) -> torch.Tensor:
        """the device's status words on their way into a pooled page-locked buffer"""
        from .pipeline import _POOL
        status_h = _POOL.get(status.numel(), torch.int32)
        status_h.copy_(status, non_blocking=True)
        return status_h

    def discard(self) -> None:
        """a batch that will never reach ``to_device``: hand its page-locked buffer back"""
        from .pipeline import _POOL
        _POOL.release((self.staging,))

    def to_device(self, device) -> torch.Tensor:
        """the device half on the current stream -> the uint8 pixel buffer: one copy, the decoder's launches, the status read-back and
        its wait, Pillow for what the device flagged"""
        from .pipeline import _POOL
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"{self.NAME}'s {self.KERNELS} kernels run on a HIP device (got {device}); there is no CPU fallback")
        stream = torch.cuda.current_stream(device)
        out = (torch.zeros if self.ZEROED else torch.empty)(self.out_bytes, dtype=torch.uint8, device=device)
        used = [self.staging]
        verdicts = None
        if self.n_device:
            dev = self.staging.to(device, non_blocking=True)  # records, tables and descriptors: one copy
            verdicts = self.launch(dev.data_ptr(), out, stream)
        if verdicts is not None:
            status_h, wait = verdicts
            wait()  # what the device flagged is Pillow's: known only now
            codes = status_h.tolist()
            _POOL.release((status_h,))
            try:
                for k, rc in enumerate(codes):
                    if rc == self.UNSUPPORTED:
                        b = self.device_slots[k]
                        px = self.pillow(self._sources[b], _read(self._sources[b]))
                        if (int(px.shape[0]), int(px.shape[1])) != tuple(self.shapes[b]):
                            raise ValueError(f"{self.NAME}: file {b}: Pillow decodes {px.shape[:2]}, its header says {self.shapes[b]}")
                        self.fallback[b] = px
                        self.flags[b] = "fallback"
                    elif rc != 0:
                        raise RuntimeError(f"{self.LAUNCH}: file {self.device_slots[k]}: status {rc} (a record the prepare step did not write)")
            except BaseException:
                _POOL.release_after(used, stream)  # Pillow raised on a damaged file: the copy has been waited for
                self.queued = True
                raise
        for b, px in self.fallback.items():
            n = px.size
            h = _POOL.get(n, torch.uint8)
            h.numpy()[:] = px.reshape(-1)
            out[self.offsets[b]:self.offsets[b] + n].copy_(h, non_blocking=True)
            used.append(h)
        _POOL.release_after(used, stream)
        self.queued = True
        return out
