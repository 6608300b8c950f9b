"""Bulk prediction for images WITHOUT ground truth: a list of image files in, the model's saliency mask per file out, at the
file's own size and at device throughput.

    SaliencyPredictor(network)(p_images, output="rle")  -> {file name: COCO uncompressed RLE dict}
    SaliencyPredictor(network)(p_images, output="objects", objects={"min_area": 64})  -> {file name: the mask's objects}

The sibling of ``Evaluator.__call__`` (which needs a ground truth per image and returns metrics, not masks) and of
``MaskGenerator.__call__`` (pseudo-masks from clustering, not from the decoder): headers probed and checked before anything is
queued, token-grid buckets at native resolution (``pipeline.native_buckets``) or S x S batches, decode workers and device
preprocessing, the graphed forward, one batch per stream of a ``StreamRing`` and - new - a fused finish (``ops.predict_masks``,
csrc/predict.hip) that goes from the last decoder layer's query masks straight to run boundaries (or packed planes), read back
``streams`` batches later through page-locked buffers.  The mask of a file is the one the evaluator would score: the arg-max
objectness query, up-sampled by ``patch // scale_factor`` and cropped (native) or resized to the file's size (``img_size``),
thresholded at ``evaluator.MASK_THRESHOLD``.
"""
import argparse
import os
from collections import deque
from typing import Dict, Optional, Sequence

import numpy as np
import torch

OUTPUTS = ("rle", "binary", "soft", "soft_png", "objects")
PNG_ENCODERS = ("host", "device")
DEFAULT_CAP = 8192       # run boundaries stored per image before the retry, as voting.rle_runs_async
MAX_PIXELS = 1 << 22     # sm_predict_masks_f32's largest image
MAX_OBJECTS_WIDTH = 16384  # sm_mask_objects' widest image
DECODES = ("host", "device")
ENTROPIES = ("host", "device")  # who Huffman-decodes the scans of decode="device" (selfmask_amd/jpeg.py)


class _Files:
    """what PrefetchingLoader needs of a dataset: image paths, no ground truth"""

    def __init__(self, p_imgs):
        self.p_imgs, self.p_gts = list(p_imgs), [None] * len(p_imgs)


def _probe(p):
    """(H, W) from the library's own header parser where the device decode takes the file, from Pillow's otherwise"""
    from .datasets import probe_size
    from .jpeg import probe_jpeg
    h = probe_jpeg(p)
    return (h.height, h.width) if h.supported else probe_size(p)


class _DeviceDecoded:
    """``decode="device"``: the loader of the loop - ((host half of ``jpeg.decode_jpeg_batch``, shapes), None, positions) per batch.
    One feeder thread runs the host halves (file reads + entropy decode on the thread pool) ``depth`` batches ahead; the consumer
    queues the device half on its batch's stream (``HostBatch.to_device``)."""

    def __init__(self, p_images, batches, threads, depth, entropy="host"):
        self.p_images, self.batches, self.threads, self.depth, self.entropy = p_images, batches, threads, max(1, depth), entropy

    def __iter__(self):
        from concurrent.futures import ThreadPoolExecutor
        from .jpeg import HostBatch
        with ThreadPoolExecutor(max_workers=1, thread_name_prefix="sm_jpeg_feed") as feeder:
            def submit(k):
                return feeder.submit(HostBatch, [self.p_images[i] for i in self.batches[k]], self.threads, self.entropy)
            inflight = deque(submit(k) for k in range(min(self.depth, len(self.batches))))
            hb = None
            try:
                for k in range(len(self.batches)):
                    hb = inflight.popleft().result()
                    if k + self.depth < len(self.batches):
                        inflight.append(submit(k + self.depth))
                    yield (hb, hb.shapes), None, self.batches[k]
                    hb = None  # the consumer came back for more: it has queued this batch's copy
            finally:  # the loop ended early: batches prepared ahead (and one the consumer may not have queued) go back to the pool
                for fut in inflight:
                    fut.cancel()
                for left in [hb] + [f.result() for f in inflight if not f.cancelled() and f.exception() is None]:
                    if left is not None and not left.queued:
                        left.discard()


class SaliencyPredictor:
    def __init__(self, network, device: torch.device = torch.device("cuda:0"), batch_size: int = 64, streams: int = 3,
                 workers: Optional[int] = None, hip_graph: bool = True, cap: int = DEFAULT_CAP, decode: str = "host", png_encoder: str = "host",
                 entropy: str = "host"):
        """``network``: a ``selfmask_amd.MaskFormer`` with ``use_binary_classifier=True`` on ``device``; ``batch_size``: the most
        images per forward (of ONE token grid at native resolution); ``streams``: batches in flight; ``workers``: decode processes
        (default: this rank's share of the host cores); ``hip_graph``: replay recurring batch shapes as captured graphs;
        ``decode``: "host" = Pillow in the decode worker processes; "device" = ``selfmask_amd.jpeg.decode_jpeg_batch`` - baseline
        JPEGs entropy-decoded on at most 16 host THREADS (``workers`` caps them) and finished on the device, every other file by
        Pillow on those threads: the same pixels, so the same results, without worker processes; ``png_encoder``: who writes the
        soft maps' PNG files (output ``"soft_png"``, ``--png_dir``): "host" = Pillow from the soft maps copied to the host; "device" =
        csrc/png.hip on the packed planes, only the files cross - other bytes, the same pixels for whoever reads them; ``entropy``
        (with ``decode="device"`` only): "host" = those threads Huffman-decode; "device" = they only strip markers and byte stuffing
        and the GPU decodes the scans (csrc/jpeg_entropy.hip) - the same pixels, at the price of one wait per batch for its verdicts."""
        if decode not in DECODES:
            raise ValueError(f"decode={decode!r}: one of {DECODES}")
        if entropy not in ENTROPIES:
            raise ValueError(f"entropy={entropy!r}: one of {ENTROPIES}")
        if entropy == "device" and decode != "device":
            raise ValueError(f"entropy={entropy!r} needs decode='device' (got decode={decode!r}): the device decodes the scans of the "
                             f"files it also finishes")
        if png_encoder not in PNG_ENCODERS:
            raise ValueError(f"png_encoder={png_encoder!r}: one of {PNG_ENCODERS}")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"SaliencyPredictor runs on a HIP device (got {device}); there is no CPU fallback")
        if network is None:
            raise ValueError("SaliencyPredictor needs `network` (a selfmask_amd.MaskFormer holding the SelfMask weights)")
        if not getattr(network, "use_binary_classifier", False):
            raise RuntimeError("the predictor picks the arg-max objectness query: use_binary_classifier=True is required")
        params = getattr(network, "parameters", None)
        p = next(iter(params()), None) if callable(params) else None
        if p is not None and p.device.type != "cuda":
            raise RuntimeError(f"SaliencyPredictor needs `network` on a HIP device (its weights are on {p.device}); there is no CPU "
                               f"fallback - call network.to(device)")
        self.network, self.device, self.batch_size = network, device, max(1, int(batch_size))
        self.streams, self.workers, self.hip_graph, self.cap = max(1, int(streams)), workers, bool(hip_graph), int(cap)
        self.decode, self.png_encoder, self.entropy = decode, png_encoder, entropy
        self.last_best: Dict[str, int] = {}
        self._ring = None

    # ---- planning: everything that can be refused is refused here, before a byte is queued ------------------------------------
    def _plan(self, p_images: Sequence[str], img_size: Optional[int], outputs, refine):
        from .datasets import probe_size
        for o in outputs:
            if o not in OUTPUTS:
                raise ValueError(f"output={o!r}: one of {OUTPUTS}")
        if refine not in (None, "bilateral"):
            raise ValueError(f"refine={refine!r}: None or 'bilateral'")
        if refine and ("soft" in outputs or "soft_png" in outputs):
            raise ValueError("output='soft' with refine='bilateral': the solver's soft output is not a [0, 1] sigmoid map; ask for "
                             "'rle' or 'binary'")
        if img_size is not None and int(img_size) < 1:
            raise ValueError(f"img_size={img_size}")
        p_images = [str(p) for p in p_images]
        names = [p.split("/")[-1] for p in p_images]
        seen = {}
        for p, n in zip(p_images, names):
            if n in seen:
                raise ValueError(f"SaliencyPredictor: {p} and {seen[n]} share the file name {n!r}, which keys the result; nothing was run")
            seen[n] = p
        sizes = []
        for p in p_images:
            if not os.path.isfile(p):
                raise FileNotFoundError(f"SaliencyPredictor: {p} does not exist; nothing was run")
            try:
                hw = _probe(p) if self.decode == "device" else probe_size(p)
            except Exception as e:
                raise ValueError(f"SaliencyPredictor: {p} is not a readable image ({type(e).__name__}: {e}); nothing was run") from e
            if hw[0] < 1 or hw[1] < 1 or hw[0] * hw[1] > MAX_PIXELS:
                raise ValueError(f"SaliencyPredictor: {p} is {hw[0]} x {hw[1]}: 1 .. {MAX_PIXELS} pixels per image; nothing was run")
            if "objects" in outputs and hw[1] > MAX_OBJECTS_WIDTH:
                raise ValueError(f"SaliencyPredictor: {p} is {hw[1]} pixels wide: objects are found in images of at most "
                                 f"{MAX_OBJECTS_WIDTH} columns; nothing was run")
            sizes.append((int(hw[0]), int(hw[1])))
        return self._batches(p_images, names, sizes, img_size)

    def _batches(self, p_images, names, sizes, img_size):
        """-> the plan (paths, names, sizes, batches of positions): token-grid buckets at native resolution, plain slices otherwise"""
        from .pipeline import native_buckets
        if img_size is None:
            batches = native_buckets(sizes, self.network.encoder.patch_size, self.batch_size)
        else:
            batches = [list(range(s, min(s + self.batch_size, len(sizes)))) for s in range(0, len(sizes), self.batch_size)]
        return p_images, names, sizes, batches

    @torch.no_grad()
    def __call__(self, p_images: Sequence[str], img_size: Optional[int] = None, scale_factor: int = 2, output: str = "rle",
                 refine: Optional[str] = None, comm=None, objects=None) -> Dict[str, object]:
        """-> {file name: COCO uncompressed RLE dict (``output="rle"``) | (H, W) uint8 array: 0/1 (``"binary"``) or
        clip(p, 0, 1) * 255 truncated (``"soft"``) | that soft map as an 8-bit grey PNG file, bytes, encoded on the device
        (``"soft_png"``) | the mask's connected components (``"objects"``: the dict of
        ``ops.predict_masks(objects=)`` + "best"; ``objects``: an ``ops.ObjectOptions`` or a dict of its keys)}, in list order;
        ``.last_best`` {file name: query index}.
        ``img_size=None``: native resolution in token-grid buckets, the mask up-sampled by ``patch // scale_factor`` and cropped -
        the evaluator's reference mode; ``img_size=S``: inputs resized to S x S, the mask resized to the file's own size.
        ``refine="bilateral"``: the mask the metrics would score goes through the bilateral solver against the decoded pixels (native:
        one mixed-size solve per bucket; ``img_size``: the S x S solve of the evaluator, its binary mask then resized to the file's
        size like any mask) and the solver's binary result is returned.  ``comm``: this rank takes files rank, rank + W, ... of the
        list and every rank returns the codes of ALL files (RLE only)."""
        sharded = comm is not None and comm.world_size > 1
        assert not sharded or output == "rle", "the gather exchanges run-length codes"
        plan = self._plan(p_images, img_size, (output,), refine)
        if sharded:
            from .distributed import gather_dicts, shard_indices
            paths, names = plan[0], plan[1]
            idx = shard_indices(len(paths), comm.rank, comm.world_size)  # this rank's files, with the sizes already probed
            mine = self._run([paths[i] for i in idx], img_size, scale_factor, ("rle",), refine,
                             plan=self._batches([paths[i] for i in idx], [names[i] for i in idx], [plan[2][i] for i in idx], img_size))
            best = gather_dicts(self.last_best, comm, self.device)
            merged = gather_dicts(mine["rle"], comm, self.device)
            self.last_best = {n: best[n] for n in names}
            return {n: merged[n] for n in names}  # the list's order, whatever the sharding
        if output == "objects":
            return self._run(plan[0], img_size, scale_factor, (output,), refine, plan=plan, objects=objects)[output]
        return self._run(plan[0], img_size, scale_factor, (output,), refine, plan=plan)[output]

    # ---- one rank's files -----------------------------------------------------------------------------------------------------
    def _finish(self, out, shapes, u8, scale, img_size, outputs, refine, objects=None):
        """the forward's outputs of one batch -> a pending result (``.result()`` -> {"best", "rle" / "binary" / "soft"})"""
        from . import ops
        mask_pred, obj = out["mask_pred"], out["objectness"]
        if mask_pred.dim() == 5:  # last decoder layer
            mask_pred, obj = mask_pred[:, -1], obj[:, -1]
        obj = obj.squeeze(-1)
        want = dict(rle="rle" in outputs, binary="binary" in outputs, soft="soft" in outputs, cap=self.cap, objects=objects,
                    soft_png="soft_png" in outputs)
        if not refine:
            return ops.predict_masks(mask_pred, obj, ops.PackedImages(shapes, self.device), scale, **want)
        B = mask_pred.shape[0]
        if img_size is None:
            from .bilateral_solver import MixedBatch, bilateral_solver_mixed_packed
            from .pipeline import packed_pixel_offsets
            mb = MixedBatch(shapes, self.device, packed_pixel_offsets(shapes))
            head = ops.predict_masks(mask_pred, obj, mb, scale, rle=False)  # the arg-max alone
            rows = torch.zeros((B, 16), dtype=torch.float32, device=self.device)
            rows[:, 14] = head.best.float()
            target = ops.upsample_selected_native(mask_pred, rows, mb, scale, "pick")
            _, binary, _ = bilateral_solver_mixed_packed(u8, target, mb)
            return _Refined(head, ops.rle_runs_packed_async(binary, mb, self.cap, objects) if want["rle"] or objects is not None else None,
                            binary if want["binary"] else None, mb)
        from .bilateral_solver import bilateral_solver_batch_device
        head = ops.predict_masks(mask_pred, obj, ops.PackedImages([(img_size, img_size)] * B, self.device), 0.0, rle=False)
        rows = torch.zeros((B, 16), dtype=torch.float32, device=self.device)
        rows[:, 14] = head.best.float()
        target = ops.upsample_selected(mask_pred, rows, (img_size, img_size), "pick")
        _, binary = bilateral_solver_batch_device(u8, target)
        # the solver's S x S binary as a one-query mask: resized to the file's own size exactly as the evaluator scores it
        tail = ops.predict_masks(ops.mask_u8_to_f32(binary).unsqueeze(1), torch.ones((B, 1), dtype=torch.float32, device=self.device),
                                 ops.PackedImages(shapes, self.device), 0.0, **want)
        return _Refined(head, tail, None, None)

    def _run(self, p_images, img_size, scale_factor, outputs, refine, plan=None, objects=None) -> Dict[str, Dict[str, object]]:
        from .graphs import GraphedForward
        from .pipeline import PrefetchingLoader, preprocess_on_device
        from .streams import StreamRing
        p_images, names, sizes, batches = plan if plan is not None else self._plan(p_images, img_size, outputs, refine)
        from .ops import ObjectOptions
        objects = (ObjectOptions.of(objects) or ObjectOptions()) if "objects" in outputs else None
        results = {o: {} for o in outputs}
        best: Dict[str, int] = {}
        self.last_best = best
        if not p_images:
            return results
        model, device = self.network, self.device
        patch = model.encoder.patch_size
        native = img_size is None
        scale = float(patch // scale_factor) if native else 0.0  # exactly the evaluator's choice
        # the evaluator's admission policy per mode: S x S shapes recur from the second batch on; token-grid buckets are captured
        # from their 32nd sighting per stream (a capture costs ~10 ms and ~50 grids on three streams rarely come back that often)
        graphed = GraphedForward(model, enabled=self.hip_graph and isinstance(model, torch.nn.Module), max_graphs=24 if native else 8,
                                 admit_after=31 if native else 2)
        # one encoder attention path for the whole call: a file's result must not depend on the batch it lands in
        prev_path = getattr(model, "attention_path", None)
        pin_path = ("fused" if (not native and self.batch_size >= 16) else "unfused") if prev_path == "auto" else None
        if self._ring is None:
            self._ring = StreamRing(device, self.streams)
        ring = self._ring
        ring.home = torch.cuda.current_stream(device)
        ring.fork()
        pending = deque()

        def settle():
            # a batch is settled before the next one is queued on ITS stream, so a replayed graph's outputs are still that batch's
            # should the run boundaries have to be found again (more than ``cap`` of them)
            bnames, pend = pending.popleft()
            res = pend.result()
            best.update(zip(bnames, res["best"]))
            for o in outputs:
                for n, v, q in zip(bnames, res[o], res["best"]):
                    results[o][n] = v if o in ("rle", "soft_png") else {**v, "best": q} if o == "objects" else v.copy()

        from .decode_pool import default_workers
        avg = max(1, len(p_images) // len(batches))  # buckets are often smaller than batch_size: keep every decode worker busy
        depth = max(len(ring.streams) + 1, -(-2 * (self.workers or default_workers()) // avg))
        if self.decode == "device":
            loader = _DeviceDecoded(p_images, batches, self.workers, len(ring.streams) + 1, self.entropy)
        else:
            loader = PrefetchingLoader(_Files(p_images), range(len(p_images)), self.batch_size, workers=self.workers, depth=depth,
                                       batches=batches, pack=True, pack_size=img_size)
        try:
            if pin_path is not None:
                model.attention_path = pin_path
            for ((packed, shapes), _gts, idx) in loader:
                with ring.next():
                    if self.decode == "device":  # the batch's pixels are decoded on the device, on this batch's stream
                        from .jpeg import packed_from_device
                        packed = packed_from_device(packed.to_device(device), shapes, img_size)
                    if native:
                        Hp = -(-max(h for h, _ in shapes) // patch) * patch
                        Wp = -(-max(w for _, w in shapes) // patch) * patch
                        x = preprocess_on_device(shapes, None, device, packed=packed, pad_to=(Hp, Wp), return_u8=bool(refine))
                    else:
                        x = preprocess_on_device(shapes, img_size, device, packed=packed, return_u8=bool(refine))
                    x, u8 = x if refine else (x, None)
                    assert [sizes[i] for i in idx] == [tuple(s) for s in shapes], "a file's header and its decoded size differ"
                    pending.append(([names[i] for i in idx], self._finish(graphed(x), shapes, u8, scale, img_size, outputs, refine, objects)))
                if len(pending) >= len(ring.streams):
                    settle()
            while pending:
                settle()
        finally:
            ring.join()  # also when a batch raised: the caller's stream waits for whatever is still queued on the ring
            if prev_path == "auto":
                model.attention_path = prev_path
        self.graph_stats = {"captures": graphed.captures, "replays": graphed.replays, "failed": graphed.failed}
        order = {n: k for k, n in enumerate(names)}
        self.last_best = {n: best[n] for n in names}
        return {o: dict(sorted(r.items(), key=lambda kv: order[kv[0]])) for o, r in results.items()}


class _Refined:
    """pending result of a refined batch: the arg-max of ``head`` and the solver's binary as runs (``runs``) or packed planes"""

    def __init__(self, head, runs, binary, table):
        self.head, self.runs, self.table = head, runs, table
        self._binary_h = None
        if binary is not None:
            self._binary_h = torch.empty(binary.shape, dtype=torch.uint8, pin_memory=True)
            self._binary_h.copy_(binary, non_blocking=True)
            self._done = torch.cuda.Event()
            self._done.record(torch.cuda.current_stream(binary.device))

    def result(self):
        out = {"best": self.head.result()["best"]}
        if self.table is None:  # resized mode: ``runs`` is the second finish, with whatever was asked for
            out.update({k: v for k, v in self.runs.result().items() if k != "best"})
            for im in out.get("objects", ()):  # a solver's binary mask has no soft values to score
                for o in im["objects"]:
                    o["score"] = None
            return out
        if self.runs is not None:
            res = self.runs.result()
            if isinstance(res, tuple):  # the packed planes' codes and their objects
                out["rle"], out["objects"] = res
            else:
                out["rle"] = res
        if self._binary_h is not None:
            self._done.synchronize()
            flat = self._binary_h.numpy()
            out["binary"] = [flat[o:o + h * w].reshape(h, w) for o, (h, w) in zip(self.table.px_off, self.table.shapes)]
        return out


IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png", ".bmp", ".webp")


def list_images(src: str):
    """a directory (its image files, sorted) or a text file with one path per line"""
    if os.path.isdir(src):
        return sorted(os.path.join(src, f) for f in os.listdir(src) if f.lower().endswith(IMAGE_SUFFIXES))
    with open(src) as f:
        return [ln.strip() for ln in f if ln.strip()]


def write_pngs(soft: Dict[str, object], png_dir: str, threads: int = 4) -> None:
    """the soft maps as 8-bit greyscale PNGs (<file stem>.png: what the external SOD toolkits read), on a small host thread pool: an
    array is encoded by Pillow, ``bytes`` (a file the device encoded, output "soft_png") are written as they are"""
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    os.makedirs(png_dir, exist_ok=True)
    stems = [os.path.splitext(n)[0] for n in soft]
    assert len(set(stems)) == len(stems), "two files share a stem: their PNGs would overwrite each other"

    def one(item):
        name, arr = item
        path = os.path.join(png_dir, os.path.splitext(name)[0] + ".png")
        if isinstance(arr, bytes):
            with open(path, "wb") as f:
                f.write(arr)
        else:
            Image.fromarray(np.ascontiguousarray(arr, np.uint8)).save(path)

    with ThreadPoolExecutor(max_workers=max(1, threads)) as pool:
        list(pool.map(one, soft.items()))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m selfmask_amd.predictor",
                                 description="masks for a directory (or a list file) of images without ground truth")
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--p_state_dict", type=str, required=True)
    ap.add_argument("--images", type=str, required=True, help="a directory, or a text file with one image path per line")
    ap.add_argument("--out", type=str, required=True, help="JSON: {file name: COCO uncompressed RLE}")
    ap.add_argument("--img_size", type=int, default=None, help="resize inputs to S x S (default: native resolution in token-grid buckets)")
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--refine", type=str, default=None, choices=["bilateral"])
    ap.add_argument("--png_dir", type=str, default=None, help="also write the soft maps as 8-bit PNGs into this directory")
    ap.add_argument("--png_encoder", type=str, default="host", choices=list(PNG_ENCODERS),
                    help="device: the PNG files of --png_dir are encoded on the GPU (same pixels, other bytes than Pillow's)")
    ap.add_argument("--objects_out", type=str, default=None, help="also write the masks' objects (boxes, areas, centroids, scores, "
                    "per-object RLE) as JSON: {file name: {...}}")
    ap.add_argument("--connectivity", type=int, default=8, choices=[4, 8])
    ap.add_argument("--min_area", type=int, default=0, help="objects of fewer pixels are dropped")
    ap.add_argument("--max_objects", type=int, default=16, help="the largest objects kept per image (1 .. 64)")
    ap.add_argument("--decode", type=str, default="host", choices=list(DECODES),
                    help="device: baseline JPEGs are entropy-decoded on host threads and finished on the GPU (same pixels as Pillow)")
    ap.add_argument("--entropy", type=str, default="host", choices=list(ENTROPIES),
                    help="device (with --decode device): the GPU also Huffman-decodes the scans; the host threads only strip markers and stuffing")
    ap.add_argument("--gpu_id", type=int, default=0)
    return ap


def main(argv=None):
    import json
    import yaml
    from .maskformer import load_checkpoint
    from .misc import get_model
    args = build_parser().parse_args(argv)
    if args.png_dir and args.refine:
        raise SystemExit("--png_dir writes soft maps, which --refine does not produce")
    cfg = argparse.Namespace(**yaml.safe_load(open(args.config)))
    device = torch.device("cuda", args.gpu_id)
    model = get_model("maskformer", configs=cfg)
    load_checkpoint(model, args.p_state_dict)
    model = model.to(device).eval()
    pred = SaliencyPredictor(model, device=device, batch_size=args.batch_size, decode=args.decode, png_encoder=args.png_encoder,
                             entropy=args.entropy)
    soft = "soft_png" if pred.png_encoder == "device" else "soft"
    outputs = ("rle",) + ((soft,) if args.png_dir else ()) + (("objects",) if args.objects_out else ())
    objects = dict(connectivity=args.connectivity, min_area=args.min_area, max_objects=args.max_objects) if args.objects_out else None
    res = pred._run(list_images(args.images), args.img_size, getattr(cfg, "scale_factor", 2), outputs, args.refine, objects=objects)
    with open(args.out, "w") as f:
        json.dump(res["rle"], f, separators=(",", ":"))
    if args.objects_out:
        with open(args.objects_out, "w") as f:
            json.dump(res["objects"], f, separators=(",", ":"))
    if args.png_dir:
        write_pngs(res[soft], args.png_dir)
    print(f"{len(res['rle'])} masks -> {args.out}" + (f", PNGs -> {args.png_dir}" if args.png_dir else "") +
          (f", objects -> {args.objects_out}" if args.objects_out else ""))
    return res


if __name__ == "__main__":
    main()
