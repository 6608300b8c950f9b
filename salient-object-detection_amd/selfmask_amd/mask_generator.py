"""Mirror of the reference's ``datasets.mask_generator.MaskGenerator`` (bytecode only: SURVEY.md Appendix B, mask_generator.pyc@L21-252;
its constants are pinned by tests/golden/evaluator_constants.json) on the MI355X:

    MaskGenerator(cluster_sizes=(2, 3, 4), cluster_type="spectral", feature_types=["mocov2", "swav", "dino"], network=model,
                  backbones={"mocov2": r1, "swav": r2})(p_images)      -> {filename: run-length-encoded salient mask}

``extract_candidate_masks`` (@L136-200): every image at its native resolution, normalised as ``CustomDataset`` does
(/root/reference/datasets/custom_dataset.py:26-32: RGB, ``to_tensor``, ImageNet mean / std), zero-padded to a multiple of the stride
(``pad_input_image`` @L124-134 = what ``make_input_divisible`` does inside the encoder), layer-12 tokens -> bilinear x2
(``align_corners=True``) -> ``clusterer(features, k)`` for k in cluster_sizes -> one-hot -> nearest up-sample -> crop.  Images that pad to
one patch grid share a batch (the reference's DataLoader runs batch 1; images are independent, and an image's padded input is the same
in a batch as alone): the crop to its own H x W happens inside the vote and the run-length kernels.  ``vote_mask`` (@L202-230) picks the candidate that
agrees most with the others.  ``__call__`` (@L232-252) returns the winner per file name, run-length encoded.

The ResNet feature types ("mocov2", "swav": ``backbones={type: selfmask_amd.ResNet50}``) give nine more candidates each
(``voting.extract_candidate_masks_resnet``: the image padded to a multiple of 8, the dilated ResNet-50's last map, the same x2
up-sample, the spectral clusterer at 2048 dimensions, nearest up-sample by 4), and all 27 go into one vote.

Differences kept on purpose: (1) k-means on the 2048-d points of a ResNet type is not built (``cluster_type="k-means"`` with such a
type raises); (2) the encoder is the ``network`` handed in (a ``selfmask_amd.MaskFormer`` whose encoder holds the DINO weights) and the
ResNets are the ``backbones`` handed in: the reference fetches all of them from the network at construction time
(utils/misc.py:196,243), which must never happen here; (3) the reference encodes with ``pycocotools.mask.encode`` (absent from this
image): ``rle_encode`` writes COCO's UNCOMPRESSED run-length form ({"size": [h, w], "counts": [n0, n1, ...]}, column-major, first run =
zeros), which ``pycocotools.mask.frPyObjects`` turns into the compressed string; (4) both clusterers are parity UNPINNED - the
reference's ``clusterings`` module is absent in every form (voting.py)."""
from collections import defaultdict
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import voting as VT
from .datasets import MEAN, STD


def rle_encode(mask: np.ndarray) -> dict:
    """(H, W) 0/1 -> COCO uncompressed RLE: runs over the column-major (Fortran) order, starting with the zeros."""
    m = np.asarray(mask).astype(bool)
    flat = m.flatten(order="F")
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    bounds = np.concatenate([[0], change, [flat.size]])
    counts = np.diff(bounds).tolist()
    if flat.size and flat[0]:
        counts = [0] + counts
    return {"size": [int(m.shape[0]), int(m.shape[1])], "counts": [int(c) for c in counts]}


def rle_decode(rle: dict) -> np.ndarray:
    h, w = rle["size"]
    vals = np.zeros(len(rle["counts"]), bool)
    vals[1::2] = True
    return np.repeat(vals, rle["counts"]).reshape((h, w), order="F").astype(np.uint8)


class _Files:
    """what PrefetchingLoader needs of a dataset: image paths, no ground truth"""

    def __init__(self, p_imgs):
        self.p_imgs, self.p_gts = list(p_imgs), [None] * len(p_imgs)


class MaskGenerator:
    def __init__(self, cluster_sizes: Sequence[int] = VT.DEFAULT_CLUSTER_SIZES, cluster_type: str = VT.DEFAULT_CLUSTER_TYPE,
                 feature_types: Sequence[str] = ("dino",), use_gpu: bool = True, device: torch.device = torch.device("cuda:0"),
                 network=None, batch_size: int = 128, n_neighbors: int = 10, streams: int = 3, workers: Optional[int] = None,
                 max_stream_bytes: int = 16 << 30, backbones: Optional[Dict[str, object]] = None):
        """``batch_size``: the most images of ONE size clustered together - the eigen-solver runs one workgroup per image, so a launch
        takes about as long for 128 images as for 8 (profiles/r04_pseudo_masks_by_batch.log); ``streams``: batches in flight (one's
        eigen-solve, half of the CUs at 128 images, runs beside the next one's encoder); ``workers``: decode processes
        (default: this rank's share of the host cores); ``max_stream_bytes``: for patch grids of more than 8192 clustered points
        (n = 4 gh gw: above about 1024 x 512 pixels at P = 16) - and for EVERY size once a ResNet type is asked for - the batch is cut
        so that the clusterer's and the networks' scratch of one stream stay within this many bytes (default 16 GiB; at least one
        image per batch); ``feature_types=["dino"]`` on smaller grids keeps ``batch_size``.  ``backbones``: {"mocov2" | "swav": a
        ``selfmask_amd.ResNet50`` whose weights the caller has loaded (``load_pretrained``)} - one per ResNet feature type asked for;
        nothing is fetched or read from a fixed path."""
        assert cluster_type in VT.CLUSTER_TYPES + ("kmeans",), cluster_type  # mask_generator.pyc@L30: ('k-means', 'spectral')
        backbones = dict(backbones or {})
        unsupported = [f for f in feature_types if f != "dino" and (f not in VT.RESNET_FEATURE_TYPES or backbones.get(f) is None)]
        if unsupported:
            raise NotImplementedError(f"feature types {unsupported}: the MoCo-v2 / SwAV ResNet-50 checkpoints are absent from the reference "
                                      f"repository and nothing is downloaded; hand each one in as `backbones={{type: ResNet50}}` with its "
                                      f"weights loaded ('dino' needs `network`)")
        self.resnet_types = [f for f in feature_types if f != "dino"]
        if "dino" in feature_types and network is None:
            raise ValueError("MaskGenerator needs `network` (a selfmask_amd.MaskFormer whose encoder holds the DINO ViT-S weights): the "
                             "reference downloads them at construction time, which this build never does")
        if not feature_types:
            raise ValueError("MaskGenerator needs at least one feature type")
        if not use_gpu:
            raise RuntimeError("the MI355X build has no CPU path")
        if self.resnet_types and cluster_type != "spectral":
            raise NotImplementedError(f"cluster_type={cluster_type!r} with feature types {self.resnet_types}: k-means on 2048-d points is "
                                      f"not built (kmeans_kernel keeps its centres for 384-d points in the LDS); use 'spectral'")
        self.cluster_sizes, self.cluster_type, self.feature_types = tuple(int(k) for k in cluster_sizes), cluster_type, list(feature_types)
        n_cand = sum(self.cluster_sizes) * len(self.feature_types)
        if n_cand > VT.MAX_VOTE_CANDIDATES:
            raise ValueError(f"MaskGenerator: {sum(self.cluster_sizes)} candidates x {len(self.feature_types)} feature types = {n_cand} "
                             f"planes; the vote takes at most {VT.MAX_VOTE_CANDIDATES}")
        self.backbones = {f: backbones[f] for f in self.resnet_types}
        self.device, self.network, self.batch_size, self.n_neighbors = torch.device(device), network, int(batch_size), int(n_neighbors)
        self.streams, self.workers, self.max_stream_bytes = max(1, int(streams)), workers, int(max_stream_bytes)
        self._ring = None  # the streams of __call__, made once: the per-stream scratch of the clusterer (voting._arena) stays bounded

    # ---- mask_generator.pyc@L136-200 --------------------------------------------------------------------------------------------
    def _load(self, p_image: str) -> torch.Tensor:
        """one file as ``CustomDataset`` prepares it on the host (custom_dataset.py:26-32) - what the batches below hold, per image
        (tests compare the two)"""
        from PIL import Image
        rgb = np.asarray(Image.open(p_image).convert("RGB"), np.float32) / np.float32(255.0)  # to_tensor
        x = (rgb - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)               # normalize
        return torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))

    def _patch(self) -> int:
        """the DINO encoder's patch size (total stride); without the "dino" type the ResNets' stride stands in"""
        return self.network.encoder.patch_size if "dino" in self.feature_types else VT.RESNET_TOTAL_STRIDE

    def _bucket_stride(self) -> int:
        """images share a batch when they pad to one grid of this stride: the ResNets' 8 when one is asked for (the reference pads every
        image alone to a multiple of 8 for them, and the size of that grid enters the align_corners up-sample; P is a multiple of 8, so
        such a bucket shares the DINO grid too), else the patch size"""
        return VT.RESNET_TOTAL_STRIDE if self.resnet_types else self._patch()

    def _points(self, hw) -> int:
        """points the clusterer sees for an image of size hw: the patch tokens of its padded grid after the x2 up-sample"""
        P = self._patch()
        return 4 * (-(-int(hw[0]) // P)) * (-(-int(hw[1]) // P))

    def _points_resnet(self, hw) -> int:
        """the same for a ResNet type: the stride-8 grid of the image padded to a multiple of 8, after the x2 up-sample"""
        s = VT.RESNET_TOTAL_STRIDE
        return 4 * (-(-int(hw[0]) // s)) * (-(-int(hw[1]) // s))

    def _batch_cap(self, hw) -> int:
        """the most images of the padded size of hw in one batch: ``batch_size``, and above 8192 clustered points as many as the
        clusterer's plus the encoder's workspace allow within ``max_stream_bytes`` (both grow linearly in the batch).  With a ResNet
        type every size is counted: per image the backbone's workspace, its 2048-d rows and the clusterer's workspace at that width
        (the Gram matrix, n^2 * 4 B, is part of it to 8192 points: 225 MB at 300 x 400), beside the DINO type's share."""
        n = self._points(hw)
        if not self.resnet_types and (self.cluster_type != "spectral" or n <= VT.SPECTRAL_GRAM_POINTS):
            return self.batch_size
        from . import _native as N
        lib = N.load()
        P = self._patch()
        Hp, Wp = -(-int(hw[0]) // P) * P, -(-int(hw[1]) // P) * P
        per = 0
        if "dino" in self.feature_types:
            per += (lib.sm_spectral_workspace_bytes(1, n, self.n_neighbors, max(self.cluster_sizes))
                    + lib.sm_forward_workspace_bytes(self.network._weights(), 1, Hp, Wp))
        if self.resnet_types:
            s = VT.RESNET_TOTAL_STRIDE
            H8, W8, nr = -(-int(hw[0]) // s) * s, -(-int(hw[1]) // s) * s, self._points_resnet(hw)
            # (the types run one after the other on the stream: their scratch is shared, counted once)
            per += (lib.sm_resnet50_workspace_bytes(1, H8, W8, 1) + nr * N.RESNET_EMBED * 4
                    + lib.sm_spectral_workspace_bytes_dim(1, nr, N.RESNET_EMBED, self.n_neighbors, max(self.cluster_sizes)))
        return max(1, min(self.batch_size, self.max_stream_bytes // max(per, 1)))

    def _plan(self, p_images: Sequence[str]):
        """-> (paths, sizes, batches): the headers' sizes, every one checked against the clusterer's limits BEFORE anything is
        queued (a file out of range raises ValueError naming it), grouped into native buckets of at most ``_batch_cap`` images"""
        from .datasets import probe_size
        from .pipeline import native_buckets
        p_images = list(p_images)
        sizes = [probe_size(p) for p in p_images]  # headers only
        self._check_points(p_images, sizes)
        batches = []
        for b in native_buckets(sizes, self._bucket_stride(), self.batch_size):
            cap = self._batch_cap(sizes[b[0]])
            batches += [b[s:s + cap] for s in range(0, len(b), cap)]
        return p_images, sizes, sorted(batches, key=len, reverse=True)

    def _check_points(self, p_images, sizes) -> None:
        """every feature type's point count of every file against the spectral clusterer's limits"""
        if self.cluster_type != "spectral":
            return
        for p, hw in zip(p_images, sizes):
            counts = ([("dino", self._points(hw))] if "dino" in self.feature_types else []) + \
                     [(f, self._points_resnet(hw)) for f in self.resnet_types]
            for f, n in counts:
                if not VT.SPECTRAL_MIN_POINTS <= n <= VT.SPECTRAL_MAX_POINTS:
                    raise ValueError(f"MaskGenerator: {p} ({hw[0]} x {hw[1]}) gives {n} points to the spectral clusterer for "
                                     f"feature type {f!r} ({VT.SPECTRAL_MIN_POINTS} <= n <= {VT.SPECTRAL_MAX_POINTS}); nothing was run")

    def _batches(self, p_images: Sequence[str], pack: bool = False, plan=None):
        """-> (file names, decoded uint8 RGB arrays) per batch of at most ``batch_size`` images that pad to ONE patch grid
        (``pipeline.native_buckets``: the evaluator's native-resolution buckets): the headers give the sizes, the decode processes of the
        input pipeline (decode_pool.py) the pixels, a few batches ahead of the device.  Largest buckets first.  ``pack``: the second item
        is (page-locked staging buffers of the batch, [(H, W)]) assembled on the loader's packing thread - what ``__call__`` consumes."""
        from .pipeline import PrefetchingLoader
        p_images, _sizes, batches = plan if plan is not None else self._plan(p_images)
        loader = PrefetchingLoader(_Files(p_images), range(len(p_images)), self.batch_size, workers=self.workers, batches=batches, pack=pack)
        for rgbs, _gts, idx in loader:
            yield [p_images[i].split("/")[-1] for i in idx], rgbs

    def _candidates(self, rgbs):
        """decoded images of one grid (arrays, or the loader's (staging buffers, shapes)) -> ((B, M, Hp, Wp) uint8 candidates, [(H_b, W_b)]),
        queued on the current stream, M = sum(cluster_sizes) per feature type in ``feature_types`` order (the reference appends them per
        image in that order): every image zero-padded to the grid's Hp x Wp after normalisation - what ``pad_input_image`` (@L124-134) builds
        for it alone - and its candidates are the top-left H_b x W_b of its planes.  A ResNet type sees the top-left ceil8 region of the
        same batch: the image padded to a multiple of 8, as the reference pads it for that type."""
        from .pipeline import preprocess_on_device
        P = self._patch()
        packed = None
        if isinstance(rgbs, tuple):
            packed, rgbs = rgbs
        sizes = [(int(r[0]), int(r[1])) if packed is not None else (int(r.shape[0]), int(r.shape[1])) for r in rgbs]
        Hp, Wp = -(-max(h for h, _ in sizes) // P) * P, -(-max(w for _, w in sizes) // P) * P
        x = preprocess_on_device(rgbs, None, self.device, pinned=True, packed=packed, pad_to=(Hp, Wp))  # to_tensor + normalize + pad (device)
        if not self.resnet_types:
            cands = VT.extract_candidate_masks(self.network, x, self.cluster_sizes, cluster_type=self.cluster_type, n_neighbors=self.n_neighbors)
            return (cands[None] if cands.dim() == 3 else cands), sizes
        s = VT.RESNET_TOTAL_STRIDE
        H8, W8 = -(-max(h for h, _ in sizes) // s) * s, -(-max(w for _, w in sizes) // s) * s  # (one bucket: every image's own ceil8)
        k = sum(self.cluster_sizes)
        out = torch.zeros((len(sizes), k * len(self.feature_types), Hp, Wp), dtype=torch.uint8, device=x.device)
        xr = x[:, :, :H8, :W8].contiguous() if (H8, W8) != (Hp, Wp) else x
        for t, f in enumerate(self.feature_types):
            if f == "dino":
                c = VT.extract_candidate_masks(self.network, x, self.cluster_sizes, cluster_type=self.cluster_type, n_neighbors=self.n_neighbors)
                out[:, t * k:(t + 1) * k] = c[None] if c.dim() == 3 else c
            else:
                c = VT.extract_candidate_masks_resnet(self.backbones[f], xr, self.cluster_sizes, self.n_neighbors, self.cluster_type)
                out[:, t * k:(t + 1) * k, :H8, :W8] = c[None] if c.dim() == 3 else c
        return out, sizes

    @torch.no_grad()
    def extract_candidate_masks(self, p_images: Sequence[str]) -> Dict[str, torch.Tensor]:
        """file name -> (sum(cluster_sizes) * len(feature_types), H, W) uint8 on the device: the candidates of the feature types
        concatenated in ``feature_types`` order, as the reference appends them per file name."""
        out: Dict[str, torch.Tensor] = {}
        for names, rgbs in self._batches(p_images):
            cands, sizes = self._candidates(rgbs)
            for n, c, (h, w) in zip(names, cands, sizes):
                out[n] = c[:, :h, :w]
        return out

    # ---- mask_generator.pyc@L202-230 --------------------------------------------------------------------------------------------
    def vote_mask(self, batch_pred_masks: torch.Tensor, remove_long_masks: bool = True, remove_small_large_masks: bool = False):
        return VT.vote_mask(batch_pred_masks, remove_long_masks, remove_small_large_masks)

    # ---- mask_generator.pyc@L232-252 --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, p_images: Sequence[str], remove_long_masks: bool = True, remove_small_large_masks: bool = False,
                 encode: Optional[bool] = True, comm=None) -> Dict[str, object]:
        """Candidates and vote of one batch are queued on one stream of a ring and read back ``streams`` batches later: images are
        independent, so the result per file is what the reference's extract-everything-then-vote order gives.  ``comm`` (a
        ``distributed.TorchDistComm``): this rank takes files rank, rank + W, ... of the list (``shard_indices``, as the evaluator
        shards its images), and every rank returns the codes of ALL files (one all-gather of the encoded shards at the end).
        Every file's size is checked before anything is queued: one out of the clusterer's range raises ValueError naming it."""
        plan = self._plan(p_images)
        p_images = plan[0]
        if comm is not None and comm.world_size > 1:
            from .distributed import gather_dicts, shard_indices
            assert encode, "the gather exchanges run-length codes"
            p_images = list(p_images)
            names = [p.split("/")[-1] for p in p_images]
            assert len(set(names)) == len(names), "file names must be unique (they key the result)"
            mine = self([p_images[i] for i in shard_indices(len(p_images), comm.rank, comm.world_size)], remove_long_masks,
                        remove_small_large_masks, True)
            merged = gather_dicts(mine, comm, self.device)
            return {n: merged[n] for n in names}  # the list's order, whatever the sharding
        from collections import deque
        from .streams import StreamRing
        if self._ring is None:
            self._ring = StreamRing(self.device, self.streams)
        ring = self._ring
        ring.home = torch.cuda.current_stream(self.device)  # whatever the caller queued so far is visible to the ring's streams
        ring.fork()
        pending = deque()
        result: Dict[str, object] = {}

        def settle():
            names, votes, runs = pending.popleft()
            names, sizes = names
            if runs is not None:  # the run boundaries were found on the device: two small copies per batch instead of the masks
                votes.result()    # (raises if a batch came back without a winner)
                result.update(zip(names, runs.result()))
            else:
                for n, m, (h, w) in zip(names, votes.winners_host().numpy(), sizes):
                    result[n] = m[:h, :w].copy()

        for names, rgbs in self._batches(p_images, pack=True, plan=plan):
            with ring.next():
                cands, sizes = self._candidates(rgbs)
                votes = VT.vote_mask_batch_async(cands, remove_long_masks, remove_small_large_masks, winners="device" if encode else True,
                                                 sizes=sizes)
                pending.append(((names, sizes), votes, VT.rle_runs_async(votes.winners, sizes=sizes) if encode else None))
            if len(pending) >= len(ring.streams):
                settle()
        while pending:
            settle()
        ring.join()
        return result
