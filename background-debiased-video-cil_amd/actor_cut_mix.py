"""ActorCutMix clip loader: ``ActorCutMixDataset`` of the reference (libs/loader/actor_cut_mix_loader.py) for whole batches, from JPEG
frames and a human-detection file, with the composite on the GPU (``bdv_actor_cut_mix_u8``, csrc/actor_cut_mix.hip).

Per sample the reference draws ``random.random() < acm_prob`` (:117-126).  If true (``actor_cut_mix``, :135-164) the sample's own
clip is the actor and a random video of the training set (``random.randrange``, merged exemplars included, possibly the same video)
the scene; both go through SampleFrames -> decode -> DetectionLoad(0.4) -> ResizeWithBox(-1, 256) -> FlipWithBox(0.5) ->
ResizeWithBox((224, 224)), the actor's boxes become the human mask, the scene's own boxes are painted 127 (ActorCutOut), and the
frames are ``actor * mask + scene * (1 - mask)``; ``foreground_ratio`` = mask pixels / (T*H*W), ``background_label`` = the scene's
label.  Otherwise (:121-124) the sample takes the RandAugment(2, 10, prob=1) -> MultiScaleCrop(13 crops) -> Resize(224) path with
``foreground_ratio = 1`` and ``background_label = -1``, and no background mix.

The box arithmetic (libs/pipelines/box.py) is done here in numpy with the reference's operations, so dtype promotion matches: scale
factors are float32 ``new_w / img_w``, boxes are ``np.clip(det * sf, 0, new_w)`` in the detection array's own dtype, the flip maps
x0 -> W - x2 and x2 -> W - x0 at the 256 scale, and the final boxes are cut with ``.astype(int)``.  Only the resampling (cv2's
INTER_LINEAR, see include/bdvcil_hip.h) is unpinned, as for ``RawFrameClipLoader``."""
from __future__ import annotations

import os.path as osp
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from .decode import RawFrameClipLoader, jpeg_parse, rescale_size, sample_frames
from .frontend import IMG_MEAN, IMG_STD

FILL_COLOR = 127          # SceneCutOut / ActorCutOut(fill_color=127), actor_cut_mix_loader.py:82, :95


def detection_key(frame_dir: str, det_file: str) -> str:
    """Key of a video in the detection file (``load_detections``, actor_cut_mix_loader.py:105-115): the last path component of
    ``frame_dir``, or its first 11 characters when ``'kinetics'`` is in the detection file's path (YouTube ids)."""
    name = frame_dir.split('/')[-1]
    return name[:11] if 'kinetics' in det_file else name


def load_detections(det_file: str) -> dict:
    """``np.load(det_file, allow_pickle=True).item()``: video key -> per-frame arrays of (x0, y0, x1, y1, score) rows."""
    return np.load(det_file, allow_pickle=True).item()


def detection_load(all_detections, frame_inds, thres: float = 0.4, offset: int = 0) -> List[np.ndarray]:
    """``DetectionLoad`` (box.py:27-54): per sampled frame the rows with ``score > thres`` (strict), first four columns.

    Reference quirk, kept: the detections are indexed with the 1-based file numbers ``SampleFrames`` emits (``start_index`` is
    already added), so frame number i reads entry i of the per-video list.  An index past its end raises, as in the reference."""
    dets = []
    for frame_idx in np.asarray(frame_inds).reshape(-1):
        cur = all_detections[frame_idx + offset]
        dets.append(cur[cur[:, -1] > thres, :4])
    return dets


def resize_boxes(dets: List[np.ndarray], img_w: int, img_h: int, new_w: int, new_h: int) -> List[np.ndarray]:
    """The box half of ``ResizeWithBox`` (box.py:249-267), in place and in each array's own dtype."""
    sf = np.array([new_w / img_w, new_h / img_h], dtype=np.float32)
    for cur in dets:
        cur[:, 0::2] = np.clip(cur[:, 0::2] * sf[0], 0, new_w)
        cur[:, 1::2] = np.clip(cur[:, 1::2] * sf[1], 0, new_h)
    return dets


def flip_boxes(dets: List[np.ndarray], img_w: int) -> List[np.ndarray]:
    """The box half of a horizontal ``FlipWithBox`` (box.py:362-371): x0 -> img_w - x2, x2 -> img_w - x0."""
    out = []
    for cur in dets:
        f = cur.copy()
        f[:, 0] = img_w - cur[:, 2]
        f[:, 2] = img_w - cur[:, 0]
        out.append(f)
    return out


def clip_boxes(all_detections, frame_inds, img_w: int, img_h: int, short_edge: int, out_w: int, out_h: int, flip: bool,
               thres: float = 0.4) -> List[np.ndarray]:
    """The box chain of both pipelines (actor_cut_mix_loader.py:74-96): DetectionLoad -> ResizeWithBox((-1, short_edge)) ->
    FlipWithBox -> ResizeWithBox((out_w, out_h), keep_ratio=False), cut with ``.astype(int)`` as BuildHumanMask and the cut-outs
    do.  ``img_w`` x ``img_h``: the decoded frame size.  Returns T int arrays (n_t, 4) of (x0, y0, x1, y1)."""
    dets = detection_load(all_detections, frame_inds, thres)
    w1, h1 = rescale_size(img_w, img_h, (-1, short_edge))
    resize_boxes(dets, img_w, img_h, w1, h1)
    if flip:
        dets = flip_boxes(dets, w1)
    resize_boxes(dets, w1, h1, out_w, out_h)
    return [d.astype(int) for d in dets]


@dataclass
class AcmDraw:
    """The random decisions of one sample.  ActorCutMix rows: ``frame_inds`` / ``flip`` of the actor, the scene's index into the
    plan's pool, its frame numbers and flip.  RandAugment rows: ``frame_inds``, ``RandAugment.draw``'s result and the MultiScaleCrop
    box (x, y, w, h)."""
    acm: bool
    frame_inds: np.ndarray
    flip: bool = False
    scene_index: int = -1
    scene_inds: Optional[np.ndarray] = None
    scene_flip: bool = False
    randaug: object = None
    crop: Optional[tuple] = None


@dataclass
class AcmPlan:
    rows: List[AcmDraw]
    scene_infos: List[dict]        # the pool the scene indices refer to


class ActorCutMixClipLoader(RawFrameClipLoader):
    """``clip_loader`` of ``CILTaskLoop`` for the ActorCutMix configs (configs/ucf101/seed_*_ActorCutMix_plus_randAug.py).

    ``train``: ``draw(video_infos, frame_hw)`` makes every host draw, per sample in the reference's order -- the acm draw
    (``random``), then for an ActorCutMix row the actor's frame offsets (``np.random``), its flip (``np.random.rand``), the scene
    index (``random.randrange`` over the scene pool), the scene's offsets and its flip; for a RandAugment row its frame offsets,
    RandAugment's draws and MultiScaleCrop's two ``random.choice`` -- and returns an ``AcmPlan``; ``run(plan, video_infos)``
    executes it.  Actor and scene frames are decoded by ``JpegDecoder`` and resized by ``resize_linear_u8`` (the RandAugment rows'
    clips first, so that they are a leading view of the batch); one ``bdv_actor_cut_mix_u8`` launch composites and normalises every
    ActorCutMix row into the output, and the RandAugment rows go through the existing RandAugment -> MultiScaleCrop + Resize ->
    Normalize path (no mix), copied into their rows in a mixed batch (the one extra device copy).  A scene whose
    actor clip has no box is not decoded: the output is then the actor clip alone (the draws are still made).
    ``foreground_ratio`` (B,) float64 comes from the kernel's mask counts; ``background_label`` (B, 1) int64 is the scene's label,
    -1 on RandAugment rows.  Within a batch the samples' frames share one size and the decoded scenes share one size
    (else ``ValueError`` naming the videos).

    Other phases: exactly ``RawFrameClipLoader``'s batches.  ``set_scene_infos(video_infos)``: the training set the scenes are
    drawn from (``CILTaskLoop`` passes the merged train + exemplar list before each fit); without it, the batch itself."""

    def __init__(self, det_file: str, acm_prob: float = 0.5, device='cuda', filename_tmpl: str = 'img_{:05}.jpg', num_segments: int = 8,
                 start_index: int = 1, short_edge: int = 256, input_size: int = 224, randAug=None, multi_scale_crop: dict = None,
                 test_crop=('TenCrop', 256), threads: int = 8, det_thres: float = 0.4, flip_ratio: float = 0.5, seed=None):
        from .augment import RandAugment
        super().__init__(device, filename_tmpl=filename_tmpl, num_segments=num_segments, start_index=start_index, short_edge=short_edge,
                         input_size=input_size, randAug=randAug if randAug is not None else RandAugment(2, 10, 1.0),
                         multi_scale_crop=multi_scale_crop, test_crop=test_crop, threads=threads, seed=seed)
        self.det_file = str(det_file)
        self.detections = load_detections(self.det_file)
        self.acm_prob, self.det_thres, self.flip_ratio = float(acm_prob), float(det_thres), float(flip_ratio)
        self.scene_infos: Optional[List[dict]] = None
        self._sizes = {}

    def set_scene_infos(self, video_infos: Sequence[dict]) -> None:
        """The pool ``random.randrange`` draws scenes from.  Every video's detections are looked up now, as the reference's
        ``load_detections`` does when the dataset is built or merged (libs/cil/cil.py:394-396): a missing key raises ``KeyError``."""
        infos = list(video_infos) if video_infos else None
        for v in infos or ():
            self.video_detections(v)
        self.scene_infos = infos

    def video_detections(self, info: dict):
        return self.detections[detection_key(info['frame_dir'], self.det_file)]

    # ---- host side ------------------------------------------------------------------------------------------------------------
    def _source_size(self, info: dict):
        """(W, H) of a video's frames, from the header of its first file (cached per frame_dir)."""
        d = info['frame_dir']
        if d not in self._sizes:
            hdr = jpeg_parse(self._read(osp.join(d, self.tmpl.format(self.start_index))))
            self._sizes[d] = (int(hdr.width), int(hdr.height))
        return self._sizes[d]

    def _common_size(self, infos: Sequence[dict], what: str):
        sizes = {}
        for v in infos:
            sizes.setdefault(self._source_size(v), []).append(v['frame_dir'])
        if len(sizes) != 1:
            raise ValueError(f'ActorCutMixClipLoader: {what} frames of different sizes in one batch: '
                             + '; '.join(f'{w}x{h}: {", ".join(ds)}' for (w, h), ds in sizes.items()))
        return next(iter(sizes))

    def draw(self, video_infos: Sequence[dict], frame_hw) -> AcmPlan:
        """All host draws of a train batch (see the class docstring).  ``frame_hw``: (H, W) of the batch's frames after
        Resize(-1, short_edge), which RandAugment's and MultiScaleCrop's draws read."""
        H, W = frame_hw
        pool = self.scene_infos if self.scene_infos else list(video_infos)
        rows = []
        random, np_random, d = self.draws.py, self.draws.np, self.draws
        for v in video_infos:
            total = int(v['total_frames'])
            if random.random() < self.acm_prob:
                inds = sample_frames(total, self.T, start_index=self.start_index, draws=d)
                flip = bool(np_random.rand() < self.flip_ratio)
                si = random.randrange(len(pool))
                sinds = sample_frames(int(pool[si]['total_frames']), self.T, start_index=self.start_index, draws=d)
                sflip = bool(np_random.rand() < self.flip_ratio)
                rows.append(AcmDraw(True, inds, flip, si, sinds, sflip))
            else:
                inds = sample_frames(total, self.T, start_index=self.start_index, draws=d)
                ra = self.train_front.randaug.draw(H, W)
                crop = self.train_front.crop_resize.draw(W, H)
                rows.append(AcmDraw(False, inds, randaug=ra, crop=crop))
        return AcmPlan(rows, pool)

    def _decode(self, infos: Sequence[dict], inds: Sequence[np.ndarray]) -> torch.Tensor:
        """Frames (n, T, Hr, Wr, 3) uint8 after Resize(-1, short_edge)."""
        from . import kernels as K
        paths = [osp.join(v['frame_dir'], self.tmpl.format(int(i))) for v, ii in zip(infos, inds) for i in ii]
        streams = list(self.decoder.pool.map(self._read, paths))
        frames = self.decoder.decode_clips([streams[k * self.T:(k + 1) * self.T] for k in range(len(infos))])
        H0, W0 = int(frames.shape[2]), int(frames.shape[3])
        Wr, Hr = rescale_size(W0, H0, (-1, self.short_edge))
        return K.resize_linear_u8(frames, Hr, Wr)

    def run(self, plan: AcmPlan, video_infos: Sequence[dict]) -> dict:
        """Execute a ``draw`` plan: the collated train batch."""
        from . import kernels as K
        B, T, S, dev = len(video_infos), self.T, self.input_size, self.device
        rows = plan.rows
        W0, H0 = self._common_size(video_infos, 'sample')
        rand_idx = [k for k, r in enumerate(rows) if not r.acm]
        acm_idx = [k for k, r in enumerate(rows) if r.acm]
        # decoded RandAugment rows first, so that they are a leading view of the frames (no gather): the ActorCutMix clips follow
        order = rand_idx + acm_idx
        frames = self._decode([video_infos[k] for k in order], [rows[k].frame_inds for k in order])
        out = torch.empty(B, T, 3, S, S, dtype=torch.float32, device=dev)
        fg = torch.ones(B, dtype=torch.float64, device=dev)
        bg_label = [-1] * B
        if rand_idx:
            sub = frames[:len(rand_idx)]
            sub = self.train_front.randaug.apply_draws(sub, [rows[k].randaug for k in rand_idx])
            sub, _ = self.train_front.crop_resize(sub, None, boxes=[rows[k].crop for k in rand_idx])
            imgs = self.train_front.mix.as_nchw(sub)                         # Normalize only: no background mix in this branch
            if len(rand_idx) == B:
                out = imgs
            else:                                                            # the one extra device copy of these rows
                out[torch.as_tensor(rand_idx, device=dev)] = imgs
        if acm_idx:
            scenes = [plan.scene_infos[rows[k].scene_index] for k in acm_idx]
            actor_boxes, scene_boxes, scene_rows, decode = [], [], [], []
            for k, sv in zip(acm_idx, scenes):
                r = rows[k]
                ab = clip_boxes(self.video_detections(video_infos[k]), r.frame_inds, W0, H0, self.short_edge, S, S, r.flip, self.det_thres)
                sw, sh = self._source_size(sv)
                sb = clip_boxes(self.video_detections(sv), r.scene_inds, sw, sh, self.short_edge, S, S, r.scene_flip, self.det_thres)
                if sum(len(b) for b in ab) == 0:        # all actor: the scene is never read, and not decoded
                    scene_rows.append(-1)
                    sb = [np.zeros((0, 4), int)] * T
                else:
                    scene_rows.append(len(decode))
                    decode.append((sv, r.scene_inds))
                actor_boxes.append(ab)
                scene_boxes.append(sb)
            scene = None
            if decode:
                self._common_size([d[0] for d in decode], 'scene')
                scene = self._decode([d[0] for d in decode], [d[1] for d in decode])
            nr = len(rand_idx)
            table = acm_plan_table([(k, nr + j, int(rows[k].flip), s, int(rows[k].scene_flip))
                                    for j, (k, s) in enumerate(zip(acm_idx, scene_rows))],
                                   actor_boxes, scene_boxes)
            counts = K.actor_cut_mix_u8(frames, scene, table, len(acm_idx), out, IMG_MEAN, IMG_STD)
            c = counts.to(torch.float64)
            # an IEEE division like the reference's foreground_area / total_area (torch turns a division by a Python scalar into a
            # multiplication by its reciprocal, which can differ in the last bit)
            fg[torch.as_tensor(acm_idx, device=dev)] = c / torch.full_like(c, float(T * S * S))
            for k, sv in zip(acm_idx, scenes):
                bg_label[k] = int(sv['label'])
        return {'imgs': out,
                'label': torch.tensor([[v['label']] for v in video_infos], dtype=torch.int64, device=dev),
                'foreground_ratio': fg,
                'background_label': torch.tensor([[x] for x in bg_label], dtype=torch.int64, device=dev),
                'frame_dir': [v['frame_dir'] for v in video_infos],
                'total_frames': torch.tensor([int(v['total_frames']) for v in video_infos], dtype=torch.int64, device=dev),
                'clip_len': torch.ones(B, dtype=torch.int64, device=dev),
                'num_clips': torch.full((B,), T, dtype=torch.int64, device=dev),
                'frame_inds': torch.from_numpy(np.stack([r.frame_inds for r in rows])).to(dev)}

    def __call__(self, video_infos: List[dict], phase: str):
        if phase != 'train':
            return super().__call__(video_infos, phase)
        W0, H0 = self._common_size(video_infos, 'sample')
        Wr, Hr = rescale_size(W0, H0, (-1, self.short_edge))
        return self.run(self.draw(video_infos, (Hr, Wr)), video_infos)


def acm_plan_table(clips, actor_boxes, scene_boxes) -> np.ndarray:
    """The int32 plan of ``bdv_actor_cut_mix_u8``: ``clips`` = per clip (out_row, actor_row, actor_flip, scene_row, scene_flip);
    ``actor_boxes`` / ``scene_boxes`` = per clip T int arrays (n, 4) of (x0, y0, x1, y1)."""
    def csr(per_clip):
        frames = [np.asarray(f, dtype=np.int64).reshape(-1, 4) for c in per_clip for f in c]
        off = np.zeros(len(frames) + 1, np.int64)
        off[1:] = np.cumsum([len(f) for f in frames])
        return off, (np.concatenate(frames) if frames else np.zeros((0, 4), np.int64))
    aoff, abox = csr(actor_boxes)
    soff, sbox = csr(scene_boxes)
    parts = [np.asarray(clips, dtype=np.int64).reshape(-1), aoff, soff, abox.reshape(-1), sbox.reshape(-1)]
    allv = np.concatenate(parts)
    if allv.size and (allv.min() < np.iinfo(np.int32).min or allv.max() > np.iinfo(np.int32).max):
        raise ValueError('acm_plan_table: a value does not fit in int32')
    return allv.astype(np.int32)
