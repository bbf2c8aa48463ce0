"""How much does a trained recognizer rely on the background?  Two measurements over validation records, both built on what the
loaders already do:

``actor_attention``      the share of the Grad-CAM map (``gradcam.GradCAM``) that falls inside the person boxes of a detection file --
                         the file the ActorCutMix loader reads -- per class and over all clips.  1 = the evidence for the label lies on the
                         actor, the boxes' share of the frame area = the map ignores where the actor is.
``scene_only_accuracy``  top-1 when every clip is replaced by its video's extracted background image (no actor in any frame), per
                         task and overall.  A high value means the scene alone gives the class away.

Neither exists in the reference or upstream; the box chain reuses ``actor_cut_mix`` (DetectionLoad, ResizeWithBox) up to the centre
crop, where the boxes stay float: this is a measurement, not the cut-out's ``.astype(int)``."""
from __future__ import annotations

import math
import os.path as osp
import pathlib
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .actor_cut_mix import detection_key, detection_load, load_detections, resize_boxes
from .background import bg_file_for
from .decode import JpegDecoder, jpeg_parse, rescale_size
from .frontend import IMG_MEAN, IMG_STD, CropFrontEnd, crop_offsets
from .gradcam import GradCAM
from .task_loop import AverageMeter, epoch_batches


def center_crop_boxes(dets: Sequence[np.ndarray], img_w: int, img_h: int, short_edge: int, crop: int) -> List[np.ndarray]:
    """Detection rows (x0, y0, x1, y1) of a ``img_w`` x ``img_h`` frame -> float boxes in the pixels of the evaluation clip:
    ``ResizeWithBox((-1, short_edge))`` (``resize_boxes``), shifted by the ``CenterCrop(crop)`` offset and clipped to the crop."""
    w1, h1 = rescale_size(img_w, img_h, (-1, short_edge))
    out = [np.array(d, dtype=d.dtype if np.issubdtype(np.asarray(d).dtype, np.floating) else np.float32).reshape(-1, 4) for d in dets]
    resize_boxes(out, img_w, img_h, w1, h1)
    (x_off, y_off, _), = crop_offsets('CenterCrop', h1, w1, crop, crop)
    for cur in out:
        cur[:, 0::2] = np.clip(cur[:, 0::2] - x_off, 0, crop)
        cur[:, 1::2] = np.clip(cur[:, 1::2] - y_off, 0, crop)
    return out


def _mean(values: Sequence[float]) -> float:
    return float(np.mean(values)) if len(values) else float('nan')


def actor_attention(model, clip_loader, records, det_file: str, target_layer: str = 'backbone.layer4', batch_size: int = 8,
                    det_thres: float = 0.4, phase: str = 'val', cam: Optional[GradCAM] = None, detections: Optional[dict] = None) -> Dict:
    """Mean ``actor_attention`` of ``GradCAM(model, target_layer)`` for the ground-truth label, over the clips ``clip_loader(infos,
    phase)`` makes of ``records`` (a ``RawFrameClipLoader`` or a subclass: its ``short_edge``, ``input_size``, file template and the
    ``frame_inds`` of its batches are read).  Boxes: ``detection_load`` on the frames ``SampleFrames(test_mode)`` picked, then
    ``center_crop_boxes``.  A video missing from the detection file raises ``KeyError`` (as ``ActorCutMixClipLoader`` does) before
    anything runs.

    -> ``{'mean', 'per_class': {label: mean}, 'clips': clips the mean rests on, 'undefined': clips without any box or with an empty
    map (left out of the means), 'values': per clip, nan where undefined}``."""
    dets = load_detections(str(det_file)) if detections is None else detections
    infos = list(records.video_infos)
    per_video = [dets[detection_key(v['frame_dir'], str(det_file))] for v in infos]          # KeyError names the video
    cam = cam if cam is not None else GradCAM(model, target_layer)
    S, sizes, values = int(clip_loader.input_size), {}, []
    for idx in epoch_batches(len(infos), batch_size, False):
        batch_infos = [infos[i] for i in idx]
        batch = clip_loader(batch_infos, phase)
        inds = batch['frame_inds'].cpu().numpy()
        boxes = []
        for k, (i, v) in enumerate(zip(idx, batch_infos)):
            d = v['frame_dir']
            if d not in sizes:
                with open(osp.join(d, clip_loader.tmpl.format(clip_loader.start_index)), 'rb') as f:
                    hdr = jpeg_parse(f.read())
                sizes[d] = (int(hdr.width), int(hdr.height))
            boxes.append(center_crop_boxes(detection_load(per_video[i], inds[k], det_thres), *sizes[d], clip_loader.short_edge, S))
        out = cam(batch['imgs'], batch['label'], boxes=boxes)
        values.extend(float(x) for x in out['actor_attention'].cpu())
    per_class: Dict[int, List[float]] = {}
    for v, a in zip(infos, values):
        if not math.isnan(a):
            per_class.setdefault(int(v['label']), []).append(a)
    good = [a for a in values if not math.isnan(a)]
    return {'mean': _mean(good), 'per_class': {c: _mean(per_class[c]) for c in sorted(per_class)}, 'clips': len(good),
            'undefined': len(values) - len(good), 'values': values}


def scene_clips(streams: Sequence[bytes], decoder: JpegDecoder, num_segments: int, short_edge: int = 256, input_size: int = 224,
                mean=IMG_MEAN, std=IMG_STD) -> torch.Tensor:
    """Background images (JPEG bytes, any sizes) -> (n, T, 3, S, S): each decoded, put through the ``val`` chain ``Resize(-1,
    short_edge)`` -> ``CenterCrop(input_size)`` -> ``Normalize`` and repeated over the T segments."""
    from . import kernels as K
    front = CropFrontEnd('CenterCrop', input_size, mean, std)
    groups: Dict[tuple, List[int]] = {}
    for i, s in enumerate(streams):
        hdr = jpeg_parse(s)
        groups.setdefault((int(hdr.height), int(hdr.width)), []).append(i)
    out = torch.empty(len(streams), num_segments, 3, input_size, input_size, dtype=torch.float32, device=decoder.device)
    for (H, W), idx in groups.items():
        imgs = decoder.decode([streams[i] for i in idx])                                        # (n, H, W, 3)
        Wr, Hr = rescale_size(W, H, (-1, short_edge))
        one = front.as_nchw(K.resize_linear_u8(imgs.unsqueeze(1), Hr, Wr))                       # (n, 1, 3, S, S)
        out[torch.as_tensor(idx, device=out.device)] = one.expand(-1, num_segments, -1, -1, -1)
    return out


def scene_only_accuracy(model, records, bg_files: Sequence[str], task_sizes: Optional[Sequence[int]] = None, num_segments: int = 8,
                        short_edge: int = 256, input_size: int = 224, batch_size: int = 8, decoder: Optional[JpegDecoder] = None,
                        device='cuda', mean=IMG_MEAN, std=IMG_STD) -> Dict:
    """Top-1 of ``model`` on clips that show only the scene: video v's clip is its background image ``bg_file_for(frame_dir)`` found by
    name among ``bg_files`` (what ``resolve_bg_files`` returned).  ``task_sizes``: the records' consecutive per-task counts (default:
    one task).  A video without a background file is counted in ``missing`` and left out of the accuracies.

    -> ``{'meter': AverageMeter of the per-task accuracies in percent (as ``task_accuracies`` makes them), 'per_task', 'overall',
    'clips', 'missing', 'missing_videos'}``."""
    infos = list(records.video_infos)
    sizes = [len(infos)] if task_sizes is None else [int(n) for n in task_sizes]
    if sum(sizes) != len(infos):
        raise ValueError(f'scene_only_accuracy: task sizes {sizes} do not add up to {len(infos)} records')
    by_name = {pathlib.Path(p).name: str(p) for p in bg_files}
    paths = [by_name.get(bg_file_for(v['frame_dir'], pathlib.Path('.')).name) for v in infos]
    present = [i for i, p in enumerate(paths) if p is not None]
    decoder = decoder if decoder is not None else JpegDecoder(device)
    correct = np.zeros(len(infos), dtype=bool)
    flags = [(m, m.training) for m in model.modules()]          # restored module by module: a mixed pattern stays mixed
    model.eval()
    try:
        with torch.no_grad():
            for lo in range(0, len(present), batch_size):
                idx = present[lo:lo + batch_size]
                streams = []
                for i in idx:
                    with open(paths[i], 'rb') as f:
                        streams.append(f.read())
                imgs = scene_clips(streams, decoder, num_segments, short_edge, input_size, mean, std)
                pred = model(imgs, return_loss=False).argmax(dim=1).cpu().numpy()
                correct[idx] = pred == np.array([int(infos[i]['label']) for i in idx])
    finally:
        for m, t in flags:
            m.training = t
    have = np.zeros(len(infos), dtype=bool)
    have[present] = True
    meter, start = AverageMeter(), 0
    for n in sizes:
        k = int(have[start:start + n].sum())
        meter.update(float(correct[start:start + n][have[start:start + n]].mean()) * 100 if k else float('nan'), k)
        start += n
    total = int(have.sum())
    return {'meter': meter, 'per_task': list(meter.values), 'overall': float(correct[have].mean()) * 100 if total else float('nan'),
            'clips': total, 'missing': len(infos) - total, 'missing_videos': [infos[i]['frame_dir'] for i in range(len(infos)) if not have[i]]}


def overlay_strip(overlay_clip: torch.Tensor) -> torch.Tensor:
    """(T, H, W, 3) uint8 overlay of one clip -> the (H, T*W, 3) image written per clip: its frames side by side."""
    T, H, W, _ = overlay_clip.shape
    return overlay_clip.permute(1, 0, 2, 3).reshape(H, T * W, 3).contiguous()
