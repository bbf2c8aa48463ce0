"""Background extraction on the GPU: what ``BackgroundMixDataset.__init__`` does with
``extract_bg_if_not_found=True`` (libs/loader/comix_loader.py:60-100) -- map every video to ``bg_dir/<frame_dir name>.jpg`` and
make each missing one with ``bg_extraction_tmf`` (:148-164): decode every file of the frame directory, take the per-pixel
``np.median`` over time, ``.astype(np.uint8)``, ``cv2.imwrite`` (baseline JPEG, libjpeg-turbo defaults: quality 95, 4:2:0).

Here the frames are decoded by ``JpegDecoder`` (bit-exact with libjpeg-turbo), the median runs as one launch for a batch of videos
(``bdv_temporal_median_u8``), the JPEG forward stage -- colour conversion, downsampling, DCT, quantisation -- as one more
(``bdv_jpeg_forward_u8``), and the Huffman stage on host threads (``bdv_jpeg_entropy_encode_batch``): the written bytes are
libjpeg-turbo's.  The reference works in BGR (cv2) and returns the BGR median; per-channel medians and the colour conversion of
the encoder make the file the same, and the arrays returned here are RGB.

``method='sim_cam'`` is the other extraction of the reference, ``sim_cam_motion_bg_extract`` (cil_tools/extract_background.py:78-99),
for videos shot with a moving camera: the sorted files of the directory but the last, every ``interval``-th, at most ``max_frames``;
each frame as a float image through torchvision's ``RandomResizedCrop(size=100)``; exact zeros become NaN; ``np.nanmedian`` or
``np.nanmean`` over time; ``.astype(np.uint8)``; written as it is (the reference's BGR2RGB before ``cv2.imwrite`` undoes imwrite's
own channel swap).  Here: one crop launch (``bdv_resized_crop_f32``) and one reduce launch (``bdv_temporal_nanreduce_f32``) per batch
of videos.  The box draws restate UPSTREAM torchvision ``RandomResizedCrop.get_params`` from its published behaviour -- parity
unpinned: torchvision is not importable here (its version is not pinned by the reference either); the resampling follows ATen's
bilinear kernels, which torchvision calls, and is pinned by ``torch.nn.functional.interpolate`` on the CPU."""
from __future__ import annotations

import ctypes
import math
import os
import pathlib
import tempfile
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import JpegInfo, check, lib

DEFAULT_QUALITY = 95                    # cv2.IMWRITE_JPEG_QUALITY's default
MAX_BATCH_BYTES = 2 << 30               # device bytes of decoded frames per extraction launch
METHODS = ('tmf', 'sim_cam', 'person_masked')   # --method of cil_tools/extract_background.py, and the detection-file median
AVG_METHODS = ('median', 'mean')        # --avg_method (sim_cam only: bg_extraction_tmf ignores it)
SIM_CAM_SIZE = 100                      # RandomResizedCrop(size=100), extract_background.py:82
SIM_CAM_MAX_FRAMES = 500                # --max_frames' default
FILENAME_TMPL = 'img_{:05}.jpg'         # person_masked: the RGB frames of a directory (RawframeDataset's default)
REPORT_NAME = 'person_masked_report.json'
# person_masked's own keywords and their defaults (extract_backgrounds; data.train.bg_extraction; tools/extract_background.py)
PERSON_MASKED_DEFAULTS = dict(det_file=None, det_thres=0.4, dilate=0.1, min_visible=1, max_hole_fraction=None, filename_tmpl=FILENAME_TMPL)


def _device(device) -> torch.device:
    return torch.device(device if device is not None else 'cuda')


def encode_info(width: int, height: int, quality: int = DEFAULT_QUALITY) -> JpegInfo:
    """Geometry of the 4:2:0 stream the encoder writes for this size, and its quantisation tables (``jpeg_set_quality``)."""
    info = JpegInfo()
    check(lib().bdv_jpeg_encode_info(int(width), int(height), int(quality), ctypes.byref(info)), 'bdv_jpeg_encode_info')
    return info


def jpeg_forward(images_u8: torch.Tensor, quality: int = DEFAULT_QUALITY) -> torch.Tensor:
    """Device stage of the encoder: ``(B, H, W, 3)`` uint8 RGB on the GPU -> ``(B, coef_count)`` int16 quantised coefficients in
    the layout ``bdv_jpeg_entropy_decode`` produces."""
    from .kernels import _p, _stream
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3 or not images_u8.is_cuda:
        raise ValueError(f'jpeg_forward: expected a (B, H, W, 3) uint8 CUDA tensor, got {tuple(images_u8.shape)} {images_u8.dtype}')
    images_u8 = images_u8.contiguous()
    B, H, W = int(images_u8.shape[0]), int(images_u8.shape[1]), int(images_u8.shape[2])
    info = encode_info(W, H, quality)
    coefs = torch.empty(B, info.coef_count, dtype=torch.int16, device=images_u8.device)
    check(lib().bdv_jpeg_forward_u8(_p(images_u8), B, H, W, int(quality), _p(coefs), _stream()), 'bdv_jpeg_forward_u8')
    return coefs


def entropy_encode(coefs: np.ndarray, width: int, height: int, quality: int = DEFAULT_QUALITY, threads: int = 8) -> List[bytes]:
    """Host stage of the encoder: ``(n, coef_count)`` int16 coefficients -> n JPEG files (bytes)."""
    coefs = np.ascontiguousarray(coefs, dtype=np.int16)
    if coefs.ndim == 1:
        coefs = coefs[None]
    n = int(coefs.shape[0])
    if coefs.shape[1] != encode_info(width, height, quality).coef_count:
        raise ValueError(f'entropy_encode: {coefs.shape[1]} coefficients per image do not fit a {width} x {height} image')
    stride = int(lib().bdv_jpeg_encode_bound(int(width), int(height)))
    out = np.empty(n * stride, dtype=np.uint8)
    sizes = (ctypes.c_size_t * n)()
    check(lib().bdv_jpeg_entropy_encode_batch(coefs.ctypes.data, n, int(width), int(height), int(quality), out.ctypes.data, stride,
                                              ctypes.cast(sizes, ctypes.c_void_p), max(1, min(int(threads), 256))),
          'bdv_jpeg_entropy_encode_batch')
    return [out[i * stride:i * stride + sizes[i]].tobytes() for i in range(n)]


def encode_jpeg(images_u8, quality: int = DEFAULT_QUALITY, device=None, threads: int = 8) -> List[bytes]:
    """``cv2.imwrite``'s bytes for each image (RGB here, BGR there): a ``(B, H, W, 3)`` uint8 tensor / array, or a sequence of
    ``(H, W, 3)`` images of any sizes (encoded size group by size group).  Quality 25..100 (else ``RuntimeError``)."""
    whole = isinstance(images_u8, (torch.Tensor, np.ndarray)) and images_u8.ndim == 4
    images = images_u8 if whole else list(images_u8)
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i in range(len(images)):
        im = images[i]
        if im.ndim != 3 or im.shape[2] != 3:
            raise ValueError(f'encode_jpeg: image {i} has shape {tuple(im.shape)}, expected (H, W, 3)')
        groups.setdefault((int(im.shape[0]), int(im.shape[1])), []).append(i)
    on_gpu = isinstance(images_u8, torch.Tensor) and images_u8.is_cuda
    dev = _device(device if device is not None else (images_u8.device if on_gpu else None))
    out: List[bytes] = [b''] * len(images)
    for (H, W), idx in groups.items():
        batch = torch.as_tensor(images) if whole else torch.stack([torch.as_tensor(images[i]) for i in idx])
        if batch.dtype != torch.uint8:
            raise ValueError(f'encode_jpeg: expected uint8 images, got {batch.dtype}')
        coefs = jpeg_forward(batch.to(dev), quality)
        for i, data in zip(idx, entropy_encode(coefs.cpu().numpy(), W, H, quality, threads)):
            out[i] = data
    return out


def temporal_median(frames_u8, counts: Sequence[int], device=None) -> torch.Tensor:
    """``np.median(frames_v, axis=0).astype(np.uint8)`` for every video v of a ragged batch: ``frames_u8`` ``(sum(counts), H, W, 3)``
    uint8 (tensor or array; the videos' frames back to back), ``counts`` the frames per video -> ``(V, H, W, 3)`` uint8 on the device."""
    from .kernels import _p, _stream, _video_runs
    counts = [int(c) for c in counts]
    frames = torch.as_tensor(frames_u8)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f'temporal_median: expected (F, H, W, 3) uint8 frames, got {tuple(frames.shape)} {frames.dtype}')
    if not counts or min(counts) < 1 or sum(counts) != frames.shape[0]:
        raise ValueError(f'temporal_median: frame counts {counts} do not partition {frames.shape[0]} frames')
    dev = frames.device if frames.is_cuda else _device(device)
    frames = frames.to(dev).contiguous()
    V, H, W = len(counts), int(frames.shape[1]), int(frames.shape[2])
    first_h, counts_h, first_d, counts_d = _video_runs(counts, dev)
    out = torch.empty(V, H, W, 3, dtype=torch.uint8, device=dev)
    check(lib().bdv_temporal_median_u8(_p(frames), int(frames.shape[0]), _p(first_d), _p(counts_d), first_h.data_ptr(), counts_h.data_ptr(),
                                       V, H, W, _p(out), _stream()), 'bdv_temporal_median_u8')
    return out


def person_box_table(per_video_detections, frame_numbers, img_w: int, img_h: int, det_thres: float = 0.4,
                     dilate: float = 0.1) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The person boxes of one video's frames as the CSR table ``temporal_masked_median`` takes: ``(box_first (n + 1,) int32, boxes
    (nb, 4) int32, have_entry (n,) bool)`` for the n ``frame_numbers``.

    ``per_video_detections`` is a video's value in the ActorCutMix detection file: per frame an array of ``(x0, y0, x1, y1, score)``
    rows.  Frame number i reads entry i, ``detection_load``'s indexing with the 1-based file numbers (entry 0 is never read), so a
    detection file means the same here as in ``ActorCutMixClipLoader``; the rows with ``score > det_thres`` (strict) are kept.  Each
    kept box grows, in float64, by ``dilate`` times its own width on the left and on the right and ``dilate`` times its height above
    and below, then ``floor`` for x0 / y0 and ``ceil`` for x1 / y1 -- a partly covered pixel counts as covered -- clipped to the
    ``img_w`` x ``img_h`` frame; a box left empty is dropped.  A frame number past the end of the list (or negative) has no rows
    and ``have_entry`` False: nothing is known about it, which is not the same as an entry without boxes."""
    numbers = [int(i) for i in np.asarray(frame_numbers).reshape(-1)]
    n_entries = len(per_video_detections)
    have = np.zeros(len(numbers), dtype=bool)
    box_first = np.zeros(len(numbers) + 1, dtype=np.int32)
    rows: List[np.ndarray] = []
    total = 0
    for k, i in enumerate(numbers):
        if 0 <= i < n_entries:
            have[k] = True
            cur = np.asarray(per_video_detections[i], dtype=np.float64)
            if cur.size:
                cur = cur.reshape(-1, cur.shape[-1])
                b = cur[cur[:, -1] > det_thres, :4]
                w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
                x0 = np.clip(np.floor(b[:, 0] - dilate * w), 0, img_w)
                y0 = np.clip(np.floor(b[:, 1] - dilate * h), 0, img_h)
                x1 = np.clip(np.ceil(b[:, 2] + dilate * w), 0, img_w)
                y1 = np.clip(np.ceil(b[:, 3] + dilate * h), 0, img_h)
                keep = (x1 > x0) & (y1 > y0)
                if keep.any():
                    rows.append(np.stack([x0, y0, x1, y1], 1)[keep].astype(np.int32))
                    total += int(keep.sum())
        box_first[k + 1] = total
    boxes = np.concatenate(rows) if rows else np.zeros((0, 4), dtype=np.int32)
    return box_first, boxes, have


def temporal_masked_median(frames_u8, counts: Sequence[int], box_first, boxes, min_visible: int = 1,
                           device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The person-masked median of a ragged batch (``bdv_temporal_masked_median_u8``): ``frames_u8`` / ``counts`` as for
    ``temporal_median``; ``box_first`` ``(sum(counts) + 1,)`` and ``boxes`` ``(nb, 4)`` the CSR table of half-open ``x0, y0, x1, y1``
    boxes per frame of the batch (``person_box_table`` per video, concatenated).  Returns ``(out (V, H, W, 3) uint8, visible (V, H, W)
    uint16)`` on the device: ``visible`` counts the video's frames in which no box covers the pixel; ``out`` is ``np.median`` over
    those frames, ``.astype(np.uint8)``, where there are at least ``min_visible`` of them and ``temporal_median``'s value elsewhere
    (a hole).  Everything is checked on the host first (``ValueError``, nothing launched)."""
    from . import kernels as K
    counts = [int(c) for c in counts]
    frames = torch.as_tensor(frames_u8)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f'temporal_masked_median: expected (F, H, W, 3) uint8 frames, got {tuple(frames.shape)} {frames.dtype}')
    if not counts or min(counts) < 1 or max(counts) > 65535 or sum(counts) != frames.shape[0]:
        raise ValueError(f'temporal_masked_median: frame counts {counts} do not partition {frames.shape[0]} frames (1..65535 per video)')
    if int(min_visible) < 1:
        raise ValueError(f'temporal_masked_median: min_visible {min_visible} (at least 1)')
    H, W = int(frames.shape[1]), int(frames.shape[2])
    bf = np.asarray(box_first.cpu() if isinstance(box_first, torch.Tensor) else box_first, dtype=np.int64).reshape(-1)
    bx = np.asarray(boxes.cpu() if isinstance(boxes, torch.Tensor) else boxes, dtype=np.int64).reshape(-1, 4)
    if bf.shape[0] != frames.shape[0] + 1:
        raise ValueError(f'temporal_masked_median: box_first has {bf.shape[0]} entries, expected {frames.shape[0] + 1} (frames + 1)')
    if bf[0] != 0 or bf[-1] != bx.shape[0] or (np.diff(bf) < 0).any():
        raise ValueError(f'temporal_masked_median: box_first must rise from 0 to the {bx.shape[0]} box rows without decreasing')
    if bx.shape[0] and ((bx[:, 0] < 0).any() or (bx[:, 0] > bx[:, 2]).any() or (bx[:, 2] > W).any() or
                        (bx[:, 1] < 0).any() or (bx[:, 1] > bx[:, 3]).any() or (bx[:, 3] > H).any()):
        raise ValueError(f'temporal_masked_median: a box is not 0 <= x0 <= x1 <= {W}, 0 <= y0 <= y1 <= {H}')
    dev = frames.device if frames.is_cuda else _device(device)
    return K.temporal_masked_median_u8(frames.to(dev).contiguous(), counts, bf.astype(np.int32), bx.astype(np.int32), int(min_visible))


def hole_fractions(visible: torch.Tensor, min_visible: int = 1) -> List[float]:
    """Per video the share of pixels with ``visible < min_visible`` (``visible`` as ``temporal_masked_median`` returns it), counted
    on the device."""
    V = int(visible.shape[0])
    lo_hi = visible.contiguous().view(torch.uint8).view(V, -1, 2).to(torch.int32)       # uint16 as its two bytes
    holes = ((lo_hi[..., 0] + 256 * lo_hi[..., 1]) < int(min_visible)).sum(1)
    return [int(h) / (visible.shape[1] * visible.shape[2]) for h in holes.cpu().tolist()]


def template_frame_files(frame_dir, filename_tmpl: str = FILENAME_TMPL) -> List[Tuple[int, pathlib.Path]]:
    """``(number, path)`` of the directory's files named ``filename_tmpl.format(number)``, by number: the RGB frames as the datasets
    address them.  Flow frames (``flow_x_00001.jpg``) and anything else are left out."""
    import re
    d = pathlib.Path(frame_dir)
    if not d.is_dir():
        raise FileNotFoundError(f'extract_background: {d} is not a directory')
    m = re.fullmatch(r'([^{}]*)\{[^{}]*\}([^{}]*)', filename_tmpl)
    if m is None:
        raise ValueError(f'extract_background: filename_tmpl {filename_tmpl!r} must hold exactly one format field')
    name = re.compile(re.escape(m.group(1)) + r'(\d+)' + re.escape(m.group(2)))
    found = []
    for p in d.iterdir():
        hit = name.fullmatch(p.name)
        if hit and p.is_file() and filename_tmpl.format(int(hit.group(1))) == p.name:
            found.append((int(hit.group(1)), p))
    return sorted(found)


def sim_cam_frame_files(frame_dir, interval: int = 1, max_frames: int = SIM_CAM_MAX_FRAMES) -> List[pathlib.Path]:
    """The frames ``sim_cam_motion_bg_extract`` reads (extract_background.py:83-89): ``sorted(glob('*'))[:-1:interval]`` -- the last
    file is always left out -- cut off after ``max_frames``.  A directory that yields no frame (a single file) raises ``ValueError``."""
    d = pathlib.Path(frame_dir)
    if not d.is_dir():
        raise FileNotFoundError(f'extract_background: {d} is not a directory')
    if int(interval) < 1 or int(max_frames) < 1:
        raise ValueError(f'extract_background: interval {interval} and max_frames {max_frames} must be positive')
    files = sorted(d.glob('*'))[:-1:int(interval)][:int(max_frames)]
    if not files:
        raise ValueError(f'extract_background: {d} yields no frames (sim_cam leaves the last file of a directory out)')
    return files


def random_resized_crop_boxes(n: int, height: int, width: int, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), draws=None) -> np.ndarray:
    """``n`` boxes ``[top, left, h, w]`` (int32) as UPSTREAM torchvision ``RandomResizedCrop.get_params`` draws them for ``n`` frames
    of ``height x width``, one frame after the other (parity unpinned, see the module docstring).  Per frame up to 10 attempts, each
    two uniform draws on the torch generator -- the area fraction in ``scale``, then the log of the aspect ratio between the float32
    logs of ``ratio`` -- ``w = round(sqrt(area * aspect))``, ``h = round(sqrt(area / aspect))``; the first pair that fits the frame
    is placed with ``randint(0, height - h + 1)`` then ``randint(0, width - w + 1)``.  After 10 misses no further draw is made: the
    frame is cut to the nearest allowed aspect ratio and the box centred.  ``draws``: a ``decode.Draws`` bundle or a seed; ``None`` =
    torch's global generator."""
    from .decode import Draws
    d = Draws.of(draws)
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError(f'random_resized_crop_boxes: bad frame size {height} x {width}')
    log_ratio = torch.log(torch.tensor([float(ratio[0]), float(ratio[1])]))
    lo, hi = float(log_ratio[0]), float(log_ratio[1])
    area = height * width
    boxes = np.empty((int(n), 4), dtype=np.int32)
    for k in range(int(n)):
        for _ in range(10):
            target_area = area * torch.empty(1).uniform_(float(scale[0]), float(scale[1]), generator=d.torch).item()
            aspect = torch.exp(torch.empty(1).uniform_(lo, hi, generator=d.torch)).item()
            w = int(round(math.sqrt(target_area * aspect)))
            h = int(round(math.sqrt(target_area / aspect)))
            if 0 < w <= width and 0 < h <= height:
                top = d.randint(height - h + 1)
                left = d.randint(width - w + 1)
                break
        else:
            in_ratio = float(width) / float(height)
            if in_ratio < min(ratio):
                w = width
                h = int(round(w / min(ratio)))
            elif in_ratio > max(ratio):
                h = height
                w = int(round(h * max(ratio)))
            else:
                w, h = width, height
            top, left = (height - h) // 2, (width - w) // 2
        boxes[k] = (top, left, h, w)
    return boxes


def _size_hw(size) -> Tuple[int, int]:
    hw = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if min(hw) < 1:
        raise ValueError(f'resized_crop: bad output size {size}')
    return hw


def resized_crop(frames_u8, boxes, size=SIM_CAM_SIZE, antialias: bool = False, device=None) -> torch.Tensor:
    """torchvision's ``resized_crop`` of float frames, bilinear: ``frames_u8`` ``(F, H, W, 3)`` uint8 (tensor or array), ``boxes``
    ``(F, 4)`` ``[top, left, h, w]`` -> ``(F, size_h, size_w, 3)`` fp32 pixel values on the device.  ``antialias=False`` is the
    torchvision of the reference's era (tensors were not antialiased), ``True`` the current default."""
    from . import kernels as K
    frames = torch.as_tensor(frames_u8)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f'resized_crop: expected (F, H, W, 3) uint8 frames, got {tuple(frames.shape)} {frames.dtype}')
    b = np.asarray(boxes.cpu() if isinstance(boxes, torch.Tensor) else boxes, dtype=np.int64).reshape(-1, 4)
    H, W = int(frames.shape[1]), int(frames.shape[2])
    if b.shape[0] != frames.shape[0]:
        raise ValueError(f'resized_crop: {b.shape[0]} boxes for {frames.shape[0]} frames')
    if b.shape[0] and ((b[:, :2] < 0).any() or (b[:, 2:] < 1).any() or (b[:, 0] + b[:, 2] > H).any() or (b[:, 1] + b[:, 3] > W).any()):
        raise ValueError(f'resized_crop: a box leaves the {H} x {W} frame')
    dev = frames.device if frames.is_cuda else _device(device)
    sh, sw = _size_hw(size)
    return K.resized_crop_f32(frames.to(dev).contiguous(), b.astype(np.int32), sh, sw, bool(antialias))


def temporal_nanreduce(frames_f32, counts: Sequence[int], avg_method: str = 'median', zero_is_missing: bool = True, device=None) -> torch.Tensor:
    """``np.nanmedian(frames_v, axis=0).astype(np.uint8)`` (or ``np.nanmean``) for every video v of a ragged batch, after
    ``frames_v[frames_v == 0] = nan`` when ``zero_is_missing``: ``frames_f32`` ``(sum(counts), ...)`` fp32 (tensor or array; the
    videos' frames back to back) -> ``(V, ...)`` uint8 on the device.  A position missing in every frame gives 0."""
    from . import kernels as K
    if avg_method not in AVG_METHODS:
        raise ValueError(f'temporal_nanreduce: avg_method {avg_method!r} (one of {AVG_METHODS})')
    counts = [int(c) for c in counts]
    frames = torch.as_tensor(frames_f32)
    if frames.dtype != torch.float32 or frames.dim() < 2:
        raise ValueError(f'temporal_nanreduce: expected (F, ...) float32 frames, got {tuple(frames.shape)} {frames.dtype}')
    if not counts or min(counts) < 1 or max(counts) > 65535 or sum(counts) != frames.shape[0]:
        raise ValueError(f'temporal_nanreduce: frame counts {counts} do not partition {frames.shape[0]} frames (1..65535 per video)')
    dev = frames.device if frames.is_cuda else _device(device)
    return K.temporal_nanreduce_f32(frames.to(dev).contiguous(), counts, AVG_METHODS.index(avg_method), bool(zero_is_missing))


def _frame_files(frame_dir: pathlib.Path) -> List[pathlib.Path]:
    """Every regular file of the directory, as the reference's ``data_path.glob('*')`` (flow frames included); sorted, which the
    median does not see."""
    if not frame_dir.is_dir():
        raise FileNotFoundError(f'extract_background: {frame_dir} is not a directory')
    files = sorted(p for p in frame_dir.glob('*') if p.is_file())
    if not files:
        raise ValueError(f'extract_background: {frame_dir} holds no frames')
    return files


def _read_frames(frame_dir: pathlib.Path, files: Optional[List[pathlib.Path]] = None) -> Tuple[List[bytes], Tuple[int, int]]:
    from .decode import jpeg_parse
    streams, size = [], None
    for p in (files if files is not None else _frame_files(frame_dir)):
        data = p.read_bytes()
        try:
            info = jpeg_parse(data)
        except RuntimeError as e:
            raise ValueError(f'extract_background: {p}: not a JPEG frame the decoder covers ({e})') from None
        if size is None:
            size, size_file = (info.height, info.width), p
        elif (info.height, info.width) != size:
            raise ValueError(f'extract_background: {p} is {info.width} x {info.height}, but {size_file} is {size[1]} x {size[0]} '
                             f'(frames of {frame_dir} must share one size)')
        streams.append(data)
    return streams, size


def _write_atomic(dest: pathlib.Path, data: bytes) -> None:
    """A temporary file in the destination's directory, then ``os.replace``: an interrupted run never leaves a truncated file that
    a later run would take as found."""
    fd, tmp = tempfile.mkstemp(prefix='.' + dest.name + '.', suffix='.tmp', dir=str(dest.parent))
    try:
        with os.fdopen(fd, 'wb') as f:
            f.write(data)
        os.replace(tmp, dest)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


def _check_method(method: str, avg_method: str, interval: int, max_frames: int, det_file=None, det_thres: float = 0.4,
                  dilate: float = 0.1, min_visible: int = 1, max_hole_fraction=None, filename_tmpl: str = FILENAME_TMPL,
                  report=None) -> None:
    if method not in METHODS:
        raise ValueError(f'extract_background: method {method!r} (one of {METHODS})')
    if avg_method not in AVG_METHODS:
        raise ValueError(f'extract_background: avg_method {avg_method!r} (one of {AVG_METHODS})')
    if method != 'sim_cam' and (avg_method != 'median' or int(interval) != 1 or int(max_frames) != SIM_CAM_MAX_FRAMES):
        raise ValueError(f"extract_background: method {method!r} is the median of every frame it takes; avg_method, interval and "
                         "max_frames belong to method 'sim_cam'")
    given = dict(det_file=det_file, det_thres=det_thres, dilate=dilate, min_visible=min_visible, max_hole_fraction=max_hole_fraction,
                 filename_tmpl=filename_tmpl)
    if method != 'person_masked':
        extra = [k for k, v in given.items() if v != PERSON_MASKED_DEFAULTS[k]] + (['report'] if report is not None else [])
        if extra:
            raise ValueError(f"extract_background: {', '.join(extra)} belong{'s' if len(extra) == 1 else ''} to method 'person_masked', "
                             f"not {method!r}")
        return
    if not det_file:
        raise ValueError("extract_background: method 'person_masked' needs det_file, the ActorCutMix detection file")
    if int(min_visible) < 1:
        raise ValueError(f'extract_background: min_visible {min_visible} (at least 1)')
    if not float(dilate) >= 0.0:
        raise ValueError(f'extract_background: dilate {dilate} (a non-negative share of the box size)')
    if max_hole_fraction is not None and not 0.0 <= float(max_hole_fraction) <= 1.0:
        raise ValueError(f'extract_background: max_hole_fraction {max_hole_fraction} (None, or 0..1)')
    if report is not None and not isinstance(report, list):
        raise ValueError('extract_background: report must be a list (one dict per job is appended)')


def _person_masked_plan(jobs, detections, det_file: str, filename_tmpl: str) -> List[tuple]:
    """Per job ``(numbers, files, frames_without_entry, detections of the video)`` of the frames that have a detection entry.  Every
    job is checked here, before any of them is decoded or written: a video the detection file does not list, or without a usable
    frame, raises ``ValueError`` naming it."""
    from .actor_cut_mix import detection_key
    plan = []
    for d, _ in jobs:
        key = detection_key(str(d).rstrip('/'), det_file)
        if key not in detections:
            raise ValueError(f'extract_background: video {key!r} ({d}) is not in the detection file {det_file}')
        dets = detections[key]
        found = template_frame_files(d, filename_tmpl)
        usable = [(i, p) for i, p in found if 0 <= i < len(dets)]
        if not usable:
            raise ValueError(f'extract_background: {d} has no frame named {filename_tmpl!r} with an entry in the detection file '
                             f'({len(found)} frames, {len(dets)} entries for {key!r})')
        plan.append(([i for i, _ in usable], [p for _, p in usable], len(found) - len(usable), dets))
    return plan


def extract_backgrounds(jobs: Sequence[Tuple[str, str]], decoder=None, quality: int = DEFAULT_QUALITY,
                        max_batch_bytes: int = MAX_BATCH_BYTES, return_arrays: bool = False, method: str = 'tmf',
                        avg_method: str = 'median', interval: int = 1, max_frames: int = SIM_CAM_MAX_FRAMES, size=SIM_CAM_SIZE,
                        antialias: bool = False, draws=None, det_file=None, det_thres: float = 0.4, dilate: float = 0.1,
                        min_visible: int = 1, max_hole_fraction: Optional[float] = None, filename_tmpl: str = FILENAME_TMPL,
                        report: Optional[list] = None) -> Optional[List[np.ndarray]]:
    """``bg_extraction_tmf`` for many ``(frame_dir, dest)`` pairs: videos of one frame size are batched into one median launch, one
    forward-stage launch and one threaded Huffman call, up to ``max_batch_bytes`` of decoded frames per batch (a single longer video
    is a batch of its own).  A frame directory that fails its checks raises before its file is written.

    ``method='sim_cam'``: ``sim_cam_motion_bg_extract`` instead (see the module docstring) -- per batch decode, one crop launch, one
    reduce launch (``avg_method`` 'median' | 'mean'), encode, write; a video's share of the budget is its selected frames plus their
    fp32 crops.  The crop boxes are drawn video by video in job order from ``draws`` (a ``decode.Draws`` bundle or a seed; ``None`` =
    torch's global generator); ``size`` (int or ``(h, w)``) and ``antialias`` as in ``resized_crop``.

    ``method='person_masked'``: person-free backgrounds from the ActorCutMix detection file ``det_file``, the stand-in for the
    reference's Mask-RCNN filter (cil_tools/type_b_and_c_bg.py).  The frames are the directory's files named by ``filename_tmpl``
    (flow frames and strays are left out) whose number has an entry in the video's detection list (``detection_key`` names the video;
    a frame without an entry is left out and counted -- unknown is not empty); per batch decode, one ``temporal_masked_median`` launch
    over the boxes of ``person_box_table(det_thres, dilate)`` with ``min_visible``, encode, write.  One dict per job is appended to
    ``report`` (a list): ``frame_dir``, ``dest``, ``frames``, ``frames_without_entry``, ``boxes``, ``hole_fraction`` (the share of
    pixels seen uncovered in fewer than ``min_visible`` frames) and ``written``.  With ``max_hole_fraction`` a video above it is not
    written (its array is still returned): a person who never moved leaves holes, and such a background cannot be certified
    person-free.  A video missing from the detection file, or without a usable frame, raises ``ValueError`` naming it before any
    file of the call is written."""
    from .decode import Draws, JpegDecoder
    _check_method(method, avg_method, interval, max_frames, det_file, det_thres, dilate, min_visible, max_hole_fraction, filename_tmpl,
                  report)
    decoder = decoder if decoder is not None else JpegDecoder('cuda')
    results: Optional[List[np.ndarray]] = [None] * len(jobs) if return_arrays else None
    pending: Dict[Tuple[int, int], List[tuple]] = {}
    if method == 'sim_cam':
        draws = Draws.of(draws)
        sh, sw = _size_hw(size)

        def flush(batch, H, W):
            _extract_batch_sim_cam(batch, H, W, decoder, quality, results, (sh, sw), antialias, avg_method)
    elif method == 'person_masked':
        from .actor_cut_mix import load_detections
        plan = _person_masked_plan(jobs, load_detections(str(det_file)), str(det_file), filename_tmpl)
        rows: List[Optional[dict]] = [None] * len(jobs)

        def flush(batch, H, W):
            _extract_batch_person_masked(batch, H, W, decoder, quality, results, int(min_visible), max_hole_fraction, rows)
    else:
        def flush(batch, H, W):
            _extract_batch(batch, H, W, decoder, quality, results)
    for pos, (d, dest) in enumerate(jobs):
        if method == 'sim_cam':
            streams, (H, W) = _read_frames(pathlib.Path(d), sim_cam_frame_files(d, interval, max_frames))
            item = (pathlib.Path(dest), streams, pos, random_resized_crop_boxes(len(streams), H, W, draws=draws))
            per_frame = H * W * 3 + sh * sw * 3 * 4
        elif method == 'person_masked':
            numbers, files, without, dets = plan[pos]
            streams, (H, W) = _read_frames(pathlib.Path(d), files)
            box_first, boxes, _ = person_box_table(dets, numbers, W, H, det_thres, dilate)
            rows[pos] = dict(frame_dir=str(d), dest=str(dest), frames=len(streams), frames_without_entry=without, boxes=int(len(boxes)),
                             hole_fraction=None, written=False)
            item = (pathlib.Path(dest), streams, pos, box_first, boxes)
            per_frame = H * W * 3
        else:
            streams, (H, W) = _read_frames(pathlib.Path(d))
            item = (pathlib.Path(dest), streams, pos)
            per_frame = H * W * 3
        batch = pending.setdefault((H, W), [])
        if batch and (sum(len(it[1]) for it in batch) + len(streams)) * per_frame > max_batch_bytes:
            flush(batch, H, W)
            batch.clear()
        batch.append(item)
    for (H, W), batch in pending.items():
        if batch:
            flush(batch, H, W)
    if method == 'person_masked' and report is not None:
        report.extend(rows)
    return results


def _decode_items(items, H, W, decoder) -> torch.Tensor:
    frames = torch.empty(sum(len(it[1]) for it in items), H, W, 3, dtype=torch.uint8, device=decoder.device)
    at = 0
    for it in items:
        for s in range(0, len(it[1]), 256):                  # bounded staging buffers for the coefficient upload
            part = it[1][s:s + 256]
            frames[at:at + len(part)] = decoder.decode(part)
            at += len(part)
    return frames


def _write_items(items, images, decoder, quality, results) -> None:
    files = encode_jpeg(images, quality, threads=decoder.threads)
    host = images.cpu().numpy() if results is not None else None
    for k, (it, data) in enumerate(zip(items, files)):
        it[0].parent.mkdir(parents=True, exist_ok=True)
        _write_atomic(it[0], data)
        if results is not None:
            results[it[2]] = host[k]


def _extract_batch(items, H, W, decoder, quality, results):
    frames = _decode_items(items, H, W, decoder)
    med = temporal_median(frames, [len(it[1]) for it in items])
    del frames
    _write_items(items, med, decoder, quality, results)


def _extract_batch_sim_cam(items, H, W, decoder, quality, results, size, antialias, avg_method):
    frames = _decode_items(items, H, W, decoder)
    crops = resized_crop(frames, np.concatenate([it[3] for it in items]), size, antialias)
    del frames
    bg = temporal_nanreduce(crops, [len(it[1]) for it in items], avg_method, zero_is_missing=True)
    del crops
    _write_items(items, bg, decoder, quality, results)


def _extract_batch_person_masked(items, H, W, decoder, quality, results, min_visible, max_hole_fraction, rows):
    frames = _decode_items(items, H, W, decoder)
    box_first, at = [np.zeros(1, dtype=np.int32)], 0
    for it in items:
        box_first.append(it[3][1:] + at)
        at += int(it[3][-1])
    bg, visible = temporal_masked_median(frames, [len(it[1]) for it in items], np.concatenate(box_first),
                                         np.concatenate([it[4] for it in items]), min_visible)
    del frames
    keep = []
    for k, (it, hf) in enumerate(zip(items, hole_fractions(visible, min_visible))):
        rows[it[2]]['hole_fraction'] = hf
        if max_hole_fraction is None or hf <= float(max_hole_fraction):
            rows[it[2]]['written'] = True
            keep.append(k)
    if results is not None:
        host = bg.cpu().numpy()
        for k, it in enumerate(items):
            results[it[2]] = host[k]
    if keep:
        _write_items([items[k] for k in keep], bg[torch.as_tensor(keep, device=bg.device)], decoder, quality, None)


def extract_background(frame_dir, dest, decoder=None, quality: int = DEFAULT_QUALITY, method: str = 'tmf', avg_method: str = 'median',
                       interval: int = 1, max_frames: int = SIM_CAM_MAX_FRAMES, size=SIM_CAM_SIZE, antialias: bool = False,
                       draws=None, **person_masked) -> np.ndarray:
    """``bg_extraction_tmf(data_path, dest)``: the median frame of every file of ``frame_dir``, written to ``dest`` as JPEG;
    returns it as an ``(H, W, 3)`` uint8 RGB array.  ``method='sim_cam'``: ``sim_cam_motion_bg_extract`` with the keywords of
    ``extract_backgrounds``; returns the ``(size_h, size_w, 3)`` image.  ``method='person_masked'`` takes ``det_file`` and the other
    keywords of ``extract_backgrounds`` (``person_masked``)."""
    return extract_backgrounds([(str(frame_dir), str(dest))], decoder, quality, return_arrays=True, method=method, avg_method=avg_method,
                               interval=interval, max_frames=max_frames, size=size, antialias=antialias, draws=draws, **person_masked)[0]


def bg_file_for(frame_dir: str, bg_dir: pathlib.Path, bg_image_extension: str = '.jpg') -> pathlib.Path:
    """``(bg_dir / Path(frame_dir).name).with_suffix(ext)`` -- with the reference's quirk: a dotted directory name loses its last
    suffix (``v_a.b`` -> ``v_a.jpg``)."""
    return (bg_dir / pathlib.Path(frame_dir).name).with_suffix(bg_image_extension)


def _report_params(bg_extraction: dict) -> dict:
    """What decides a person_masked result, as the report file stores it."""
    params = {k: bg_extraction.get(k, v) for k, v in PERSON_MASKED_DEFAULTS.items()}
    params['det_file'] = str(params['det_file'])
    return params


def load_person_masked_report(bg_dir) -> Optional[dict]:
    """``bg_dir/person_masked_report.json`` -- ``{'params': the extraction parameters, 'videos': {background file name: report
    row}}`` -- or None when there is none (or it cannot be read)."""
    import json
    try:
        with open(pathlib.Path(bg_dir) / REPORT_NAME) as f:
            rep = json.load(f)
    except (OSError, ValueError):
        return None
    return rep if isinstance(rep, dict) and isinstance(rep.get('videos'), dict) and isinstance(rep.get('params'), dict) else None


def write_person_masked_report(bg_dir, params: dict, rows: Sequence[dict]) -> dict:
    """Merge ``rows`` (the dicts ``extract_backgrounds`` appends to ``report``) into ``bg_dir/person_masked_report.json``, written
    atomically.  Rows of an earlier run are kept when it ran under the same ``params``, else dropped."""
    import json
    old = load_person_masked_report(bg_dir)
    videos = dict(old['videos']) if old is not None and old['params'] == params else {}
    for r in rows:
        videos[pathlib.Path(r['dest']).name] = r
    rep = dict(params=params, videos=videos)
    _write_atomic(pathlib.Path(bg_dir) / REPORT_NAME, (json.dumps(rep, indent=1, sort_keys=True) + '\n').encode())
    return rep


def resolve_bg_files(video_infos: Sequence[dict], bg_dir, map_bg_to_video: bool = True, extract_bg_if_not_found: bool = True,
                     bg_image_extension: str = '.jpg', decoder=None, quality: int = DEFAULT_QUALITY,
                     max_batch_bytes: int = MAX_BATCH_BYTES, bg_extraction: Optional[dict] = None) -> List[str]:
    """The background list of ``BackgroundMixDataset.__init__`` (libs/loader/comix_loader.py:67-100).

    ``bg_dir`` is resolved with ``realpath`` and created.  With ``map_bg_to_video``: per video, in the order of ``video_infos``,
    ``bg_file_for(frame_dir)`` -- used as it is when it exists, extracted when it does not and ``extract_bg_if_not_found``, else
    skipped.  Without it: every file of ``bg_dir``, sorted (the reference takes the file system's order; a person_masked report
    is not a background).

    ``bg_extraction``: how the missing files are made -- ``method`` and the further keywords of ``extract_backgrounds`` (None: its
    defaults, the temporal median).  With ``method='person_masked'`` a video above ``max_hole_fraction`` gets no file and so is not
    in the list; each extraction merges its report rows into ``bg_dir/person_masked_report.json``, and a video recorded there as
    rejected under the same parameters is not extracted again."""
    bg = pathlib.Path(os.path.realpath(str(bg_dir)))
    bg.mkdir(parents=True, exist_ok=True)
    if not map_bg_to_video:
        return sorted(str(p) for p in bg.glob('*') if p.name != REPORT_NAME)
    paths = [bg_file_for(v['frame_dir'], bg, bg_image_extension) for v in video_infos]
    missing: Dict[pathlib.Path, str] = {}
    for v, p in zip(video_infos, paths):
        if not p.exists() and p not in missing:
            missing[p] = v['frame_dir']
    if missing and extract_bg_if_not_found:
        if bg_extraction is None:
            extract_backgrounds([(d, str(p)) for p, d in missing.items()], decoder, quality, max_batch_bytes)
        elif bg_extraction.get('method', 'tmf') != 'person_masked':
            extract_backgrounds([(d, str(p)) for p, d in missing.items()], decoder, quality, max_batch_bytes, **bg_extraction)
        else:
            params = _report_params(bg_extraction)
            old = load_person_masked_report(bg)
            rejected = {n for n, r in old['videos'].items() if not r.get('written')} if old is not None and old['params'] == params else set()
            jobs = [(d, str(p)) for p, d in missing.items() if p.name not in rejected]
            if jobs:
                rows: List[dict] = []
                extract_backgrounds(jobs, decoder, quality, max_batch_bytes, report=rows, **bg_extraction)
                write_person_masked_report(bg, params, rows)
    return [str(p) for p in paths if p.exists()]
