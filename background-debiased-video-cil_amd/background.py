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
METHODS = ('tmf', 'sim_cam')            # --method of cil_tools/extract_background.py
AVG_METHODS = ('median', 'mean')        # --avg_method (sim_cam only: bg_extraction_tmf ignores it)
SIM_CAM_SIZE = 100                      # RandomResizedCrop(size=100), extract_background.py:82
SIM_CAM_MAX_FRAMES = 500                # --max_frames' default


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
    from .kernels import _p, _stream
    counts = [int(c) for c in counts]
    frames = torch.as_tensor(frames_u8)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f'temporal_median: expected (F, H, W, 3) uint8 frames, got {tuple(frames.shape)} {frames.dtype}')
    if not counts or min(counts) < 1 or sum(counts) != frames.shape[0]:
        raise ValueError(f'temporal_median: frame counts {counts} do not partition {frames.shape[0]} frames')
    dev = frames.device if frames.is_cuda else _device(device)
    frames = frames.to(dev).contiguous()
    V, H, W = len(counts), int(frames.shape[1]), int(frames.shape[2])
    first_h = np.zeros(V, dtype=np.int64)
    first_h[1:] = np.cumsum(counts[:-1])
    counts_h = np.asarray(counts, dtype=np.int32)
    first_d, counts_d = torch.from_numpy(first_h).to(dev), torch.from_numpy(counts_h).to(dev)
    out = torch.empty(V, H, W, 3, dtype=torch.uint8, device=dev)
    check(lib().bdv_temporal_median_u8(_p(frames), int(frames.shape[0]), _p(first_d), _p(counts_d), first_h.ctypes.data, counts_h.ctypes.data,
                                       V, H, W, _p(out), _stream()), 'bdv_temporal_median_u8')
    return out


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


def _check_method(method: str, avg_method: str, interval: int, max_frames: int) -> None:
    if method not in METHODS:
        raise ValueError(f'extract_background: method {method!r} (one of {METHODS})')
    if avg_method not in AVG_METHODS:
        raise ValueError(f'extract_background: avg_method {avg_method!r} (one of {AVG_METHODS})')
    if method == 'tmf' and (avg_method != 'median' or int(interval) != 1 or int(max_frames) != SIM_CAM_MAX_FRAMES):
        raise ValueError("extract_background: method 'tmf' is the median of every frame; avg_method, interval and max_frames "
                         "belong to method 'sim_cam'")


def extract_backgrounds(jobs: Sequence[Tuple[str, str]], decoder=None, quality: int = DEFAULT_QUALITY,
                        max_batch_bytes: int = MAX_BATCH_BYTES, return_arrays: bool = False, method: str = 'tmf',
                        avg_method: str = 'median', interval: int = 1, max_frames: int = SIM_CAM_MAX_FRAMES, size=SIM_CAM_SIZE,
                        antialias: bool = False, draws=None) -> Optional[List[np.ndarray]]:
    """``bg_extraction_tmf`` for many ``(frame_dir, dest)`` pairs: videos of one frame size are batched into one median launch, one
    forward-stage launch and one threaded Huffman call, up to ``max_batch_bytes`` of decoded frames per batch (a single longer video
    is a batch of its own).  A frame directory that fails its checks raises before its file is written.

    ``method='sim_cam'``: ``sim_cam_motion_bg_extract`` instead (see the module docstring) -- per batch decode, one crop launch, one
    reduce launch (``avg_method`` 'median' | 'mean'), encode, write; a video's share of the budget is its selected frames plus their
    fp32 crops.  The crop boxes are drawn video by video in job order from ``draws`` (a ``decode.Draws`` bundle or a seed; ``None`` =
    torch's global generator); ``size`` (int or ``(h, w)``) and ``antialias`` as in ``resized_crop``."""
    from .decode import Draws, JpegDecoder
    _check_method(method, avg_method, interval, max_frames)
    decoder = decoder if decoder is not None else JpegDecoder('cuda')
    results: Optional[List[np.ndarray]] = [None] * len(jobs) if return_arrays else None
    pending: Dict[Tuple[int, int], List[tuple]] = {}
    if method == 'sim_cam':
        draws = Draws.of(draws)
        sh, sw = _size_hw(size)

        def flush(batch, H, W):
            _extract_batch_sim_cam(batch, H, W, decoder, quality, results, (sh, sw), antialias, avg_method)
    else:
        def flush(batch, H, W):
            _extract_batch(batch, H, W, decoder, quality, results)
    for pos, (d, dest) in enumerate(jobs):
        if method == 'sim_cam':
            streams, (H, W) = _read_frames(pathlib.Path(d), sim_cam_frame_files(d, interval, max_frames))
            item = (pathlib.Path(dest), streams, pos, random_resized_crop_boxes(len(streams), H, W, draws=draws))
            per_frame = H * W * 3 + sh * sw * 3 * 4
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


def extract_background(frame_dir, dest, decoder=None, quality: int = DEFAULT_QUALITY, method: str = 'tmf', avg_method: str = 'median',
                       interval: int = 1, max_frames: int = SIM_CAM_MAX_FRAMES, size=SIM_CAM_SIZE, antialias: bool = False,
                       draws=None) -> np.ndarray:
    """``bg_extraction_tmf(data_path, dest)``: the median frame of every file of ``frame_dir``, written to ``dest`` as JPEG;
    returns it as an ``(H, W, 3)`` uint8 RGB array.  ``method='sim_cam'``: ``sim_cam_motion_bg_extract`` with the keywords of
    ``extract_backgrounds``; returns the ``(size_h, size_w, 3)`` image."""
    return extract_backgrounds([(str(frame_dir), str(dest))], decoder, quality, return_arrays=True, method=method, avg_method=avg_method,
                               interval=interval, max_frames=max_frames, size=size, antialias=antialias, draws=draws)[0]


def bg_file_for(frame_dir: str, bg_dir: pathlib.Path, bg_image_extension: str = '.jpg') -> pathlib.Path:
    """``(bg_dir / Path(frame_dir).name).with_suffix(ext)`` -- with the reference's quirk: a dotted directory name loses its last
    suffix (``v_a.b`` -> ``v_a.jpg``)."""
    return (bg_dir / pathlib.Path(frame_dir).name).with_suffix(bg_image_extension)


def resolve_bg_files(video_infos: Sequence[dict], bg_dir, map_bg_to_video: bool = True, extract_bg_if_not_found: bool = True,
                     bg_image_extension: str = '.jpg', decoder=None, quality: int = DEFAULT_QUALITY,
                     max_batch_bytes: int = MAX_BATCH_BYTES) -> List[str]:
    """The background list of ``BackgroundMixDataset.__init__`` (libs/loader/comix_loader.py:67-100).

    ``bg_dir`` is resolved with ``realpath`` and created.  With ``map_bg_to_video``: per video, in the order of ``video_infos``,
    ``bg_file_for(frame_dir)`` -- used as it is when it exists, extracted when it does not and ``extract_bg_if_not_found``, else
    skipped.  Without it: every file of ``bg_dir``, sorted (the reference takes the file system's order)."""
    bg = pathlib.Path(os.path.realpath(str(bg_dir)))
    bg.mkdir(parents=True, exist_ok=True)
    if not map_bg_to_video:
        return sorted(str(p) for p in bg.glob('*'))
    paths = [bg_file_for(v['frame_dir'], bg, bg_image_extension) for v in video_infos]
    missing: Dict[pathlib.Path, str] = {}
    for v, p in zip(video_infos, paths):
        if not p.exists() and p not in missing:
            missing[p] = v['frame_dir']
    if missing and extract_bg_if_not_found:
        extract_backgrounds([(d, str(p)) for p, d in missing.items()], decoder, quality, max_batch_bytes)
    return [str(p) for p in paths if p.exists()]
