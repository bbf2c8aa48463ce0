"""Background extraction on the GPU: what ``BackgroundMixDataset.__init__`` does with
``extract_bg_if_not_found=True`` (libs/loader/comix_loader.py:60-100) -- map every video to ``bg_dir/<frame_dir name>.jpg`` and
make each missing one with ``bg_extraction_tmf`` (:148-164): decode every file of the frame directory, take the per-pixel
``np.median`` over time, ``.astype(np.uint8)``, ``cv2.imwrite`` (baseline JPEG, libjpeg-turbo defaults: quality 95, 4:2:0).

Here the frames are decoded by ``JpegDecoder`` (bit-exact with libjpeg-turbo), the median runs as one launch for a batch of videos
(``bdv_temporal_median_u8``), the JPEG forward stage -- colour conversion, downsampling, DCT, quantisation -- as one more
(``bdv_jpeg_forward_u8``), and the Huffman stage on host threads (``bdv_jpeg_entropy_encode_batch``): the written bytes are
libjpeg-turbo's.  The reference works in BGR (cv2) and returns the BGR median; per-channel medians and the colour conversion of
the encoder make the file the same, and the arrays returned here are RGB."""
from __future__ import annotations

import ctypes
import os
import pathlib
import tempfile
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import JpegInfo, check, lib

DEFAULT_QUALITY = 95                    # cv2.IMWRITE_JPEG_QUALITY's default
MAX_BATCH_BYTES = 2 << 30               # device bytes of decoded frames per extraction launch


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


def _frame_files(frame_dir: pathlib.Path) -> List[pathlib.Path]:
    """Every regular file of the directory, as the reference's ``data_path.glob('*')`` (flow frames included); sorted, which the
    median does not see."""
    if not frame_dir.is_dir():
        raise FileNotFoundError(f'extract_background: {frame_dir} is not a directory')
    files = sorted(p for p in frame_dir.glob('*') if p.is_file())
    if not files:
        raise ValueError(f'extract_background: {frame_dir} holds no frames')
    return files


def _read_frames(frame_dir: pathlib.Path) -> Tuple[List[bytes], Tuple[int, int]]:
    from .decode import jpeg_parse
    streams, size = [], None
    for p in _frame_files(frame_dir):
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


def extract_backgrounds(jobs: Sequence[Tuple[str, str]], decoder=None, quality: int = DEFAULT_QUALITY,
                        max_batch_bytes: int = MAX_BATCH_BYTES, return_arrays: bool = False) -> Optional[List[np.ndarray]]:
    """``bg_extraction_tmf`` for many ``(frame_dir, dest)`` pairs: videos of one frame size are batched into one median launch, one
    forward-stage launch and one threaded Huffman call, up to ``max_batch_bytes`` of decoded frames per batch (a single longer video
    is a batch of its own).  A frame directory that fails its checks raises before its file is written."""
    from .decode import JpegDecoder
    decoder = decoder if decoder is not None else JpegDecoder('cuda')
    results: Optional[List[np.ndarray]] = [None] * len(jobs) if return_arrays else None
    pending: Dict[Tuple[int, int], List[tuple]] = {}
    for pos, (d, dest) in enumerate(jobs):
        streams, (H, W) = _read_frames(pathlib.Path(d))
        item = (pathlib.Path(dest), streams, pos)
        batch = pending.setdefault((H, W), [])
        if batch and (sum(len(it[1]) for it in batch) + len(streams)) * H * W * 3 > max_batch_bytes:
            _extract_batch(batch, H, W, decoder, quality, results)
            batch.clear()
        batch.append(item)
    for (H, W), batch in pending.items():
        if batch:
            _extract_batch(batch, H, W, decoder, quality, results)
    return results


def _extract_batch(items, H, W, decoder, quality, results):
    counts = [len(it[1]) for it in items]
    frames = torch.empty(sum(counts), H, W, 3, dtype=torch.uint8, device=decoder.device)
    at = 0
    for it in items:
        for s in range(0, len(it[1]), 256):                  # bounded staging buffers for the coefficient upload
            part = it[1][s:s + 256]
            frames[at:at + len(part)] = decoder.decode(part)
            at += len(part)
    med = temporal_median(frames, counts)
    del frames
    files = encode_jpeg(med, quality, threads=decoder.threads)
    host = med.cpu().numpy() if results is not None else None
    for k, (it, data) in enumerate(zip(items, files)):
        it[0].parent.mkdir(parents=True, exist_ok=True)
        _write_atomic(it[0], data)
        if results is not None:
            results[it[2]] = host[k]


def extract_background(frame_dir, dest, decoder=None, quality: int = DEFAULT_QUALITY) -> np.ndarray:
    """``bg_extraction_tmf(data_path, dest)``: the median frame of every file of ``frame_dir``, written to ``dest`` as JPEG;
    returns it as an ``(H, W, 3)`` uint8 RGB array."""
    return extract_backgrounds([(str(frame_dir), str(dest))], decoder, quality, return_arrays=True)[0]


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
