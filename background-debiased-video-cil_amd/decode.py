"""``RawFrameDecode`` of the configs' pipelines on the GPU: JPEG bytes -> uint8 RGB frames in HBM.

The reference decodes on CPU workers (UPSTREAM mmaction2 ``RawFrameDecode`` -> ``mmcv.imfrombytes(channel_order='rgb')`` ->
``cv2.imdecode``: libjpeg-turbo's defaults; configs/ucf101/bgmix_plus_randAug/...py:126).  Here the Huffman stage -- a serial bit
stream -- runs on host threads (``bdv_jpeg_entropy_decode_batch``: std::thread workers inside the library, one image each), the coefficients cross
PCIe once as int16 (about the size of the decoded image), and dequantisation, inverse DCT, chroma upsampling and colour conversion
run as two launches for the whole batch (``bdv_jpeg_reconstruct_u8``), bit-identical to libjpeg-turbo (tests/test_jpeg_gpu.py).
The output is the ``(N, H, W, 3)`` uint8 layout ``RandAugment`` / ``TrainClipFrontEnd`` / ``CropFrontEnd`` take."""
from __future__ import annotations

import ctypes
from concurrent.futures import ThreadPoolExecutor
from typing import List, Sequence, Tuple

import numpy as np
import torch

from ._lib import JpegInfo, check, lib


def jpeg_parse(data: bytes) -> JpegInfo:
    """Header of a JPEG stream (sizes, sampling factors, block grids, quantisation tables).  Raises on anything the decoder does
    not cover (progressive / arithmetic-coded / CMYK / 12-bit streams), with the reason."""
    info = JpegInfo()
    check(lib().bdv_jpeg_parse(data, len(data), ctypes.byref(info)), 'bdv_jpeg_parse')
    return info


def jpeg_entropy_decode(data: bytes, info: JpegInfo = None, out: np.ndarray = None) -> Tuple[JpegInfo, np.ndarray]:
    """Host stage: the stream's quantised DCT coefficients, ``info.coef_count`` int16 values (component rasters of 64-value blocks
    in natural order).  ``out``: a C-contiguous int16 buffer to fill (a row of the batch's pinned staging tensor)."""
    if info is None:
        info = jpeg_parse(data)
    if out is None:
        out = np.empty(info.coef_count, dtype=np.int16)
    assert out.dtype == np.int16 and out.flags['C_CONTIGUOUS'] and out.size == info.coef_count
    check(lib().bdv_jpeg_entropy_decode(data, len(data), ctypes.byref(info), out.ctypes.data), 'bdv_jpeg_entropy_decode')
    return info, out


class JpegDecoder:
    """Batched decode of JPEG streams (the frames of the UCF101 rawframe dataset share one size and sampling; those of HMDB51 and
    Something-Something-v2 differ in width from video to video).

    ``decode(streams) -> (N, H, W, 3) uint8`` on ``device``; ``decode_clips(clips) -> (B, T, H, W, 3)``.  Streams of different
    geometry in one call are decoded group by group and must then share ``(H, W)`` (else ``ValueError``: a batch tensor needs one
    size).  ``decode_clips_ragged(clips) -> RaggedClips`` takes clips of different sizes: one packed buffer, size group by size group."""

    def __init__(self, device='cuda', threads: int = 8):
        self.device = torch.device(device)
        self.threads = max(1, int(threads))
        self.pool = ThreadPoolExecutor(max_workers=self.threads)      # file reads and header parses; the Huffman stage threads in C

    def _staging(self, ncoef: int, nqt: int):
        """Two pinned staging sets used in turn (a fresh pinned allocation per batch costs several milliseconds, and torch's
        host allocator cannot hand a block back while its upload is still queued): (coefs, qts, event) -- the event marks the
        last upload from the set; waited on before the host threads overwrite it."""
        pin = self.device.type == 'cuda'
        if not hasattr(self, '_sets'):
            self._sets, self._turn = [None, None], 0
        self._turn ^= 1
        cur = self._sets[self._turn]
        if cur is None or cur[0].numel() < ncoef or cur[1].numel() < nqt:
            cur = (torch.empty(max(ncoef, cur[0].numel() if cur else 0), dtype=torch.int16, pin_memory=pin),
                   torch.empty(max(nqt, cur[1].numel() if cur else 0), dtype=torch.int16, pin_memory=pin),
                   torch.cuda.Event() if pin else None)
            self._sets[self._turn] = cur
        elif cur[2] is not None:
            cur[2].synchronize()
        return cur

    def _group(self, streams: Sequence[bytes]):
        infos = list(self.pool.map(jpeg_parse, streams))
        groups = {}
        for i, inf in enumerate(infos):
            groups.setdefault(inf.geometry_key(), []).append(i)
        return infos, groups

    def decode(self, streams: Sequence[bytes]) -> torch.Tensor:
        if len(streams) == 0:
            raise ValueError('JpegDecoder.decode: empty batch')
        # the common case -- every stream has the first one's geometry (frames of one dataset) -- needs no per-stream Python work: the
        # batch call checks each stream against `info` itself and names the first that differs; only then are the streams grouped
        try:
            return self._decode_group(list(streams), [jpeg_parse(streams[0])])
        except RuntimeError as e:
            if 'does not have the geometry' not in str(e):
                raise
        infos, groups = self._group(streams)
        sizes = {(k[0], k[1]) for k in groups}
        if len(sizes) != 1:
            raise ValueError(f'JpegDecoder.decode: images of different sizes in one batch: {sorted(sizes)}')
        W, H = next(iter(sizes))
        out = torch.empty(len(streams), H, W, 3, dtype=torch.uint8, device=self.device)
        for idx in groups.values():
            rgb = self._decode_group([streams[i] for i in idx], [infos[i] for i in idx])
            if len(groups) == 1:
                return rgb
            out[torch.as_tensor(idx, device=self.device)] = rgb
        return out

    def _decode_group(self, streams: List[bytes], infos: List[JpegInfo], out: torch.Tensor = None) -> torch.Tensor:
        """``out``: a contiguous (n, H, W, 3) uint8 tensor on the device to decode into (a size group's slice of a packed buffer)."""
        n, info = len(streams), infos[0]
        coefs, qts, done = self._staging(n * info.coef_count, n * 192)
        coefs, qts = coefs[:n * info.coef_count].view(n, info.coef_count), qts[:n * 192].view(n, 3, 64)
        ptrs = (ctypes.c_char_p * n)(*streams)
        sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
        check(lib().bdv_jpeg_entropy_decode_batch(ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(sizes, ctypes.c_void_p), n, ctypes.byref(info),
                                                  coefs.data_ptr(), qts.data_ptr(), self.threads), 'bdv_jpeg_entropy_decode_batch')
        coefs_d, qts_d = coefs.to(self.device, non_blocking=True), qts.to(self.device, non_blocking=True)
        ws_bytes = lib().bdv_jpeg_workspace_bytes(ctypes.byref(info), n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        from .kernels import _chk, _p, _stream
        if out is None:
            rgb = torch.empty(n, info.height, info.width, 3, dtype=torch.uint8, device=self.device)
        else:
            rgb = _chk(out, (n, info.height, info.width, 3), torch.uint8, 'out')
        check(lib().bdv_jpeg_reconstruct_u8(_p(coefs_d), _p(qts_d), ctypes.byref(info), n, _p(ws), ws_bytes, _p(rgb), _stream()),
              'bdv_jpeg_reconstruct_u8')
        if done is not None:
            done.record()         # the staging set may be refilled once the stream has passed the uploads
        return rgb

    def decode_clips(self, clips: Sequence[Sequence[bytes]]) -> torch.Tensor:
        """``clips``: B lists of T streams each -> (B, T, H, W, 3) uint8."""
        T = len(clips[0])
        if any(len(c) != T for c in clips):
            raise ValueError('JpegDecoder.decode_clips: clips of different lengths')
        flat = [s for c in clips for s in c]
        rgb = self.decode(flat)
        return rgb.view(len(clips), T, *rgb.shape[1:])

    def decode_clips_ragged(self, clips: Sequence[Sequence[bytes]]) -> 'RaggedClips':
        """``clips``: B lists of T streams each, the sizes differing from clip to clip (not inside one) -> ``RaggedClips``.  Each size
        group is decoded by the two kernels of ``decode`` straight into its dense slice of the packed buffer (JPEG geometry by
        geometry when a size group mixes samplings).  As in ``decode``, only one header per clip is parsed in Python: the batch
        call checks every other frame against it, and only a clip whose frames disagree is parsed stream by stream."""
        if len(clips) == 0:
            raise ValueError('JpegDecoder.decode_clips_ragged: empty batch')
        T = len(clips[0])
        if T == 0 or any(len(c) != T for c in clips):
            raise ValueError('JpegDecoder.decode_clips_ragged: clips of different lengths')
        first = [jpeg_parse(c[0]) for c in clips]
        out = RaggedClips(RaggedLayout([(inf.height, inf.width) for inf in first], T), device=self.device)
        for g, rows in enumerate(out.layout.rows):
            H, W = out.layout.groups[g]
            geo = {}
            for r, b in enumerate(rows):
                geo.setdefault(first[b].geometry_key(), []).append(r)
            dense = out.group_frames(g)            # None when the group's clips are padded apart
            tmp = dense if dense is not None else torch.empty(len(rows) * T, H, W, 3, dtype=torch.uint8, device=self.device)
            for rs in geo.values():
                streams = [s for r in rs for s in clips[rows[r]]]
                into = tmp if len(geo) == 1 else None
                try:
                    rgb = self._decode_group(streams, [first[rows[rs[0]]]], out=into)
                except RuntimeError as e:
                    if 'does not have the geometry' not in str(e):
                        raise
                    rgb = self._decode_one_size(streams, H, W, [rows[r] for r in rs], T, into)
                if into is None:
                    tmp.view(len(rows), T, H, W, 3)[torch.as_tensor(rs, device=self.device)] = rgb.view(len(rs), T, H, W, 3)
            if dense is None:
                out.groups[g].copy_(tmp.view(len(rows), T, H, W, 3))
        return out

    def _decode_one_size(self, streams: List[bytes], H: int, W: int, samples: List[int], T: int, out: torch.Tensor = None) -> torch.Tensor:
        """The clips ``samples`` (T streams each) whose frames do not all have their first frame's geometry: JPEG geometry by
        geometry, as long as every frame is H x W."""
        infos, groups = self._group(streams)
        for k, inf in enumerate(infos):
            if (inf.height, inf.width) != (H, W):
                raise ValueError(f'JpegDecoder.decode_clips_ragged: clip {samples[k // T]} has frames of different sizes: '
                                 f'{sorted({(H, W), (inf.height, inf.width)})}')
        rgb = out if out is not None else torch.empty(len(streams), H, W, 3, dtype=torch.uint8, device=self.device)
        for idx in groups.values():
            rgb[torch.as_tensor(idx, device=self.device)] = self._decode_group([streams[i] for i in idx], [infos[i] for i in idx])
        return rgb


RAGGED_ALIGN = 256      # every clip of a packed buffer starts at a multiple of this many bytes


class RaggedLayout:
    """Where the clips of a mixed-size batch lie in one packed uint8 buffer (host-side plan, no GPU): size group by size group in
    order of first appearance, the clips of a group in sample order, ``clip_stride[g]`` bytes apart (the clip's ``T * H * W * 3``
    bytes rounded up to ``align``, so that every clip starts aligned).

      ``sizes[b] = (H, W)``    ``groups[g] = (H, W)``    ``rows[g]`` = the samples of group g    ``where[b] = (g, row)``
      ``group_offsets[g]``, ``offsets[b]``: byte offsets    ``nbytes``: size of the buffer"""

    def __init__(self, sizes, T: int, align: int = RAGGED_ALIGN):
        self.T, self.align = int(T), int(align)
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        if self.T <= 0 or not self.sizes or any(h <= 0 or w <= 0 for h, w in self.sizes):
            raise ValueError(f'RaggedLayout: needs T > 0 and positive frame sizes, got T = {T}, sizes = {self.sizes}')
        self.groups, self.rows, index = [], [], {}
        for b, hw in enumerate(self.sizes):
            if hw not in index:
                index[hw] = len(self.groups)
                self.groups.append(hw)
                self.rows.append([])
            self.rows[index[hw]].append(b)
        self.group_offsets, self.clip_stride = [], []
        self.offsets, self.where = [0] * len(self.sizes), [None] * len(self.sizes)
        off = 0
        for g, (h, w) in enumerate(self.groups):
            stride = -(-(self.T * h * w * 3) // self.align) * self.align
            self.group_offsets.append(off)
            self.clip_stride.append(stride)
            for r, b in enumerate(self.rows[g]):
                self.offsets[b], self.where[b] = off + r * stride, (g, r)
            off += len(self.rows[g]) * stride
        self.nbytes = off

    def clip_bytes(self, b: int) -> int:
        return self.T * self.sizes[b][0] * self.sizes[b][1] * 3

    def table(self) -> np.ndarray:
        """(B, 3) int64 rows (byte offset, H, W): the per-clip source descriptor of ``bdv_crop_normalize_ragged_u8``."""
        return np.array([[o, h, w] for o, (h, w) in zip(self.offsets, self.sizes)], dtype=np.int64)


def plan_resize_stage(src: RaggedLayout, out_sizes=None, boxes=None, uniform=None):
    """Plans one resize stage over a packed buffer on the host: the descriptor table of ``bdv_resize_linear_ragged_u8`` and the
    layout of what it writes.  ``out_sizes``: per-sample ``(Hd, Wd)`` -> the destination is a second packed buffer (``Resize(-1, S)``);
    ``uniform = (Hd, Wd)`` -> the destination is the dense ``(B, T, Hd, Wd, 3)`` tensor in sample order (MultiScaleCrop + Resize).
    ``boxes``: per-sample ``(x0, y0, w, h)`` inside the source frame, default the whole frame.  Returns ``(dst_layout | None,
    table (B, 10) int64)``; the rows are validated by the library at the launch, not here."""
    B = len(src.sizes)
    if (out_sizes is None) == (uniform is None):
        raise ValueError('plan_resize_stage: give either per-sample out_sizes or one uniform size')
    if boxes is None:
        boxes = [(0, 0, w, h) for h, w in src.sizes]
    if len(boxes) != B or (out_sizes is not None and len(out_sizes) != B):
        raise ValueError(f'plan_resize_stage: {B} clips, {len(boxes)} boxes, {len(out_sizes) if out_sizes is not None else B} output sizes')
    if uniform is not None:
        dst, hd, wd = None, int(uniform[0]), int(uniform[1])
        dst_sizes, dst_offsets = [(hd, wd)] * B, [b * src.T * hd * wd * 3 for b in range(B)]
    else:
        dst = RaggedLayout(out_sizes, src.T, src.align)
        dst_sizes, dst_offsets = dst.sizes, dst.offsets
    table = np.empty((B, 10), dtype=np.int64)
    for b in range(B):
        table[b] = (src.offsets[b], *src.sizes[b], *(int(v) for v in boxes[b]), dst_offsets[b], *dst_sizes[b])
    return dst, table


class RaggedClips:
    """Clips of different sizes on the device: ``buffer`` (``layout.nbytes`` uint8) laid out by ``layout`` (a ``RaggedLayout``), and
    ``groups[g]``: the ``(n_g, T, H_g, W_g, 3)`` view of size group g that the per-size kernels (decode, RandAugment) take.  A group's
    view is contiguous when its clips need no padding between them (``T * H * W * 3`` a multiple of the alignment -- 240-high frames
    of even width -- or a single clip); otherwise it is a strided view and ``group_frames`` / ``dense`` say so."""

    def __init__(self, layout: RaggedLayout, buffer: torch.Tensor = None, device='cuda'):
        self.layout = layout
        if buffer is None:
            buffer = torch.empty(layout.nbytes, dtype=torch.uint8, device=device)
        if buffer.dtype != torch.uint8 or buffer.dim() != 1 or buffer.numel() != layout.nbytes or not buffer.is_contiguous():
            raise ValueError(f'RaggedClips: the buffer must be {layout.nbytes} contiguous uint8 values')
        self.buffer = buffer
        T = layout.T
        self.groups = [buffer.as_strided((len(rows), T, h, w, 3), (stride, h * w * 3, w * 3, 3, 1), buffer.storage_offset() + off)
                       for (h, w), rows, stride, off in zip(layout.groups, layout.rows, layout.clip_stride, layout.group_offsets)]

    T = property(lambda self: self.layout.T)
    sizes = property(lambda self: self.layout.sizes)
    device = property(lambda self: self.buffer.device)

    def __len__(self) -> int:
        return len(self.layout.sizes)

    def clip(self, b: int) -> torch.Tensor:
        """The ``(T, H, W, 3)`` view of sample b."""
        g, r = self.layout.where[b]
        return self.groups[g][r]

    def group_frames(self, g: int):
        """Group g as contiguous ``(n_g * T, H, W, 3)`` frames, or None when its clips are padded apart."""
        v = self.groups[g]
        return v.view(-1, *v.shape[2:]) if v.is_contiguous() else None


def rescale_size(w: int, h: int, scale) -> Tuple[int, int]:
    """UPSTREAM ``mmcv.rescale_size((w, h), scale)``: ``(-1, S)`` = short edge to S; sizes ``int(x * factor + 0.5)``."""
    a, b = scale
    long_edge, short_edge = (float('inf'), max(a, b)) if (a == -1 or b == -1) else (max(a, b), min(a, b))
    factor = min(long_edge / max(h, w), short_edge / min(h, w))
    return int(w * float(factor) + 0.5), int(h * float(factor) + 0.5)


class Draws:
    """The random state a loader draws from: ``py`` (the ``random`` module or a ``random.Random``), ``np`` (the ``np.random`` module or
    an ``np.random.RandomState``) and ``torch`` (``None`` = torch's global CPU generator, or a CPU ``torch.Generator``).

    ``Draws()`` is the three process-global generators: every draw lands where it always did, in the same order.  ``Draws(seed)`` owns
    ``random.Random(seed)``, ``np.random.RandomState(seed)`` and ``torch.Generator().manual_seed(seed)`` -- the MT19937 / Philox streams
    that ``random.seed(seed)``, ``np.random.seed(seed)`` and ``torch.manual_seed(seed)`` start -- so a loader built with ``seed=s`` returns
    the batches the unseeded loader returns after seeding the globals with ``s``, without touching the globals.  A loader that runs on
    a worker thread (``PrefetchLoader``) needs this to be reproducible: the training thread draws from the globals too
    (``cil_step.tubemix_draw``)."""

    def __init__(self, seed: int = None):
        import random
        self.seed = seed
        if seed is None:
            self.py, self.np, self.torch = random, np.random, None
        else:
            self.py, self.np, self.torch = random.Random(seed), np.random.RandomState(seed), torch.Generator().manual_seed(seed)

    @staticmethod
    def of(x) -> 'Draws':
        """``None`` -> the globals, a ``Draws`` -> itself, anything else -> ``Draws(seed)``."""
        if x is None:
            return _GLOBAL_DRAWS
        return x if isinstance(x, Draws) else Draws(int(x))

    def randint(self, high: int, low: int = 0) -> int:
        """``int(torch.randint(low, high, (1,)))`` on this bundle's torch generator."""
        return int(torch.randint(low, high, (1,), generator=self.torch).item())


_GLOBAL_DRAWS = Draws()


def sample_frames(total_frames: int, num_clips: int = 8, clip_len: int = 1, frame_interval: int = 1, test_mode: bool = False,
                  start_index: int = 1, draws=None) -> np.ndarray:
    """UPSTREAM mmaction2 0.24 ``SampleFrames`` as the configs use it (``clip_len=1, frame_interval=1, num_clips=8``, no temporal
    jitter, ``out_of_bound_opt='loop'``): 1-based numbers of the ``img_{:05}.jpg`` files; the train form draws from ``np.random``
    (``draws``: a ``Draws`` bundle or a seed; ``None`` = the global generator)."""
    ori = clip_len * frame_interval
    rs = Draws.of(draws).np
    if test_mode:
        avg = (total_frames - ori + 1) / float(num_clips)
        offsets = (np.arange(num_clips) * avg + avg / 2.0).astype(np.int64) if total_frames > ori - 1 else np.zeros((num_clips,), dtype=np.int64)
    else:
        avg = (total_frames - ori + 1) // num_clips
        if avg > 0:
            offsets = np.arange(num_clips) * avg + rs.randint(avg, size=num_clips)
        elif total_frames > max(num_clips, ori):
            offsets = np.sort(rs.randint(total_frames - ori + 1, size=num_clips))
        elif avg == 0:
            offsets = np.around(np.arange(num_clips) * ((total_frames - ori + 1.0) / num_clips))
        else:
            offsets = np.zeros((num_clips,), dtype=np.int64)
    inds = (offsets[:, None] + np.arange(clip_len)[None, :] * frame_interval).reshape(-1)
    return (np.mod(inds, total_frames).astype(np.int64) + start_index)


class RawFrameClipLoader:
    """The configs' four pipelines (configs/ucf101/bgmix_plus_randAug/bgmix_seed_1000_inc_10_stages_bgmix_plus_randAug.py:124-182) for a
    whole batch, as the ``clip_loader`` of ``CILTaskLoop``: ``video_infos`` + phase -> the collated batch dict, frames never leaving HBM
    after the coefficient upload.

      train:                SampleFrames -> RawFrameDecode -> Resize(-1, 256) -> RandAugment -> MultiScaleCrop + Resize(224) -> Normalize,
                            then the background mix of BackgroundMixDataset for the samples RandAugment skipped (comix_loader.py:105-145)
      val / features_extraction: SampleFrames(test_mode) -> decode -> Resize(-1, 256) -> CenterCrop(224) -> Normalize
      test:                 SampleFrames(test_mode) -> decode -> Resize(-1, 256) -> TenCrop(256) -> Normalize

    Host work per batch: reading the files, the Huffman stage (thread pool) and the random draws -- per sample in the reference's order
    (frame offsets from ``np.random``; RandAugment's own draws; crop size and offset from ``random``; background index and crop from
    torch's generator), though a multi-worker DataLoader interleaves samples differently anyway.  ``bg_files``: JPEG backgrounds
    (``back_ground_from_bg_dir``); without it a random frame of a random video of the batch's dataset serves (comix_loader.py:134-137
    draws it from the whole dataset: pass ``bg_video_infos``).

    The dataset families of the configs (``config_run.clip_loader_spec`` maps a config onto these):
      ``with_randAug=True`` (default)   BackgroundMixDataset(with_randAug=True): a sample is mixed exactly when RandAugment skipped it
      ``with_randAug=False, prob=p``    BackgroundMixDataset(with_randAug=False, prob=p): mixed with probability p, one ``random.random()`` each
      ``bg_mix=False``                  plain RawframeDataset: RandAugment on its own, no background is read and nothing is blended
    A setting under which no sample can be mixed (``bg_mix=False``; ``with_randAug`` with a RandAugment probability >= 1;
    ``with_randAug=False`` with ``prob <= 0``) reads no background file and makes no background draw.

    ``seed``: ``None`` = every draw goes to the process-global generators, in the order given above; an int (or a ``Draws``) = the loader
    owns its generators (see ``Draws``) and passes them to every stage it builds, and to a ``randAug`` it was given.

    ``ragged``: a batch whose clips share one size (every UCF101 batch) runs on dense ``(B, T, H, W, 3)`` tensors.  A batch that mixes
    sizes (HMDB51, Something-Something-v2: 240 high, the width differs per video) runs the same stages over packed buffers
    (``RaggedClips``): decode per size group, ``Resize`` in one launch, RandAugment drawn per sample in sample order and applied per
    size group, then MultiScaleCrop + Resize (train) or crop + Normalize (eval) in one launch into the uniform batch -- the same
    arithmetic and the same draws in the same order.  ``'auto'`` (default) picks by the batch; ``'always'`` sends every batch through the
    packed path (same bits on a same-size batch; for tests)."""

    def __init__(self, device='cuda', filename_tmpl: str = 'img_{:05}.jpg', num_segments: int = 8, start_index: int = 1,
                 short_edge: int = 256, input_size: int = 224, randAug=None, randAug_prob: float = 0.75, alpha: float = 0.5,
                 multi_scale_crop: dict = None, bg_files: Sequence[str] = None, bg_video_infos: Sequence[dict] = None,
                 bg_resize: int = 256, test_crop=('TenCrop', 256), threads: int = 8, with_randAug: bool = True, prob: float = 0.25,
                 bg_mix: bool = True, seed=None, ragged: str = 'auto'):
        from .augment import RandAugment
        from .frontend import BackgroundCropFrontEnd, BackgroundMixFrontEnd, CropFrontEnd, MultiScaleCropResize, TrainClipFrontEnd
        self.device = torch.device(device)
        self.tmpl, self.T, self.start_index, self.short_edge = filename_tmpl, int(num_segments), int(start_index), int(short_edge)
        self.decoder = JpegDecoder(self.device, threads)
        self.draws = Draws.of(seed)
        msc = dict(input_size=input_size, scales=(1, 0.875, 0.75, 0.66), random_crop=False, max_wh_scale_gap=1, num_fixed_crops=13)
        msc.update(multi_scale_crop or {})
        if randAug is None:
            randAug = RandAugment(2, 10, randAug_prob, draws=self.draws)
        elif isinstance(randAug, dict):            # the stage's arguments, as a config spells them: dict(n=, m=, prob=)
            randAug = RandAugment(**randAug, draws=self.draws)
        elif seed is not None:
            randAug.draws = self.draws
        self.bg_mix = bool(bg_mix)
        self.train_front = TrainClipFrontEnd(randAug, alpha=alpha, prob=prob, with_randAug=bool(with_randAug),
                                             crop_resize=MultiScaleCropResize(**msc, draws=self.draws), bg_mix=self.bg_mix, draws=self.draws)
        self.bg_front = BackgroundCropFrontEnd(bg_resize, (input_size, input_size), draws=self.draws)
        self.center = CropFrontEnd('CenterCrop', input_size)
        self.test = CropFrontEnd(*test_crop)
        self.bg_files, self.bg_video_infos = (list(bg_files) if bg_files else None), bg_video_infos
        self.input_size = int(input_size)
        if ragged not in ('auto', 'always'):
            raise ValueError(f"RawFrameClipLoader: ragged must be 'auto' or 'always', got {ragged!r}")
        self.ragged = ragged

    def set_bg_files(self, bg_files: Sequence[str]) -> None:
        """The background list of the dataset being trained on (``CILTaskLoop`` calls this before each fit when the config names
        a ``bg_dir``); an empty list means the random-frame fallback."""
        self.bg_files = list(bg_files) if bg_files else None

    # ---- host side ------------------------------------------------------------------------------------------------------------
    def _read(self, path: str) -> bytes:
        with open(path, 'rb') as f:
            return f.read()

    def _clips(self, video_infos: List[dict], test_mode: bool):
        """The sampled frame numbers (B, T) and their files' bytes, B lists of T streams."""
        import os.path as osp
        inds = [sample_frames(int(v['total_frames']), self.T, test_mode=test_mode, start_index=self.start_index, draws=self.draws)
                for v in video_infos]
        paths = [osp.join(v['frame_dir'], self.tmpl.format(int(i))) for v, ii in zip(video_infos, inds) for i in ii]
        streams = list(self.decoder.pool.map(self._read, paths))
        clips = [streams[k * self.T:(k + 1) * self.T] for k in range(len(video_infos))]
        return clips, np.stack(inds)

    def _resized(self, clips) -> torch.Tensor:
        """decode + ``Resize(-1, short_edge)`` of a batch whose clips share one size: (B, T, Hr, Wr, 3)."""
        from . import kernels as K
        frames = self.decoder.decode_clips(clips)
        H, W = int(frames.shape[2]), int(frames.shape[3])
        Wr, Hr = rescale_size(W, H, (-1, self.short_edge))
        return K.resize_linear_u8(frames, Hr, Wr)

    def _resized_ragged(self, clips) -> RaggedClips:
        """The same two stages for clips of different sizes: a packed buffer in, one launch, a second packed buffer out."""
        from . import kernels as K
        src = self.decoder.decode_clips_ragged(clips)
        out_sizes = [rescale_size(w, h, (-1, self.short_edge))[::-1] for h, w in src.sizes]
        layout, table = plan_resize_stage(src.layout, out_sizes=out_sizes)
        dst = RaggedClips(layout, device=self.device)
        K.resize_linear_ragged_u8(src.buffer, table, src.T, dst.buffer)
        return dst

    def _backgrounds(self, B: int, video_infos: List[dict]) -> torch.Tensor:
        """One background per sample, cropped: (B, S, S, 3) fp32 pixel values (only the mixed samples' rows are read)."""
        import os.path as osp
        paths = []
        for _ in range(B):
            if self.bg_files:
                paths.append(self.bg_files[self.draws.randint(len(self.bg_files))])
            else:
                v = self.draws.py.choice(self.bg_video_infos or video_infos)
                idx = self.draws.py.randint(self.start_index, int(v['total_frames']) - 1 + self.start_index)
                paths.append(osp.join(v['frame_dir'], self.tmpl.format(idx)))
        streams = list(self.decoder.pool.map(self._read, paths))
        infos = [jpeg_parse(s) for s in streams]
        out = torch.empty(B, self.input_size, self.input_size, 3, dtype=torch.float32, device=self.device)
        groups = {}
        for i, inf in enumerate(infos):
            groups.setdefault((inf.width, inf.height), []).append(i)
        for idx in groups.values():            # the crop draws stay in sample order inside a size group; sizes rarely differ
            bg = self.decoder.decode([streams[i] for i in idx])
            out[torch.as_tensor(idx, device=self.device)] = self.bg_front(bg)
        return out

    def __call__(self, video_infos: List[dict], phase: str):
        B = len(video_infos)
        clips, inds = self._clips(video_infos, test_mode=phase != 'train')
        # clips of one size (every UCF101 batch) take the dense path; a batch that mixes sizes goes through packed buffers, the
        # stages below taking either form.  A clip's size is its first frame's (sizes do not differ inside a video)
        if self.ragged == 'always' or len({(i.height, i.width) for i in (jpeg_parse(c[0]) for c in clips)}) > 1:
            frames = self._resized_ragged(clips)
        else:
            frames = self._resized(clips)
        extra = {}
        if phase == 'train':
            bg = None if self.train_front.never_mixes() else self._backgrounds(B, video_infos)
            imgs, rand_flags, _ = self.train_front(frames, bg, as_nchw=True)
            extra['randAug'] = rand_flags
        elif phase == 'test':
            imgs = self.test.as_nchw(frames)
        else:
            imgs = self.center.as_nchw(frames)
        dev = self.device
        return {**extra, 'imgs': imgs,
                'label': torch.tensor([[v['label']] for v in video_infos], dtype=torch.int64, device=dev),
                'frame_dir': [v['frame_dir'] for v in video_infos],
                'total_frames': torch.tensor([int(v['total_frames']) for v in video_infos], dtype=torch.int64, device=dev),
                'clip_len': torch.ones(B, dtype=torch.int64, device=dev),
                'num_clips': torch.full((B,), self.T, dtype=torch.int64, device=dev),
                'frame_inds': torch.from_numpy(inds).to(dev)}


class PrefetchLoader:
    """Runs a ``clip_loader`` ahead on a worker thread and its own HIP stream, so that reading, the Huffman stage, the
    per-sample draws and the decode / augment kernels of batch i + 1 overlap the training step of batch i (the reference gets the same
    from its DataLoader workers).  ``submit(video_infos, phase)`` queues a batch, ``get()`` returns the oldest queued batch after making
    the caller's stream wait for it; or iterate: ``for batch in PrefetchLoader(loader).iterate(list_of_video_info_lists, phase)``,
    which keeps ``depth`` batches in flight and leaves nothing queued when it ends, however it ends.
    The batch's tensors are handed to the consumer's stream with ``record_stream`` (a handful of tensors per step).

    Works with any loader.  Reproducibility needs a seeded one (``RawFrameClipLoader(..., seed=s)``): an unseeded loader draws from the
    process-global ``random`` / ``np.random`` / torch generators on the worker thread while the training thread draws from the same
    three (``cil_step.tubemix_draw``), so the order of the draws depends on timing.  With a seeded loader the batches are those of the
    inline calls, bit for bit: one worker thread serves the batches in submission order.

    An exception the loader raises on the worker thread is re-raised, unchanged, by the ``get()`` of its batch; the batches queued
    behind it are cancelled (the one already running is waited for) before it propagates.  ``close()`` releases the thread; a later
    ``submit`` starts a new one.  ``stream``: run the loader on this stream instead of one of the prefetcher's own."""

    def __init__(self, loader, depth: int = 2, stream=None):
        self.loader, self.depth = loader, max(1, int(depth))
        self.stream = stream if stream is not None else torch.cuda.Stream()
        self.pool = None                # the worker thread, started by the first submit
        self.queue = []
        self._bg_files = None           # set_bg_files: the list handed to the loader with each batch submitted after it
        self._scene_infos = None        # set_scene_infos: handed to the loader once, with the first batch submitted after it

    def set_bg_files(self, bg_files: Sequence[str]) -> None:
        """Forwarded to the loader; takes effect from the next submitted batch (batches already queued keep the list they were
        submitted with)."""
        self._bg_files = list(bg_files) if bg_files is not None else []

    def set_scene_infos(self, video_infos: Sequence[dict]) -> None:
        """Forwarded to the loader (``ActorCutMixClipLoader``'s scene pool) with the next submitted batch only: the loader keeps
        the pool, and its ``set_scene_infos`` looks up every video's detections, which is not repeated per batch."""
        self._scene_infos = list(video_infos) if video_infos is not None else []

    def _work(self, video_infos, phase, bg_files=None, scene_infos=None):
        if bg_files is not None and hasattr(self.loader, 'set_bg_files'):
            self.loader.set_bg_files(bg_files)
        if scene_infos is not None and hasattr(self.loader, 'set_scene_infos'):
            self.loader.set_scene_infos(scene_infos)
        with torch.cuda.stream(self.stream):
            batch = self.loader(video_infos, phase)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return batch, ev

    def submit(self, video_infos, phase: str):
        if self.pool is None:
            self.pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix='bdv_prefetch')
        self.queue.append(self.pool.submit(self._work, video_infos, phase, self._bg_files, self._scene_infos))
        self._scene_infos = None

    def get(self):
        fut = self.queue.pop(0)
        try:
            batch, ev = fut.result()
        except BaseException:
            self.cancel()
            raise
        cur = torch.cuda.current_stream()
        cur.wait_event(ev)
        for v in batch.values():
            if torch.is_tensor(v) and v.is_cuda:
                v.record_stream(cur)
        return batch

    def cancel(self) -> None:
        """Drop every queued batch: those not started are cancelled, the one running is waited for (its result, or its exception,
        is discarded).  Afterwards nothing of this prefetcher runs."""
        queue, self.queue = self.queue, []
        for fut in queue:
            fut.cancel()
        for fut in queue:
            if not fut.cancelled():
                try:
                    fut.result()
                except BaseException:      # discarded with the batch it belongs to
                    pass

    def close(self) -> None:
        """``cancel()``, then end the worker thread (joined before this returns)."""
        self.cancel()
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            self.pool = None

    def iterate(self, batches_of_infos, phase: str):
        it = iter(batches_of_infos)
        try:
            for infos in it:
                self.submit(infos, phase)
                if len(self.queue) >= self.depth:
                    break
            for infos in it:
                out = self.get()
                self.submit(infos, phase)
                yield out
            while self.queue:
                yield self.get()
        finally:
            self.cancel()       # a consumer that stopped early (an exception in its step) leaves nothing queued
