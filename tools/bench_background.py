"""Background extraction (bg_extraction_tmf) on synthetic UCF101-sized videos: the CPU path the reference takes against the GPU path
of bdvcil_amd.background, and the median / forward-DCT kernels alone.  Dev tool; every phase is a process of its own, so that a
job script can give each its own time limit:

    python tools/bench_background.py --phase make    --data DIR          # 64 videos x 187 frames of 240 x 320, q95, Pillow
    python tools/bench_background.py --phase cpu     --data DIR --out R  # Pillow decode + np.median + Pillow encode, 16 processes
    python tools/bench_background.py --phase gpu     --data DIR --out R  # resolve_bg_files end to end (decode, median, encode, write)
    rocprofv3 --kernel-trace --stats --output-format csv -d S -- python tools/bench_background.py --phase kernels --data DIR
    python tools/bench_background.py --phase report  --out R --stats S > profiles/r04_background.txt
    python tools/bench_background.py --phase masked  > profiles/person_masked.txt   # person-masked median beside the plain one

The CPU path decodes with Pillow (cv2 is not installed; both run libjpeg-turbo with the same defaults).

``--method sim_cam`` (with ``--avg_method median|mean``) runs the same phases for sim_cam_motion_bg_extract: ``make --frames 121`` writes
121 files per video, of which the extraction reads 120; ``cpu`` is the restatement (Pillow decode, torch crop + bilinear resize, zeros ->
NaN, numpy nanmedian / nanmean, Pillow encode) on 16 processes with one torch thread each; ``gpu`` times the stages one by one (host
read + decode, crop, reduce, encode) and then ``extract_backgrounds`` end to end, and sets the reduce kernel's time against its byte
model (passes x F x P x 4 bytes at the achievable HBM rate); ``report`` prints both."""
import argparse
import glob
import io
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

VIDEOS, FRAMES, H, W = 64, 187, 240, 320


def _make_video(args):
    root, v = args
    from PIL import Image
    d = os.path.join(root, 'frames', f'v_{v:03d}')
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(v)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(xx / (7.0 + v % 5) + yy / 13.0), 128 + 90 * np.cos(xx / 5.0 + v),
                     128 + 80 * np.sin(yy / 3.0 + xx / 11.0)], -1)
    for i in range(1, FRAMES + 1):
        f = np.roll(base, 2 * i, axis=1) + rng.normal(0, 10, base.shape)
        f[60:120, (3 * i) % 200:(3 * i) % 200 + 80] = 40 + (i % 7) * 30           # a moving foreground block
        Image.fromarray(np.clip(f, 0, 255).astype(np.uint8)).save(os.path.join(d, f'img_{i:05}.jpg'), quality=95)


def _cpu_one(args):
    d, dest = args
    from PIL import Image
    frames = [np.asarray(Image.open(p).convert('RGB')) for p in sorted(glob.glob(os.path.join(d, '*')))]
    med = np.median(frames, axis=0).astype(np.uint8)
    Image.fromarray(med).save(dest, quality=95)


def _cpu_sim_cam(args):
    d, dest, avg_method, seed = args
    import warnings
    import torch
    import torch.nn.functional as Fn
    from PIL import Image
    from bdvcil_amd.background import random_resized_crop_boxes, sim_cam_frame_files
    torch.set_num_threads(1)
    files = sim_cam_frame_files(d)
    boxes = random_resized_crop_boxes(len(files), H, W, draws=seed)
    crops = []
    for p, (t, l, h, w) in zip(files, boxes):
        chw = torch.from_numpy(np.asarray(Image.open(p).convert('RGB'))).permute(2, 0, 1).float()[:, t:t + h, l:l + w].contiguous()
        crops.append(Fn.interpolate(chw[None], size=(100, 100), mode='bilinear', align_corners=False)[0].permute(1, 2, 0).numpy())
    stack = np.stack(crops)
    stack[stack == 0] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        r = (np.nanmedian if avg_method == 'median' else np.nanmean)(stack, axis=0)
    Image.fromarray(np.nan_to_num(r).astype(np.uint8)).save(dest, quality=95)


def _gpu_sim_cam(a):
    """Stage times of the sim_cam path on the first-listed videos, then the whole call."""
    import torch
    from bdvcil_amd import background as BG
    from bdvcil_amd.decode import JpegDecoder
    dec = JpegDecoder('cuda', threads=16)
    vids = _videos(a.data)
    key = 'gpu_sim_cam_' + a.avg_method
    BG.extract_backgrounds([(d, os.path.join(a.data, 'bg_gpu_warm', os.path.basename(d) + '.jpg')) for d in vids[:2]], dec, method='sim_cam',
                           avg_method=a.avg_method, draws=0)                  # library load, kernel load, allocator warm-up

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t

    files = [BG.sim_cam_frame_files(d) for d in vids]
    counts = [len(f) for f in files]
    boxes = np.concatenate([BG.random_resized_crop_boxes(n, H, W, draws=0) for n in counts])
    streams, t_read = timed(lambda: [p.read_bytes() for f in files for p in f])
    frames, t_dec = timed(lambda: torch.cat([dec.decode(streams[s:s + 256]) for s in range(0, len(streams), 256)]))
    crops, t_crop = timed(lambda: BG.resized_crop(frames, boxes, 100, False))
    bg, t_red = timed(lambda: BG.temporal_nanreduce(crops, counts, a.avg_method))
    _, t_enc = timed(lambda: BG.encode_jpeg(bg, threads=16))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    reps = 10
    ev[0].record()
    for _ in range(reps):
        BG.temporal_nanreduce(crops, counts, a.avg_method)
    ev[1].record()
    torch.cuda.synchronize()
    red_ms = ev[0].elapsed_time(ev[1]) / reps
    ev[0].record()
    for _ in range(reps):
        BG.resized_crop(frames, boxes, 100, False)
    ev[1].record()
    torch.cuda.synchronize()
    crop_ms = ev[0].elapsed_time(ev[1]) / reps
    del frames, crops
    dest = os.path.join(a.data, 'bg_gpu_sim_cam_' + a.avg_method)
    _, t_all = timed(lambda: BG.extract_backgrounds([(d, os.path.join(dest, os.path.basename(d) + '.jpg')) for d in vids], dec, method='sim_cam',
                                                    avg_method=a.avg_method, draws=0))
    passes = 8 if a.avg_method == 'median' else 1
    model = passes * sum(counts) * 100 * 100 * 3 * 4
    res = dict(videos=len(vids), frames=sum(counts), read_s=t_read, decode_s=t_dec, crop_s=t_crop, reduce_s=t_red, encode_s=t_enc,
               crop_kernel_ms=crop_ms, reduce_kernel_ms=red_ms, reduce_model_bytes=model, reduce_model_ms=model / 6.3e12 * 1e3, seconds=t_all)
    _record(a.out, key, res)
    print(key, json.dumps(res))


def _masked_phase(a):
    """The person-masked median beside the plain one on one random stack (64 videos x 150 frames of 240 x 320), interleaved in one
    process: per round one launch of each variant between device events; medians and minima over the rounds.  The C entry points are
    called on tensors uploaded beforehand, so the events bracket the host-side table check and the kernel, not Python's part."""
    import torch
    from bdvcil_amd import background as BG
    from bdvcil_amd._lib import check, lib
    from bdvcil_amd.kernels import _p, _stream
    videos, frames_per, rounds = 64, 150, 12
    total = videos * frames_per
    frames = torch.randint(0, 256, (total, H, W, 3), dtype=torch.uint8, device='cuda')
    counts_h = torch.full((videos,), frames_per, dtype=torch.int32)
    first_h = torch.arange(videos, dtype=torch.int64) * frames_per
    counts_d, first_d = counts_h.cuda(), first_h.cuda()
    out = torch.empty(videos, H, W, 3, dtype=torch.uint8, device='cuda')
    visible = torch.empty(videos, H, W, dtype=torch.uint16, device='cuda')

    def table(second):
        """Per frame a person walking through (80 x 160, two pixels a frame); ``second``: 'walks' adds another one (40 x 100, three
        pixels a frame), 'stays' one who never moves (40 x 100: every pixel of it is a hole)."""
        rows = []
        for v in range(videos):
            for f in range(frames_per):
                rows.append([(2 * f + 7 * v) % 240, 40, (2 * f + 7 * v) % 240 + 80, 200])
                if second:
                    x = (3 * f + 11 * v) % 280 if second == 'walks' else 260
                    rows.append([x, 120, x + 40, 220])
        per = 2 if second else 1
        bf, bx = torch.arange(0, per * total + 1, per, dtype=torch.int32), torch.tensor(rows, dtype=torch.int32)
        return bf, bx, bf.cuda(), bx.cuda()

    def plain():
        check(lib().bdv_temporal_median_u8(_p(frames), total, _p(first_d), _p(counts_d), first_h.data_ptr(), counts_h.data_ptr(), videos, H, W,
                                           _p(out), _stream()), 'bdv_temporal_median_u8')

    def masked(t):
        bf, bx, bf_d, bx_d = t
        nb = int(bx.shape[0])
        check(lib().bdv_temporal_masked_median_u8(_p(frames), total, _p(first_d), _p(counts_d), first_h.data_ptr(), counts_h.data_ptr(), videos,
                                                  H, W, _p(bf_d), _p(bx_d) if nb else None, bf.data_ptr(), bx.data_ptr() if nb else None, nb, 1,
                                                  _p(out), _p(visible), _stream()), 'bdv_temporal_masked_median_u8')

    none = (torch.zeros(total + 1, dtype=torch.int32), torch.zeros((0, 4), dtype=torch.int32))
    none = none + (none[0].cuda(), none[1].cuda())
    variants = [('bdv_temporal_median_u8', plain),
                ('masked, empty box table', lambda: masked(none)),
                ('masked, 1 box per frame, no holes', lambda t=table(None): masked(t)),
                ('masked, 2 boxes per frame, no holes', lambda t=table('walks'): masked(t)),
                ('masked, 2 boxes per frame, one never moves (holes)', lambda t=table('stays'): masked(t))]
    shares = {}
    for name, fn in variants:                   # code objects, and the hole share of each table
        fn()
        if fn is not plain:
            shares[name] = sum(BG.hole_fractions(visible)) / videos
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]))
    stack = total * H * W * 3
    print(f'# tools/bench_background.py --phase masked: {videos} videos x {frames_per} frames of {W} x {H} (random bytes, {stack / 2**30:.2f} GiB), '
          f'one MI355X; {rounds} interleaved rounds, one launch of each per round, device events around the C call (tables uploaded beforehand)')
    base = float(np.median(ms[variants[0][0]]))
    for name, _ in variants:
        t = np.asarray(ms[name])
        holes = f', {shares[name] * 100:.2f} % of the pixels are holes' if name in shares else ''
        print(f'{name}: median {np.median(t):.3f} ms, min {t.min():.3f} ms, {2 * stack / np.median(t) / 1e9:.2f} TB/s over two reads of the stack, '
              f'{np.median(t) / base:.2f}x the plain median{holes}')


def _videos(data):
    return sorted(glob.glob(os.path.join(data, 'frames', 'v_*')))


def _record(out, key, value):
    res = {}
    if os.path.exists(out):
        with open(out) as f:
            res = json.load(f)
    res[key] = value
    with open(out, 'w') as f:
        json.dump(res, f, indent=1)


def main():
    global FRAMES
    ap = argparse.ArgumentParser()
    ap.add_argument('--phase', required=True, choices=['make', 'cpu', 'gpu', 'kernels', 'report', 'masked'])
    ap.add_argument('--data', default='bench_out/background')
    ap.add_argument('--out', default='bench_out/background.json')
    ap.add_argument('--stats', default=None)
    ap.add_argument('--procs', type=int, default=16)
    ap.add_argument('--method', default='tmf', choices=['tmf', 'sim_cam'])
    ap.add_argument('--avg_method', default='median', choices=['median', 'mean'])
    ap.add_argument('--frames', type=int, default=FRAMES, help='files per video written by --phase make')
    a = ap.parse_args()
    FRAMES = a.frames
    if a.phase == 'masked':
        return _masked_phase(a)
    if a.method == 'sim_cam' and a.phase in ('cpu', 'gpu', 'report'):
        return _sim_cam_phase(a)
    frame_bytes, stack = H * W * 3, VIDEOS * FRAMES * H * W * 3
    if a.phase == 'make':
        with ProcessPoolExecutor(a.procs) as ex:
            list(ex.map(_make_video, [(a.data, v) for v in range(VIDEOS)]))
        n = sum(os.path.getsize(p) for p in glob.glob(os.path.join(a.data, 'frames', '*', '*.jpg')))
        print(f'{VIDEOS} videos x {FRAMES} frames of {W} x {H}, q95: {n / 2**20:.1f} MiB of JPEG')
    elif a.phase == 'cpu':
        dest = os.path.join(a.data, 'bg_cpu')
        os.makedirs(dest, exist_ok=True)
        jobs = [(d, os.path.join(dest, os.path.basename(d) + '.jpg')) for d in _videos(a.data)]
        t = time.perf_counter()
        with ProcessPoolExecutor(a.procs) as ex:
            list(ex.map(_cpu_one, jobs))
        dt = time.perf_counter() - t
        _record(a.out, 'cpu', dict(seconds=dt, videos=len(jobs), procs=a.procs))
        print(f'cpu: {len(jobs)} videos in {dt:.2f} s on {a.procs} processes ({dt / len(jobs) * 1e3:.1f} ms per video)')
    elif a.phase == 'gpu':
        import torch
        from bdvcil_amd.background import resolve_bg_files
        from bdvcil_amd.decode import JpegDecoder
        dec = JpegDecoder('cuda', threads=16)
        infos = [dict(frame_dir=d, total_frames=FRAMES, label=0) for d in _videos(a.data)]
        warm = os.path.join(a.data, 'bg_gpu_warm')
        resolve_bg_files(infos[:2], warm, decoder=dec)           # library load, kernel load, allocator warm-up
        dest = os.path.join(a.data, 'bg_gpu')
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = resolve_bg_files(infos, dest, decoder=dec)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        assert len(out) == len(infos)
        same = sum(open(p, 'rb').read() == open(os.path.join(a.data, 'bg_cpu', os.path.basename(p)), 'rb').read()
                   for p in out if os.path.exists(os.path.join(a.data, 'bg_cpu', os.path.basename(p))))
        _record(a.out, 'gpu', dict(seconds=dt, videos=len(out), identical_to_cpu=same))
        print(f'gpu: {len(out)} videos in {dt:.2f} s ({dt / len(out) * 1e3:.1f} ms per video), {same} files identical to the CPU path')
    elif a.phase == 'kernels':
        import torch
        from bdvcil_amd.background import jpeg_forward, temporal_median
        frames = torch.randint(0, 256, (VIDEOS * FRAMES, H, W, 3), dtype=torch.uint8, device='cuda')
        for _ in range(5):
            med = temporal_median(frames, [FRAMES] * VIDEOS)
            jpeg_forward(med, 95)
        torch.cuda.synchronize()
        print('kernels: 5 x (median of 64 x 187 frames, forward stage of 64 images)')
    else:
        with open(a.out) as f:
            res = json.load(f)
        print(f'# tools/bench_background.py: {VIDEOS} videos x {FRAMES} frames of {W} x {H}, Pillow q95 frames, one MI355X')
        c, g = res.get('cpu'), res.get('gpu')
        if c:
            print(f'cpu path (Pillow decode + np.median + Pillow encode, {c["procs"]} processes): {c["seconds"]:.2f} s, '
                  f'{c["seconds"] / c["videos"] * 1e3:.1f} ms per video')
        if g:
            print(f'gpu path (resolve_bg_files: read, host Huffman decode, decode kernels, median, forward stage, host encode, '
                  f'write): {g["seconds"]:.2f} s, {g["seconds"] / g["videos"] * 1e3:.1f} ms per video; '
                  f'{g["identical_to_cpu"]} of {g["videos"]} files identical to the cpu path')
        if c and g:
            print(f'speed-up end to end: {c["seconds"] / g["seconds"]:.1f}x')
        if a.stats:
            files = glob.glob(os.path.join(a.stats, '**', '*kernel_stats.csv'), recursive=True)
            import csv
            want = {'temporal_median_kernel': 2 * stack + VIDEOS * frame_bytes,      # two reads of the stack, one write
                    'jpeg_forward_kernel': VIDEOS * frame_bytes + VIDEOS * 2 * (1200 + 300 + 300) * 64}
            for fn in files:
                for row in csv.DictReader(open(fn)):
                    for k, nbytes in want.items():
                        if k in row['Name']:
                            avg_ns = float(row['AverageNs'])
                            print(f'{k}: {int(row["Calls"])} calls, {avg_ns / 1e3:.1f} us average, {nbytes / 2**20:.1f} MiB moved '
                                  f'(minimum), {nbytes / avg_ns:.0f} GB/s = {nbytes / avg_ns / 8000 * 100:.0f} % of 8 TB/s HBM')


def _sim_cam_phase(a):
    key = 'sim_cam_' + a.avg_method
    if a.phase == 'cpu':
        dest = os.path.join(a.data, 'bg_cpu_' + key)
        os.makedirs(dest, exist_ok=True)
        jobs = [(d, os.path.join(dest, os.path.basename(d) + '.jpg'), a.avg_method, v) for v, d in enumerate(_videos(a.data))]
        t = time.perf_counter()
        with ProcessPoolExecutor(a.procs) as ex:
            list(ex.map(_cpu_sim_cam, jobs))
        dt = time.perf_counter() - t
        _record(a.out, 'cpu_' + key, dict(seconds=dt, videos=len(jobs), procs=a.procs))
        print(f'cpu {key}: {len(jobs)} videos in {dt:.2f} s on {a.procs} processes ({dt / len(jobs) * 1e3:.1f} ms per video)')
    elif a.phase == 'gpu':
        _gpu_sim_cam(a)
    else:
        with open(a.out) as f:
            res = json.load(f)
        c, g = res.get('cpu_' + key), res.get('gpu_' + key)
        if c:
            print(f'{key} cpu restatement (Pillow decode, torch crop + resize, numpy nan-reduce, Pillow encode; {c["procs"]} processes): '
                  f'{c["seconds"]:.2f} s, {c["seconds"] / c["videos"] * 1e3:.1f} ms per video')
        if g:
            print(f'{key} gpu, {g["videos"]} videos / {g["frames"]} frames of {W} x {H}: extract_backgrounds {g["seconds"]:.2f} s '
                  f'({g["seconds"] / g["videos"] * 1e3:.1f} ms per video); stages: read {g["read_s"] * 1e3:.0f} ms, decode {g["decode_s"] * 1e3:.0f} ms, '
                  f'crop {g["crop_s"] * 1e3:.1f} ms, reduce {g["reduce_s"] * 1e3:.1f} ms, encode {g["encode_s"] * 1e3:.1f} ms')
            print(f'{key} kernels (events, 10 launches): crop {g["crop_kernel_ms"]:.3f} ms; reduce {g["reduce_kernel_ms"]:.3f} ms against '
                  f'{g["reduce_model_ms"]:.3f} ms for {g["reduce_model_bytes"] / 2**30:.2f} GiB at 6.3 TB/s')
        if c and g:
            print(f'{key} speed-up end to end: {c["seconds"] / g["seconds"]:.1f}x')


if __name__ == '__main__':
    main()
