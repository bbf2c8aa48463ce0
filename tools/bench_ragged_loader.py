"""RawFrameClipLoader alone, train phase, on batches that mix frame sizes against batches of one size, in one session: 32 clips of 8
frames, 4:2:0 JPEG files of 240 x {320, 352, 384, 427} mixed within every batch (the HMDB51 / Something-Something-v2 case) and of
240 x 320 only (UCF101).  Prints clips/s of the loader by itself (every batch ends in a device synchronise), where the time goes
(reading the files, decode, Resize, the rest of the batch) and the kernel launches per batch.  The yardstick is the resident-batch
training rate of ``python bench.py`` in the same session: the loader has to stay above it for the prefetcher to hide it.  Dev tool.
    python tools/bench_ragged_loader.py [--threads 8] [--steps 20] [--rounds 5] [--out profiles/ragged_loader.txt]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

ap = argparse.ArgumentParser()
ap.add_argument('--threads', type=int, default=8)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=4)
ap.add_argument('--rounds', type=int, default=5, help='timed windows per tree, the trees alternating')
ap.add_argument('--out', default=None, help='also append the result lines to this file')
args = ap.parse_args()

import bdvcil_amd as bd

B, T, VIDEOS, FRAMES = 32, 8, 64, 16
dev = torch.device('cuda:0')
rng = np.random.default_rng(0)


def make_tree(root, widths):
    infos = []
    for v in range(VIDEOS):
        w = widths[v % len(widths)]
        yy, xx = np.mgrid[0:240, 0:w]
        d = os.path.join(root, f'v_{v}')
        os.makedirs(d)
        base = np.stack([128 + 100 * np.sin(xx / (7.0 + v % 5) + yy / 13.0), 128 + 90 * np.cos(xx / 5.0 + v), 128 + 80 * np.sin(yy / 3.0 + xx / 11.0)], -1)
        base = base + rng.normal(0, 10, base.shape)
        for i in range(1, FRAMES + 1):
            a = np.clip(np.roll(base, (2 * i, 3 * i), axis=(0, 1)), 0, 255).astype(np.uint8)
            Image.fromarray(a).save(os.path.join(d, f'img_{i:05}.jpg'), quality=85, subsampling=2)
        infos.append({'frame_dir': d, 'total_frames': FRAMES, 'label': v % 51})
    return infos


def sync_time(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def launches(fn):
    """Kernel launches of one call, counted from the profiler's device trace."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(0)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'memcpy' not in e.name.lower()
               and 'memset' not in e.name.lower())


root = tempfile.mkdtemp(prefix='bdv_ragged_')
lines = []
try:
    bgs = []
    for k in range(8):
        p = os.path.join(root, f'bg_{k}.jpg')
        Image.fromarray(rng.integers(0, 256, (256, 340, 3)).astype(np.uint8)).save(p, quality=85)
        bgs.append(p)
    trees = {'240x320 only': make_tree(os.path.join(root, 'same'), (320,)),
             '240x{320,352,384,427} mixed': make_tree(os.path.join(root, 'mixed'), (320, 352, 384, 427))}
    runs = {}
    for name, infos in trees.items():
        loader = bd.RawFrameClipLoader(dev, bg_files=bgs, threads=args.threads, seed=0)
        batch_infos = lambda i, infos=infos: [infos[(B * i + k) % VIDEOS] for k in range(B)]   # consecutive videos: all four widths in every batch
        ragged = len({Image.open(os.path.join(v['frame_dir'], 'img_00001.jpg')).size for v in batch_infos(0)}) > 1
        full = lambda i, loader=loader, batch_infos=batch_infos: loader(batch_infos(i), 'train')
        for i in range(args.warmup):
            full(i)
        runs[name] = dict(loader=loader, batch_infos=batch_infos, ragged=ragged, full=full, rates=[])
    for _ in range(args.rounds):            # the two trees in turn: other work shares the host, a single window says little
        for r in runs.values():
            r['rates'].append(B / sync_time(r['full'], args.steps))
    for name, r in runs.items():
        loader, batch_infos, ragged = r['loader'], r['batch_infos'], r['ragged']
        read = lambda i: loader._clips(batch_infos(i), test_mode=False)
        held = [read(i)[0] for i in range(4)]                                          # bytes in memory: the two device stages alone
        decode = lambda i: (loader.decoder.decode_clips_ragged if ragged else loader.decoder.decode_clips)(held[i % 4])
        resized = lambda i: (loader._resized_ragged if ragged else loader._resized)(held[i % 4])
        t_read, t_dec, t_res = (sync_time(f, args.steps) for f in (read, decode, resized))
        try:
            n_launch = str(launches(r['full']))
        except Exception as e:      # the count is a by-product; the timings above stand without it
            n_launch = f'not measured ({type(e).__name__}: {e})'
        rates = sorted(r['rates'])
        lines.append(f'{name}: loader alone, train phase, B {B} x T {T}, {args.threads} host threads, {"packed" if ragged else "dense"} path: '
                     f'median {rates[len(rates) // 2]:.1f} clips/s ({B / rates[len(rates) // 2] * 1e3:.2f} ms/batch) of {args.rounds} rounds of {args.steps} '
                     f'batches [{" ".join(f"{v:.1f}" for v in r["rates"])}]; stages alone: sampling + reading the files {1e3 * t_read:.2f} ms, '
                     f'decode {1e3 * t_dec:.2f} ms, decode + Resize {1e3 * t_res:.2f} ms; kernel launches per batch: {n_launch}')
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
finally:
    shutil.rmtree(root, ignore_errors=True)
