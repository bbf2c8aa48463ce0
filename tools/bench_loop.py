"""What prefetching is worth inside the product loop: one epoch of ``CILTaskLoop.fit`` on TSM-R50 (``videos_per_gpu=32``, 8 x 224 x 224)
from 320 x 240 JPEG files generated as tools/bench_files.py generates them, ``prefetch=0`` against ``prefetch=2``, interleaved rounds in
one process.  Prints clips/s per round and one summary line.  With BDVCIL_FORCE_DIST=1 the loop runs in a one-rank process group, which
adds the reducer's communication stream (and RCCL's own) to the streams that share the hardware queues.  Dev tool.
    python tools/bench_loop.py [--rounds 3] [--batches 12] [--prefetch 2] [--caller-stream]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from PIL import Image

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--batches', type=int, default=24, help='batches of 32 clips per epoch')
ap.add_argument('--prefetch', type=int, default=2)
ap.add_argument('--threads', type=int, default=8)
ap.add_argument('--caller-stream', action='store_true', help='the prefetcher runs the loader on the stream current at construction')
args = ap.parse_args()

import bdvcil_amd as bd
import torch
import torch.distributed as dist
from bench import model_cfg

dist_on = os.environ.get('BDVCIL_FORCE_DIST', '0') != '0'
if dist_on:
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29533')
    dist.init_process_group('nccl', rank=0, world_size=1)
dev = torch.device('cuda:0')
rng = np.random.default_rng(0)
yy, xx = np.mgrid[0:240, 0:320]
root = tempfile.mkdtemp(prefix='bdv_loop_')
try:
    frames = os.path.join(root, 'rawframes')
    n_videos = 32 * args.batches
    lines = []
    for v in range(n_videos):
        d = os.path.join(frames, f'v_{v}')
        os.makedirs(d)
        if v < 64:
            base = np.stack([128 + 100 * np.sin(xx / (7.0 + v % 5) + yy / 13.0), 128 + 90 * np.cos(xx / 5.0 + v), 128 + 80 * np.sin(yy / 3.0 + xx / 11.0)], -1)
            for i in range(1, 33):
                a = np.clip(np.roll(base, 3 * i, axis=1) + rng.normal(0, 10, base.shape), 0, 255).astype(np.uint8)
                Image.fromarray(a).save(os.path.join(d, f'img_{i:05}.jpg'), quality=85, subsampling=2)
        else:                                   # the same 64 videos' files under further names: the epoch is long, the encode time is not
            src = os.path.join(frames, f'v_{v % 64}')
            for name in os.listdir(src):
                os.link(os.path.join(src, name), os.path.join(d, name))
        lines.append(f'v_{v} 32 {v % 101}\n')
    for name in ('train', 'val'):
        with open(os.path.join(root, f'{name}.txt'), 'w') as f:
            f.writelines(lines if name == 'train' else lines[:101])
    bgs = []
    for k in range(8):
        p = os.path.join(root, f'bg_{k}.jpg')
        Image.fromarray(rng.integers(0, 256, (256, 340, 3)).astype(np.uint8)).save(p, quality=85)
        bgs.append(p)
    opt = dict(type='SGD', constructor='CILTSMOptimizerConstructorImprovised', paramwise_cfg=dict(fc_lr_scale_factor=5.0), lr=0.01,
               momentum=0.9, weight_decay=1e-4)
    cfg = dict(work_dir=os.path.join(root, 'work'), task_splits=[list(range(101))], methods='base', starting_task=0, ending_task=0,
               num_epochs_per_task=1, videos_per_gpu=32, testing_videos_per_gpu=4, accumulate_grad_batches=1, budget_size=5,
               optimizer=opt, data_root=frames, train_ann_file=os.path.join(root, 'train.txt'), val_ann_file=os.path.join(root, 'val.txt'),
               model=model_cfg(50, 101, 'SimpleLinear', 'CrossEntropyLoss', 0.5))
    torch.manual_seed(0)
    loops = {}
    for n in (0, args.prefetch):
        loader = bd.RawFrameClipLoader(dev, bg_files=bgs, threads=args.threads, seed=1)
        loops[n] = bd.CILTaskLoop(dict(cfg), loader, device=dev, seed=0, log=lambda *a: None, prefetch=n)
        if n and args.caller_stream:
            loops[n]._prefetcher.stream = torch.cuda.current_stream()
    loops[args.prefetch].current_model = loops[0].current_model            # one model: the same kernels, plans and allocator state

    def epoch(n):
        loop = loops[n]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop.fit(loop.train_dataset, 1)
        torch.cuda.synchronize()
        return n_videos / (time.perf_counter() - t0)

    epoch(0)                                    # warm-up: kernels' first launches, allocator, pinned staging
    rates = {0: [], args.prefetch: []}
    for r in range(args.rounds):
        for n in (0, args.prefetch):
            rates[n].append(epoch(n))
        print(f'round {r}: prefetch=0 {rates[0][-1]:.1f} clips/s, prefetch={args.prefetch} {rates[args.prefetch][-1]:.1f} clips/s', flush=True)
    a, b = rates[0], rates[args.prefetch]
    print(f'loop_prefetch dist={int(dist_on)} GPU_MAX_HW_QUEUES={os.environ.get("GPU_MAX_HW_QUEUES")} '
          f'stream={"caller" if args.caller_stream else "own"} batches={args.batches}: prefetch=0 {" ".join(f"{x:.1f}" for x in a)} clips/s '
          f'(mean {sum(a) / len(a):.1f}); prefetch={args.prefetch} {" ".join(f"{x:.1f}" for x in b)} clips/s (mean {sum(b) / len(b):.1f}); '
          f'gain {100 * (sum(b) / sum(a) - 1):+.1f} %; prefetch faster in {sum(y > x for x, y in zip(a, b))} of {len(a)} rounds', flush=True)
    for loop in loops.values():
        loop.close()
finally:
    if dist_on and dist.is_initialized():
        dist.destroy_process_group()
    shutil.rmtree(root, ignore_errors=True)
