"""Device-event times of the loader kernels that share the pieces of csrc/resize_linear.h and csrc/loader_pieces.h, each through its
kernels.py wrapper at a loader-sized workload (B 32, T 8): Resize 240x320 -> 256x341, MultiScaleCrop boxes of 256x341 -> 224x224, an
exact 2x shrink 448 -> 224, the ragged Resize of 240 x {320, 352, 384, 427} -> 256 high, three 224x224 crops of 8 clips (dense and
ragged) and the ActorCutMix composite of 32 clips at 224x224 from 256x341 sources.  20 back-to-back calls between two device events,
the median of five such windows, microseconds per call; prints one JSON line.  The library is the one ``BDVCIL_LIB_PATH`` names
(unset: this tree's), so two builds are compared by running the tool once per library, alternating (profiles/loader_kernel_dedupe.txt).
Information only: nothing in the suite depends on these numbers.

    [BDVCIL_LIB_PATH=other/libbdvcil_hip.so] python tools/bench_loader_kernels.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdvcil_amd import decode as D      # noqa: E402
from bdvcil_amd import kernels as K     # noqa: E402
from bdvcil_amd.actor_cut_mix import acm_plan_table  # noqa: E402

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def timeit(fn, iters=20, rounds=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b) / iters * 1000.0)
    return round(float(np.median(best)), 2)


def main():
    dev = torch.device('cuda:0')
    g = torch.Generator(device='cuda').manual_seed(0)
    u8 = lambda *s: torch.randint(0, 256, s, dtype=torch.uint8, device=dev, generator=g)     # noqa: E731
    B, T = 32, 8
    res = {'lib': os.environ.get('BDVCIL_LIB_PATH', 'new')}
    fr = u8(B, T, 240, 320, 3)
    res['resize_240x320_to_256x341_us'] = timeit(lambda: K.resize_linear_u8(fr, 256, 341))
    big = u8(B, T, 256, 341, 3)
    boxes = [(10 + b, 5, 224 + (b % 3) * 20, 224) for b in range(B)]
    res['resize_boxes_to_224_us'] = timeit(lambda: K.resize_linear_u8(big, 224, 224, boxes=boxes))
    half = u8(B, T, 448, 448, 3)
    res['resize_2x_448_to_224_us'] = timeit(lambda: K.resize_linear_u8(half, 224, 224))
    sizes = [(240, (320, 352, 384, 427)[b % 4]) for b in range(B)]
    src = D.RaggedLayout(sizes, T)
    out_sizes = [D.rescale_size(w, h, (-1, 256))[::-1] for h, w in sizes]
    dst, table = D.plan_resize_stage(src, out_sizes=out_sizes)
    sbuf, dbuf = u8(src.nbytes), torch.zeros(dst.nbytes, dtype=torch.uint8, device=dev)
    res['resize_ragged_240_to_256_us'] = timeit(lambda: K.resize_linear_ragged_u8(sbuf, table, T, dbuf))
    crops = [(0, 16, 0), (58, 16, 1), (117, 16, 0)]
    cf = u8(8, T, 256, 341, 3)
    res['crop_normalize_3x224_us'] = timeit(lambda: K.crop_normalize_u8(cf, crops, 224, 224, MEAN, STD))
    L = D.RaggedLayout(out_sizes[:8], T)
    rbuf = u8(L.nbytes)
    rcrops = [[(0, 16, 0), (w - 224, 16, 1), ((w - 224) // 2, 16, 0)] for h, w in out_sizes[:8]]
    res['crop_normalize_ragged_3x224_us'] = timeit(lambda: K.crop_normalize_ragged_u8(rbuf, L.table(), T, rcrops, 224, 224, MEAN, STD))
    actor, scene = u8(B, T, 256, 341, 3), u8(B, T, 256, 341, 3)
    box = [np.array([[40, 30, 130, 200], [100, 60, 180, 150]])] * T
    plan = acm_plan_table([(k, k, k % 2, k, (k // 2) % 2) for k in range(B)], [box] * B, [box] * B)
    out = torch.empty(B, T, 3, 224, 224, device=dev)
    res['actor_cut_mix_224_us'] = timeit(lambda: K.actor_cut_mix_u8(actor, scene, plan, B, out, MEAN, STD))
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
