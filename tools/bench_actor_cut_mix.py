"""Loader throughput of ``ActorCutMixClipLoader`` (train phase, acm_prob 0.5) next to ``RawFrameClipLoader`` on the same JPEG files,
and the composite kernel alone for ``rocprofv3 --kernel-trace --stats``.

    python tools/bench_actor_cut_mix.py                      # clips/s at B = 48 and 32, T = 8, 320 x 240 frames -> one JSON line
    python tools/bench_actor_cut_mix.py --kernel-only        # 20 launches of an all-ActorCutMix batch of 32 at 224^2 (341 x 256 sources)

The files are written to a temporary directory (Pillow, quality 90, 4:2:0); the detections are synthetic, one or two boxes per frame."""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_data(root, videos=24, frames=40):
    from PIL import Image
    rng = np.random.default_rng(0)
    infos, dets = [], {}
    yy, xx = np.mgrid[0:240, 0:320]
    for v in range(videos):
        d = os.path.join(root, f'v_bench_{v}')
        os.makedirs(d)
        base = np.stack([128 + 90 * np.sin((v + 1) * xx / 17.0), 128 + 90 * np.cos((v % 3 + 1) * yy / 13.0), np.full(xx.shape, 7.0 * v)], -1)
        for i in range(1, frames + 1):
            img = np.clip(np.roll(base, 3 * i, axis=1) + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(d, f'img_{i:05}.jpg'), quality=90, subsampling=2)
        per = []
        for i in range(frames + 1):
            x0, y0 = rng.uniform(0, 200), rng.uniform(0, 120)
            per.append(np.array([[x0, y0, x0 + 90, y0 + 110, 0.9], [x0 + 30, y0 + 10, x0 + 60, y0 + 40, rng.uniform(0.2, 0.8)]], np.float32))
        dets[f'v_bench_{v}'] = per
        infos.append({'frame_dir': d, 'total_frames': frames, 'label': v % 10})
    det_file = os.path.join(root, 'detections.npy')
    np.save(det_file, np.array(dets, dtype=object), allow_pickle=True)
    return infos, det_file


def clips_per_s(loader, infos, B, iters, warmup):
    import torch
    rng = random.Random(1)
    batches = [[infos[rng.randrange(len(infos))] for _ in range(B)] for _ in range(iters + warmup)]
    for b in batches[:warmup]:
        loader(b, 'train')
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in batches[warmup:]:
        loader(b, 'train')
    torch.cuda.synchronize()
    return B * iters / (time.perf_counter() - t0)


def kernel_only(launches=20):
    import torch
    from bdvcil_amd import kernels as K
    from bdvcil_amd.actor_cut_mix import acm_plan_table
    from bdvcil_amd.frontend import IMG_MEAN, IMG_STD
    B, T, S = 32, 8, 224
    g = torch.Generator(device='cuda').manual_seed(0)
    actor = torch.randint(0, 256, (B, T, 256, 341, 3), dtype=torch.uint8, device='cuda', generator=g)
    scene = torch.randint(0, 256, (B, T, 256, 341, 3), dtype=torch.uint8, device='cuda', generator=g)
    box = [np.array([[40, 30, 130, 200], [100, 60, 180, 150]])] * T
    table = acm_plan_table([(k, k, k % 2, k, (k // 2) % 2) for k in range(B)], [box] * B, [box] * B)
    out = torch.empty(B, T, 3, S, S, device='cuda')
    for _ in range(launches):
        K.actor_cut_mix_u8(actor, scene, table, B, out, IMG_MEAN, IMG_STD)
    torch.cuda.synchronize()
    wrote = out.numel() * 4
    print(json.dumps({'kernel_only': True, 'launches': launches, 'B': B, 'T': T, 'out_bytes': wrote}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--iters', type=int, default=6)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--threads', type=int, default=8)
    a = ap.parse_args()
    import torch  # noqa: F401
    import bdvcil_amd  # noqa: F401
    if a.kernel_only:
        return kernel_only()
    from bdvcil_amd.actor_cut_mix import ActorCutMixClipLoader
    from bdvcil_amd.decode import RawFrameClipLoader
    with tempfile.TemporaryDirectory() as root:
        infos, det_file = make_data(root)
        random.seed(0); np.random.seed(0)
        acm = ActorCutMixClipLoader(det_file, acm_prob=0.5, device='cuda', threads=a.threads)
        acm.set_scene_infos(infos)
        raw = RawFrameClipLoader('cuda', threads=a.threads)
        res = {'frames': '320x240 jpeg q90 4:2:0', 'T': 8, 'threads': a.threads}
        for B in (48, 32):
            res[f'acm_clips_per_s_B{B}'] = round(clips_per_s(acm, infos, B, a.iters, a.warmup), 1)
            res[f'rawframe_clips_per_s_B{B}'] = round(clips_per_s(raw, infos, B, a.iters, a.warmup), 1)
        print(json.dumps(res))


if __name__ == '__main__':
    main()
