"""Times of the Grad-CAM kernels (csrc/gradcam.hip) at the TSM-R50 evaluation size: B clips of 8 frames at 224 x 224, layer4 =
7 x 7 x 2048.  Device events around ``--iters`` back-to-back launches after a warm-up; bytes are the algorithm's (inputs read once,
outputs written once), computed from the shapes here.  Information only: nothing in the suite depends on these numbers.

    python tools/bench_gradcam.py [--batch 32] [--iters 200] [--out profiles/gradcam_kernels.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import bdvcil_amd as bd
    import torch
    K = bd.kernels
    dev = torch.device('cuda:0')
    B, T, h, w, C, H, W = args.batch, 8, 7, 7, 2048, 224, 224
    g = torch.Generator(device=dev).manual_seed(0)
    A = torch.randn(B * T, h, w, C, device=dev, generator=g)
    G = torch.randn(B * T, h, w, C, device=dev, generator=g)
    frames = torch.randn(B * T, H, W, 4, device=dev, generator=g)
    lut = torch.from_numpy(bd.gradcam.builtin_colormap()).to(dev)
    boxes = [[[[40.0, 30.0, 180.0, 200.0]]] * T] * B
    off, rows = bd.gradcam.box_table(boxes, B, T)
    wgt = K.avgpool_fwd(G)
    m = K.gradcam_map(A, wgt)
    mm = K.gradcam_minmax(m, B, T, H, W)
    px = B * T * H * W
    cases = [
        ('avgpool_fwd (channel weights)', lambda: K.avgpool_fwd(G), G.numel() * 4 + wgt.numel() * 4),
        ('gradcam_map', lambda: K.gradcam_map(A, wgt), A.numel() * 4 + wgt.numel() * 4 + m.numel() * 4),
        ('gradcam_minmax', lambda: K.gradcam_minmax(m, B, T, H, W), m.numel() * 4 + 8 * B),
        ('gradcam_render map', lambda: K.gradcam_render(m, mm, B, T, H, W), m.numel() * 4 + px * 4),
        ('gradcam_render map+overlay', lambda: K.gradcam_render(m, mm, B, T, H, W, True, frames, lut, 0.5, bd.frontend.IMG_MEAN, bd.frontend.IMG_STD),
         m.numel() * 4 + px * (4 + 16 + 3)),
        ('gradcam_render map+sums', lambda: K.gradcam_render(m, mm, B, T, H, W, True, box_offsets=off, boxes=rows),
         m.numel() * 4 + px * 4 + 2 * B * T * H * 16),
    ]
    lines = [f'Grad-CAM kernels, B={B} T={T} layer4 {h}x{w}x{C} -> {H}x{W}, {args.iters} launches each (device events; the render / box rows '
             f'include the wrapper\'s host work: allocation, and for the sums the table upload)']
    for name, fn, nbytes in cases:
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1000.0 / args.iters
        lines.append(f'{name:32s} {us:9.1f} us   {nbytes / 1e6:9.1f} MB   {nbytes / us / 1e6:7.2f} TB/s')
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
