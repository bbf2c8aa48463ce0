"""Times of the clip-blend kernels (csrc/blend.hip) against the torch expressions they replace, at the benchmark's batch: 32 clips of
8 frames at 224 x 224, as the (B, T, 3, H, W) tensor and as the front-end's NHWC4 frames (B * T, H, W, 4).

  blend_mix    against  lam * x + (1 - lam) * x[perm]
  blend_box_   against  x[..., r1:r2, c1:c2] = x[perm][..., r1:r2, c1:c2]   for a box of a quarter of the frame and for the full frame

Each pair is timed interleaved in one process: ``--rounds`` times, ``--iters`` back-to-back calls of the fused form between two device
events, then the same of the torch form; the median round is reported with the fastest and the slowest.  Both forms get the
permutation already on the device and include their host work (allocation of the result, the wrapper's checks).  Bytes are the
algorithm's, computed from the shapes here: mix = 3 passes over the batch (two reads, one write; the torch form moves 9: gather,
two products, sum); box = 4 x the box bytes for the fused form (pack, unpack), 2 x the batch + 2 x the box for the torch form.
Information only: nothing in the suite depends on these numbers.

    python tools/bench_blend.py [--batch 32] [--iters 200] [--rounds 7] [--out profiles/blend.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


NOTE = ('note: the batch (154 MB planar, 206 MB NHWC4) and the scratch of a box are smaller than the 256 MiB Infinity Cache and every call of a '
        'window touches the same buffers, so the rates shown include cache hits and may exceed what HBM alone delivers; both forms of a '
        'pair run under the same conditions.  The full-frame box rows move the same bytes in both forms (4 x the batch).')


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import bdvcil_amd as bd
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_blend.py needs a GPU: a CPU run gives no time')
    K = bd.kernels
    dev = torch.device('cuda:0')
    B, T, H, W = args.batch, 8, args.size, args.size
    torch.manual_seed(0)
    perm = torch.randperm(B)
    perm_dev = perm.to(dev)
    lam = 0.3
    lam_t = torch.tensor(lam, dtype=torch.float32)
    quarter = (H // 4, W // 4, H // 4 + H // 2, W // 4 + W // 2)
    full = (0, 0, H, W)
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f'clip blending, B={B} T={T} {H}x{W}, perm = randperm({B}) (seed 0, {int((perm == torch.arange(B)).sum())} fixed points), '
             f'{args.rounds} interleaved rounds of {args.iters} calls (device events; median [min .. max] us per call)']

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / args.iters

    def pair(name, fused, torch_form, fused_bytes, torch_bytes):
        for _ in range(3):
            fused(); torch_form()
        torch.cuda.synchronize()
        tf, tt = [], []
        for _ in range(args.rounds):
            tf.append(timed(fused))
            tt.append(timed(torch_form))
        mf, mt = statistics.median(tf), statistics.median(tt)
        verdict = 'fused is NOT slower' if mf <= mt else 'fused is SLOWER'
        lines.append(f'{name:34s} fused {mf:8.1f} [{min(tf):8.1f} .. {max(tf):8.1f}] us {fused_bytes / 1e6:7.1f} MB {fused_bytes / mf / 1e6:5.2f} TB/s | '
                     f'torch {mt:8.1f} [{min(tt):8.1f} .. {max(tt):8.1f}] us {torch_bytes / 1e6:7.1f} MB | x{mt / mf:5.2f}  {verdict}')
        print(lines[-1], flush=True)

    for layout in ('NCHW', 'NHWC4'):
        if layout == 'NCHW':
            x = torch.randn(B, T, 3, H, W, device=dev, generator=g)
            outer, inner = T * 3, 1
            view = x
            def box_torch(b, v=view):
                r1, c1, r2, c2 = b
                v[..., r1:r2, c1:c2] = v[perm_dev][..., r1:r2, c1:c2]
        else:
            x = torch.randn(B * T, H, W, 4, device=dev, generator=g)
            outer, inner = T, 4
            view = x.view(B, T, H, W, 4)
            def box_torch(b, v=view):
                r1, c1, r2, c2 = b
                v[:, :, r1:r2, c1:c2, :] = v[perm_dev][:, :, r1:r2, c1:c2, :]
        flat = x.view(B, -1)
        nbytes = x.numel() * 4
        pair(f'{layout} mix', lambda: K.blend_mix(flat, perm, lam, perm_dev=perm_dev), lambda: lam_t * flat + (1 - lam_t) * flat[perm_dev],
             3 * nbytes, 9 * nbytes)
        for bname, b in (('quarter box', quarter), ('full frame', full)):
            bb = B * outer * (b[2] - b[0]) * (b[3] - b[1]) * inner * 4
            pair(f'{layout} box, {bname}', lambda b=b: K.blend_box_(x, perm, b, outer, H, W, inner, perm_dev=perm_dev), lambda b=b: box_torch(b),
                 4 * bb, 2 * nbytes + 2 * bb)
        del x, view, flat
        torch.cuda.empty_cache()
    lines.append(NOTE)
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
