"""Times of the fused foreground-merging chain (csrc/fg_merge.hip: ``foreground_mask`` + ``fg_merge_``, what ``ForegroundMergeBlending``
runs at prob = 1) against the torch expression of the same definition on the same device, at the benchmark's batch: 32 clips of 8
frames at 224 x 224, as the (B, T, 3, H, W) tensor and as the front-end's NHWC4 frames (B * T, H, W, 4).

The chain and each of its four stages are timed as pairs, interleaved in one process: ``--rounds`` times, ``--iters`` back-to-back calls
of the fused form between two device events, then the same of the torch form; the median round is reported with the fastest and the
slowest.  Both forms get the permutation on the host and include their host work (allocations, the wrappers' checks, the uploads).
Bytes are the algorithm's for the FUSED form, computed from the shapes here (C = clip bytes, M = one fp32 map per clip = C / 24 planar):
  motion + blur + quantise   C read; d, tmp, g written and read (6 M), q written (M / 4)
  histograms + refined map   C read; q read, 16-bit bin indices written and read (2 x C / 6 planar), s written
  selection                  5 reads of s, mask written
  merge                      4 x the background half of C (pack and assign; every source is itself merged at prob = 1), masks read
With ``--step`` (default) the default training step of bench.py (TSM-R50, batch 32, fp32 frames) is timed in the same process and
the chain is also reported as a share of it.  Information only: nothing in the suite depends on these numbers.

    python tools/bench_fg_merge.py [--batch 32] [--iters 20] [--rounds 5] [--no-step] [--out profiles/fg_merge.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOTE = ('note: the batch (154 MB planar, 206 MB NHWC4) is smaller than the 256 MiB Infinity Cache and every call of a window touches the '
        'same buffers, so the rates shown include cache hits; both forms of a pair run under the same conditions.  The merge rewrites '
        'the batch, so later calls of a window see merged clips: the work is the same, the masks are not.')


def torch_stages(T, H, W, bins, k_fg, taps, lo, sc, chan_last):
    """The torch expression of every stage on a (B, T, 3 or 4, H, W) view ``x`` (a permuted view of the NHWC4 frames)."""
    import torch
    import torch.nn.functional as Fnn
    k = taps.numel()
    r = k // 2

    def motion_q(x):
        c = x[:, :, :3]
        d = (c[:, 1:] - c[:, :-1]).abs().sum(dim=(1, 2)) / (T - 1)
        g = Fnn.conv2d(Fnn.pad(d.unsqueeze(1), (r, r, 0, 0), mode='reflect'), taps.view(1, 1, 1, k))
        g = Fnn.conv2d(Fnn.pad(g, (0, 0, r, r), mode='reflect'), taps.view(1, 1, k, 1)).squeeze(1)
        lo_, hi_ = g.amin(dim=(1, 2), keepdim=True), g.amax(dim=(1, 2), keepdim=True)
        q = torch.floor(255.0 * ((g - lo_) / (hi_ - lo_ + 1e-8)) + 0.5)
        return torch.where(hi_ == lo_, torch.zeros_like(q), q).to(torch.uint8)

    def hist_refine(x, q):
        B = x.shape[0]
        nb = bins ** 3
        v = torch.floor((x[:, :, :3] - lo.view(1, 1, 3, 1, 1)) * sc.view(1, 1, 3, 1, 1))
        v = torch.nan_to_num(v, nan=0.0).clamp(0, bins - 1).long()
        idx = ((v[:, :, 0] * bins + v[:, :, 1]) * bins + v[:, :, 2]).view(B, -1)
        flat = (idx + torch.arange(B, device=x.device).view(B, 1) * nb).view(-1)
        w = q.view(B, 1, -1).expand(B, T, H * W).reshape(-1).double()
        F = torch.bincount(flat, weights=w, minlength=B * nb)
        N = torch.bincount(flat, minlength=B * nb)
        ratio = (F / (255.0 * N.clamp(min=1))).float().view(B, nb)
        return torch.gather(ratio, 1, idx).view(B, T, H, W).sum(1) / T

    def select(s):
        B = s.shape[0]
        v = torch.topk(s.view(B, -1), k_fg, dim=1).values[:, -1].view(B, 1, 1)
        mask = (s >= v) & (s > 0)
        return mask, mask.view(B, -1).sum(1)

    def merge(x, mask, count, perm_dev, apply_dev):
        B = x.shape[0]
        active = apply_dev & (perm_dev != torch.arange(B, device=x.device)) & (count > 0)
        keep = mask.view(B, 1, 1, H, W) | ~active.view(B, 1, 1, 1, 1)
        x.copy_(torch.where(keep, x, x[perm_dev]))
        return x

    return motion_q, hist_refine, select, merge


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-step', action='store_true', help='do not time the default training step')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import bdvcil_amd as bd
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_fg_merge.py needs a GPU: a CPU run gives no time')
    K = bd.kernels
    dev = torch.device('cuda:0')
    B, T, H, W = args.batch, 8, args.size, args.size
    bins, beta = 8, 0.5
    k_fg = K.fg_k_fg(beta, H, W)
    torch.manual_seed(0)
    perm = torch.randperm(B)
    apply = torch.ones(B, dtype=torch.bool)
    perm_dev, apply_dev = perm.to(dev), apply.to(dev)
    lo, sc = K.fg_colour_params(bins, bd.frontend.IMG_MEAN, bd.frontend.IMG_STD)
    lo_dev, sc_dev, taps_dev = lo.to(dev), sc.to(dev), K.fg_blur_taps(H, W).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f'foreground merging, B={B} T={T} {H}x{W}, beta={beta} bins={bins} prob=1, perm = randperm({B}) (seed 0, '
             f'{int((perm == torch.arange(B)).sum())} fixed points), {args.rounds} interleaved rounds of {args.iters} calls '
             f'(device events; median [min .. max] us per call)']
    slower = []

    def timed(fn, iters=args.iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / iters

    def pair(name, fused, torch_form, fused_bytes):
        for _ in range(2):
            fused(); torch_form()
        torch.cuda.synchronize()
        tf, tt = [], []
        for _ in range(args.rounds):
            tf.append(timed(fused))
            tt.append(timed(torch_form))
        mf, mt = statistics.median(tf), statistics.median(tt)
        verdict = 'fused is NOT slower' if mf <= mt else 'fused is SLOWER'
        if mf > mt:
            slower.append(name)
        lines.append(f'{name:36s} fused {mf:9.1f} [{min(tf):9.1f} .. {max(tf):9.1f}] us {fused_bytes / 1e6:7.1f} MB {fused_bytes / mf / 1e6:5.2f} TB/s | '
                     f'torch {mt:9.1f} [{min(tt):9.1f} .. {max(tt):9.1f}] us | x{mt / mf:6.2f}  {verdict}')
        print(lines[-1], flush=True)
        return mf

    chain_us = {}
    for layout in ('tchw', 'thwc4'):
        # a scene with moving content on a static ground, normalised: motion maps with structure, colours spread over the bins
        raw = torch.randint(0, 256, (B, 1, 3, H, W), device=dev, generator=g).float().repeat(1, T, 1, 1, 1)
        raw[:, :, :, H // 4:H // 2, : W // 2] = torch.randint(0, 256, (B, T, 3, H // 4, W // 2), device=dev, generator=g).float()
        mean = torch.tensor(bd.frontend.IMG_MEAN, device=dev).view(1, 1, 3, 1, 1)
        std = torch.tensor(bd.frontend.IMG_STD, device=dev).view(1, 1, 3, 1, 1)
        planar = ((raw - mean) / std).contiguous()
        del raw
        if layout == 'tchw':
            x, imgs, view = planar, planar, planar
        else:
            x = torch.zeros(B * T, H, W, 4, device=dev)
            x[..., :3] = planar.view(B * T, 3, H, W).permute(0, 2, 3, 1)
            imgs, view = bd.Nhwc4Frames(x, B, T), x.view(B, T, H, W, 4).permute(0, 1, 4, 2, 3)
            del planar
        C = x.numel() * 4
        M = B * H * W * 4
        t_motion, t_hist, t_select, t_merge = torch_stages(T, H, W, bins, k_fg, taps_dev, lo_dev, sc_dev, layout == 'thwc4')
        q, _, _ = K.fg_motion_q(x, B, T, H, W, layout)
        s, _, _ = K.fg_hist_refine(x, q, B, T, H, W, layout, bins, lo, sc)
        _, mask, count = K.fg_select(s, k_fg)
        mask_b = mask.bool()
        idx_bytes = 2 * B * T * H * W
        bytes_motion = C + 6 * M + M // 4
        bytes_hist = C + M // 4 + 2 * idx_bytes + M
        bytes_select = 5 * M + M // 4
        bytes_merge = 2 * C + M // 2          # 4 x the background half
        pair(f'{layout} motion + blur + quantise', lambda: K.fg_motion_q(x, B, T, H, W, layout), lambda: t_motion(view), bytes_motion)
        pair(f'{layout} histograms + refined map', lambda: K.fg_hist_refine(x, q, B, T, H, W, layout, bins, lo, sc), lambda: t_hist(view, q), bytes_hist)
        pair(f'{layout} selection', lambda: K.fg_select(s, k_fg), lambda: t_select(s), bytes_select)
        pair(f'{layout} merge', lambda: K.fg_merge_(x, mask, count, perm, apply, B, T, H, W, layout),
             lambda: t_merge(view, mask_b, count, perm_dev, apply_dev), bytes_merge)

        def fused_chain():
            _, m, c = bd.foreground_mask(imgs, beta, bins)
            K.fg_merge_(x, m, c, perm, apply, B, T, H, W, layout)

        def torch_chain():
            m, c = t_select(t_hist(view, t_motion(view)))
            t_merge(view, m, c, perm.to(dev), apply.to(dev))
        chain_us[layout] = pair(f'{layout} WHOLE CHAIN', fused_chain, torch_chain, bytes_motion + bytes_hist + bytes_select + bytes_merge)
        del x, imgs, view, q, s, mask, mask_b, count
        torch.cuda.empty_cache()

    if not args.no_step:
        import bench
        torch.manual_seed(0)
        model = bd.build_model(bench.model_cfg(50, 101, 'SimpleLinear', 'CrossEntropyLoss', 0.5)).to(dev)
        model.train()
        opt = bd.build_optimizer(model, dict(type='SGD', constructor='CILTSMOptimizerConstructorImprovised',
                                             paramwise_cfg=dict(fc_lr_scale_factor=5.0), lr=0.01, momentum=0.9, weight_decay=1e-4))
        engine = bd.TrainEngine(model, opt, grad_clip=None)
        batch = dict(imgs=torch.randn(B, T, 3, H, W, device=dev, generator=g), label=torch.randint(0, 101, (B, 1), device=dev, generator=g))
        for _ in range(3):
            engine.step(batch)
        torch.cuda.synchronize()
        steps = [timed(lambda: engine.step(batch), iters=5) for _ in range(3)]
        step_us = statistics.median(steps)
        lines.append(f'default training step (TSM-R50, batch {B}, same process): {step_us / 1000:.2f} ms [{min(steps) / 1000:.2f} .. {max(steps) / 1000:.2f}]; '
                     + '; '.join(f'{lay} chain = {100 * us / step_us:.2f} % of it' for lay, us in chain_us.items()))
        print(lines[-1], flush=True)
    lines.append('slower than the torch form: ' + (', '.join(slower) if slower else 'none'))
    lines.append(NOTE)
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
