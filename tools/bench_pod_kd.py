"""Times of the pooled-output distillation kernels (csrc/pod_kd.hip) at the five KD tensors of TSM-R50 with B = 32, T = 8 --
(256, 256, 56, 56), (256, 512, 28, 28), (256, 1024, 14, 14), (256, 2048, 7, 7) and the pooled (256, 2048, 1, 1) -- in fp32 and bf16
storage, forward + backward through autograd, against

  mse        ``functional.kd_mse``, the loss kd_type='pod' replaces (csrc/head_loss.hip)
  composite  the same POD formula written with torch ops (pow, two sums, cat, normalize, norm / cosine_embedding_loss) on the same
             tensors, in their storage type

The three forms are timed interleaved in one process: ``--rounds`` times, ``--iters`` back-to-back forward + backward calls of each
form between two device events; the median round is reported with the fastest and the slowest.  The maps are channels-last views, as
the hooked stage outputs are.  The forward alone (3 launches) and the backward alone (1 launch) of the new kernels are timed the
same way.  Bytes are the algorithm's, computed from the shapes here: with T the bytes of one map and P = N (H + W) C 4 the bytes of
one fp32 profile, POD-spatial moves 2 T + 2 P forward in the profile pass, 4 P + P in the per-frame pass (both profiles twice, G
once) and 2 T + P backward; the MSE moves 2 T forward and 3 T backward.  Information only: nothing in the suite depends on these
numbers.

    python tools/bench_pod_kd.py [--frames 256] [--iters 20] [--rounds 7] [--out profiles/pod_kd.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(256, 56, 56), (512, 28, 28), (1024, 14, 14), (2048, 7, 7), (2048, 1, 1)]      # (C, H, W) per frame


def pod_spatial_torch(cur, prev):
    import torch.nn.functional as F
    import torch
    a, b = cur.pow(2), prev.pow(2)
    p = torch.cat([a.sum(3).flatten(1), a.sum(2).flatten(1)], dim=1)
    q = torch.cat([b.sum(3).flatten(1), b.sum(2).flatten(1)], dim=1)
    return torch.linalg.vector_norm(F.normalize(p, dim=1, eps=1e-12) - F.normalize(q, dim=1, eps=1e-12), dim=1).mean()


def pod_flat_torch(cur, prev, ones):
    import torch.nn.functional as F
    return F.cosine_embedding_loss(cur.flatten(1), prev.flatten(1), ones)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import bdvcil_amd as bd
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_pod_kd.py needs a GPU: a CPU run gives no time')
    K, Fn = bd.kernels, bd.functional
    dev = torch.device('cuda:0')
    N = args.frames
    lines = [f'pooled-output distillation, N={N} frames, {args.rounds} interleaved rounds of {args.iters} calls '
             f'(device events; median [min .. max] us per call); fwd+bwd through autograd unless marked']

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / args.iters

    def stat(ts):
        return f'{statistics.median(ts):8.1f} [{min(ts):8.1f} .. {max(ts):8.1f}] us'

    for storage, dtype in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
        for C, H, W in SIZES:
            g = torch.Generator(device=dev).manual_seed(0)
            x = torch.relu(torch.randn(N, H, W, C, device=dev, generator=g))
            y = torch.relu(x + 0.3 * torch.randn(N, H, W, C, device=dev, generator=g))
            cur = x.to(dtype).permute(0, 3, 1, 2).requires_grad_(True)         # channels-last views, as the hooks return them
            prev = y.to(dtype).permute(0, 3, 1, 2)
            del x, y
            spatial = H * W > 1
            ones = torch.ones(N, dtype=dtype, device=dev)
            new_fn = Fn.kd_pod_spatial if spatial else Fn.kd_pod_flat
            comp_fn = pod_spatial_torch if spatial else (lambda c, p: pod_flat_torch(c, p, ones))

            def run(fn):
                cur.grad = None
                fn(cur, prev).backward()

            forms = {'new': lambda: run(new_fn), 'mse': lambda: run(Fn.kd_mse), 'composite': lambda: run(comp_fn)}
            if spatial:
                _, G, _ = K.pod_spatial_fwd(cur.detach(), prev)
                one = torch.ones(1, device=dev)
                forms['new fwd only'] = lambda: K.pod_spatial_fwd(cur.detach(), prev)
                forms['new bwd only'] = lambda: K.pod_spatial_bwd(cur.detach(), G, one)
            else:
                forms['new fwd only'] = lambda: K.pod_flat(cur.detach(), prev)
            for fn in forms.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in forms}
            for _ in range(args.rounds):
                for k, fn in forms.items():
                    times[k].append(timed(fn))
            med = {k: statistics.median(v) for k, v in times.items()}
            T = cur.numel() * cur.element_size()
            P = N * (H + W) * C * 4
            if spatial:
                by = {'new': 4 * T + 8 * P, 'new fwd only': 2 * T + 7 * P, 'new bwd only': 2 * T + P}
            else:
                by = {'new': 2 * T + 2 * N * C * 4, 'new fwd only': 2 * T + N * C * 4}
            by['mse'] = 5 * T
            head = f'{storage} ({N}, {C}, {H}, {W}) map {T / 1e6:7.1f} MB'
            lines.append(f'{head} | new {stat(times["new"])} {by["new"] / 1e6:7.1f} MB | mse {stat(times["mse"])} {by["mse"] / 1e6:7.1f} MB | '
                         f'composite {stat(times["composite"])} | new/mse {med["new"] / med["mse"]:5.2f} '
                         f'({"within" if med["new"] <= 1.15 * med["mse"] else "OVER"} the 1.15 allowance) | composite/new {med["composite"] / med["new"]:5.2f}')
            print(lines[-1], flush=True)
            for k in ('new fwd only', 'new bwd only'):
                if k in times:
                    lines.append(f'{"":>{len(head)}} | {k} {stat(times[k])} {by[k] / 1e6:7.1f} MB {by[k] / med[k] / 1e6:5.2f} TB/s')
                    print(lines[-1], flush=True)
            del cur, prev, forms
            torch.cuda.empty_cache()
    lines.append('note: every call of a window touches the same buffers; maps up to the 256 MiB Infinity Cache (all but the fp32 and bf16 layer-1 '
                 'and the fp32 layer-2 maps) are served partly from it, so their rates may exceed what HBM alone delivers; the three forms '
                 'run under the same conditions.  fwd+bwd includes the autograd node, the allocation of dcur and the host checks.')
    text = '\n'.join(lines) + '\n'
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
