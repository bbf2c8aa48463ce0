"""A/B of the row-run activation path (bdv_conv_debug_row_run) at the 3x3 stride-1 sites of TSM-R50 (N = 256 frames), in ONE
process, the calls as the training step makes them (tools/tune_conv.py FUSED=1: fprop with the BatchNorm statistics in its
epilogue, dgrad with the BatchNorm-backward statistics).

    python tools/ab_row_run.py time            rows per site and direction: per-tap loader / row run, alternating rounds, median ms
    python tools/ab_row_run.py launch 0|1      the 64-channel site only, switch off | on: a warm-up and two launches per direction,
                                               for rocprofv3 (--pmc passes or --kernel-trace --stats; counters in runs of their own)

Sites on tiles that keep the per-tap loader show the run-to-run spread of the measurement.  Dev tool, GPU only."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bdvcil_amd import kernels as K
from bdvcil_amd._lib import check, lib
from tools.bench_conv import SHAPES, timeit  # noqa: E402

N = int(os.environ.get('N', 256))
dev = torch.device('cuda:0')


def site_calls(Cin, Cout, H):
    g = K.make_geom(N, H, H, Cin, Cout, 3, 3, 1, 1, 8, 0)
    x = torch.randn(N, H, H, Cin, device=dev)
    w = torch.randn(Cout, 3, 3, Cin, device=dev) * 0.05
    dy = torch.randn(N, H, H, Cout, device=dev)
    yprev = torch.randn(N, H, H, Cin, device=dev)
    mask = torch.randint(-2 ** 31, 2 ** 31 - 1, (yprev.numel() // 32,), dtype=torch.int32, device=dev)
    stats = (yprev, mask, torch.randn(Cin, device=dev), torch.rand(Cin, device=dev) + 0.5)
    return g, (lambda: K.conv_fprop(x, w, g, bn_stats=True)), (lambda: K.conv_dgrad(dy, w, g, bn_stats=stats))


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else 'time'
    if mode == 'launch':
        check(lib().bdv_conv_debug_row_run(int(sys.argv[2])), 'bdv_conv_debug_row_run')
        g, fp, dg = site_calls(64, 64, 56)
        for _ in range(3):
            fp()
            dg()
        torch.cuda.synchronize()
        print('done')
        return
    rounds = int(os.environ.get('ROUNDS', 5))
    print(f'{"site":24s} dir    kernel{"":44s} {"per-tap":>8s} {"row run":>8s}  ratio   (median of {rounds} alternating rounds of 7 calls, ms)')
    tot = {0: 0.0, 1: 0.0}
    for (Cin, Cout, k, st, H, cnt, sh) in SHAPES:
        if k != 3 or st != 1:
            continue
        g, fp, dg = site_calls(Cin, Cout, H)
        for name, fn in (('fprop', fp), ('dgrad', dg)):
            ts = {0: [], 1: []}
            for _ in range(rounds):
                for on in (0, 1):
                    check(lib().bdv_conv_debug_row_run(on), 'bdv_conv_debug_row_run')
                    ts[on].append(timeit(fn))
            check(lib().bdv_conv_debug_row_run(1), 'bdv_conv_debug_row_run')
            med = {on: sorted(v)[len(v) // 2] for on, v in ts.items()}
            print(f'{str((Cin, Cout, H)):20s} x{cnt:<2d} {name}  {K.conv_kernel_name(g, name):50s} {med[0]:8.4f} {med[1]:8.4f}  {med[1] / med[0]:.3f}'
                  f'   per-tap {" ".join("%.4f" % t for t in ts[0])} | row run {" ".join("%.4f" % t for t in ts[1])}', flush=True)
            for on in (0, 1):
                tot[on] += med[on] * cnt
    print(f'sum over the step (launches x count): per-tap {tot[0]:.3f} ms, row run {tot[1]:.3f} ms')


if __name__ == '__main__':
    main()
