"""Extract background images for ``BackgroundMixDataset`` on the GPU: the reference's ``cil_tools/extract_background.py`` with its flags.

    python tools/extract_background.py --video_dir DATA/rawframes --output_dir DATA/bg --method sim_cam [--avg_method mean] [--seed S]

Every entry of ``--video_dir`` that matches ``--glob_pattern`` is a frame directory; its background goes to ``<output_dir>/<name>.jpg``.
A video whose ``<output_dir>/<name><image_suffix>`` exists is not redone (the reference's rule), and the two counts the reference prints
are printed.  ``--method sim_cam`` is ``sim_cam_motion_bg_extract`` (RandomResizedCrop to ``--sim_cam_size``, zeros missing, nanmedian /
nanmean over time); ``--method tmf`` is the temporal median of EVERY frame of the directory (``bdvcil_amd.extract_backgrounds``, what
the dataset's own fallback runs).  Videos are taken in sorted order, so that ``--seed`` fixes every crop box."""
import argparse
import os
import pathlib
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--video_dir', required=True)
    ap.add_argument('--glob_pattern', default='*')
    ap.add_argument('--output_dir', required=True)
    ap.add_argument('--num_workers', type=int, default=4, help="host threads of the JPEG entropy stages (the reference's process count)")
    ap.add_argument('--from_video', action='store_true', help='not supported: there is no video decoder, extract the frames first')
    ap.add_argument('--image_suffix', default='.jpg', help='suffix of the files that count as already extracted')
    ap.add_argument('--interval', type=int, default=1, help='sim_cam: take every interval-th frame')
    ap.add_argument('--max_frames', type=int, default=500, help='sim_cam: read at most this many frames')
    ap.add_argument('--size', type=int, default=256, help='accepted and ignored, as the reference ignores it')
    ap.add_argument('--method', default='tmf', choices=['tmf', 'sim_cam'],
                    help="tmf: the median of all frames of the directory; --interval and --max_frames do not apply (the reference's own tmf "
                         "branch for frame directories cannot run: it tests `if img:` on an array)")
    ap.add_argument('--avg_method', default='median', choices=['median', 'mean'], help='sim_cam: np.nanmedian or np.nanmean over time')
    ap.add_argument('--sim_cam_size', type=int, default=100, help='sim_cam: output size of RandomResizedCrop')
    ap.add_argument('--antialias', action='store_true', help="sim_cam: resize with the antialiasing filter (current torchvision's default)")
    ap.add_argument('--seed', type=int, default=None, help="sim_cam: seed of the crop boxes (default: torch's global generator)")
    ap.add_argument('--device', default='cuda')
    return ap


def pending_videos(video_dir, glob_pattern, output_dir, image_suffix):
    """``(found, todo)``: the videos whose background exists, and the others, both sorted."""
    video_dir, output_dir = pathlib.Path(video_dir), pathlib.Path(output_dir)
    paths = sorted(set(video_dir.glob(glob_pattern)))
    found = [p for p in paths if (output_dir / p.name).with_suffix(image_suffix).exists()]
    return found, [p for p in paths if p not in set(found)]


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.from_video:
        ap.exit(2, 'extract_background.py: --from_video is not supported (there is no video decoder); extract the frames and pass their '
                   'directories\n')
    output_dir = pathlib.Path(args.output_dir)
    output_dir.mkdir(exist_ok=True)
    found, todo = pending_videos(args.video_dir, args.glob_pattern, output_dir, args.image_suffix)
    print('Found {} backgrounds'.format(len(found)))
    print('Extracting background from {} videos'.format(len(todo)))
    if not todo:
        return 0

    import bdvcil_amd as bd           # before the first torch.cuda call (GPU_MAX_HW_QUEUES)
    from bdvcil_amd.background import extract_backgrounds
    from bdvcil_amd.decode import JpegDecoder
    decoder = JpegDecoder(args.device, threads=max(1, args.num_workers))
    jobs = [(str(p), str((output_dir / p.name).with_suffix('.jpg'))) for p in todo]
    if args.method == 'sim_cam':
        extract_backgrounds(jobs, decoder, method='sim_cam', avg_method=args.avg_method, interval=args.interval, max_frames=args.max_frames,
                            size=args.sim_cam_size, antialias=args.antialias, draws=args.seed)
    else:
        extract_backgrounds(jobs, decoder)
    return 0


if __name__ == '__main__':
    sys.exit(main())
