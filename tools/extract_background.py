"""Extract background images for ``BackgroundMixDataset`` on the GPU: the reference's ``cil_tools/extract_background.py`` with its flags.

    python tools/extract_background.py --video_dir DATA/rawframes --output_dir DATA/bg --method sim_cam [--avg_method mean] [--seed S]

Every entry of ``--video_dir`` that matches ``--glob_pattern`` is a frame directory; its background goes to ``<output_dir>/<name>.jpg``.
A video whose ``<output_dir>/<name><image_suffix>`` exists is not redone (the reference's rule), and the two counts the reference prints
are printed.  ``--method sim_cam`` is ``sim_cam_motion_bg_extract`` (RandomResizedCrop to ``--sim_cam_size``, zeros missing, nanmedian /
nanmean over time); ``--method tmf`` is the temporal median of EVERY frame of the directory (``bdvcil_amd.extract_backgrounds``, what
the dataset's own fallback runs).  Videos are taken in sorted order, so that ``--seed`` fixes every crop box.

``--method person_masked --det_file DET.npy`` makes person-free backgrounds from the ActorCutMix detection file, in place of the
reference's Mask-RCNN filter ``cil_tools/type_b_and_c_bg.py``: the median over the frames in which a pixel lies outside every person
box (``--det_thres``, ``--dilate``), of the frames named by ``--filename_tmpl``.  ``--max_hole_fraction`` rejects a video in which more
than that share of the pixels was seen uncovered in fewer than ``--min_visible`` frames; ``<output_dir>/person_masked_report.json``
lists every video, and the numbers written and rejected are printed after the reference's two lines."""
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
    ap.add_argument('--method', default='tmf', choices=['tmf', 'sim_cam', 'person_masked'],
                    help="tmf: the median of all frames of the directory; --interval and --max_frames do not apply (the reference's own tmf "
                         "branch for frame directories cannot run: it tests `if img:` on an array); person_masked: the median outside the "
                         "person boxes of --det_file")
    ap.add_argument('--avg_method', default='median', choices=['median', 'mean'], help='sim_cam: np.nanmedian or np.nanmean over time')
    ap.add_argument('--sim_cam_size', type=int, default=100, help='sim_cam: output size of RandomResizedCrop')
    ap.add_argument('--antialias', action='store_true', help="sim_cam: resize with the antialiasing filter (current torchvision's default)")
    ap.add_argument('--seed', type=int, default=None, help="sim_cam: seed of the crop boxes (default: torch's global generator)")
    ap.add_argument('--det_file', default=None, help='person_masked: the ActorCutMix detection file (.npy)')
    ap.add_argument('--det_thres', type=float, default=0.4, help='person_masked: keep boxes with a score above this')
    ap.add_argument('--dilate', type=float, default=0.1, help='person_masked: grow each box by this share of its size on every side')
    ap.add_argument('--min_visible', type=int, default=1, help='person_masked: uncovered frames a pixel needs, else it is a hole')
    ap.add_argument('--max_hole_fraction', type=float, default=None, help='person_masked: reject a video with a larger share of holes')
    ap.add_argument('--filename_tmpl', default='img_{:05}.jpg', help='person_masked: name of the RGB frames')
    ap.add_argument('--device', default='cuda')
    return ap


PERSON_MASKED_FLAGS = ('det_file', 'det_thres', 'dilate', 'min_visible', 'max_hole_fraction', 'filename_tmpl')


def parse_args(argv=None):
    """The parsed flags; a person_masked flag with another method, or person_masked without ``--det_file``, is a usage error."""
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.method != 'person_masked':
        given = [k for k in PERSON_MASKED_FLAGS if getattr(args, k) != ap.get_default(k)]
        if given:
            ap.error('--{} belongs to --method person_masked, not {}'.format(given[0], args.method))
    elif not args.det_file:
        ap.error('--method person_masked needs --det_file')
    return ap, args


def pending_videos(video_dir, glob_pattern, output_dir, image_suffix):
    """``(found, todo)``: the videos whose background exists, and the others, both sorted."""
    video_dir, output_dir = pathlib.Path(video_dir), pathlib.Path(output_dir)
    paths = sorted(set(video_dir.glob(glob_pattern)))
    found = [p for p in paths if (output_dir / p.name).with_suffix(image_suffix).exists()]
    return found, [p for p in paths if p not in set(found)]


def main(argv=None):
    ap, args = parse_args(argv)
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
    if args.method == 'person_masked':
        from bdvcil_amd.background import write_person_masked_report
        params = {k: getattr(args, k) for k in PERSON_MASKED_FLAGS}
        rows = []
        extract_backgrounds(jobs, decoder, method='person_masked', report=rows, **params)
        write_person_masked_report(output_dir, params, rows)
        print('Wrote {} backgrounds'.format(sum(1 for r in rows if r['written'])))
        print('Rejected {} videos'.format(sum(1 for r in rows if not r['written'])))
    elif args.method == 'sim_cam':
        extract_backgrounds(jobs, decoder, method='sim_cam', avg_method=args.avg_method, interval=args.interval, max_frames=args.max_frames,
                            size=args.sim_cam_size, antialias=args.antialias, draws=args.seed)
    else:
        extract_backgrounds(jobs, decoder)
    return 0


if __name__ == '__main__':
    sys.exit(main())
