"""From a reference config file to a running loop: ``load_config`` reads the file, ``clip_loader_spec`` turns its ``data.train`` and
its four pipelines into the loader class and constructor arguments that compute the same thing, ``build_clip_loader`` instantiates it.

The reference builds its datasets through mmaction2's registry (libs/cil/cil.py:128-135): ``data.train.type`` names the dataset class,
its other keys are constructor arguments, and the pipelines are lists of stage dicts.  The loaders of this package run fixed chains of
device stages instead, so only configs that describe such a chain can be honoured.  ``clip_loader_spec`` therefore checks every stage and
every argument it reads, and a stage or value the loaders cannot reproduce raises a ``ValueError`` naming it: a loader that silently
computes something else than the config says is the failure this module exists to prevent.

Dataset families (``data.train.type``):

  ``BackgroundMixDataset``   ``RawFrameClipLoader(with_randAug=..., prob=..., alpha=..., bg_mix=True)``; the constructor defaults are the
                             reference's (libs/loader/comix_loader.py:18-40: ``with_randAug=False, prob=0.25, alpha=0.5``), not the loader's
  ``RawframeDataset``        ``RawFrameClipLoader(bg_mix=False)``: RandAugment on its own, no background
  ``ActorCutMixDataset``     ``ActorCutMixClipLoader(det_file, acm_prob)``; its train chain is fixed inside the dataset class
                             (libs/loader/actor_cut_mix_loader.py:37-96), ``data.train`` carries no pipeline

``clip_loader_spec`` is plain Python on plain dicts (a config, or its JSON dump): no GPU, no library."""
from __future__ import annotations

import os
import types
from typing import Optional, Sequence

IMG_MEAN = (123.675, 116.28, 103.53)          # frontend.IMG_MEAN / IMG_STD (kept literal: this module imports nothing of the package
IMG_STD = (58.395, 57.12, 57.375)             # at import time)

_TEST_CROPS = ('CenterCrop', 'ThreeCrop', 'FiveCrop', 'TenCrop')
_PASSIVE = ('RawFrameDecode', 'Collect', 'ToTensor')        # stages without arithmetic: decode is the loader's, the rest is collation


def load_config(path: str):
    """Execute a config file (Python source, as the reference's ``mmcv.Config.fromfile`` does) and return its public names as an
    ``AttrDict``: everything not starting with ``__`` that is not a module or a function, nested dicts reachable by attribute and by
    item.  The CIL configs are self-contained and read ``VIDEO_CIL_ROOT`` from the environment."""
    from .task_loop import AttrDict
    path = os.path.abspath(os.fspath(path))
    with open(path, 'r') as f:
        source = f.read()
    scope = {'__file__': path, '__name__': '_bdvcil_config_'}
    exec(compile(source, path, 'exec'), scope)
    return AttrDict({k: v for k, v in scope.items()
                     if not k.startswith('__') and not isinstance(v, (types.ModuleType, types.FunctionType))})


def _fail(stage: str, why: str):
    raise ValueError(f'{stage}: {why}')


def _pair(v):
    return (v, v) if isinstance(v, (int, float)) else tuple(v)


def _close(a: Sequence[float], b: Sequence[float]) -> bool:
    return len(a) == len(b) and all(abs(float(x) - float(y)) <= 1e-6 * max(1.0, abs(float(y))) for x, y in zip(a, b))


def _stages(pipeline, where: str, allowed: Sequence[str]):
    """The stage dicts of a pipeline with their types checked against ``allowed`` (order is checked by the callers)."""
    if not isinstance(pipeline, (list, tuple)) or not pipeline:
        _fail(where, 'no pipeline (a list of stage dicts) in the config')
    for st in pipeline:
        t = st.get('type')
        if t not in allowed:
            _fail(f'{where} stage {t}', 'not a stage the clip loaders run (they run ' + ' -> '.join(a for a in allowed if a not in _PASSIVE) + ')')
    return list(pipeline)


def _only(stages, kind: str, where: str, required: bool = True):
    got = [s for s in stages if s.get('type') == kind]
    if len(got) > 1 or (required and not got):
        _fail(f'{where} stage {kind}', f'expected exactly one, found {len(got)}')
    return got[0] if got else None


def _sample_frames(stages, where: str, test_mode: bool) -> int:
    if stages[0].get('type') != 'SampleFrames':
        _fail(f'{where} stage {stages[0].get("type")}', 'the pipeline must start with SampleFrames')
    st = _only(stages, 'SampleFrames', where)
    name = f'{where} stage SampleFrames'
    if st.get('clip_len', None) != 1:
        _fail(name, f'clip_len={st.get("clip_len")!r}: the loaders sample clip_len=1 segments (TSM)')
    if st.get('frame_interval', 1) != 1:
        _fail(name, f'frame_interval={st.get("frame_interval")!r}: only 1 is implemented')
    if bool(st.get('test_mode', False)) != test_mode:
        _fail(name, f'test_mode={st.get("test_mode", False)!r} in the {where}')
    for key, default in (('temporal_jitter', False), ('twice_sample', False), ('out_of_bound_opt', 'loop'), ('start_index', None),
                         ('keep_tail_frames', False)):
        if st.get(key, default) != default:
            _fail(name, f'{key}={st[key]!r} is not implemented')
    return int(st.get('num_clips', 1))


def _short_edge(stages, where: str) -> int:
    """The first Resize: ``scale=(-1, S)``, keep_ratio."""
    resizes = [s for s in stages if s.get('type') == 'Resize']
    if not resizes:
        _fail(f'{where} stage Resize', 'missing: the loaders resize the short edge first')
    st, name = resizes[0], f'{where} stage Resize'
    scale = _pair(st.get('scale'))
    if len(scale) != 2 or -1 not in scale or max(scale) < 1 or not st.get('keep_ratio', True):
        _fail(name, f'scale={st.get("scale")!r}, keep_ratio={st.get("keep_ratio", True)!r}: the first Resize must be (-1, S) with keep_ratio')
    for key in ('interpolation', 'lazy'):
        if st.get(key, {'interpolation': 'bilinear', 'lazy': False}[key]) != {'interpolation': 'bilinear', 'lazy': False}[key]:
            _fail(name, f'{key}={st[key]!r} is not implemented')
    return int(max(scale))


def _fixed_resize(st, size: int, name: str):
    """A ``Resize(scale=(size, size), keep_ratio=False)``: the second Resize of the train chain, or a no-op after a crop of that size."""
    if tuple(_pair(st.get('scale'))) != (size, size) or st.get('keep_ratio', True):
        _fail(name, f'scale={st.get("scale")!r}, keep_ratio={st.get("keep_ratio", True)!r}: expected ({size}, {size}) with keep_ratio=False')


def _normalize(stages, where: str):
    st, name = _only(stages, 'Normalize', where), f'{where} stage Normalize'
    if not _close(st.get('mean', ()), IMG_MEAN) or not _close(st.get('std', ()), IMG_STD):
        _fail(name, f'mean={st.get("mean")!r}, std={st.get("std")!r}: the loaders normalise with {IMG_MEAN} / {IMG_STD}')
    if st.get('to_bgr', False):
        _fail(name, 'to_bgr=True is not implemented')
    fmt = _only(stages, 'FormatShape', where, required=False)
    if fmt is not None and fmt.get('input_format') != 'NCHW':
        _fail(f'{where} stage FormatShape', f'input_format={fmt.get("input_format")!r}: the loaders emit NCHW clips')


def _order(stages, order: Sequence[str], where: str):
    """The arithmetic stages must come in the loaders' order (``order`` may name optional stages)."""
    pos = 0
    for st in stages:
        t = st['type']
        if t in _PASSIVE:
            continue
        if t not in order[pos:]:
            _fail(f'{where} stage {t}', f'out of order or repeated: the loaders run {" -> ".join(order)}')
        pos = order.index(t, pos) + 1


def _train_pipeline(pipeline, where='train pipeline'):
    stages = _stages(pipeline, where, ('SampleFrames', 'RawFrameDecode', 'Resize', 'RandAugment', 'MultiScaleCrop', 'Normalize',
                                       'FormatShape', 'Collect', 'ToTensor'))
    _order(stages, ('SampleFrames', 'Resize', 'RandAugment', 'MultiScaleCrop', 'Resize', 'Normalize', 'FormatShape'), where)
    out = dict(num_segments=_sample_frames(stages, where, False), short_edge=_short_edge(stages, where))
    ra = _only(stages, 'RandAugment', where, required=False)
    out['randAug'] = None if ra is None else dict(n=int(ra.get('n')), m=int(ra.get('m')), prob=ra.get('prob', 0.5))
    msc = _only(stages, 'MultiScaleCrop', where)
    name = f'{where} stage MultiScaleCrop'
    size = msc.get('input_size')
    if not isinstance(size, int) and len(set(_pair(size))) != 1:
        _fail(name, f'input_size={size!r}: the loaders crop to a square input')
    size = int(_pair(size)[0])
    crop = dict(input_size=size, scales=tuple(msc.get('scales', (1,))), max_wh_scale_gap=int(msc.get('max_wh_scale_gap', 1)),
                random_crop=bool(msc.get('random_crop', False)), num_fixed_crops=int(msc.get('num_fixed_crops', 5)))
    if crop['num_fixed_crops'] not in (5, 13):
        _fail(name, f'num_fixed_crops={crop["num_fixed_crops"]}: 5 or 13')
    if msc.get('lazy', False):
        _fail(name, 'lazy=True is not implemented')
    out['input_size'], out['multi_scale_crop'] = size, crop
    resizes = [s for s in stages if s['type'] == 'Resize']
    if len(resizes) != 2:
        _fail(f'{where} stage Resize', f'expected two (short edge, then the fixed size after MultiScaleCrop), found {len(resizes)}')
    _fixed_resize(resizes[1], size, f'{where} stage Resize (after MultiScaleCrop)')
    _normalize(stages, where)
    return out


def _eval_pipeline(pipeline, where: str, crops: Sequence[str]):
    """val / features_extraction / test: SampleFrames(test_mode) -> decode -> Resize(-1, S) -> one crop -> Normalize.  Returns
    ``(num_segments, short_edge, (crop kind, crop size))``."""
    stages = _stages(pipeline, where, ('SampleFrames', 'RawFrameDecode', 'Resize') + tuple(crops) + ('Normalize', 'FormatShape', 'Collect', 'ToTensor'))
    found = [s for s in stages if s['type'] in crops]
    if len(found) != 1:
        _fail(f'{where} stage {"/".join(crops)}', f'expected exactly one crop stage, found {len(found)}')
    kind = found[0]['type']
    _order(stages, ('SampleFrames', 'Resize', kind, 'Resize', 'Normalize', 'FormatShape'), where)
    size = found[0].get('crop_size')
    if not isinstance(size, int) and len(set(_pair(size))) != 1:
        _fail(f'{where} stage {kind}', f'crop_size={size!r}: a square crop is expected')
    size = int(_pair(size)[0])
    if found[0].get('lazy', False):
        _fail(f'{where} stage {kind}', 'lazy=True is not implemented')
    for extra in [s for s in stages if s['type'] == 'Resize'][1:]:         # the features_extraction pipelines resize to the crop's size again
        _fixed_resize(extra, size, f'{where} stage Resize (after {kind})')
    _normalize(stages, where)
    return _sample_frames(stages, where, True), _short_edge(stages, where), (kind, size)


_DATASET_COMMON = dict(with_offset=False, multi_class=False, num_classes=None, modality='RGB', sample_by_class=False, power=0.0,
                       dynamic_length=False)


_BG_METHODS = ('tmf', 'sim_cam', 'person_masked')          # background.METHODS
_BG_EXTRACTION_KEYS = ('method', 'det_file', 'det_thres', 'dilate', 'min_visible', 'max_hole_fraction', 'filename_tmpl')


def bg_extraction_spec(train) -> Optional[dict]:
    """``data.train.bg_extraction`` checked and as ``resolve_bg_files`` takes it, or None when the config has none (missing backgrounds
    are then made as the reference makes them, by the temporal median).  The key is this package's own: ``dict(method='person_masked',
    det_file=..., det_thres=..., dilate=..., min_visible=..., max_hole_fraction=...)`` extracts person-free backgrounds from the
    ActorCutMix detection file; ``filename_tmpl`` defaults to the dataset's."""
    ext = train.get('bg_extraction')
    if ext is None:
        return None
    where = 'data.train bg_extraction'
    if not hasattr(ext, 'items'):
        _fail(where, f'{ext!r} is not a dict')
    ext = dict(ext)
    for key in ext:
        if key not in _BG_EXTRACTION_KEYS:
            _fail(f'{where} {key}', f'unknown key (the keys are {", ".join(_BG_EXTRACTION_KEYS)})')
    method = ext.setdefault('method', 'tmf')               # extract_backgrounds' default
    if method not in _BG_METHODS:
        _fail(f'{where} method', f'{method!r} is not one of {_BG_METHODS}')
    if method != 'person_masked':
        if len(ext) > 1:
            _fail(f'{where} {[k for k in ext if k != "method"][0]}', f"belongs to method 'person_masked', not {method!r}")
        return ext
    if not ext.get('det_file'):
        _fail(f'{where} det_file', "missing: method 'person_masked' reads the ActorCutMix detection file")
    ext.setdefault('filename_tmpl', train.get('filename_tmpl', 'img_{:05}.jpg'))
    return ext


def clip_loader_spec(config) -> dict:
    """``{'loader': class name, 'kwargs': constructor arguments, 'dataset': what the loop reads from data.train}`` for a config (see the
    module docstring).  ``kwargs['randAug']`` is the ``dict(n, m, prob)`` of the RandAugment stage, which the loaders accept in place of
    an instance.  Raises ``ValueError`` naming the stage or argument that cannot be honoured."""
    data = config.get('data') if hasattr(config, 'get') else None
    if not data or not data.get('train'):
        _fail('data.train', 'missing from the config')
    train = dict(data['train'])
    kind = train.get('type')
    if kind not in ('BackgroundMixDataset', 'RawframeDataset', 'ActorCutMixDataset'):
        _fail(f'data.train type {kind!r}', 'unknown dataset type (BackgroundMixDataset, RawframeDataset and ActorCutMixDataset have loaders)')
    for key, default in _DATASET_COMMON.items():
        if train.get(key, default) != default:
            _fail(f'data.train ({kind}) {key}', f'{train[key]!r} is not implemented')
    if train.get('test_mode', False):
        _fail(f'data.train ({kind}) test_mode', 'True in the training set')
    kw = dict(filename_tmpl=train.get('filename_tmpl', 'img_{:05}.jpg'), start_index=int(train.get('start_index', 1)))
    for part in ('val', 'test', 'features_extraction'):
        d = data.get(part) or {}
        for key in ('filename_tmpl', 'start_index'):
            if key in d and d[key] != kw[key]:
                _fail(f'data.{part} {key}', f'{d[key]!r} differs from data.train\'s {kw[key]!r}: one loader reads every phase')

    # the three evaluation pipelines
    for part in ('val', 'test', 'features_extraction'):
        if not (data.get(part) or {}).get('pipeline'):
            _fail(f'data.{part}', 'no pipeline in the config')
    val_T, val_S, val_crop = _eval_pipeline(data['val']['pipeline'], 'val pipeline', ('CenterCrop',))
    fe_T, fe_S, fe_crop = _eval_pipeline(data['features_extraction']['pipeline'], 'features_extraction pipeline', ('CenterCrop',))
    test_T, test_S, test_crop = _eval_pipeline(data['test']['pipeline'], 'test pipeline', _TEST_CROPS)
    if data.get('features_extraction_epochs', 1) != 1:
        _fail('data.features_extraction_epochs', f'{data["features_extraction_epochs"]!r}: the feature pipeline is deterministic, 1 epoch')

    if kind == 'ActorCutMixDataset':
        # the dataset's own chains (actor_cut_mix_loader.py:37-96): 8 segments, Resize(-1, 256), 224 x 224, RandAugment(2, 10, prob=1)
        if not train.get('det_file'):
            _fail('data.train (ActorCutMixDataset) det_file', 'missing')
        tr = dict(num_segments=8, short_edge=256, input_size=224)
        kw.update(det_file=train['det_file'], acm_prob=train.get('acm_prob', 1), **tr)
        loader = 'ActorCutMixClipLoader'
    else:
        tr = _train_pipeline(train.get('pipeline'))
        ra = tr.pop('randAug')
        loader = 'RawFrameClipLoader'
        if kind == 'BackgroundMixDataset':
            with_ra = bool(train.get('with_randAug', False))
            if with_ra and ra is None:
                _fail('train pipeline stage RandAugment', 'missing, but data.train.with_randAug=True mixes the samples RandAugment skipped')
            S = tr['input_size']
            if tuple(_pair(train.get('bg_crop_size', (224, 224)))) != (S, S):
                _fail('data.train (BackgroundMixDataset) bg_crop_size', f'{train.get("bg_crop_size", (224, 224))!r} is not the clips\' {S} x {S}')
            if not _close(train.get('bg_mean', IMG_MEAN), IMG_MEAN) or not _close(train.get('bg_std', IMG_STD), IMG_STD):
                _fail('data.train (BackgroundMixDataset) bg_mean / bg_std', f'the loaders normalise backgrounds with {IMG_MEAN} / {IMG_STD}')
            kw.update(with_randAug=with_ra, prob=train.get('prob', 0.25), alpha=train.get('alpha', 0.5), bg_mix=True,
                      bg_resize=int(train.get('bg_resize', 256)))
        else:
            kw.update(bg_mix=False)
        # a pipeline without the stage never augments; the loaders' RandAugment with prob -1 never fires
        kw.update(randAug=ra if ra is not None else dict(n=2, m=10, prob=-1), **tr)

    for name, T, S in (('val', val_T, val_S), ('features_extraction', fe_T, fe_S), ('test', test_T, test_S)):
        if T != kw['num_segments']:
            _fail(f'{name} pipeline stage SampleFrames', f'num_clips={T}, the train chain samples {kw["num_segments"]}: one loader reads every phase')
        if S != kw['short_edge']:
            _fail(f'{name} pipeline stage Resize', f'short edge {S}, the train chain resizes to {kw["short_edge"]}')
    for name, crop in (('val', val_crop), ('features_extraction', fe_crop)):
        if crop[1] != kw['input_size']:
            _fail(f'{name} pipeline stage CenterCrop', f'crop_size={crop[1]}, the training clips are {kw["input_size"]}')
    kw['test_crop'] = test_crop
    dataset = dict(type=kind)
    if kind == 'BackgroundMixDataset':
        dataset.update(bg_dir=train.get('bg_dir'), extract_bg_if_not_found=train.get('extract_bg_if_not_found', True),
                       back_ground_from_bg_dir=train.get('back_ground_from_bg_dir', True), map_bg_to_video=train.get('map_bg_to_video', True),
                       merge_bg_files=train.get('merge_bg_files', True), bg_image_extension=train.get('bg_image_extension', '.jpg'))
        ext = bg_extraction_spec(train)
        if ext is not None:
            dataset.update(bg_extraction=ext)
    elif train.get('bg_extraction') is not None:
        _fail(f'data.train ({kind}) bg_extraction', 'only BackgroundMixDataset reads a bg_dir')
    return dict(loader=loader, kwargs=kw, dataset=dataset)


def build_clip_loader(config, device='cuda', seed: Optional[int] = None, **overrides):
    """The ``clip_loader`` of ``CILTaskLoop`` for a config: ``clip_loader_spec`` instantiated on ``device``.  ``seed``: the loader's own
    random state (``decode.Draws``); None = the process-global generators.  ``overrides``: further constructor arguments
    (``threads=...``)."""
    spec = clip_loader_spec(config)
    from . import actor_cut_mix, decode
    cls = {'RawFrameClipLoader': decode.RawFrameClipLoader, 'ActorCutMixClipLoader': actor_cut_mix.ActorCutMixClipLoader}[spec['loader']]
    kw = dict(spec['kwargs'])
    kw.update(overrides)
    return cls(device=device, seed=seed, **kw)
