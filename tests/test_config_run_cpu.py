"""``config_run``: a reference config -> loader class and arguments (against the settings of ten reference configs, one per dataset
family, dumped by tests/golden/make_golden_cil_configs.py), the rejections, ``load_config``, and the loader-owned random state
(``decode.Draws``): a seeded bundle yields what the process-global generators yield after seeding them alike, and leaves them alone."""
import copy
import json
import os
import random

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cil_configs.json')
BGMIX = 'ucf101/bgmix_plus_randAug/bgmix_seed_1000_inc_10_stages_bgmix_plus_randAug.py'
BGMIX_ONLY = 'ucf101/bgmix_only/seed_1000_inc_5_stages_bgmix_only.py'
RANDAUG_ONLY = 'ucf101/randaug_only/seed_1000_inc_5_stages_randAug_only.py'
NO_AUG = 'ucf101/no_aug/seed_1000_inc_10_stages_no_aug.py'
ICARL = 'ucf101/icarl/icarl_seed_1000_inc_10_stages_bgmix_plus_randAug.py'
VIDEO_MIX = 'ucf101/icarl_video_mix/icarl_seed_1000_inc_10_stages_video_mix.py'
ACM = 'ucf101/seed_1000_inc_10_stages_ActorCutMix_plus_randAug.py'
PLACES = 'ucf101/predefined_background/seed_1000_inc_10_stages_bgmix_plus_randAug_place365_bg.py'
STH = 'sth-sthv2/seed_1000_inc_18_stages_bgmix_plus_randAug.py'
HMDB = 'HMDB51/bgmix_seed_1000_inc_5_stages_bgmix_plus_randAug.py'


@pytest.fixture(scope='module')
def configs():
    with open(GOLDEN) as f:
        return json.load(f)


def _stage(pipeline, kind, nth=0):
    return [s for s in pipeline if s['type'] == kind][nth]


def test_fixture_has_one_config_per_family(configs):
    assert sorted(configs) == sorted([BGMIX, BGMIX_ONLY, RANDAUG_ONLY, NO_AUG, ICARL, VIDEO_MIX, ACM, PLACES, STH, HMDB])


@pytest.mark.parametrize('name', [BGMIX, BGMIX_ONLY, RANDAUG_ONLY, NO_AUG, ICARL, PLACES, STH, HMDB])
def test_background_mix_family(configs, name):
    """BackgroundMixDataset: every loader argument is the value the config spells out (or the reference constructor's default)."""
    from bdvcil_amd.config_run import clip_loader_spec
    cfg = configs[name]
    train = cfg['data']['train']
    assert train['type'] == 'BackgroundMixDataset'
    spec = clip_loader_spec(cfg)
    kw = spec['kwargs']
    assert spec['loader'] == 'RawFrameClipLoader' and kw['bg_mix'] is True
    assert kw['with_randAug'] is train.get('with_randAug', False)            # comix_loader.py:33: the reference's default is False
    assert kw['prob'] == train.get('prob', 0.25) and kw['alpha'] == train['alpha'] == 0.5
    ra = _stage(train['pipeline'], 'RandAugment')
    assert kw['randAug'] == dict(n=ra['n'], m=ra['m'], prob=ra['prob']) and ra['prob'] == cfg['randAug_prob']
    sf = _stage(train['pipeline'], 'SampleFrames')
    assert kw['num_segments'] == sf['num_clips'] == 8
    assert kw['short_edge'] == max(_stage(train['pipeline'], 'Resize')['scale']) == 256
    msc = _stage(train['pipeline'], 'MultiScaleCrop')
    assert kw['input_size'] == msc['input_size'] == 224
    assert kw['multi_scale_crop'] == dict(input_size=224, scales=tuple(msc['scales']), max_wh_scale_gap=msc['max_wh_scale_gap'],
                                          random_crop=msc['random_crop'], num_fixed_crops=msc['num_fixed_crops'])
    assert kw['multi_scale_crop']['num_fixed_crops'] == 13
    ds = spec['dataset']
    assert ds['bg_dir'] == train['bg_dir']
    assert ds['extract_bg_if_not_found'] is train.get('extract_bg_if_not_found', True)
    assert ds['map_bg_to_video'] is train.get('map_bg_to_video', True) and ds['merge_bg_files'] is train.get('merge_bg_files', True)


def test_decisive_arguments_per_family(configs):
    from bdvcil_amd.config_run import clip_loader_spec
    kw = {name: clip_loader_spec(cfg)['kwargs'] for name, cfg in configs.items()}
    for name in (BGMIX, ICARL, HMDB, STH, PLACES):
        assert (kw[name]['with_randAug'], kw[name]['randAug']['prob']) == (True, 0.75)
    assert (kw[RANDAUG_ONLY]['with_randAug'], kw[RANDAUG_ONLY]['randAug']['prob']) == (True, 2)
    assert (kw[BGMIX_ONLY]['with_randAug'], kw[BGMIX_ONLY]['prob'], kw[BGMIX_ONLY]['randAug']['prob']) == (False, 0.25, -1)
    assert (kw[NO_AUG]['with_randAug'], kw[NO_AUG]['prob'], kw[NO_AUG]['randAug']['prob']) == (False, -1, -1)
    assert kw[VIDEO_MIX]['bg_mix'] is False and kw[VIDEO_MIX]['randAug'] == dict(n=2, m=10, prob=0.5)
    assert 'with_randAug' not in kw[VIDEO_MIX] and 'prob' not in kw[VIDEO_MIX]
    for name in configs:
        assert kw[name]['test_crop'] == (('CenterCrop', 224) if name == STH else ('TenCrop', 256)), name
    places = clip_loader_spec(configs[PLACES])['dataset']
    assert (places['extract_bg_if_not_found'], places['map_bg_to_video'], places['merge_bg_files']) == (False, False, False)
    assert places['bg_dir'].endswith('place365_val_no_person')


def test_plain_rawframe_and_actor_cut_mix(configs):
    from bdvcil_amd.config_run import clip_loader_spec
    spec = clip_loader_spec(configs[VIDEO_MIX])
    assert configs[VIDEO_MIX]['data']['train']['type'] == 'RawframeDataset' and configs[VIDEO_MIX]['methods'] == 'icarl_video_mix'
    assert spec['loader'] == 'RawFrameClipLoader' and spec['dataset'] == dict(type='RawframeDataset')
    train = configs[ACM]['data']['train']
    spec = clip_loader_spec(configs[ACM])
    assert spec['loader'] == 'ActorCutMixClipLoader'
    assert spec['kwargs']['det_file'] == train['det_file'] and train['det_file'].endswith('detections.npy')
    assert spec['kwargs']['acm_prob'] == train['acm_prob'] == 0.5
    assert (spec['kwargs']['num_segments'], spec['kwargs']['short_edge'], spec['kwargs']['input_size']) == (8, 256, 224)
    assert 'randAug' not in spec['kwargs'] and 'bg_mix' not in spec['kwargs']


def test_rejections_name_the_stage(configs):
    from bdvcil_amd.config_run import clip_loader_spec
    base = configs[BGMIX]

    def changed(edit):
        cfg = copy.deepcopy(base)
        edit(cfg)
        return cfg

    flip = changed(lambda c: c['data']['train']['pipeline'].insert(3, dict(type='Flip', flip_ratio=0.5)))
    with pytest.raises(ValueError, match='train pipeline stage Flip'):
        clip_loader_spec(flip)
    clip2 = changed(lambda c: _stage(c['data']['train']['pipeline'], 'SampleFrames').update(clip_len=2))
    with pytest.raises(ValueError, match='train pipeline stage SampleFrames.*clip_len=2'):
        clip_loader_spec(clip2)
    norm = changed(lambda c: _stage(c['data']['test']['pipeline'], 'Normalize').update(mean=[128.0, 128.0, 128.0]))
    with pytest.raises(ValueError, match='test pipeline stage Normalize'):
        clip_loader_spec(norm)
    norm = changed(lambda c: _stage(c['data']['train']['pipeline'], 'Normalize').update(std=[1.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match='train pipeline stage Normalize'):
        clip_loader_spec(norm)
    kind = changed(lambda c: c['data']['train'].update(type='VideoDataset'))
    with pytest.raises(ValueError, match="data.train type 'VideoDataset'"):
        clip_loader_spec(kind)
    # further settings that would otherwise run as something else
    cases = [
        (lambda c: _stage(c['data']['val']['pipeline'], 'SampleFrames').update(num_clips=16), 'val pipeline stage SampleFrames'),
        (lambda c: _stage(c['data']['val']['pipeline'], 'CenterCrop').update(crop_size=256), 'val pipeline stage CenterCrop'),
        (lambda c: _stage(c['data']['train']['pipeline'], 'Resize', 1).update(scale=(256, 256)), r'train pipeline stage Resize \(after MultiScaleCrop\)'),
        (lambda c: _stage(c['data']['test']['pipeline'], 'Resize').update(scale=(-1, 320)), 'test pipeline stage Resize'),
        (lambda c: c['data']['train']['pipeline'].pop(3), 'train pipeline stage RandAugment'),          # with_randAug=True needs it
        (lambda c: c['data']['train'].update(bg_crop_size=(256, 256)), 'bg_crop_size'),
        (lambda c: c['data']['train']['pipeline'].reverse(), 'train pipeline stage'),
        (lambda c: c['data'].pop('train'), 'data.train'),
    ]
    for edit, pattern in cases:
        with pytest.raises(ValueError, match=pattern):
            clip_loader_spec(changed(edit))
    acm = copy.deepcopy(configs[ACM])
    del acm['data']['train']['det_file']
    with pytest.raises(ValueError, match='det_file'):
        clip_loader_spec(acm)


def test_spec_is_pure(configs):
    """No GPU and no library: the spec of every fixture entry is computed with the kernel library unloadable."""
    import bdvcil_amd._lib as L
    from bdvcil_amd.config_run import clip_loader_spec
    real, L.lib = L.lib, lambda: (_ for _ in ()).throw(AssertionError('clip_loader_spec loaded the kernel library'))
    try:
        before = copy.deepcopy(configs)
        for cfg in configs.values():
            clip_loader_spec(cfg)
        assert before == configs                 # and it does not edit the config
    finally:
        L.lib = real


def test_load_config(tmp_path, monkeypatch):
    from bdvcil_amd.config_run import clip_loader_spec, load_config
    monkeypatch.setenv('VIDEO_CIL_ROOT', str(tmp_path / 'data'))
    path = tmp_path / 'toy_config.py'
    path.write_text('''
import os
data_dir = os.environ['VIDEO_CIL_ROOT']
_private = 3
randAug_prob = 0.75
norm = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_bgr=False)
def helper(crop):
    return [dict(type='SampleFrames', clip_len=1, frame_interval=1, num_clips=8, test_mode=True), dict(type='RawFrameDecode'),
            dict(type='Resize', scale=(-1, 256)), crop, dict(type='Normalize', **norm), dict(type='FormatShape', input_format='NCHW')]
train_pipeline = [dict(type='SampleFrames', clip_len=1, frame_interval=1, num_clips=8), dict(type='RawFrameDecode'),
                  dict(type='Resize', scale=(-1, 256)), dict(type='RandAugment', n=2, m=10, prob=randAug_prob),
                  dict(type='MultiScaleCrop', input_size=224, scales=(1, 0.875), num_fixed_crops=13),
                  dict(type='Resize', scale=(224, 224), keep_ratio=False), dict(type='Normalize', **norm)]
data_root = os.path.join(data_dir, 'rawframes')
optimizer = dict(type='SGD', paramwise_cfg=dict(fc_lr_scale_factor=5.0), lr=0.01)
data = dict(train=dict(type='RawframeDataset', ann_file='', data_prefix=data_root, pipeline=train_pipeline),
            val=dict(type='RawframeDataset', pipeline=helper(dict(type='CenterCrop', crop_size=224))),
            test=dict(type='RawframeDataset', pipeline=helper(dict(type='ThreeCrop', crop_size=256))),
            features_extraction=dict(type='RawframeDataset', pipeline=helper(dict(type='CenterCrop', crop_size=224))))
''')
    cfg = load_config(str(path))
    assert cfg.data_dir == cfg['data_dir'] == str(tmp_path / 'data')
    assert cfg.data_root == os.path.join(str(tmp_path / 'data'), 'rawframes')
    assert cfg.optimizer.paramwise_cfg.fc_lr_scale_factor == cfg['optimizer']['paramwise_cfg']['fc_lr_scale_factor'] == 5.0
    assert cfg.data.train.type == cfg['data']['train']['type'] == 'RawframeDataset'
    assert cfg.data.train.pipeline[3]['prob'] == 0.75 and cfg.get('missing', 5) == 5
    assert 'os' not in cfg and 'helper' not in cfg and '__file__' not in cfg and '__builtins__' not in cfg
    with pytest.raises(AttributeError):
        cfg.no_such_key
    spec = clip_loader_spec(cfg)
    assert spec['loader'] == 'RawFrameClipLoader' and spec['kwargs']['bg_mix'] is False
    assert spec['kwargs']['test_crop'] == ('ThreeCrop', 256) and spec['kwargs']['multi_scale_crop']['scales'] == (1, 0.875)


# ---- loader-owned random state ------------------------------------------------------------------------------------------------------

def _seed_globals(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _global_states():
    return random.getstate(), np.random.get_state(), torch.get_rng_state()


def _same_states(a, b):
    return (a[0] == b[0] and a[1][0] == b[1][0] and (a[1][1] == b[1][1]).all() and a[1][2:] == b[1][2:] and torch.equal(a[2], b[2]))


def _drive(draws):
    """Every host draw site of the loaders, once or more, in one fixed order; ``draws`` None = the globals."""
    from bdvcil_amd.augment import RandAugment
    from bdvcil_amd.decode import sample_frames
    from bdvcil_amd.frontend import BackgroundCropFrontEnd, MultiScaleCropResize, TrainClipFrontEnd
    out = []
    for total in (20, 11, 9, 8, 5, 1):                       # avg > 0; the sorted-randint branch (8 < total < 16); below num_clips: no draw
        out.append(sample_frames(total, 8, draws=draws).tolist())
    for crops in (5, 13):
        m = MultiScaleCropResize(input_size=112, num_fixed_crops=crops, draws=draws)
        out.append([m.draw(170, 128) for _ in range(6)])
    out.append(MultiScaleCropResize(input_size=112, random_crop=True, draws=draws).draw(170, 128))
    bg = BackgroundCropFrontEnd(128, (112, 112), draws=draws)
    out.append(bg.draw(4, 128, 170))
    out.append(bg.draw(3, 112, 112))                         # the resized image has the crop's size: no draw
    out.append(bg.draw(2, 128, 170))
    ra = RandAugment(2, 10, 0.75, draws=draws)
    out.append([ra.draw(128, 170) for _ in range(8)])
    front = TrainClipFrontEnd(None, prob=0.25, with_randAug=False, draws=draws)
    out.append(front.decide(torch.zeros(6, 1, 2, 2, 3, dtype=torch.uint8))[2].tolist())
    return out


def test_seeded_draws_equal_seeded_globals_and_leave_them_alone():
    from bdvcil_amd.decode import Draws
    _seed_globals(7)
    want = _drive(None)
    _seed_globals(99)
    before = _global_states()
    got = _drive(Draws(7))
    assert _same_states(before, _global_states())
    assert repr(got) == repr(want)
    assert want[10] == ([0, 0, 0], [0, 0, 0]) and want[1] == sorted(want[1]) and want[4] == [1, 2, 2, 3, 3, 4, 5, 5]
    # one bundle is one stream: it goes on where it stopped
    d = Draws(7)
    first = _drive(d)
    assert repr(first) == repr(want) and repr(_drive(d)) != repr(want)
    assert _same_states(before, _global_states())


def test_unseeded_stages_still_use_the_globals():
    """``seed=None`` is today's behaviour: the draws come from the process-global generators and advance them."""
    _seed_globals(7)
    a = _drive(None)
    after = _global_states()
    _seed_globals(7)
    before = _global_states()
    b = _drive(None)
    assert repr(a) == repr(b) and not _same_states(before, _global_states()) and _same_states(after, _global_states())
