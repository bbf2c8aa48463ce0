"""Host side of the Grad-CAM / bias-report feature, no GPU: the built-in colormap and the lookup, the box table, the box-shift
arithmetic of ``bias.center_crop_boxes``, the three entry points in header / binding / library, and the report tool's parser."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import bdvcil_amd as bd
from bdvcil_amd import bias, gradcam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('bdv_gradcam_map', 'bdv_gradcam_minmax', 'bdv_gradcam_render', 'bdv_gradcam_workspace_bytes')


def _tool():
    spec = importlib.util.spec_from_file_location('bias_report_tool', os.path.join(ROOT, 'tools', 'bias_report.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_builtin_colormap_table():
    t = gradcam.builtin_colormap()
    assert t.shape == (256, 3) and t.dtype == np.float32 and t.min() >= 0.0 and t.max() <= 1.0
    for i in (0, 1, 63, 64, 127, 128, 191, 200, 255):                  # the formula of the issue, by hand, in fp64
        x = (i + 0.5) / 256
        want = [min(1.0, max(0.0, 1.5 - abs(4 * x - c))) for c in (3, 2, 1)]
        assert np.array_equal(t[i], np.array(want, dtype=np.float32)), i
    assert t[0, 2] > 0.5 and t[0, 0] == 0 and t[255, 0] > 0.5 and t[255, 2] == 0           # blue at 0, red at 1
    assert t[127, 1] == 1.0 and t[128, 1] == 1.0                                           # green plateau in the middle
    assert gradcam.check_colormap(t) is not None


def test_colormap_lookup_is_monotone_and_ends_in_the_last_bin():
    v = np.linspace(0.0, 1.0, 4097)
    idx = gradcam.colormap_index(v)
    assert idx[0] == 0 and idx[-1] == 255 and (np.diff(idx) >= 0).all() and set(idx) == set(range(256))
    assert gradcam.colormap_index(np.float32(255 / 256)) == 255 and gradcam.colormap_index(np.nextafter(np.float32(255 / 256), 0)) == 254
    assert gradcam.colormap_index(1.0 / (1.0 + 1e-20)) == 255


@pytest.mark.parametrize('bad', [np.zeros((255, 3)), np.zeros((256, 4)), np.full((256, 3), 1.5), np.full((256, 3), -0.1),
                                 np.full((256, 3), np.nan)])
def test_colormap_of_wrong_shape_or_range(bad):
    with pytest.raises(ValueError, match='colormap'):
        gradcam.check_colormap(bad)


def test_box_table_is_csr():
    boxes = [[np.array([[1, 2, 3, 4.5]]), np.zeros((0, 4))], [np.array([[0, 0, 1, 1], [5, 5, 6, 6]]), [[7, 7, 8, 8]]]]
    off, rows = gradcam.box_table(boxes, 2, 2)
    assert off.tolist() == [0, 1, 1, 3, 4] and rows.shape == (4, 4) and rows.dtype == np.float32 and rows[0, 3] == 4.5
    off0, rows0 = gradcam.box_table([[[], []]], 1, 2)
    assert off0.tolist() == [0, 0, 0] and rows0.shape == (0, 4)
    assert gradcam.box_table((off, rows), 2, 2)[0] is not None
    with pytest.raises(ValueError, match='clips'):
        gradcam.box_table(boxes, 2, 3)


def test_box_shift_hand_case():
    """320 x 240 -> Resize(-1, 256): 341 x 256 (mmcv: int(x * f + 0.5)), float32 factors 341/320 and 256/240; CenterCrop(224) starts at
    ((341 - 224) // 2, (256 - 224) // 2) = (58, 16)."""
    d = [np.array([[10., 20., 100., 200.], [300., 0., 320., 240.]]), np.zeros((0, 4))]
    keep = [a.copy() for a in d]
    out = bias.center_crop_boxes(d, 320, 240, 256, 224)
    fx, fy = float(np.float32(341 / 320)), float(np.float32(256 / 240))       # the float32 factors of ResizeWithBox, in fp64
    want = np.array([[0.0, 20 * fy - 16, 100 * fx - 58, 200 * fy - 16], [224.0, 0.0, 224.0, 224.0]])     # 300 * fx - 58 = 261.7: clipped to the crop, an empty box
    assert np.allclose(out[0], want, rtol=0, atol=1e-12) and out[1].shape == (0, 4)
    assert out[0].dtype == np.float64 and (out[0] != np.floor(out[0])).any()               # float, not the cut-out's astype(int)
    assert all(np.array_equal(a, b) for a, b in zip(d, keep))                              # the detections are not edited
    ints = bias.center_crop_boxes([np.array([[10, 20, 100, 200]])], 320, 240, 256, 224)
    assert ints[0].dtype == np.float32 and abs(ints[0][0, 1] - (20 * fy - 16)) < 1e-4


def test_header_binding_and_library_agree_on_the_gradcam_symbols():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bdvcil_hip.h')).read(), flags=re.S)
    lib = ctypes.CDLL(bd._lib.LIB_PATH)
    for name in NEW:
        m = re.search(r'^(?:int|size_t)\s+' + name + r'\s*\((.*?)\);', hdr, re.S | re.M)
        assert m, f'{name} is not declared in include/bdvcil_hip.h'
        params = [p.strip() for p in m.group(1).split(',')]
        assert hasattr(lib, name) and name in bd._lib.SIGNATURES
        res, args = bd._lib.SIGNATURES[name]
        assert len(args) == len(params), (name, len(args), params)
        for p, a in zip(params, args):
            assert ('*' in p or '[' in p) == (a is bd._lib.P or a is bd._lib._F3), (name, p, a)
    assert 'gradcam.hip' in bd._lib.HASHED_SOURCES
    mk = open(os.path.join(ROOT, 'background-debiased-video-cil_amd', 'csrc', 'Makefile')).read()
    assert 'gradcam.hip' in re.search(r'^SRCS = (.*)$', mk, re.M).group(1).split()
    assert bd._lib.lib().bdv_gradcam_workspace_bytes(2, 8, 224) == 2 * 8 * 224 * 16
    assert bd._lib.lib().bdv_gradcam_workspace_bytes(0, 8, 224) == 0
    for fn in ('gradcam_map', 'gradcam_minmax', 'gradcam_render'):
        assert callable(getattr(bd.kernels, fn))
    assert bd.GradCAM is gradcam.GradCAM


def test_library_validates_before_any_launch():
    """The pointers are never dereferenced: every call fails on its arguments (the box table on its host copy)."""
    L = bd._lib.lib()
    A, Bp = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)
    f3 = (ctypes.c_float * 3)(0, 0, 0)
    assert L.bdv_gradcam_map(A, A, Bp, 1, 4, 6, None) != 0 and b'multiple of 4' in L.bdv_last_error()
    assert L.bdv_gradcam_map(ctypes.c_void_p((1 << 20) + 4), A, Bp, 1, 4, 8, None) != 0 and b'aligned' in L.bdv_last_error()
    assert L.bdv_gradcam_minmax(A, 70000, 1, 2, 2, 4, 4, Bp, None) != 0 and b'bad shape' in L.bdv_last_error()
    render = lambda off, boxes, n: L.bdv_gradcam_render(A, A, 1, 2, 2, 2, 4, 4, None, None, None, 0.5, f3, f3, None, A, off.ctypes.data, A,
                                                        boxes.ctypes.data, n, Bp, Bp, 1 << 20, None)
    one = np.zeros((1, 4), np.float32)
    assert render(np.array([0, 1, 0], np.int32), one, 1) != 0 and b'decrease' in L.bdv_last_error()
    assert render(np.array([0, 1, 2], np.int32), one, 1) != 0 and b'end at 2' in L.bdv_last_error()
    assert render(np.array([1, 1, 1], np.int32), one, 1) != 0 and b'start at 0' in L.bdv_last_error()
    assert render(np.array([0, 1, 1], np.int32), np.full((1, 4), np.nan, np.float32), 1) != 0 and b'NaN' in L.bdv_last_error()
    assert L.bdv_gradcam_render(A, A, 1, 2, 2, 2, 4, 4, None, None, None, 0.5, f3, f3, None, None, None, None, None, 0, None, None, 0,
                                None) != 0 and b'no output' in L.bdv_last_error()


def test_gradcam_refuses_what_it_cannot_do():
    import torch
    from oracle import tsm_oracle as O
    model = bd.build_model(O.r50_cfg(num_classes=5, depth=18, head='LocalSimilarityClassifier', loss='LSCLoss'))
    with pytest.raises(AttributeError, match='backbone.layer9'):
        bd.GradCAM(model, 'backbone.layer9')
    with pytest.raises(ValueError, match='colormap'):
        bd.GradCAM(model, colormap=np.zeros((16, 3)))
    cam = bd.GradCAM(model)
    with pytest.raises(ValueError, match='one clip per sample'):
        cam(torch.zeros(1, 16, 3, 32, 32))
    with pytest.raises(ValueError, match='alpha'):
        cam(torch.zeros(1, 8, 3, 32, 32), alpha=1.5)
    with pytest.raises(ValueError, match='labels'):
        cam(torch.zeros(2, 8, 3, 32, 32), [1])
    prev = bd.set_conv_arith('bf16')
    try:
        with pytest.raises(NotImplementedError, match='bf16x1'):
            cam(torch.zeros(1, 8, 3, 32, 32))
    finally:
        bd.set_conv_arith('bf16x3')
        bd.kernels.FPROP_X3, bd.kernels.DGRAD_X3, bd.kernels.WGRAD_X3 = prev
    i3d = object.__new__(bd.Recognizer3D)
    with pytest.raises(NotImplementedError, match='Recognizer3D'):
        bd.GradCAM(i3d)


def test_tool_parser_and_missing_checkpoints(tmp_path):
    tool = _tool()
    a = tool.build_parser().parse_args(['work', 'cfg.py', '--det-file', 'd.npy', '--tasks', '0', '2', '--overlays', '3',
                                        '--target-layer', 'backbone.layer3', '--conv-arith', 'f32mfma', '--seed', '7'])
    assert (a.work_dir, a.config, a.det_file, a.tasks, a.overlays, a.target_layer, a.conv_arith, a.seed) == \
        ('work', 'cfg.py', 'd.npy', [0, 2], 3, 'backbone.layer3', 'f32mfma', 7)
    d = tool.build_parser().parse_args(['work', 'cfg.py'])
    assert d.det_file is None and d.tasks is None and d.overlays == 0 and d.target_layer == 'backbone.layer4' and d.conv_arith is None
    with pytest.raises(SystemExit):
        tool.build_parser().parse_args(['work', 'cfg.py', '--conv-arith', 'bf16'])          # no eval-mode backward in that storage
    assert set(tool.CONV_ARITH_MODES) == set(bd.CONV_ARITH_MODES) - {'bf16'}
    with pytest.raises(FileNotFoundError, match='ckpt_task'):
        tool.main([str(tmp_path), str(tmp_path / 'cfg.py')])                               # refused before config, GPU or any write
    assert list(tmp_path.iterdir()) == []
    (tmp_path / 'ckpt').mkdir()
    for t in (0, 1, 10):
        (tmp_path / 'ckpt' / f'ckpt_task_{t}.pt').write_bytes(b'')
    (tmp_path / 'ckpt' / 'exemplar_class_mean_task_0.pt').write_bytes(b'')
    assert list(tool.find_checkpoints(tmp_path)) == [0, 1, 10]
    assert list(tool.find_checkpoints(tmp_path, [10, 0])) == [0, 10]
    with pytest.raises(FileNotFoundError, match=r'\[3\]'):
        tool.find_checkpoints(tmp_path, [0, 3])
    (tmp_path / 'cnn_result.txt').write_text('CNN Accuraciesrange      0-1    2-3    Avg\n-------  -----  -----  -----\ntask 0   75.00         75.00\n'
                                             'task 1   50.00  25.00  37.50\navg_acc                56.25\n')
    assert tool.cnn_result_averages(tmp_path) == {0: 75.0, 1: 37.5}
    assert tool.json_ready({'a': [float('nan'), 1.0]}) == {'a': [None, 1.0]}
    table = tool.report_table([dict(task=0, cnn_top1=None, scene_only_top1=50.0, scene_clips=4, scene_missing=1)], False)
    assert 'task 0' in table and '50.00' in table and 'actor_attention' not in table
