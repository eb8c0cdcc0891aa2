"""BADJA evaluation without a GPU: the annotation loader, the joint constant, the restatement of the keypoint transfer in closed
form, the command line of scripts/eval_badja.py and the host-side checks of lasr_kp_transfer."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import badja_restated as br                       # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'badja')
F32 = np.float32


def write_tree(root, seq, n=3, size=(40, 60), mask_size=None):
    from PIL import Image
    rng = np.random.default_rng(0)
    annos = []
    for i in range(n):
        img = 'DAVIS/JPEGImages/Full-Resolution/%s/%05d.jpg' % (seq, 10 + 3 * i)
        seg = 'DAVIS/Annotations/Full-Resolution/%s/%05d.png' % (seq, 10 + 3 * i)
        os.makedirs(os.path.dirname(os.path.join(root, img)), exist_ok=True)
        os.makedirs(os.path.dirname(os.path.join(root, seg)), exist_ok=True)
        Image.fromarray(rng.integers(0, 255, size + (3,), dtype=np.uint8)).save(os.path.join(root, img))
        ms = mask_size or size
        m = np.zeros(ms, np.uint8)
        m[5:20, 10:30] = 1
        pal = Image.fromarray(m, 'P')
        pal.putpalette([0, 0, 0, 128, 0, 0] + [0] * 762)
        pal.save(os.path.join(root, seg))
        joints = (np.arange(37)[:, None] * [1, 2] + i).tolist()
        annos.append({'image_path': img, 'segmentation_path': seg, 'joints': joints,
                      'visibility': [bool((k + i) % 3) for k in range(37)]})
    annos.append({'image_path': 'DAVIS/missing.jpg', 'segmentation_path': 'DAVIS/missing.png', 'joints': [[0, 0]] * 37,
                  'visibility': [False] * 37})
    os.makedirs(os.path.join(root, 'joint_annotations'), exist_ok=True)
    with open(os.path.join(root, 'joint_annotations', '%s.json' % seq), 'w') as fh:
        json.dump(annos, fh)
    return annos


def test_loader_selects_the_annotated_joints(tmp_path):
    from lasr_amd.ext_utils.badja_data import BADJAData, ANNOTATED_JOINTS, frame_number
    annos = write_tree(str(tmp_path), 'synth')
    data = BADJAData('synth', root=str(tmp_path))
    got = list(data.get_loader())
    assert len(got) == 3                                             # the entry without files is skipped
    for i, (rgb, sil, joints, visible, name) in enumerate(got):
        assert rgb.shape == (40, 60, 3) and rgb.dtype == np.uint8
        assert sil.shape == (40, 60, 3) and (sil[..., 0] > 0).sum() == 15 * 20
        np.testing.assert_array_equal(joints, np.asarray(annos[i]['joints'])[ANNOTATED_JOINTS])
        np.testing.assert_array_equal(visible, np.asarray(annos[i]['visibility'])[ANNOTATED_JOINTS])
        assert joints.shape == (20, 2) and visible.dtype == bool
        assert frame_number(name) == 10 + 3 * i


def test_loader_refuses_a_mask_of_another_size(tmp_path):
    from lasr_amd.ext_utils.badja_data import BADJAData
    write_tree(str(tmp_path), 'synth', mask_size=(20, 30))
    with pytest.raises(ValueError, match='mask is 20x30'):
        list(BADJAData('synth', root=str(tmp_path)).get_loader())


def test_joint_constant_is_the_set_ever_marked_visible():
    from lasr_amd.ext_utils.badja_data import ANNOTATED_JOINTS
    seen = set()
    for name in ('bear', 'camel', 'dog'):
        for a in json.load(open(os.path.join(GOLDEN, '%s.json' % name))):
            seen |= set(np.nonzero(a['visibility'])[0].tolist())
    assert sorted(seen) == ANNOTATED_JOINTS.tolist()
    assert len(glob.glob(os.path.join(GOLDEN, '*.json'))) == 6


def test_restatement_constant_flow():
    H, W = 30, 50
    f = np.zeros((H, W, 2), F32)
    f[...] = (F32(0.125), F32(-0.25))
    kp = np.array([[3, 4], [29, 49], [-2, 60]], F32)
    idx, pred = br.transfer(f, kp, H, W)
    np.testing.assert_array_equal(idx, [3 * W + 4, 29 * W + 49, 0 * W + 49])
    np.testing.assert_array_equal(pred, kp + np.array([-0.25 * H / 2, 0.125 * W / 2], F32))


def test_restatement_all_invalid_keeps_the_keypoints():
    H, W = 20, 20
    kp = np.array([[5, 6], [0, 19], [-3, 25]], F32)
    idx, pred = br.transfer(np.zeros((H, W, 2), F32), kp, H, W)          # the zero flow (--type zero)
    np.testing.assert_array_equal(idx, [5 * W + 6, 19, 19])
    np.testing.assert_array_equal(pred, kp)
    f = np.full((H, W, 2), F32(5e-7))                                      # |flow| = 7.1e-7 < 1e-6: invalid too
    idx, pred = br.transfer(f, kp, H, W)
    np.testing.assert_array_equal(idx, [5 * W + 6, 19, 19])


def test_restatement_ties_take_the_lowest_flat_index():
    H, W = 16, 16
    f = np.zeros((H, W, 2), F32)
    for r, c in ((5, 8), (8, 5), (8, 11), (11, 8)):
        f[r, c] = (0.5, 0.5)
    idx, _ = br.transfer(f, np.array([[8, 8]], F32), H, W)
    assert idx[0] == 5 * W + 8


def test_restatement_non_square_crop_scales_rows_by_h():
    S, H, W = 64, 24, 64
    f = np.zeros((S, S, 2), F32)
    f[30:, :] = (0.5, 0.5)                                           # outside the crop: never chosen
    f[10, 20] = (0.5, 0.25)
    idx, pred = br.transfer(f, np.array([[12, 22]], F32), H, W)
    assert idx[0] == 10 * W + 20
    np.testing.assert_array_equal(pred[0], [12 + 0.25 * H / 2, 22 + 0.5 * W / 2])


def test_restatement_flow_from_colors_background_and_grid():
    S = 5
    c = np.zeros((4, S, S), F32)
    c[2, 1, 2] = 1.
    c[0, 1, 2], c[1, 1, 2] = 0.5, -0.5
    f = br.flow_from_colors(c)
    assert (f[c[2] < 1e-9] == 0).all()
    inv = F32(1) / F32(S - 1)
    np.testing.assert_array_equal(f[1, 2], [F32(0.5) - (F32(4) * inv - F32(1)), F32(-0.5) - (F32(2) * inv - F32(1))])


def run_script(*args, cwd=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'eval_badja.py')] + list(args), cwd=cwd or ROOT,
                          timeout=300, capture_output=True, text=True)


def test_cli_refuses_flow_and_vis(tmp_path):
    r = run_script('--type', 'flow', '--seqname', 'camel', '--badja_root', str(tmp_path))
    assert r.returncode != 0 and 'VCN' in r.stderr
    r = run_script('--vis', '--badja_root', str(tmp_path))
    assert r.returncode != 0 and '--vis' in r.stderr


def test_cli_names_a_missing_prediction(tmp_path):
    root = str(tmp_path / 'db')
    write_tree(root, 'synth')
    test = tmp_path / 'test'
    test.mkdir()
    from lasr_amd.ext_utils.ply import write_ply
    for fr in (10, 13):
        write_ply(str(test / ('pred%d.ply' % fr)), np.eye(3), [[0, 1, 2]])
        np.savetxt(str(test / ('cam%d.txt' % fr)), np.eye(4))
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import eval_badja
    with pytest.raises(FileNotFoundError, match='pred16.ply'):
        eval_badja.load_meshes(str(test), [10, 13, 16])
    r = run_script('--testdir', str(test), '--seqname', 'synth', '--badja_root', root)
    assert r.returncode != 0 and 'pred16.ply' in r.stderr


def test_kp_transfer_host_checks():
    """Bad sizes and null pointers are refused before anything touches a device (the pointers below are never dereferenced)."""
    from lasr_amd import _lib
    h = _lib.lib()
    p = 1 << 20
    ok = [p, p, p, p, 1, 20, 64, 64, 64, None]
    for k, v in ((5, 0), (5, 65), (6, 1), (6, 16385), (7, 65), (8, 65), (7, 0), (8, 0), (4, -1), (1, None), (2, None), (3, None)):
        bad = list(ok)
        bad[k] = v
        assert h.lasr_kp_transfer(*bad) == -1, (k, v)
    assert h.lasr_kp_transfer(p, p, p, p, 0, 20, 64, 64, 64, None) == 0        # an empty batch launches nothing
    from lasr_amd.nnutils import keypoints
    import torch
    with pytest.raises(TypeError):
        keypoints.kp_transfer(torch.zeros(1, 4, 8, 8), torch.zeros(1, 2, 2), 8, 8)
    from lasr_amd.nnutils.geom_utils import render_flow_soft_3
    with pytest.raises(TypeError):
        render_flow_soft_3(None, torch.zeros(1, 3, 3), torch.zeros(1, 3, 3), torch.zeros(1, 1, 3, dtype=torch.int32))
