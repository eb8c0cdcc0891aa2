"""Shape scores on the device (lasr_amd/nnutils/meshcheck.py, csrc/meshcheck.hip) against the float64 restatement
(tests/meshcheck_restated.py).  The scores are this project's own addition: the restatement is the only parity there is.

The pair counts, the per-face counts and the sorted pair lists are compared for equality: tests/test_meshcheck_cpu.py shows that
no determinant of any fixture lies within 4 x the float32 / float64 spread of zero, so the strict sign tests cannot come out
differently.  Volume and area may differ by F 2^-52 sum |term|, the worst case of a float64 sum of F terms in another order; the
jitter by 4 x the float32 / float64 spread of the restatement.  No bound comes from what the kernels give.  Every test prints its
figures before it asserts.

Measured on an MI355X:
  every fixture: pair counts, per-face counts and sorted lists equal (two2 0 / 83 / 94 pairs, pinch2 10, tile256 and tile257 82);
    volume off by at most 1.3e-14 (bound 9.9e-13 there), area by 2.8e-14 (bound 3.2e-12), jitter by 5.6e-17 (bound 2.1e-8) and
    5.2e-18 (wobble, bound 9.0e-9).
  81 920 faces: 10 624 pairs and 10 624 faces involved, as the restatement of one copy says; volume off by 1.1e-13 (bound 3.9e-7).
  script: 59.0 pairs per frame, ratio 0.0917, worst frame 2 (94 pairs, 93 faces, ratio 0.1453).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import meshcheck_restated as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
_CACHE = {}


def _mc():
    from lasr_amd.nnutils import meshcheck
    return meshcheck


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _evaluated(cuda, name):
    """evaluate() of a fixture on the device, once."""
    if name not in _CACHE:
        verts, faces = mr.fixture(name)
        _CACHE[name] = _mc().evaluate(*_dev(cuda, verts, faces))
    return _CACHE[name]


def _same_pairs(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g is not None and g.dtype == np.int64 and g.shape == w.shape and (g == w).all()


@pytest.mark.parametrize('name', sorted(mr.FIXTURES))
def test_fixture_equals_the_restatement(cuda, name):
    verts, faces = mr.fixture(name)
    exp, res = mr.expected(name), _evaluated(cuda, name)
    T, F = verts.shape[0], faces.shape[0]
    vt, at = mr.volume_area_terms(verts, faces)
    bv, ba = F * 2. ** -52 * np.abs(vt).sum(1) / 6., F * 2. ** -52 * at.sum(1)
    spread = np.abs(mr.jitter(verts, np.float32).astype(np.float64) - exp['jitter'])
    bj = 4 * (np.nanmax(spread) if T >= 3 else 0.)
    ev, ea, ej = np.abs(res['volume'] - exp['volume']), np.abs(res['area'] - exp['area']), np.abs(res['jitter'] - exp['jitter'])
    print('%s: pairs %s (restatement %s), faces %s; volume %s off by %.1e (bound %.1e), area off by %.1e (bound %.1e), jitter off by '
          '%s (bound %.1e)' % (name, res['n_pairs'].tolist(), exp['n_pairs'].tolist(), res['n_faces'].tolist(),
                               np.round(res['volume'], 6).tolist(), ev.max(), bv.min(), ea.max(), ba.min(),
                               '%.1e' % np.nanmax(ej) if T >= 3 else 'n/a', bj))
    assert res['n_pairs'].dtype == np.int64 and res['n_pairs'].tolist() == exp['n_pairs'].tolist()
    assert res['face_count'].dtype == np.int32 and res['face_count'].shape == (T, F) and (res['face_count'] == exp['face_count']).all()
    _same_pairs(res['pairs'], [r['pairs'] for r in exp['frames']])
    assert res['n_faces'].tolist() == exp['n_faces'].tolist() and (res['ratio'] == exp['n_faces'] / F).all()
    assert not res['truncated'].any() and (res['inverted'] == (exp['volume'] < 0)).all()
    assert (ev <= bv).all() and (ea <= ba).all()
    assert (np.isnan(res['jitter']) == np.isnan(exp['jitter'])).all() and res['jitter'].dtype == np.float64
    if T >= 3:
        assert bj > 0 and np.nanmax(ej) <= bj
    if name == 'inverted':
        assert res['inverted'].all() and abs(res['volume'][0] + _evaluated(cuda, 'ico2')['volume'][0]) <= 2 * bv[0]


def test_batch_equals_its_single_frames_and_the_parts_equal_evaluate(cuda):
    mc = _mc()
    verts, faces = mr.fixture('two2')
    tv, tf = _dev(cuda, verts, faces)
    whole = _evaluated(cuda, 'two2')
    n, count, pairs, trunc = mc.self_intersections(tv, tf)
    assert n.dtype == torch.int64 and count.dtype == torch.int32 and n.is_cuda and count.is_cuda and trunc.dtype == torch.bool
    assert n.cpu().tolist() == whole['n_pairs'].tolist() and (count.cpu().numpy() == whole['face_count']).all()
    _same_pairs(pairs, whole['pairs'])
    vol, area = mc.volume_area(tv, tf)
    assert vol.dtype == torch.float64 and (vol.cpu().numpy() == whole['volume']).all() and (area.cpu().numpy() == whole['area']).all()
    assert np.array_equal(mc.jitter(tv).cpu().numpy(), whole['jitter'], equal_nan=True)
    for t in range(3):
        one = mc.evaluate(tv[t:t + 1], tf)
        print('frame %d alone: %d pairs, %d faces' % (t, one['n_pairs'][0], one['n_faces'][0]))
        assert one['n_pairs'][0] == whole['n_pairs'][t] and (one['face_count'][0] == whole['face_count'][t]).all()
        _same_pairs(one['pairs'], whole['pairs'][t:t + 1])
        assert one['volume'][0] == whole['volume'][t] and one['area'][0] == whole['area'][t] and np.isnan(one['jitter'][0])
        flat = mc.evaluate(tv[t], tf.long())                                      # [V,3] is one frame; any integer type of faces
        assert flat['n_pairs'].tolist() == one['n_pairs'].tolist()


def test_truncation_keeps_the_counts(cuda):
    mc = _mc()
    verts, faces = mr.fixture('two2')
    tv, tf = _dev(cuda, verts, faces)
    whole = _evaluated(cuda, 'two2')
    hits = whole['n_pairs'].tolist()                                              # 0, some, more
    assert hits[0] == 0 < hits[1] < hits[2]
    for max_pairs in (hits[2], hits[2] - 1, hits[1], hits[1] - 1, 1, 0):
        n, count, pairs, trunc = mc.self_intersections(tv, tf, max_pairs=max_pairs)
        want = [h > max_pairs for h in hits]
        print('max_pairs %d: truncated %s' % (max_pairs, trunc.cpu().tolist()))
        assert trunc.cpu().tolist() == want and n.cpu().tolist() == hits and (count.cpu().numpy() == whole['face_count']).all()
        for t in range(3):
            if want[t]:
                assert pairs[t] is None
            else:
                assert (pairs[t] == whole['pairs'][t]).all()
    res = mc.evaluate(tv, tf, max_pairs=0)
    assert res['truncated'].tolist() == [False, True, True] and res['pairs'][0].shape == (0, 2) and res['pairs'][1] is None
    assert res['n_faces'].tolist() == whole['n_faces'].tolist()


def test_two_runs_give_the_same_bits(cuda):
    mc = _mc()
    for name in ('two2', 'pinch2', 'wobble'):
        tv, tf = _dev(cuda, *mr.fixture(name))
        a, b = mc.evaluate(tv, tf), mc.evaluate(tv, tf)
        for k in ('n_pairs', 'n_faces', 'ratio', 'volume', 'area', 'jitter', 'inverted', 'truncated', 'face_count'):
            assert a[k].tobytes() == b[k].tobytes() == _evaluated(cuda, name)[k].tobytes(), (name, k)
        _same_pairs(a['pairs'], b['pairs'])


def test_mesh_of_81920_faces(cuda):
    """320 tiles, 51 360 tile pairs: the size the raster tests go up to.  128 exact translates of one 640-face mesh, whose answer
    is the restatement of one copy (tests/test_meshcheck_cpu.py checks that argument)."""
    mc = _mc()
    verts, faces, exp = mr.copies_case(128)
    assert faces.shape == (81920, 3)
    tv, tf = _dev(cuda, verts, faces)
    res = mc.evaluate(tv, tf, max_pairs=exp['n_pairs'])
    vt, at = mr.volume_area_terms(verts, faces)
    vol, area = mr.volume_area(verts, faces)
    bv, ba = 81920 * 2. ** -52 * np.abs(vt).sum() / 6., 81920 * 2. ** -52 * at.sum()
    print('81920 faces: %d pairs (restatement %d), %d faces involved, volume %.9f off by %.1e (bound %.1e), area off by %.1e (bound '
          '%.1e)' % (res['n_pairs'][0], exp['n_pairs'], res['n_faces'][0], res['volume'][0], abs(res['volume'][0] - vol[0]), bv,
                     abs(res['area'][0] - area[0]), ba))
    assert res['n_pairs'][0] == exp['n_pairs'] and (res['face_count'][0] == exp['face_count']).all()
    assert not res['truncated'][0] and (res['pairs'][0] == exp['pairs']).all()
    assert abs(res['volume'][0] - vol[0]) <= bv and abs(res['area'][0] - area[0]) <= ba
    short = mc.evaluate(tv, tf, max_pairs=exp['n_pairs'] - 1)
    assert short['truncated'][0] and short['pairs'][0] is None and short['n_pairs'][0] == exp['n_pairs']


def test_python_layer_validates_its_arguments(cuda):
    mc = _mc()
    verts, faces = mr.fixture('ico1')
    tv, tf = _dev(cuda, verts, faces)
    bad = tf.clone()
    bad[7, 1] = verts.shape[1]
    with pytest.raises(ValueError, match=r'outside \[0, 42\)'):
        mc.evaluate(tv, bad)
    bad[7, 1] = -1
    with pytest.raises(ValueError, match=r'outside \[0, 42\)'):
        mc.self_intersections(tv, bad)
    with pytest.raises(TypeError):
        mc.evaluate(tv, tf.cpu())
    with pytest.raises(ValueError, match='verts must be'):
        mc.evaluate(tv[..., :2], tf)
    with pytest.raises(ValueError, match='faces must be integers'):
        mc.evaluate(tv, tf.float())
    with pytest.raises(ValueError, match='max_pairs'):
        mc.evaluate(tv, tf, max_pairs=-1)
    empty = mc.evaluate(tv[:0], tf)                                               # no frames: empty outputs
    assert empty['n_pairs'].shape == (0,) and empty['face_count'].shape == (0, 80) and empty['pairs'] == []
    none = mc.evaluate(tv, tf[:0])                                                # no faces
    assert none['n_pairs'].tolist() == [0] and none['volume'].tolist() == [0.] and none['face_count'].shape == (1, 0)


def test_script_end_to_end(cuda, tmp_path):
    from lasr_amd.ext_utils.ply import read_ply
    verts, faces = mr.fixture('two2')
    root = str(tmp_path)
    test = mr.write_sequence(root, 'balls', verts, faces)
    out, plys = os.path.join(root, 'scores', 'shape.json'), os.path.join(root, 'plys')
    rc = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'eval_shape.py'), '--testdir', test, '--seqname', 'balls',
                         '--outpath', out, '--worst', '2', '--ply', plys], cwd=root, timeout=600, capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    print(rc.stdout.strip())
    doc = json.load(open(out))
    # the same files through the same reader, restated
    loaded = np.stack([read_ply(os.path.join(test, 'pred%d.ply' % i))['verts'] for i in range(3)]).astype(np.float32)
    spread, least = mr.det_spread(loaded, faces)
    assert mr.uncertain(loaded, faces, 4 * spread) == []                          # what was written and read back is as decided
    exp = mr.evaluate(loaded, faces)
    per = doc['per_frame']
    assert doc['frame_ids'] == [0, 1, 2] and doc['params']['faces'] == 640 and doc['params']['max_pairs'] == 4096
    assert per['n_pairs'] == exp['n_pairs'].tolist() and per['n_faces'] == exp['n_faces'].tolist()
    assert per['ratio'] == (exp['n_faces'] / 640.).tolist() and per['inverted'] == [False] * 3 and per['truncated'] == [False] * 3
    vt, at = mr.volume_area_terms(loaded, faces)
    assert (np.abs(np.array(per['volume']) - exp['volume']) <= 640 * 2. ** -52 * np.abs(vt).sum(1) / 6.).all()
    assert (np.abs(np.array(per['area']) - exp['area']) <= 640 * 2. ** -52 * at.sum(1)).all()
    bj = 4 * abs(float(mr.jitter(loaded, np.float32)[1]) - exp['jitter'][1])
    assert per['jitter'][0] is None and per['jitter'][2] is None and bj > 0 and abs(per['jitter'][1] - exp['jitter'][1]) <= bj
    assert doc['means']['n_pairs'] == float(exp['n_pairs'].mean()) and doc['nan_frames']['jitter'] == 2 and doc['n_inverted'] == 0
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import eval_shape
    lines = rc.stdout.splitlines()
    assert lines[0] == eval_shape.summary_line(doc) and len(lines) == 4
    assert lines[1].startswith('worst: frame 2 (position 2) ') and lines[2].startswith('worst: frame 1 (position 1) ')
    for t in range(3):
        m = read_ply(os.path.join(plys, 'shape-%05d.ply' % t))
        red = np.unique(faces[exp['face_count'][t] > 0].reshape(-1))
        assert (np.nonzero((m['colors'] == eval_shape.RED).all(1))[0] == red).all()
        assert ((m['colors'] == eval_shape.RED).all(1) | (m['colors'] == eval_shape.GREY).all(1)).all()
        assert (m['faces'] == faces).all() and (m['verts'].astype(np.float32) == loaded[t]).all()
