"""The neighbour pass of the shape scores on the device (scripts/shape_neighbours.py, lasr_amd/csrc/meshnbr.hip) against the float64
restatement (tests/meshnbr_restated.py).  The pass is this project's own addition: the restatement is the only parity there is.

The topology list, its counters, the pierced and creased counts, both per-face count planes and the sorted hit lists are compared
for equality: the list is integer work, and tests/test_meshnbr_cpu.py shows that no determinant and no d d - k q of any fixture lies
within 4 x its own float32 / float64 difference of zero, so the strict sign tests cannot come out differently.  min_cos is held to
1e-5 of the restatement: a division and a square root that no equality is pinned on.  Every shape is a fixture of the restatement:
at most 2560 faces and 5 frames.  No bound comes from what the kernels give.  Every fixture test prints its figures before it asserts.

Measured on an MI355X:
  every fixture: lists key for key (ico1 450 entries, ico2 1890, tile257 1353, two2 3780, crease3 7650), counters, counts, count planes
    and sorted hits equal; min_cos off by at most 1.3e-7 (creaseA; bound 1e-5).
  batch3: pierced 0 / 0 / 2, creased 0 / 2 / 3, min dihedral 144.790 / 0.787 / 5.912 degrees.
  2560 faces (eight copies): 15 120 entries, 16 pierced, 24 creased, min_cos equal to the base's.
  script on creaseA: 0 intersecting pairs, 2.0 creased pairs, sharpest dihedral 0.788 degrees.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guarded
import meshcheck_restated as mr
import meshnbr_guarded
import meshnbr_restated as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
_CACHE = {}
COUNTS = ('n_list', 'n_vertex', 'n_edge', 'n_duplicate', 'n_degenerate', 'n_same')


def _sn():
    return meshnbr_guarded.shape_neighbours()


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _evaluated(cuda, name):
    """evaluate() of a fixture on the device, once."""
    if name not in _CACHE:
        _CACHE[name] = _sn().evaluate(*_dev(cuda, *nr.fixture(name)))
    return _CACHE[name]


def _same_hits(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g is not None and g.dtype == np.int64 and g.shape == w.shape and (g == w).all()


def _close(a, b, tol=1e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.isnan(a) == np.isnan(b)).all() and (np.isnan(a) | (np.abs(a - b) <= tol)).all()


@pytest.mark.parametrize('name', sorted(nr.FIXTURES))
def test_fixture_equals_the_restatement(cuda, name):
    sn = _sn()
    verts, faces = nr.fixture(name)
    exp, res = nr.expected(name), _evaluated(cuda, name)
    T, F = verts.shape[0], faces.shape[0]
    keys, counts = sn.neighbour_list(_dev(cuda, faces)[0])
    got = {k: int(v) for k, v in counts.items()}
    err = np.nanmax(np.abs(res['min_cos'].astype(np.float64) - exp['min_cos']))
    print('%s: list %d (restatement %d), counters %s, pierced %s, creased %s, min dihedral %s, min_cos off by %.1e (bound 1e-5)'
          % (name, keys.numel(), len(exp['keys']), got, res['n_pierced'].tolist(), res['n_creased'].tolist(),
             np.round(res['min_dihedral'], 3).tolist(), err))
    assert keys.dtype == torch.int64 and keys.is_cuda and np.array_equal(keys.cpu().numpy(), exp['keys'])          # key for key
    assert got == exp['topology'] == res['topology'] and set(got) == set(COUNTS)
    assert res['n_pierced'].dtype == np.int64 and res['n_pierced'].tolist() == exp['n_pierced'].tolist()
    assert res['n_creased'].tolist() == exp['n_creased'].tolist()
    assert res['nbr_count'].dtype == np.int32 and res['nbr_count'].shape == (T, 2, F) and (res['nbr_count'] == exp['nbr_count']).all()
    _same_hits(res['hits'], exp['hits'])
    assert res['n_neighbour_faces'].tolist() == exp['n_neighbour_faces'].tolist() and not res['nbr_truncated'].any()
    assert res['min_cos'].dtype == np.float32 and _close(res['min_cos'], exp['min_cos'])
    assert _close(res['min_dihedral'], nr.dihedral(res['min_cos']), 0.) and res['min_dihedral'].dtype == np.float64
    # the keys of the pair pass are what lasr_amd/nnutils/meshcheck.py gives alone
    from lasr_amd.nnutils import meshcheck
    alone = meshcheck.evaluate(*_dev(cuda, verts, faces))
    for k in ('n_pairs', 'n_faces', 'ratio', 'volume', 'area', 'jitter', 'inverted', 'truncated', 'face_count'):
        assert alone[k].tobytes() == res[k].tobytes(), k
    assert alone['n_pairs'].tolist() == mr.evaluate(verts, faces)['n_pairs'].tolist()
    assert all((a == b).all() for a, b in zip(alone['pairs'], res['pairs']))


def test_batch_equals_its_single_frames_and_the_parts_equal_evaluate(cuda):
    sn = _sn()
    verts, faces = nr.fixture('batch3')
    tv, tf = _dev(cuda, verts, faces)
    whole = _evaluated(cuda, 'batch3')
    assert whole['n_pierced'].tolist() == [0, 0, 2] and whole['n_creased'].tolist() == [0, 2, 3]
    nbr = sn.neighbour_list(tf)
    parts = sn.neighbour_tests(tv, tf, nbr=nbr)
    assert parts['n_pierced'].dtype == torch.int64 and parts['nbr_count'].dtype == torch.int32 and parts['min_cos'].is_cuda
    assert parts['n_pierced'].cpu().tolist() == [0, 0, 2] and (parts['nbr_count'].cpu().numpy() == whole['nbr_count']).all()
    assert parts['min_cos'].cpu().numpy().tobytes() == whole['min_cos'].tobytes() and parts['nbr'][0] is nbr[0]
    assert tuple(parts['hits'].shape) == (3, 4096, 3) and parts['hits'].dtype == torch.int32
    for t in range(3):
        one = sn.evaluate(tv[t:t + 1], tf)
        print('frame %d alone: %d pierced, %d creased, min dihedral %.3f' % (t, one['n_pierced'][0], one['n_creased'][0], one['min_dihedral'][0]))
        assert one['n_pierced'][0] == whole['n_pierced'][t] and one['n_creased'][0] == whole['n_creased'][t]
        assert (one['nbr_count'][0] == whole['nbr_count'][t]).all() and one['min_cos'].tobytes() == whole['min_cos'][t:t + 1].tobytes()
        _same_hits(one['hits'], whole['hits'][t:t + 1])
        flat = sn.evaluate(tv[t], tf.long())                                      # [V,3] is one frame; any integer type of faces
        assert flat['n_creased'].tolist() == one['n_creased'].tolist() and flat['topology'] == whole['topology']
    for name, frame in (('creaseA', 1), ('creaseB', 2)):                          # the same vertices as fixtures of their own
        assert (_evaluated(cuda, name)['nbr_count'][0] == whole['nbr_count'][frame]).all()
    for deg in (5., 90.):                                                         # the threshold is the caller's; restated, and as decided there
        want = nr.neighbour_tests(verts, faces, deg)
        assert min(nr.margins(verts, faces, deg)) > 4
        other = sn.neighbour_tests(tv, tf, fold_deg=deg)
        print('fold_deg %g: creased %s' % (deg, other['n_creased'].cpu().tolist()))
        assert other['n_creased'].cpu().tolist() == [w['n_creased'] for w in want] and other['n_pierced'].cpu().tolist() == [0, 0, 2]
        assert (other['nbr_count'].cpu().numpy() == np.stack([w['nbr_count'] for w in want])).all()
    assert [w['n_creased'] for w in want] == [0, 4, 4] and [w['n_creased'] for w in nr.neighbour_tests(verts, faces, 5.)] == [0, 1, 0]


def test_two_runs_give_the_same_bits(cuda):
    sn = _sn()
    for name in ('batch3', 'crease3', 'wobble'):
        tv, tf = _dev(cuda, *nr.fixture(name))
        a, b = sn.evaluate(tv, tf), sn.evaluate(tv, tf)
        for k in ('n_pierced', 'n_creased', 'n_neighbour_faces', 'min_cos', 'min_dihedral', 'nbr_truncated', 'nbr_count'):
            assert a[k].tobytes() == b[k].tobytes() == _evaluated(cuda, name)[k].tobytes(), (name, k)
        _same_hits(a['hits'], b['hits'])
        assert a['topology'] == b['topology']
        (k1, _), (k2, _) = sn.neighbour_list(tf), sn.neighbour_list(tf)
        assert torch.equal(k1, k2)


def test_truncation_keeps_the_counts(cuda):
    sn = _sn()
    tv, tf = _dev(cuda, *nr.fixture('batch3'))
    whole = _evaluated(cuda, 'batch3')
    hits = (whole['n_pierced'] + whole['n_creased']).tolist()
    assert hits == [0, 2, 5]
    for max_pairs in (5, 4, 2, 1, 0):
        res = sn.evaluate(tv, tf, max_pairs=max_pairs)
        want = [h > max_pairs for h in hits]
        print('max_pairs %d: truncated %s' % (max_pairs, res['nbr_truncated'].tolist()))
        assert res['nbr_truncated'].tolist() == want and (res['nbr_count'] == whole['nbr_count']).all()
        assert res['n_pierced'].tolist() == [0, 0, 2] and res['n_creased'].tolist() == [0, 2, 3]
        assert res['min_cos'].tobytes() == whole['min_cos'].tobytes()
        for t in range(3):
            if want[t]:
                assert res['hits'][t] is None
            else:
                assert (res['hits'][t] == whole['hits'][t]).all()
    raw = sn.neighbour_tests(tv, tf, max_pairs=3)
    assert tuple(raw['hits'].shape) == (3, 3, 3) and not raw['hits'][0].any() and raw['n_creased'].cpu().tolist() == [0, 2, 3]
    kept = {tuple(r) for r in raw['hits'][2].cpu().tolist()}                      # any three of the five
    assert len(kept) == 3 and kept <= {tuple(r) for r in whole['hits'][2].tolist()}


def test_a_list_that_overflows_its_capacity_is_made_again_at_its_exact_size(cuda):
    sn = _sn()
    for name in ('ico1', 'crease3'):
        tf, = _dev(cuda, nr.fixture(name)[1])
        exp = nr.expected(name)
        for capacity in (8, 0, len(exp['keys']) - 1, len(exp['keys']), None):
            keys, counts = sn.neighbour_list(tf, capacity=capacity)
            assert np.array_equal(keys.cpu().numpy(), exp['keys']), (name, capacity)
            assert {k: int(v) for k, v in counts.items()} == exp['topology']
    # the entry point itself: the counters stay exact past the capacity, and nothing is written past it
    tf, = _dev(cuda, nr.fixture('ico1')[1])
    from lasr_amd import _lib
    counters = torch.full((4,), -1, dtype=torch.int64, device=cuda)
    room = torch.full((8 + 64,), -7, dtype=torch.int64, device=cuda)
    _lib.call('lasr_meshnbr_list', tf, room, counters, 80, 8)
    assert counters.cpu().tolist() == [450, 0, 0, 0] and bool((room[8:] == -7).all())
    assert set(room[:8].cpu().tolist()) <= set(nr.expected('ico1')['keys'].tolist()) and len(set(room[:8].cpu().tolist())) == 8


def test_copies_in_tile_pairs_beyond_the_first(cuda):
    """Eight exact translates of creaseB, 2560 faces in 10 tiles and 55 tile pairs: the answer is 8 x the base's
    (tests/test_meshnbr_cpu.py checks that argument)."""
    sn = _sn()
    verts, faces, exp = nr.copies_case(8)
    res = sn.evaluate(*_dev(cuda, verts, faces))
    print('copies: list %d, pierced %d, creased %d, min_cos off by %.1e' % (res['topology']['n_list'], res['n_pierced'][0],
                                                                           res['n_creased'][0], abs(res['min_cos'][0] - exp['min_cos'])))
    keys, _ = sn.neighbour_list(_dev(cuda, faces)[0])
    assert np.array_equal(keys.cpu().numpy(), exp['keys']) and res['topology'] == exp['topology']
    assert (res['n_pierced'][0], res['n_creased'][0]) == (exp['n_pierced'], exp['n_creased']) == (16, 24)
    assert (res['nbr_count'][0] == exp['nbr_count']).all() and (res['hits'][0] == exp['hits']).all()
    assert _close(res['min_cos'], [exp['min_cos']])


def test_one_face_and_faces_that_share_no_vertex(cuda):
    sn = _sn()
    verts, faces = nr.fixture('ico1')
    tv, = _dev(cuda, verts)
    apart = torch.arange(39, dtype=torch.int32, device=cuda).reshape(13, 3)      # thirteen faces, no vertex twice
    for tf in (torch.tensor([[0, 1, 2]], dtype=torch.int32, device=cuda), apart):
        keys, counts = sn.neighbour_list(tf)
        assert keys.numel() == 0 and keys.dtype == torch.int64 and all(int(v) == 0 for v in counts.values())
        res = sn.evaluate(tv, tf)                                                 # an empty list: nothing launched, zeros, no angle
        F = tf.shape[0]
        assert res['n_pierced'].tolist() == [0] and res['n_creased'].tolist() == [0] and res['n_neighbour_faces'].tolist() == [0]
        assert res['nbr_count'].shape == (1, 2, F) and not res['nbr_count'].any() and res['hits'][0].shape == (0, 3)
        assert np.isnan(res['min_cos']).all() and np.isnan(res['min_dihedral']).all() and res['topology']['n_list'] == 0
    none = sn.evaluate(tv, apart[:0])                                             # no faces
    assert none['n_pierced'].tolist() == [0] and none['nbr_count'].shape == (1, 2, 0) and np.isnan(none['min_dihedral']).all()
    empty = sn.evaluate(tv[:0], _dev(cuda, faces)[0])                             # no frames
    assert empty['n_pierced'].shape == (0,) and empty['nbr_count'].shape == (0, 2, 80) and empty['hits'] == []
    assert empty['topology']['n_edge'] == 120
    odd = torch.tensor([[0, 1, 2], [1, 0, 3], [3, 3, 4], [0, 1, 2], [2, 1, 0]], dtype=torch.int32, device=cuda)
    keys, counts = sn.neighbour_list(odd)                                         # a degenerate face and three copies of one face
    top = nr.topology(odd.cpu().numpy())
    assert np.array_equal(keys.cpu().numpy(), top['keys']) and {k: int(v) for k, v in counts.items()} == {k: top[k] for k in COUNTS}
    assert (top['n_degenerate'], top['n_duplicate'], top['n_same']) == (1, 3, 1)


def test_python_layer_validates_its_arguments(cuda):
    sn = _sn()
    verts, faces = nr.fixture('ico1')
    tv, tf = _dev(cuda, verts, faces)
    bad = tf.clone()
    bad[7, 1] = verts.shape[1]
    with pytest.raises(ValueError, match=r'outside \[0, 42\)'):
        sn.evaluate(tv, bad)
    with pytest.raises(ValueError, match=r'outside \[0, 42\)'):
        sn.neighbour_tests(tv, bad)
    with pytest.raises(TypeError):
        sn.evaluate(tv, tf.cpu())
    with pytest.raises(ValueError, match='faces must be integers'):
        sn.neighbour_list(tf.float())
    with pytest.raises(ValueError, match='faces must be integers'):
        sn.neighbour_list(tf[:, :2])
    with pytest.raises(ValueError, match='max_pairs'):
        sn.evaluate(tv, tf, max_pairs=-1)
    with pytest.raises(ValueError, match='fold_deg'):
        sn.evaluate(tv, tf, fold_deg=91.)
    with pytest.raises(ValueError, match='capacity'):
        sn.neighbour_list(tf, capacity=-1)


def test_the_script_sees_the_fold_the_pair_pass_is_blind_to(cuda, tmp_path):
    """creaseA through scripts/eval_shape.py: today's keys say 0 intersecting pairs, a clean mesh; the keys of --neighbours say 2
    creased pairs at 0.79 degrees."""
    from lasr_amd.ext_utils.ply import read_ply
    verts, faces = nr.fixture('creaseA')
    root = str(tmp_path)
    test = mr.write_sequence(root, 'crease', verts, faces)
    out, plys = os.path.join(root, 'scores', 'shape.json'), os.path.join(root, 'plys')
    base = [sys.executable, os.path.join(ROOT, 'scripts', 'eval_shape.py'), '--testdir', test, '--seqname', 'crease', '--worst', '1']
    rc = subprocess.run(base + ['--outpath', out, '--ply', plys, '--neighbours'], cwd=root, timeout=600, capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    print(rc.stdout.strip())
    doc = json.load(open(out))
    loaded = read_ply(os.path.join(test, 'pred0.ply'))['verts'].astype(np.float32)[None]
    assert min(nr.margins(loaded, faces)) > 4                                     # what was written and read back is as decided
    exp = nr.evaluate(loaded, faces)
    per = doc['per_frame']
    assert per['n_pairs'] == [0] and per['n_faces'] == [0] and per['ratio'] == [0.]                   # today's keys: a clean mesh
    assert per['n_pierced'] == [0] and per['n_creased'] == [2] and per['n_neighbour_faces'] == [4]
    back = np.cos(np.radians(180. - per['min_dihedral'][0]))                      # the cosine behind the reported angle: the 1e-5 of min_cos
    assert abs(back - exp['min_cos'][0]) <= 1e-5 + 1e-12 and 0.5 < per['min_dihedral'][0] < 1.1
    p = doc['params']
    assert (p['neighbours'], p['fold_deg'], p['vertex_pairs'], p['edge_pairs'], p['duplicate_faces'], p['degenerate_faces'],
            p['same_direction_edges']) == (True, 20., 1410, 480, 0, 0, 0)
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import eval_shape
    lines = rc.stdout.splitlines()
    assert lines[0] == eval_shape.summary_line(doc) and lines[1] == eval_shape.neighbour_line(doc) and len(lines) == 4
    m = read_ply(os.path.join(plys, 'shape-00000.ply'))
    orange = np.unique(faces[exp['nbr_count'][0].sum(0) > 0].reshape(-1))
    assert (np.nonzero((m['colors'] == eval_shape.ORANGE).all(1))[0] == orange).all() and len(orange) >= 4
    assert ((m['colors'] == eval_shape.ORANGE).all(1) | (m['colors'] == eval_shape.GREY).all(1)).all()
    # without the flag: the document it always wrote
    plain = os.path.join(root, 'scores', 'plain.json')
    rc = subprocess.run(base + ['--outpath', plain], cwd=root, timeout=600, capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    old = json.load(open(plain))
    assert set(old['per_frame']) == {'n_pairs', 'n_faces', 'ratio', 'volume', 'area', 'jitter', 'inverted', 'truncated'}
    assert set(old['params']) == {'testdir', 'seqname', 'max_pairs', 'vertices', 'faces'} and old['per_frame']['n_pairs'] == [0]
    assert all(doc['per_frame'][k] == v for k, v in old['per_frame'].items()) and rc.stdout.splitlines()[0] == lines[0]
    assert len(rc.stdout.splitlines()) == 2


# ---- guard bands and relocated inputs -------------------------------------------------------------------------------------------------

def test_the_natives_with_guard_bands_and_poison(cuda):
    sn = _sn()
    guarded.run_case(meshnbr_guarded.CASE, cuda, modules=[sn] + guarded._product_modules())


def test_the_natives_with_relocated_inputs(cuda):
    sn = _sn()
    record = guarded.run_relocated(meshnbr_guarded.CASE, cuda, modules=[sn] + guarded._product_modules())
    assert sorted(record) == sorted(meshnbr_guarded.NATIVES)
