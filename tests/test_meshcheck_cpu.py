"""Shape scores without a device: closed forms of the restatement (tests/meshcheck_restated.py), the condition the GPU equalities of
tests/test_meshcheck_gpu.py rest on (no determinant of any fixture near zero; float32 and float64 agree on every pair), header
against binding, the C ABI's host-side checks, the Python layer's refusals and the script's arguments and summary.  The scores are
this project's own addition: the restatement is the only parity there is."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

import meshcheck_restated as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = (np.float64, np.float32)


def _count(verts, faces, dt=np.float64):
    r = mr.self_intersections(np.asarray(verts, np.float32), np.asarray(faces, np.int32), dt)[0]
    return r['n_pairs'], r['n_candidates']


# a triangle in the plane z = 0 and partners given by their three vertices (indices 3, 4, 5)
BASE = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
TWO = [(0, 1, 2), (3, 4, 5)]


@pytest.mark.parametrize('dt', BOTH)
def test_two_triangles_through_each_other_are_one_pair(dt):
    n, cand = _count(BASE + [(1, 1, -1), (1, 1, 1), (5, 5, 0.5)], TWO, dt)       # edge 3-4 goes through the interior of the base
    assert (n, cand) == (1, 1)
    res = mr.self_intersections(np.array(BASE + [(1, 1, -1), (1, 1, 1), (5, 5, 0.5)], np.float32), np.array(TWO), dt)[0]
    assert res['pairs'].tolist() == [[0, 1]] and res['face_count'].tolist() == [1, 1] and res['n_faces'] == 2 and res['ratio'] == 1.
    # each triangle's edge through the other's interior (a chain link)
    n, cand = _count(BASE + [(1, -1, -1), (1, 3, 1), (1, -1, 3)], TWO, dt)
    assert (n, cand) == (1, 1)


@pytest.mark.parametrize('dt', BOTH)
def test_touching_coplanar_and_separate_triangles_are_no_pair(dt):
    cases = {
        'a vertex on the interior': [(1, 1, 0), (1, 1, 2), (2, 1, 2)],
        'a vertex on a vertex': [(0, 0, 0), (-1, -1, 2), (-2, -1, 2)],
        'an edge along an edge': [(0, 0, 0), (4, 0, 0), (2, 0, 3)],
        'an edge crossing an edge': [(2, -1, 0), (2, 1, 0), (2, 0, 3)],
        'coplanar overlap': [(1, 1, 0), (5, 1, 0), (1, 5, 0)],
        'coplanar containment': [(0.5, 0.5, 0), (1.5, 0.5, 0), (0.5, 1.5, 0)],
        'boxes overlap, far apart': [(3.5, 3.5, -1), (3.5, 3.5, 1), (4, 4, 0)],
        'an edge ends on the plane outside': [(3, 3, 0), (3, 3, 2), (3.5, 3, 2)],
    }
    for name, tri in cases.items():
        n, cand = _count(BASE + tri, TWO, dt)
        assert cand == 1, name                                                     # every case reaches the exact test
        assert n == 0, name


def test_boxes_apart_and_shared_vertices_are_not_candidates():
    assert _count(BASE + [(1, 1, 5), (1, 1, 6), (2, 1, 6)], TWO) == (0, 0)
    assert _count(BASE + [(4, 0, 1), (5, 0, 1), (4, 1, 1)], TWO) == (0, 0)        # boxes that touch in x and y but not in z
    assert _count(BASE + [(4, 4, 0), (5, 4, 0), (4, 5, 0)], TWO)[1] == 1          # closed comparisons: touching boxes are candidates
    # two faces that share vertex 0 by index and cross geometrically: excluded
    verts = BASE + [(1, 1, -1), (1, 1, 1)]
    assert _count(verts, [(0, 1, 2), (0, 3, 4)]) == (0, 0)
    assert _count(verts + [(0, 0, 0)], [(0, 1, 2), (5, 3, 4)]) == (1, 1)          # the same place under another index: tested


def test_volume_and_area_closed_forms():
    cube = np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    vol, area = mr.volume_area(cube, faces)
    assert vol.tolist() == [1.] and area.tolist() == [6.]
    assert mr.volume_area(cube + np.float32(3), faces)[0].tolist() == [1.]        # closed: the origin does not matter
    tet = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], np.float32)
    vol, area = mr.volume_area(tet, np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], np.int32))
    assert vol[0] == 1. / 6. and abs(area[0] - (1.5 + 0.5 * 3 ** 0.5)) < 1e-15
    assert mr.self_intersections(cube, faces)[0]['n_pairs'] == 0
    v2, a2 = mr.expected('ico2')['volume'], mr.expected('ico2')['area']
    vi, ai = mr.expected('inverted')['volume'], mr.expected('inverted')['area']
    assert v2[0] > 3.5 and abs(vi[0] + v2[0]) <= 1e-14 * v2[0] and abs(ai[0] - a2[0]) <= 1e-14 * a2[0]


@pytest.mark.parametrize('dt', BOTH)
def test_jitter_closed_forms(dt):
    rng = np.random.default_rng(5)
    base = rng.uniform(-1, 1, (7, 3))
    steady = np.stack([base + t * np.array([0.5, -0.25, 0.125]) for t in range(5)]).astype(np.float32)    # exact in float32
    j = mr.jitter(steady, dt)
    assert np.isnan(j[[0, -1]]).all() and (j[1:-1] <= (1e-6 if dt is np.float32 else 1e-7)).all()
    steady = np.stack([np.round(base * 64) / 64 + t * np.array([0.5, -0.25, 0.125]) for t in range(5)]).astype(np.float32)
    assert (mr.jitter(steady, dt)[1:-1] == 0).all()                               # dyadic positions: every difference is exact
    accel = np.stack([np.round(base * 64) / 64 + np.array([t * t, 0, 0]) for t in range(5)]).astype(np.float32)
    j = mr.jitter(accel, dt)
    for t in (1, 2, 3):
        e = accel[t].max(0) - accel[t].min(0)
        assert abs(j[t] - 2. / np.sqrt((e.astype(np.float64) ** 2).sum())) <= 1e-6 * j[t]
    assert np.isnan(mr.jitter(accel[:2], dt)).all() and mr.jitter(accel[:0], dt).shape == (0,)


@pytest.mark.parametrize('name', sorted(mr.FIXTURES))
def test_fixture_has_no_uncertain_pair_and_both_precisions_agree(name):
    verts, faces = mr.fixture(name)
    exp = mr.expected(name)
    spread, least = mr.det_spread(verts, faces)
    bound = 4 * spread
    unc = mr.uncertain(verts, faces, bound)
    r32 = mr.self_intersections(verts, faces, np.float32)
    print('%s: T %d V %d F %d, candidates %s, pairs %s, faces %s, most partners %d, max |det32 - det64| %.2e, bound %.2e, least |det| '
          '%.2e, %d uncertain' % (name, verts.shape[0], verts.shape[1], faces.shape[0], [r['n_candidates'] for r in exp['frames']],
                                  exp['n_pairs'].tolist(), exp['n_faces'].tolist(), max(int(r['face_count'].max()) for r in exp['frames']),
                                  spread, bound, least, len(unc)))
    assert unc == [] and least > bound
    for a, b in zip(exp['frames'], r32):
        assert a['pairs'].tolist() == b['pairs'].tolist() and (a['face_count'] == b['face_count']).all()
    assert len(mr.uncertain(verts, faces, np.inf)) == sum(r['n_candidates'] for r in exp['frames'])     # the bound is what selects


def test_fixtures_are_what_the_gpu_tests_need():
    e = {k: mr.expected(k) for k in mr.FIXTURES}
    assert mr.fixture('ico1')[1].shape == (80, 3) and mr.fixture('ico2')[1].shape == (320, 3) and mr.fixture('two2')[1].shape == (640, 3)
    assert e['ico1']['n_pairs'].tolist() == [0] and e['ico2']['n_pairs'].tolist() == [0] and e['inverted']['n_pairs'].tolist() == [0]
    n = e['two2']['n_pairs']
    assert n[0] == 0 and 0 < n[1] < n[2]                                          # far apart, overlapping, overlapping more
    pairs = e['two2']['frames'][2]['pairs']
    assert (pairs[:, 0] < 320).all() and (pairs[:, 1] >= 320).all()               # each pair joins the two spheres
    assert len({(i // 256, j // 256) for i, j in pairs}) >= 2                     # and they sit in more than one pair of tiles
    assert e['pinch2']['n_pairs'][0] > 0 and e['pinch2']['frames'][0]['face_count'].max() > 1
    assert mr.fixture('tile256')[1].shape == (256, 3) and mr.fixture('tile257')[1].shape == (257, 3)
    assert e['tile256']['n_pairs'][0] > 0 and e['tile257']['frames'][0]['face_count'][256] > 0         # the one-face tile takes part
    j = e['wobble']['jitter']
    assert np.isnan(j[[0, 4]]).all() and (j[1:4] > 1e-3).all()
    plain = mr.icosphere(2, 2, radial=0., positional=0.)                          # what the jitter is for: exactly coplanar quadruples
    assert len(mr.uncertain(plain[0], plain[1], 4 * mr.det_spread(*plain)[0])) > 0


def test_copies_fixture_is_what_its_argument_says():
    """The 81 920-face case of the GPU test takes its answer from one restatement of 640 faces: check the argument at three copies,
    where the whole mesh can be restated directly, and the condition of the equalities on the base."""
    v0, f0 = mr.copies_base()
    spread, least = mr.det_spread(v0, f0)
    r32 = mr.self_intersections(v0, f0, np.float32)[0]
    r64 = mr.self_intersections(v0, f0)[0]
    print('copies base: %d candidates, %d pairs, max |det32 - det64| %.2e, least |det| %.2e' % (r64['n_candidates'], r64['n_pairs'],
                                                                                            spread, least))
    assert mr.uncertain(v0, f0, 4 * spread) == [] and r32['pairs'].tolist() == r64['pairs'].tolist() and r64['n_pairs'] > 50
    verts, faces, exp = mr.copies_case(3)
    assert verts.shape == (1, 972, 3) and faces.shape == (1920, 3)
    for dt in BOTH:
        whole = mr.self_intersections(verts, faces, dt)[0]
        assert whole['n_candidates'] == 3 * r64['n_candidates']                   # no candidate joins two copies
        assert whole['pairs'].tolist() == exp['pairs'].tolist() and (whole['face_count'] == exp['face_count']).all()
        assert whole['n_pairs'] == exp['n_pairs']
    i, j = mr.candidates(verts[0], faces)
    d = mr.pair_determinants(verts[0], faces, i, j, np.float32)[1]
    n = len(i) // 3
    assert (d[:n] == d[n:2 * n]).all() and (d[:n] == d[2 * n:]).all()             # the same bits in every copy


def _prototype(name):
    hdr = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'\b(?:int|size_t) %s\s*\((.*?)\);' % name, hdr, re.S)
    assert m, name
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def test_header_and_binding_agree_on_the_three_entry_points():
    from lasr_amd import _lib
    scalar = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t}
    ctype = lambda a: ctypes.c_void_p if '*' in a else scalar[a.split()[0]]     # noqa: E731
    for name, res, params in (('lasr_meshcheck_workspace_bytes', ctypes.c_size_t, 'T F'),
                              ('lasr_meshcheck_faces', ctypes.c_int, 'verts faces workspace workspace_bytes volume area T V F hip_stream'),
                              ('lasr_meshcheck_pairs', ctypes.c_int,
                               'workspace workspace_bytes face_count n_pairs cursor pairs T F max_pairs hip_stream')):
        args = _prototype(name)
        assert [a.replace('*', ' ').split()[-1] for a in args] == params.split()
        got, sig = _lib.SIGNATURES[name]
        assert got is res and sig == [ctype(a) for a in args]
    hdr = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    for k, v in (('TILE', _lib.MESHCHECK_TILE), ('MAX_FACES', _lib.MESHCHECK_MAX_FACES), ('MAX_FRAMES', _lib.MESHCHECK_MAX_FRAMES)):
        assert '#define LASR_MESHCHECK_%s %d\n' % (k, v) in hdr
    assert _lib.MESHCHECK_TILE == 256 and _lib.MESHCHECK_MAX_FACES >= 81920
    assert _lib.ABI_VERSION == 13                                                 # new symbols only
    assert sorted(n for n in _lib.SIGNATURES if n.startswith('lasr_meshcheck_')) == [
        'lasr_meshcheck_faces', 'lasr_meshcheck_pairs', 'lasr_meshcheck_workspace_bytes']


def test_symbols_are_exported_and_the_host_checks_run_without_a_device():
    from lasr_amd import _lib
    h = _lib.lib()
    assert h.lasr_abi_version() == 13
    wsb = h.lasr_meshcheck_workspace_bytes
    assert wsb(0, 0) == 0 and wsb(2, 0) == 0 and wsb(-1, 5) == 0 and wsb(1, -5) == 0
    assert wsb(1, 256) == 256 * 72 + 16 and wsb(1, 257) == 257 * 72 + 32 and wsb(3, 640) == 3 * (640 * 72 + 3 * 16)
    assert wsb(1, 81920) == 81920 * 72 + 320 * 16                                 # the largest mesh of the raster tests
    assert wsb(1, 1 << 20) == (1 << 20) * 72 + 4096 * 16 and wsb(1, (1 << 20) + 1) == 0
    assert wsb(65535, 1) > 0 and wsb(65536, 1) == 0
    assert wsb(4096, 1 << 19) == 0 and wsb(4095, 1 << 19) == 4095 * ((1 << 19) * 72 + 2048 * 16)      # T F up to INT_MAX; past 2^32 bytes
    n, a, b, c, d, e, f = None, 64, 128, 192, 256, 320, 384                        # non-NULL addresses, never followed
    big = 1 << 40
    fac = lambda T=1, V=3, F=1, v=a, fa=b, ws=c, nb=big, vol=d, ar=e: h.lasr_meshcheck_faces(v, fa, ws, nb, vol, ar, T, V, F, n)   # noqa: E731
    assert fac(T=0) == 0 and fac(F=0) == 0 and fac(T=0, v=n, fa=n, ws=n, vol=n, ar=n) == 0              # nothing to do
    assert fac(T=-1) == -1 and fac(F=-1) == -1 and fac(V=-1) == -1 and fac(T=0, V=-1) == -1
    assert fac(T=65536, F=0) == -1 and fac(T=0, F=(1 << 20) + 1) == -1 and fac(T=0, F=1 << 20) == 0
    assert fac(T=4096, F=1 << 19, nb=0) == -1                                     # T F past INT_MAX
    assert fac(T=0, V=(1 << 31) // 3 + 1) == -1
    assert fac(V=0) == -1                                                         # faces without a vertex to name
    for k in ('v', 'fa', 'ws', 'vol', 'ar'):
        assert fac(**{k: n}) == -1, k                                            # null buffers
    assert fac(vol=d, ar=d) == -1 and fac(ws=d, vol=d) == -1 and fac(ws=e) == -1                        # aliasing outputs
    assert fac(v=c) == -1 and fac(fa=d) == -1 and fac(v=e) == -1                                        # an output that is an input
    assert fac(nb=72 + 16 - 1) == -3 and fac(T=2, F=300, nb=2 * (300 * 72 + 32) - 1) == -3             # LASR_E_WORKSPACE
    par = lambda T=1, F=1, mp=4, ws=a, nb=big, fc=b, np_=c, cu=d, pa=e: h.lasr_meshcheck_pairs(ws, nb, fc, np_, cu, pa, T, F, mp, n)   # noqa: E731
    assert par(T=0) == 0 and par(F=0) == 0 and par(T=0, ws=n, fc=n, np_=n, cu=n, pa=n) == 0
    assert par(T=-1) == -1 and par(F=-1) == -1 and par(mp=-1) == -1 and par(T=0, mp=-1) == -1
    assert par(T=0, F=(1 << 20) + 1) == -1 and par(T=65536, F=0) == -1
    assert par(T=0, mp=1 << 30) == 0 and par(T=2, F=0, mp=1 << 29) == -1 and par(T=2, F=0, mp=(1 << 29) - 1) == 0   # 2 T max_pairs
    for k in ('ws', 'fc', 'np_', 'cu', 'pa'):
        assert par(**{k: n}) == -1, k
    assert par(fc=c) == -1 and par(cu=b) == -1 and par(pa=c) == -1 and par(pa=d) == -1 and par(fc=a) == -1 and par(pa=a) == -1
    assert par(nb=72 + 16 - 1) == -3
    assert par(mp=0, pa=n, nb=0) == -3                                            # max_pairs = 0 needs no list: it got past the pointers
    names = [h.lasr_prof_kernel_name(i) for i in range(h.lasr_prof_kernel_count())]
    assert not any(b'meshcheck' in s for s in names)                              # the kernel table is not extended


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from lasr_amd.nnutils import meshcheck as mc
    v, f = torch.zeros(2, 3, 3), torch.tensor([[0, 1, 2]])
    for call in (lambda: mc.self_intersections(v, f), lambda: mc.volume_area(v, f), lambda: mc.evaluate(v, f), lambda: mc.jitter(v)):
        with pytest.raises(TypeError, match='support only cuda'):
            call()
    with pytest.raises(TypeError, match='must be a tensor'):
        mc.evaluate(v.numpy(), f)
    with pytest.raises(TypeError, match='must be a tensor'):
        mc.jitter(v.numpy())
    mc.check_indices(f, 3)
    mc.check_indices(f[:0], 0)
    for bad in (torch.tensor([[0, 1, 3]]), torch.tensor([[0, -1, 2]]), torch.tensor([[0, 1, 2], [2, 1, 1 << 20]])):
        with pytest.raises(ValueError, match=r'outside \[0, 3\)'):
            mc.check_indices(bad, 3)
    p = np.array([[[5, 9], [0, 7], [5, 6], [0, 0]], [[1, 2], [0, 0], [0, 0], [0, 0]]], np.int32)
    got = mc.sort_pairs(p, np.array([3, 5]), 4)
    assert got[0].tolist() == [[0, 7], [5, 6], [5, 9]] and got[0].dtype == np.int64 and got[1] is None
    assert mc.sort_pairs(p[:, :0], np.array([0, 1]), 0)[0].shape == (0, 2) and mc.DEFAULT_MAX_PAIRS == 4096


def _script():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import eval_shape
    return eval_shape


def test_script_arguments_and_summary():
    es = _script()
    a = es.parse_args(['--testdir', 'log/camel-5/', '--seqname', 'camel'])
    assert (a.testdir, a.seqname, a.outpath, a.worst, a.max_pairs, a.ply) == ('log/camel-5/', 'camel', '', 5, 4096, '')
    a = es.parse_args('--outpath s.json --worst 2 --max_pairs 16 --ply out'.split())
    assert (a.outpath, a.worst, a.max_pairs, a.ply) == ('s.json', 2, 16, 'out')
    for flag in ('--testdir', '--seqname', '--outpath', '--worst', '--max_pairs', '--ply'):
        assert flag in es.__doc__
    assert 'neighbouring faces goes' in ' '.join(es.__doc__.split())              # the blind spot is stated
    nan = float('nan')
    res = dict(n_pairs=np.array([0, 12, 3, 0]), n_faces=np.array([0, 10, 4, 0]), ratio=np.array([0., 0.5, 0.2, 0.]),
               volume=np.array([1., 2., -3., 4.]), area=np.array([6., 6., 8., 6.]), jitter=np.array([nan, 0.25, 0.75, nan]),
               inverted=np.array([False, False, True, False]), truncated=np.array([False, True, False, False]))
    doc = es.summarise(res, [0, 2, 4, 6], dict(seqname='x'))
    assert json.loads(json.dumps(doc)) == doc                                     # plain types only
    assert doc['frame_ids'] == [0, 2, 4, 6] and doc['params'] == dict(seqname='x')
    assert doc['per_frame']['jitter'] == [None, 0.25, 0.75, None] and doc['per_frame']['n_pairs'] == [0, 12, 3, 0]
    assert doc['per_frame']['inverted'] == [False, False, True, False] and doc['per_frame']['truncated'] == [False, True, False, False]
    assert doc['means'] == dict(n_pairs=3.75, n_faces=3.5, ratio=0.175, volume=1., area=6.5, jitter=0.5)
    assert doc['nan_frames'] == dict(n_pairs=0, n_faces=0, ratio=0, volume=0, area=0, jitter=2)
    assert (doc['n_inverted'], doc['n_truncated']) == (1, 1)
    assert es.summary_line(doc) == ('shape: 4 frames, 3.8 intersecting pairs and 0.1750 of the faces involved per frame, volume 1, '
                                    'area 6.5, jitter 5.000e-01, 1 inverted')
    assert es.worst_lines(doc, 3) == ['worst: frame 2 (position 1) 12 pairs, 10 faces, ratio 0.5000, truncated',
                                      'worst: frame 4 (position 2) 3 pairs, 4 faces, ratio 0.2000, inverted',
                                      'worst: frame 0 (position 0) 0 pairs, 0 faces, ratio 0.0000']
    assert es.worst_lines(doc, 0) == []
    two = es.summarise(dict({k: v[:2] for k, v in res.items()}, jitter=np.full(2, nan)), [0, 1], {})    # two frames: no jitter at all
    assert two['means']['jitter'] is None and two['nan_frames']['jitter'] == 2 and two['means']['n_pairs'] == 6.
    assert 'jitter n/a' in es.summary_line(es.summarise(dict(res, jitter=np.full(4, nan)), [0, 1, 2, 3], {}))
    col = es.vertex_colours(np.array([0, 2, 0]), np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6]]), 8)
    assert col.dtype == np.uint8 and [tuple(c) for c in col] == [es.GREY] * 2 + [es.RED] * 3 + [es.GREY] * 3
    with pytest.raises(ValueError, match='pred7 does not share the topology of pred3'):
        es.check_topology([np.array([[0, 1, 2]]), np.array([[0, 2, 1]])], [3, 7])
    with pytest.raises(ValueError, match='pred7 has a vertex that is not finite'):
        es.check_finite([np.zeros((2, 3)), np.array([[0., np.inf, 0.]])], [3, 7])


def test_script_end_to_end_on_the_restatement(tmp_path, monkeypatch, capsys):
    """main() with the float64 restatement injected: loading, the refusals, the JSON and the coloured meshes, without a device."""
    es = _script()
    from lasr_amd.ext_utils.ply import read_ply
    verts, faces = mr.fixture('two2')
    root = str(tmp_path)
    test = mr.write_sequence(root, 'balls', verts, faces)
    monkeypatch.chdir(root)

    def restated(v, f, max_pairs):
        r = mr.evaluate(v, f)
        return dict(r, ratio=r['n_faces'] / f.shape[0], inverted=r['volume'] < 0, truncated=r['n_pairs'] > max_pairs)
    doc = es.main(['--testdir', test, '--seqname', 'balls', '--worst', '1', '--ply', os.path.join(root, 'ply'), '--max_pairs', '90'],
                  evaluate=restated)
    assert json.load(open(os.path.join(test, 'shape.json'))) == doc
    loaded = np.stack([read_ply(os.path.join(test, 'pred%d.ply' % i))['verts'] for i in range(3)]).astype(np.float32)
    assert mr.uncertain(loaded, faces, 4 * mr.det_spread(loaded, faces)[0]) == []  # also after the six decimals of a .ply
    exp = mr.evaluate(loaded, faces)
    assert doc['per_frame']['n_pairs'] == exp['n_pairs'].tolist() and doc['per_frame']['volume'] == exp['volume'].tolist()
    assert doc['per_frame']['truncated'] == [False, False, True] and doc['params']['faces'] == 640 and doc['params']['vertices'] == 324
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == es.summary_line(doc) and lines[1].startswith('worst: frame 2 (position 2) ') and len(lines) == 3
    for t in range(3):
        m = read_ply(os.path.join(root, 'ply', 'shape-%05d.ply' % t))
        red = np.unique(faces[exp['face_count'][t] > 0].reshape(-1))
        assert (np.nonzero((m['colors'] == es.RED).all(1))[0] == red).all()
        assert ((m['colors'] == es.RED).all(1) | (m['colors'] == es.GREY).all(1)).all()
    bad = verts.copy()
    bad[1, 5, 2] = np.nan
    test = mr.write_sequence(root, 'broken', bad, faces)
    with pytest.raises(SystemExit, match='pred1 has a vertex that is not finite'):
        es.main(['--testdir', test, '--seqname', 'broken'], evaluate=restated)
    with pytest.raises(SystemExit, match='no config for sequence nothing'):
        es.main(['--testdir', test, '--seqname', 'nothing'], evaluate=restated)
