"""The neighbour pass of the shape scores without a device: closed forms of the restatement (tests/meshnbr_restated.py), the fixture
table of DESIGN.md section 4.18, the condition the GPU equalities of tests/test_meshnbr_gpu.py rest on, header against binding, the C
ABI's host-side checks, the Python layer's refusals, the flags of scripts/eval_shape.py and scripts/reconstruct.py, and the launch
sites of scripts/shape_neighbours.py against the guarded case (tests/meshnbr_guarded.py).

The condition: per tested pair no plane or edge determinant, and no d d - k q, lies within 4 x its own |float32 - float64|
difference of zero, so the strict sign tests cannot come out differently in the kernel.  Measured with this file, the worst ratio
|value| / |difference| over all fixtures: 197 for the determinants (crease3), 1799 for d d - k q (creaseA, creaseB), against the 4
required."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

import meshcheck_restated as mr
import meshnbr_guarded
import meshnbr_restated as nr
from test_guarded_alloc_cpu import launched_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = (np.float64, np.float32)
ENTRY_POINTS = ('lasr_meshnbr_list', 'lasr_meshnbr_test')


def _one(verts, faces, dt=np.float64, fold_deg=20.):
    return nr.neighbour_tests(np.asarray(verts, np.float32), np.asarray(faces, np.int32), fold_deg, dt)[0]


# ---- closed forms -------------------------------------------------------------------------------------------------------------------
# a triangle in the plane z = 0 with its corner 0 at the origin, and a partner that shares that corner (index 0)
BASE = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]


@pytest.mark.parametrize('dt', BOTH)
def test_a_vertex_pair_whose_opposite_edge_passes_through_the_other_is_pierced(dt):
    verts, faces = BASE + [(1, 1, -1), (1, 1, 1)], [(0, 1, 2), (0, 3, 4)]           # edge 3-4 goes through the interior of the base
    top = nr.topology(faces)
    assert top['n_list'] == 1 and top['n_vertex'] == 1 and top['keys'].tolist() == [nr.pack(0, 1, 0, 0, nr.VERTEX, 0)]
    r = _one(verts, faces, dt)
    assert (r['n_pierced'], r['n_creased']) == (1, 0) and r['hits'].tolist() == [[0, 1, nr.VERTEX]]
    assert r['nbr_count'].tolist() == [[1, 1], [0, 0]] and r['n_neighbour_faces'] == 2 and np.isnan(r['min_cos'])
    assert mr.self_intersections(np.array(verts, np.float32), np.array(faces))[0]['n_candidates'] == 0      # the pair pass never looks
    # the shared corner at other positions of both faces, and the base's opposite edge through the partner
    for fa, fb, ca, cb in (((1, 2, 0), (3, 0, 4), 2, 1), ((2, 0, 1), (4, 3, 0), 1, 2)):
        assert nr.topology([fa, fb])['keys'].tolist() == [nr.pack(0, 1, ca, cb, nr.VERTEX, 0)]
        assert _one(verts, [fa, fb], dt)['n_pierced'] == 1
    # the other way round: the partner stands in the plane x = y, its own opposite edge far outside the base, and the base's
    # opposite edge crosses it at (1, 1, 0)
    thru = [(0, 0, 0), (3, -1, 0), (-1, 3, 0), (4, 4, -5), (4, 4, 5)]
    assert _one(thru, [(0, 1, 2), (0, 3, 4)], dt)['n_pierced'] == 1 and _one(thru, [(0, 3, 4), (1, 2, 0)], dt)['n_pierced'] == 1


@pytest.mark.parametrize('dt', BOTH)
def test_touching_in_the_vertex_only_and_coplanar_vertex_pairs_are_not_pierced(dt):
    apart = BASE + [(-1, -1, -1), (-1, -1, 1)]                                    # the same partner moved away: only the corner touches
    assert _one(apart, [(0, 1, 2), (0, 3, 4)], dt)['n_pierced'] == 0
    beside = BASE + [(5, -1, -1), (5, -1, 1)]                                     # crosses the base's plane outside the base
    assert _one(beside, [(0, 1, 2), (0, 3, 4)], dt)['n_pierced'] == 0
    coplanar = BASE + [(1, 1, 0), (3, 0.5, 0)]                                    # overlaps the base in its own plane: every sign test is strict
    assert _one(coplanar, [(0, 1, 2), (0, 3, 4)], dt)['n_pierced'] == 0
    onplane = BASE + [(1, 1, 0), (1, 1, 2)]                                       # the opposite edge ends on the base
    assert _one(onplane, [(0, 1, 2), (0, 3, 4)], dt)['n_pierced'] == 0


def _hinge(deg, reverse=False):
    """Two faces on the edge (0,0,0)-(0,1,0) with the interior dihedral angle `deg` (180: flat), consistently oriented."""
    a = np.radians(deg)
    verts = [(0, 0, 0), (0, 1, 0), (1, 0.5, 0), (np.cos(a), 0.25, np.sin(a))]
    return verts, [(0, 1, 2), (1, 0, 3)[::-1] if reverse else (1, 0, 3)]


@pytest.mark.parametrize('dt', BOTH)
def test_edge_pairs_are_creased_below_the_fold_angle_whatever_the_orientation(dt):
    for deg, want in ((5, 1), (19, 1), (21, 0), (90, 0), (180, 0)):
        for reverse in (False, True):
            verts, faces = _hinge(deg, reverse)
            top = nr.topology(faces)
            assert (top['n_edge'], top['n_vertex'], top['n_same']) == (1, 0, int(reverse))
            r = _one(verts, faces, dt)
            assert r['n_creased'] == want and r['n_pierced'] == 0, (deg, reverse)
            assert r['hits'].tolist() == ([[0, 1, nr.EDGE]] if want else []) and r['nbr_count'].tolist() == [[0, 0], [want, want]]
            assert abs(float(nr.dihedral(r['min_cos'])) - deg) < 1e-3             # the same angle with one face reversed
    verts, faces = _hinge(19)
    assert _one(verts, faces, dt, 18.)['n_creased'] == 0 and _one(verts, faces, dt, 90.)['n_creased'] == 1
    assert _one(*_hinge(91), dt, 90.)['n_creased'] == 0 and _one(*_hinge(89), dt, 90.)['n_creased'] == 1
    # the apex positions and the direction bit of the key
    assert nr.topology([(0, 1, 2), (1, 0, 3)])['keys'].tolist() == [nr.pack(0, 1, 2, 2, nr.EDGE, 0)]
    assert nr.topology([(2, 0, 1), (3, 0, 1)])['keys'].tolist() == [nr.pack(0, 1, 0, 0, nr.EDGE, 1)]
    assert nr.topology([(1, 2, 0), (0, 3, 1)])['keys'].tolist() == [nr.pack(0, 1, 1, 1, nr.EDGE, 0)]
    assert float(nr.fold_k(20.)) == float(np.float32(np.cos(np.radians(20.)) ** 2)) and nr.fold_k(20.).dtype == np.float32


def test_degenerate_duplicate_and_non_manifold_faces():
    verts = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)], np.float32)
    top = nr.topology([(0, 1, 2), (0, 1, 1), (1, 2, 3)])                         # a repeated index: counted, part of nothing
    assert (top['n_degenerate'], top['n_list'], top['n_edge']) == (1, 1, 1) and (top['i'].tolist(), top['j'].tolist()) == ([0], [2])
    top = nr.topology([(0, 1, 2), (1, 2, 0), (2, 1, 0), (0, 1, 3)])              # the same three corners: counted, never tested
    assert top['n_duplicate'] == 3 and top['n_list'] == 3 and top['n_edge'] == 3 and top['j'].tolist() == [3, 3, 3]
    r = _one(verts, [(0, 1, 2), (1, 2, 0), (0, 1, 1)])
    assert (r['n_pierced'], r['n_creased']) == (0, 0) and np.isnan(r['min_cos']) and np.isnan(nr.dihedral(r['min_cos']))
    fan = nr.topology([(0, 1, 2), (1, 0, 3), (0, 1, 4)])                          # three faces on the edge 0-1: three edge pairs
    assert (fan['n_edge'], fan['n_vertex'], fan['n_same']) == (3, 0, 1)
    assert list(zip(fan['i'].tolist(), fan['j'].tolist())) == [(0, 1), (0, 2), (1, 2)]
    assert nr.topology(np.zeros((0, 3), np.int32))['n_list'] == 0 and nr.topology([(0, 1, 2), (3, 4, 5)])['n_list'] == 0
    zero = _one(np.zeros((4, 3), np.float32), [(0, 1, 2), (1, 0, 3)])             # q = 0: not creased, no angle
    assert zero['n_creased'] == 0 and np.isnan(zero['min_cos'])
    huge = _one(np.array(_hinge(5)[0], np.float32) * 1e6, _hinge(5)[1], np.float32)      # q overflows float32: not creased
    assert huge['n_creased'] == 0 and _one(np.array(_hinge(5)[0]) * 1e4, _hinge(5)[1], np.float32)['n_creased'] == 1
    assert _one(np.array(_hinge(5)[0]) * 1e-4, _hinge(5)[1], np.float32)['n_creased'] == 1             # the stated range of edge lengths
    i, j, ca, cb, kind, same = nr.unpack(nr.pack(1048575, 1048574, 2, 1, 1, 1))
    assert (int(i), int(j), int(ca), int(cb), int(kind), int(same)) == (1048575, 1048574, 2, 1, 1, 1)


# ---- the table of the fixtures ------------------------------------------------------------------------------------------------------
TABLE = {   # faces, vertex pairs, edge pairs, same, pierced pairs, creased pairs, min dihedral per frame (3 decimals), pair pass today
    'ico1': (80, 330, 120, 0, [[]], [[]], [150.002], [0]),
    'ico2': (320, 1410, 480, 0, [[]], [[]], [143.753], [0]),
    'inverted': (320, 1410, 480, 0, [[]], [[]], [143.753], [0]),
    'pinch2': (320, 1410, 480, 0, [[]], [[]], [64.590], [10]),
    'tile257': (257, 992, 361, 0, [[]], [[]], [145.201], [82]),
    'two2': (640, 2820, 960, 0, [[]] * 3, [[]] * 3, [145.201] * 3, [0, 83, 94]),
    'wobble': (320, 1410, 480, 0, [[]] * 5, [[]] * 5, [135.098, 139.317, 141.175, 131.172, 134.878], [0] * 5),
    'creaseA': (320, 1410, 480, 0, [[]], [[(152, 308), (216, 228)]], [0.788], [0]),
    'creaseB': (320, 1410, 480, 0, [[(152, 311), (216, 231)]], [[(152, 308), (216, 228), (228, 231)]], [5.912], [4]),
    'crease3': (1280, 5730, 1920, 0, [[]], [[(1220, 1223)]], [7.875], [0]),
    'flip1': (320, 1410, 480, 3, [[]], [[]], [143.753], [0]),
    'batch3': (320, 1410, 480, 0, [[], [], [(152, 311), (216, 231)]], [[], [(152, 308), (216, 228)], [(152, 308), (216, 228), (228, 231)]],
               [144.790, 0.788, 5.912], [0, 0, 4]),
}


@pytest.mark.parametrize('name', sorted(nr.FIXTURES))
def test_fixture_is_the_row_of_the_table_and_meets_the_condition_of_the_gpu_equalities(name):
    verts, faces = nr.fixture(name)
    F, n_vertex, n_edge, n_same, pierced, creased, angle, pair_pass = TABLE[name]
    exp = nr.expected(name)
    top = exp['topology']
    det, margin = nr.margins(verts, faces)
    print('%s: T %d F %d, list %d / %d, %d same, pierced %s, creased %s, min dihedral %s, worst |det| / |det32 - det64| %.0f, worst '
          '|dd - kq| ratio %.0f' % (name, verts.shape[0], F, top['n_vertex'], top['n_edge'], top['n_same'], exp['n_pierced'].tolist(),
                                    exp['n_creased'].tolist(), np.round(exp['min_dihedral'], 3).tolist(), det, margin))
    assert faces.shape == (F, 3) and (top['n_vertex'], top['n_edge'], top['n_same']) == (n_vertex, n_edge, n_same)
    assert top['n_list'] == n_vertex + n_edge == len(exp['keys']) and top['n_duplicate'] == 0 and top['n_degenerate'] == 0
    assert (np.diff(exp['keys']) > 0).all()                                       # lexicographic, and no pair twice
    for t, h in enumerate(exp['hits']):
        assert [tuple(x[:2]) for x in h.tolist() if x[2] == nr.VERTEX] == pierced[t]
        assert [tuple(x[:2]) for x in h.tolist() if x[2] == nr.EDGE] == creased[t]
    assert exp['n_pierced'].tolist() == [len(p) for p in pierced] and exp['n_creased'].tolist() == [len(c) for c in creased]
    assert np.round(exp['min_dihedral'], 3).tolist() == angle
    assert [r['n_pairs'] for r in mr.self_intersections(verts, faces)] == pair_pass                    # what the script says today
    # the condition, and both precisions name the same pairs
    assert det > 4 and margin > 4
    r32 = nr.neighbour_tests(verts, faces, dt=np.float32)
    for a, b, count in zip(exp['hits'], r32, exp['nbr_count']):
        assert a.tolist() == b['hits'].tolist() and (b['nbr_count'] == count).all()
    assert np.abs(np.array([b['min_cos'] for b in r32]) - exp['min_cos']).max() < 1e-5                 # the bound the device is held to


def test_fixtures_are_what_the_gpu_tests_need():
    a, b = nr.expected('creaseA'), nr.expected('creaseB')
    for e in (a, b):                                                              # hits inside tile 0, and hits that join tile 0 and tile 1
        assert {(i // 256, j // 256) for i, j, _ in e['hits'][0].tolist()} == {(0, 0), (0, 1)}
    assert nr.expected('crease3')['hits'][0][0, 0] // 256 == 4                    # the last of five tiles
    flip = nr.fixture('flip1')
    top = nr.topology(flip[1])
    blind = dict(top, same=np.zeros_like(top['same']))                            # without the negation the three edges read as folded flat
    creased, d, q, _ = nr.edge_pairs(flip[0][0], flip[1], blind, nr.fold_k())
    assert creased.sum() == 3 and (creased == (top['same'][top['kind'] == nr.EDGE] == 1)).all()
    assert nr.edge_pairs(flip[0][0], flip[1], top, nr.fold_k())[0].sum() == 0
    v, f = nr.fixture('batch3')
    assert (v[1] == nr.fixture('creaseA')[0][0]).all() and (v[2] == nr.fixture('creaseB')[0][0]).all() and (f == nr.fixture('creaseA')[1]).all()
    assert mr.self_intersections(*nr.fixture('creaseA'))[0]['n_pairs'] == 0 and nr.expected('creaseA')['n_creased'][0] == 2     # the blind spot


def test_copies_fixture_is_what_its_argument_says():
    """Eight exact translates of creaseB on the 2^-16 grid: 2560 faces in 10 tiles whose answer is 8 x the base's."""
    v0, f0 = nr.copies_base()
    det, margin = nr.margins(v0, f0)
    base = nr.neighbour_tests(v0, f0)[0]
    b32 = nr.neighbour_tests(v0, f0, dt=np.float32)[0]
    print('copies base: pierced %d, creased %d, worst ratios %.0f and %.0f' % (base['n_pierced'], base['n_creased'], det, margin))
    assert det > 4 and margin > 4 and base['hits'].tolist() == b32['hits'].tolist() == nr.expected('creaseB')['hits'][0].tolist()
    verts, faces, exp = nr.copies_case(8)
    assert verts.shape == (1, 8 * 162, 3) and faces.shape == (2560, 3)
    top = nr.topology(faces)
    assert (top['keys'] == exp['keys']).all() and {k: top[k] for k in exp['topology']} == exp['topology']
    assert (exp['n_pierced'], exp['n_creased']) == (16, 24) and exp['topology']['n_vertex'] == 8 * 1410
    for dt in BOTH:
        whole = nr.neighbour_tests(verts, faces, dt=dt, top=top)[0]
        assert whole['hits'].tolist() == exp['hits'].tolist() and (whole['nbr_count'] == exp['nbr_count']).all()
        assert (whole['n_pierced'], whole['n_creased']) == (exp['n_pierced'], exp['n_creased'])
    assert nr.neighbour_tests(verts, faces, dt=np.float32, top=top)[0]['min_cos'] == b32['min_cos']    # the same bits in every copy
    assert len({(i // 256, j // 256) for i, j, _ in exp['hits'].tolist()}) >= 8


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

def test_header_and_binding_agree_on_the_two_entry_points():
    from lasr_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    bare = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    scalar = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float}
    want = {'lasr_meshnbr_list': 'faces list counters F capacity hip_stream',
            'lasr_meshnbr_test': 'workspace workspace_bytes list n_list k nbr_count totals cursor hits min_cos T F max_pairs hip_stream'}
    for name in ENTRY_POINTS:
        args = [' '.join(a.split()) for a in re.search(r'\bint %s\s*\((.*?)\);' % name, bare, re.S).group(1).split(',')]
        assert [a.replace('*', ' ').split()[-1] for a in args] == want[name].split()
        res, sig = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and sig == [ctypes.c_void_p if '*' in a else scalar[a.split()[0]] for a in args]
    assert '#define LASR_MESHNBR_COUNTERS %d\n' % _lib.MESHNBR_COUNTERS in hdr and _lib.MESHNBR_COUNTERS == 4
    assert sorted(n for n in _lib.SIGNATURES if n.startswith('lasr_meshnbr_')) == sorted(ENTRY_POINTS)
    assert _lib.ABI_VERSION == 13                                                 # new symbols only
    for word in ('fold_deg = 20 is derived from nothing measured', 'about 1e-4 to 1e4', 'angle criterion'):
        assert word in ' '.join(hdr.split())


def test_symbols_are_exported_and_the_host_checks_run_without_a_device():
    from lasr_amd import _lib
    h = _lib.lib()
    n, a, b, c, d, e, f, g = None, 64, 128, 192, 256, 320, 384, 448               # non-NULL addresses, never followed
    lst = lambda F=256, cap=8, fa=a, li=b, co=c: h.lasr_meshnbr_list(fa, li, co, F, cap, n)        # noqa: E731
    assert lst(F=0) == 0 and lst(F=0, fa=n, li=n, co=n) == 0                      # nothing to do
    assert lst(F=-1) == -1 and lst(F=(1 << 20) + 1) == -1 and lst(cap=-1) == -1 and lst(F=0, cap=-1) == -1
    assert lst(fa=n) == -1 and lst(co=n) == -1 and lst(li=n) == -1                # null buffers (the list only when it has room)
    assert lst(li=a) == -1 and lst(co=a) == -1 and lst(co=b) == -1                # aliasing
    big = 1 << 40
    names = ('ws', 'li', 'nc', 'to', 'cu', 'hi', 'mc')

    def tst(T=1, F=1, nl=5, k=0.5, mp=4, nb=big, **kw):
        p = dict(zip(names, (a, b, c, d, e, f, g)))
        p.update(kw)
        return h.lasr_meshnbr_test(p['ws'], nb, p['li'], nl, k, p['nc'], p['to'], p['cu'], p['hi'], p['mc'], T, F, mp, n)
    none = {k: n for k in names}
    assert tst(T=0) == 0 and tst(F=0) == 0 and tst(nl=0) == 0 and tst(nl=0, **none) == 0 and tst(T=0, **none) == 0   # nothing launched
    assert tst(T=-1) == -1 and tst(F=-1) == -1 and tst(nl=-1) == -1 and tst(mp=-1) == -1 and tst(T=0, mp=-1) == -1
    assert tst(T=65536, F=0) == -1 and tst(T=0, F=(1 << 20) + 1) == -1 and tst(T=4096, F=1 << 19, nl=0) == -1       # T F past INT_MAX
    assert tst(k=-0.1) == -1 and tst(k=1.5) == -1 and tst(k=float('nan')) == -1 and tst(nl=0, k=2.) == -1
    assert tst(T=3, nl=0, mp=(1 << 31) // 9 + 1) == -1 and tst(T=3, nl=0, mp=(1 << 31) // 9) == 0                  # 3 T max_pairs
    for k in names:
        assert tst(**{k: n}) == -1, k
    for x, y in (('li', 'ws'), ('nc', 'ws'), ('to', 'nc'), ('cu', 'to'), ('hi', 'cu'), ('mc', 'hi'), ('mc', 'li'), ('hi', 'nc')):
        assert tst(**{x: dict(zip(names, (a, b, c, d, e, f, g)))[y]}) == -1, (x, y)
    assert tst(nb=72 + 16 - 1) == -3 and tst(T=2, F=300, nb=2 * (300 * 72 + 32) - 1) == -3                        # LASR_E_WORKSPACE
    assert tst(mp=0, hi=n, nb=0) == -3                                            # max_pairs = 0 needs no list: it got past the pointers
    table = [h.lasr_prof_kernel_name(i) for i in range(h.lasr_prof_kernel_count())]
    assert not any(b'meshnbr' in s for s in table)                                # the kernel table is not extended


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    import torch
    sn = meshnbr_guarded.shape_neighbours()
    v, f = torch.zeros(2, 3, 3), torch.tensor([[0, 1, 2]])
    for call in (lambda: sn.neighbour_list(f), lambda: sn.neighbour_tests(v, f), lambda: sn.evaluate(v, f)):
        with pytest.raises(TypeError, match='support only cuda'):
            call()
    with pytest.raises(TypeError, match='must be a tensor'):
        sn.neighbour_list(f.numpy())
    with pytest.raises(TypeError, match='must be a tensor'):
        sn.evaluate(v.numpy(), f)
    for bad in (0., -5., 90.5, float('nan'), float('inf')):                      # before the tensors are looked at: nothing is launched
        with pytest.raises(ValueError, match=r'fold_deg must be inside \(0, 90\]'):
            sn.neighbour_tests(v, f, fold_deg=bad)
        with pytest.raises(ValueError, match='fold_deg'):
            sn.evaluate(v, f, 16, bad)
    assert sn.fold_k(20.) == float(nr.fold_k(20.)) and sn.fold_k(90.) == float(nr.fold_k(90.)) and 0 < sn.fold_k(90.) < 1e-30
    with pytest.raises(ValueError, match='max_pairs'):
        sn._max_pairs(-1, 2)
    with pytest.raises(ValueError, match='max_pairs'):
        sn._max_pairs(1 << 29, 2)
    assert sn._max_pairs(0, 2) == 0 and (sn.DEFAULT_FOLD_DEG, sn.DEFAULT_MAX_PAIRS, sn.CAPACITY_PER_FACE) == (20., 4096, 16)
    h = np.array([[[5, 9, 1], [0, 7, 0], [5, 6, 1], [0, 0, 0]], [[1, 2, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]], np.int32)
    got = sn.sort_hits(h, np.array([3, 5]), 4)
    assert got[0].tolist() == [[0, 7, 0], [5, 6, 1], [5, 9, 1]] and got[0].dtype == np.int64 and got[1] is None
    assert np.array_equal(sn.dihedral(np.array([1., 0., -1., np.nan, 1.5], np.float32)), [180., 90., 0., np.nan, 180.], equal_nan=True)
    assert (sn.VERTEX, sn.EDGE) == (nr.VERTEX, nr.EDGE) and 'derived from nothing measured on a real reconstruction' in ' '.join(sn.__doc__.split())


# ---- the scripts --------------------------------------------------------------------------------------------------------------------

def _script():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import eval_shape
    return eval_shape


TODAY = dict(per_frame={'n_pairs', 'n_faces', 'ratio', 'volume', 'area', 'jitter', 'inverted', 'truncated'},
             means={'n_pairs', 'n_faces', 'ratio', 'volume', 'area', 'jitter'})
ADDED = {'n_pierced', 'n_creased', 'n_neighbour_faces', 'min_dihedral'}


def _restated(v, f, max_pairs, fold_deg=None):
    r = mr.evaluate(v, f)
    r = dict(r, ratio=r['n_faces'] / f.shape[0], inverted=r['volume'] < 0, truncated=r['n_pairs'] > max_pairs)
    return r if fold_deg is None else dict(r, **nr.evaluate(v, f, fold_deg))


def test_without_the_flag_the_script_is_what_it_was_and_with_it_the_keys_are_added(tmp_path, monkeypatch, capsys):
    es = _script()
    from lasr_amd.ext_utils.ply import read_ply
    a = es.parse_args(['--testdir', 't', '--seqname', 'x'])
    assert (a.neighbours, a.fold_deg) == (False, 20.)
    a = es.parse_args(['--neighbours', '--fold_deg', '12.5'])
    assert (a.neighbours, a.fold_deg) == (True, 12.5)
    doc = ' '.join(es.__doc__.split())
    assert 'neighbouring faces goes unseen unless --neighbours' in doc and 'derived from nothing measured on a real reconstruction' in doc
    assert '--neighbours' in es.__doc__ and '--fold_deg' in es.__doc__ and 'angle criterion' in doc
    verts, faces = nr.fixture('batch3')
    root = str(tmp_path)
    test = mr.write_sequence(root, 'fold', verts, faces)
    monkeypatch.chdir(root)
    loaded = np.stack([read_ply(os.path.join(test, 'pred%d.ply' % i))['verts'] for i in range(3)]).astype(np.float32)
    assert min(nr.margins(loaded, faces)) > 4                                     # also after the six decimals of a .ply
    # without the flag: today's keys, today's lines, today's colours; the evaluator is called with today's three arguments
    plain = es.main(['--testdir', test, '--seqname', 'fold', '--worst', '1', '--ply', os.path.join(root, 'ply0')], evaluate=_restated)
    lines0 = capsys.readouterr().out.splitlines()
    assert set(plain['per_frame']) == TODAY['per_frame'] and set(plain['means']) == set(plain['nan_frames']) == TODAY['means']
    assert set(plain) == {'params', 'frame_ids', 'per_frame', 'means', 'nan_frames', 'n_inverted', 'n_truncated'}
    assert set(plain['params']) == {'testdir', 'seqname', 'max_pairs', 'vertices', 'faces'}
    assert plain['per_frame']['n_pairs'] == [0, 0, 4] and len(lines0) == 3 and lines0[0] == es.summary_line(plain)
    exp0 = mr.evaluate(loaded, faces)
    for t in range(3):
        m = read_ply(os.path.join(root, 'ply0', 'shape-%05d.ply' % t))
        red = np.unique(faces[exp0['face_count'][t] > 0].reshape(-1))
        assert (np.nonzero((m['colors'] == es.RED).all(1))[0] == red).all()
        assert ((m['colors'] == es.RED).all(1) | (m['colors'] == es.GREY).all(1)).all()
    # with it
    doc = es.main(['--testdir', test, '--seqname', 'fold', '--worst', '1', '--ply', os.path.join(root, 'ply1'), '--neighbours',
                   '--outpath', os.path.join(root, 'nbr.json')], evaluate=_restated)
    lines1 = capsys.readouterr().out.splitlines()
    assert json.load(open(os.path.join(root, 'nbr.json'))) == doc and json.loads(json.dumps(doc)) == doc
    assert set(doc['per_frame']) == TODAY['per_frame'] | ADDED and set(doc['means']) == set(doc['nan_frames']) == TODAY['means'] | ADDED
    for k in TODAY['per_frame']:
        assert doc['per_frame'][k] == plain['per_frame'][k]                       # ratio and the rest stay defined as they are
    for k in TODAY['means']:
        assert doc['means'][k] == plain['means'][k]
    exp = nr.evaluate(loaded, faces)
    per = doc['per_frame']
    assert per['n_pierced'] == [0, 0, 2] and per['n_creased'] == [0, 2, 3] and per['n_neighbour_faces'] == exp['n_neighbour_faces'].tolist()
    assert per['min_dihedral'] == exp['min_dihedral'].tolist() and np.round(per['min_dihedral'], 2).tolist() == [144.79, 0.79, 5.91]
    assert doc['means']['n_creased'] == 5 / 3 and doc['nan_frames']['min_dihedral'] == 0
    p = doc['params']
    assert set(p) == set(plain['params']) | {'neighbours', 'fold_deg', 'vertex_pairs', 'edge_pairs', 'duplicate_faces', 'degenerate_faces',
                                             'same_direction_edges'}
    assert (p['neighbours'], p['fold_deg'], p['vertex_pairs'], p['edge_pairs'], p['duplicate_faces'], p['degenerate_faces'],
            p['same_direction_edges']) == (True, 20., 1410, 480, 0, 0, 0)
    assert lines1[0] == lines0[0] and lines1[1] == es.neighbour_line(doc) and lines1[2] == lines0[1] and len(lines1) == 4
    assert lines1[1].startswith('neighbours: 0.7 pierced and 1.7 creased pairs (below 20 degrees) per frame') and '0.788 degrees' in lines1[1]
    seen = []
    for t in range(3):
        m = read_ply(os.path.join(root, 'ply1', 'shape-%05d.ply' % t))
        red = np.unique(faces[exp0['face_count'][t] > 0].reshape(-1))
        orange = np.setdiff1d(np.unique(faces[exp['nbr_count'][t].sum(0) > 0].reshape(-1)), red)
        seen.append((len(red), len(orange)))
        assert (np.nonzero((m['colors'] == es.RED).all(1))[0] == red).all()      # red wins
        assert (np.nonzero((m['colors'] == es.ORANGE).all(1))[0] == orange).all()
        assert ((m['colors'] == es.RED).all(1) | (m['colors'] == es.GREY).all(1) | (m['colors'] == es.ORANGE).all(1)).all()
    assert seen[0] == (0, 0) and seen[1][0] == 0 and seen[1][1] > 0 and seen[2][0] > 0 and es.ORANGE == (255, 160, 0)
    col = es.vertex_colours(np.array([0, 2, 0]), np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6]]), 8, np.array([[1, 0, 0], [0, 0, 1]]))
    assert [tuple(c) for c in col] == [es.ORANGE] * 2 + [es.RED] * 3 + [es.ORANGE] * 2 + [es.GREY]
    with pytest.raises(SystemExit, match=r'--fold_deg must be inside \(0, 90\]'):
        es.main(['--testdir', test, '--seqname', 'fold', '--neighbours', '--fold_deg', '0'], evaluate=_restated)
    # a mesh without an edge pair has no angle: None in the JSON, n/a in the line
    lone = es.summarise(dict(_restated(loaded[:, :3], np.array([[0, 1, 2]], np.int32), 8, 20.)), [0, 1, 2], dict(p, faces=1))
    assert lone['per_frame']['min_dihedral'] == [None] * 3 and lone['means']['min_dihedral'] is None and lone['nan_frames']['min_dihedral'] == 3
    assert 'sharpest dihedral n/a' in es.neighbour_line(lone)


def test_reconstruct_hands_the_flag_to_the_shape_scores_and_swaps_the_caveat(tmp_path):
    from lasr_amd import pipeline as pl
    from test_reconstruct_cpu import by_name, load, make_args
    plain = pl.plan(make_args(tmp_path))
    with_flag = pl.plan(make_args(tmp_path, '--neighbours'))
    shape = by_name(with_flag)['scores-shape']
    assert shape.argv[-1] == '--neighbours' and shape.argv[:-1] == by_name(plain)['scores-shape'].argv
    a = load('scripts', 'eval_shape.py').parse_args(list(shape.argv[2:]))        # through the script's own parser
    assert a.neighbours and a.fold_deg == 20. and a.outpath == 'reconstruct/shape.json'
    assert not load('scripts', 'eval_shape.py').parse_args(list(by_name(plain)['scores-shape'].argv[2:])).neighbours
    # nothing else moves: the default plan names the flag nowhere, the other steps and every limit are the same
    assert not any('neighbours' in t for s in plain if s.argv for t in s.argv)
    assert [s for s in with_flag if s.name != 'scores-shape'] == [s for s in plain if s.name != 'scores-shape']
    assert [s.timeout_s for s in with_flag] == [s.timeout_s for s in plain]
    pieces, swapped = pl.describe(make_args(tmp_path))['pieces'], pl.describe(make_args(tmp_path, '--neighbours'))['pieces']
    assert 'eval_shape' in pieces and 'eval_shape_neighbours' not in pieces
    assert swapped == ['eval_shape_neighbours' if x == 'eval_shape' else x for x in pieces]
    text = pl.CAVEATS['eval_shape_neighbours']
    assert 'angle criterion' in text and 'nothing measured on a real reconstruction' in text and 'unverified' in text
    assert pl.CAVEATS['eval_shape'] == 'scripts/eval_shape.py does not see folds between neighbouring faces.'
    assert '--neighbours' in pl.driver_argv(make_args(tmp_path, '--neighbours')) and '--neighbours' not in pl.driver_argv(make_args(tmp_path))
    assert '--neighbours' in load('scripts', 'reconstruct.py').__doc__
    # the report shows the new means when the scores hold them
    doc = dict(sequence=dict(name='cat', frames=3, size=[8, 8], frames_kept_in_r=3), masks={}, flow_method='variational', schedule='quick',
               stages=[], exports=[], caveats=[text],
               scores=dict(shape=dict(means=dict(ratio=0., n_pierced=2 / 3, n_creased=5 / 3, min_dihedral=50.5), worst_by='ratio', worst=[])))
    md = pl.markdown(doc)
    assert 'n_pierced 0.6667' in md and 'n_creased 1.667' in md and 'min_dihedral 50.5' in md and text in md


# ---- the native scan ----------------------------------------------------------------------------------------------------------------

def test_every_native_shape_neighbours_launches_is_in_the_guarded_case():
    with open(os.path.join(ROOT, 'scripts', 'shape_neighbours.py')) as fh:
        names, opaque = launched_in(fh.read())
    assert not opaque and sorted(set(names)) == sorted(meshnbr_guarded.LAUNCHED) == sorted(ENTRY_POINTS)
    assert set(names) <= set(meshnbr_guarded.NATIVES) == set(meshnbr_guarded.CASE.natives)
    # the module reaches the per-face pass through lasr_amd/nnutils/meshcheck.py, which the table of tests/guarded_cases.py covers
    assert set(meshnbr_guarded.NATIVES) - set(names) == {'lasr_meshcheck_faces'}
    with open(os.path.join(ROOT, 'scripts', 'eval_shape.py')) as fh:
        assert launched_in(fh.read()) == ([], [])
