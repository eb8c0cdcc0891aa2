"""The fold penalty of the optimiser without a device: closed forms of the restatement (tests/foldpen_restated.py), its closed-form
gradient against float64 autograd, the conditions the GPU comparisons of tests/test_foldpen_gpu.py rest on, a descent on the
restatement alone, header against binding, the C ABI's host-side checks, the Python layer's refusals, the flags of optimize.py and
scripts/reconstruct.py, and the launch sites of scripts/fold_penalty.py against the guarded case (tests/foldpen_guarded.py).

The conditions, over every fixture the GPU test uses and at the angle it uses: no theta lies within 0.25 degrees of phi or of 0; no
determinant of a pierce test, and no |d_p| - |d_q| of a test that holds, lies within 4 x its own float32 / float64 difference of
zero.  No frame had to be left out.  Measured with this file: the nearest theta is 0.788 degrees from 0 (batch3 frame 1), the worst
determinant ratio 1375 (two2 frame 1; 2686 on batch3), the worst tie ratio 652 651 (batch3 frame 2, the only frame with a test that
holds), against the 4 required.

The descent (DESCENT below): plain gradient descent on crease + pierce of batch3, weights 1 : 1, phi = 30 degrees, rate 0.003, the
vertices kept in float32; counted after every step with meshnbr_restated.evaluate at 20 degrees.  From creased 0 / 2 / 3 and pierced
0 / 0 / 2 all counts are 0 after 36 steps in float64 and after 36 steps in float32 (cap 200), and the 4 intersecting non-neighbour
pairs meshcheck_restated counts in frame 2 are gone as well.  The crease term alone clears the creased counts after 5 steps at that
rate; the pierce term alone clears the pierced count after 4 steps at rate 0.01 and hovers at rate 0.003 (see the test).  At rate
0.01 the sum settles after 70 steps in float64 and not within 200 in float32 (the creased count of frame 2 comes and goes): that
rate is no part of the test."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

import foldpen_guarded
import foldpen_restated as fr
import meshcheck_restated as mr
import meshnbr_restated as nr
from test_guarded_alloc_cpu import launched_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = (np.float64, np.float32)
TOL = {np.float64: 2e-7, np.float32: 2e-6}          # the vertices are float32 in either precision: cos and sin rounded at 6e-8
ENTRY_POINTS = ('lasr_foldpen_scratch_bytes', 'lasr_foldpen_forward', 'lasr_foldpen_backward')
DESCENT = dict(rate=0.003, steps=200, fold_deg=30., weights=(1., 1.), count_deg=20.)
# fixture -> the angle the GPU test charges it at
GPU_FIXTURES = {'batch3': 30., 'tile257': 30., 'flip1': 30., 'pinch2': 30., 'two2': 30.}


def _one(verts, faces, dt=np.float64, fold_deg=30.):
    return fr.penalty(np.asarray(verts, np.float32)[None], np.asarray(faces, np.int32), fold_deg, dt)


# ---- closed forms -------------------------------------------------------------------------------------------------------------------
def _hinge(deg, reverse=False):
    """Two faces on the edge (0,0,0)-(0,1,0) with the interior dihedral angle `deg` (180: flat), both apexes at height 1 over it."""
    a = np.radians(deg)
    verts = [(0, 0, 0), (0, 1, 0), (1, 0.5, 0), (np.cos(a), 0.25, np.sin(a))]
    return verts, [(0, 1, 2), (1, 0, 3)[::-1] if reverse else (1, 0, 3)]


@pytest.mark.parametrize('dt', BOTH)
def test_a_hinge_opened_to_a_known_angle_gives_that_angle_and_its_square(dt):
    phi = fr.phi_of(30.)
    for deg in (0.5, 5., 12., 29.):
        got = []
        for reverse in (False, True):                                             # `same` flips nothing observable
            r = _one(*_hinge(deg, reverse), dt)
            assert r['values'].shape == (1, 1) and r['active'].all() and abs(float(r['theta'][0, 0]) - np.radians(deg)) < TOL[dt]
            assert abs(float(r['values'][0, 0]) - (phi - np.radians(deg)) ** 2) < TOL[dt]
            assert abs(float(r['loss'][0, 0]) - (phi - np.radians(deg)) ** 2) < TOL[dt] and r['loss'][0, 1] == 0
            got.append(r)
        assert abs(got[0]['values'] - got[1]['values']).max() < TOL[dt] and np.abs(got[0]['grad'] - got[1]['grad']).max() < 10 * TOL[dt]
    assert abs(float(_one(*_hinge(50.), dt, 60.)['values'][0, 0]) - np.radians(10.) ** 2) < 2 * TOL[dt]        # the angle is the caller's


@pytest.mark.parametrize('dt', BOTH)
def test_at_and_above_the_angle_the_value_and_the_gradient_are_exactly_zero(dt):
    for deg in (30.5, 31., 90., 150., 180.):
        for reverse in (False, True):
            r = _one(*_hinge(deg, reverse), dt)
            assert not r['active'].any() and not r['values'].any() and not r['loss'].any() and not r['grad'].any() and not r['rows'].any()
    loss, grad = fr.autograd(np.array(_hinge(45.)[0], np.float32)[None], np.array(_hinge(45.)[1]))
    assert not loss.any() and not grad.any()


@pytest.mark.parametrize('dt', BOTH)
def test_next_to_the_complete_fold_the_gradient_has_its_closed_form_magnitude(dt):
    """Both apexes stand at height 1 over the edge: |d value / d apex| = 2 (phi - theta) / 1, along the face's normal, where any
    function of the cosine alone would give 2 (phi - theta) sin(theta) or less: 0.0087 of it at 0.5 degrees."""
    phi, theta = fr.phi_of(30.), np.radians(0.5)
    verts, faces = _hinge(0.5)
    r = _one(verts, faces, dt)
    g = r['grad'][0, 0]
    want = 2 * (phi - theta)
    assert abs(np.linalg.norm(g[2]) - want) < 2e-4 * want and abs(np.linalg.norm(g[3]) - want) < 2e-4 * want
    assert abs(g[2, 2] - want) < 2e-4 * want and abs(g[2, 0]) < 1e-3 and abs(g[2, 1]) < 1e-6        # uphill is towards apex 3, above it
    assert np.abs(g.sum(0)).max() < 1e-5 and not r['grad'][1].any()                # no net force; no pierce term
    _, auto = fr.autograd(np.array(verts, np.float32)[None], np.array(faces))
    assert np.abs(auto[0, 0] - _one(verts, faces)['grad'][0, 0]).max() < 1e-9
    one_step = np.array(verts, np.float64) - 0.1 * _one(verts, faces)['grad'][0, 0]                    # and descent opens the fold
    assert _one(one_step, faces)['theta'][0, 0] > 10 * theta
    # the complete fold itself: the value is phi^2, the kink of the unsigned angle gets gradient 0, nothing is NaN
    flat = _one(*_hinge(0.), dt)
    assert flat['theta'][0, 0] == 0 and abs(float(flat['values'][0, 0]) - phi * phi) < TOL[dt] and not flat['grad'].any()
    assert not fr.autograd(np.array(_hinge(0.)[0], np.float32)[None], np.array(_hinge(0.)[1]))[1].any()


BASE = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]


@pytest.mark.parametrize('dt', BOTH)
def test_an_edge_through_a_triangle_at_a_known_depth_gives_the_depth(dt):
    verts, faces = BASE + [(1, 1, -0.5), (1, 1, 2)], [(0, 1, 2), (0, 3, 4)]         # edge 3-4 through the base, its end 3 half a unit below
    r = _one(verts, faces, dt)
    assert r['values'].tolist() == [[0.5]] and r['loss'].tolist() == [[0., 0.5]] and r['holds'].tolist() == [[[False, True]]]
    g = r['grad'][1, 0]
    assert np.allclose(g[3], (0, 0, -1), atol=1e-6) and not g[4].any()            # the shallower end moves on, out of the plane
    assert np.allclose(g[:3], np.array([0.5, 0.25, 0.25])[:, None] * np.array([0, 0, 1.]), atol=1e-6)  # the foot's barycentric weights
    assert r['slots'].tolist() == [[0, 1, 2, 3, 4]] and not r['grad'][0].any()
    for fa, fb in (((1, 2, 0), (3, 0, 4)), ((2, 0, 1), (4, 3, 0))):               # the shared corner at other positions of both faces
        other = _one(verts, [fa, fb], dt)
        assert other['values'].tolist() == [[0.5]] and np.abs(other['grad'] - r['grad']).max() < 1e-6
    tie = _one(BASE + [(1, 1, -1), (1, 1, 1)], faces, dt)                          # both ends at depth 1: p, the first end
    assert tie['values'].tolist() == [[1.]] and np.allclose(tie['grad'][1, 0, 3], (0, 0, -1)) and not tie['grad'][1, 0, 4].any()
    # the other way round: the partner stands in the plane x = y and the base's opposite edge crosses it at (1, 1, 0); its ends
    # (3, -1, 0) and (-1, 3, 0) are sqrt(8) away from that plane
    thru = [(0, 0, 0), (3, -1, 0), (-1, 3, 0), (4, 4, -5), (4, 4, 5)]
    r = _one(thru, faces, dt)
    assert abs(float(r['values'][0, 0]) - np.sqrt(8.)) < 4 * TOL[dt] and r['holds'].tolist() == [[[True, False]]]
    _, auto = fr.autograd(np.array(thru, np.float32)[None], np.array(faces))
    assert np.abs(auto[1, 0] - _one(thru, faces)['grad'][1, 0]).max() < 1e-9


@pytest.mark.parametrize('dt', BOTH)
def test_touching_coplanar_and_degenerate_pairs_give_zero(dt):
    faces = [(0, 1, 2), (0, 3, 4)]
    for extra in ([(-1, -1, -1), (-1, -1, 1)], [(5, -1, -1), (5, -1, 1)], [(1, 1, 0), (3, 0.5, 0)], [(1, 1, 0), (1, 1, 2)]):
        r = _one(BASE + extra, faces, dt)                                          # apart, beside, coplanar, ending on the base
        assert not r['values'].any() and not r['grad'].any() and not r['active'].any()
    verts = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)], np.float32)
    r = _one(verts, [(0, 1, 2), (0, 1, 1), (1, 2, 3)], dt)                         # a repeated index: part of nothing
    assert r['values'].shape == (1, 1) and r['slots'].tolist() == [[0, 1, 2, 3, -1]]
    zero = _one(np.zeros((4, 3), np.float32), [(0, 1, 2), (1, 0, 3)], dt)          # q = 0: value 0, gradient 0, nothing NaN
    assert not zero['values'].any() and not zero['grad'].any() and np.isfinite(zero['rows']).all()
    line = _one([(0, 0, 0), (0, 1, 0), (0, 2, 0), (1, 0.5, 0)], [(0, 1, 2), (1, 0, 3)], dt)            # one face of zero area
    assert not line['values'].any() and not line['grad'].any()
    huge = _one(np.array(_hinge(5.)[0], np.float32) * 1e6, _hinge(5.)[1], np.float32)                  # q overflows float32: not counted
    assert not huge['values'].any() and not huge['grad'].any()
    assert fr.penalty(nr.fixture('ico1')[0][:, :3], np.array([[0, 1, 2]], np.int32))['loss'].tolist() == [[0., 0.]]   # no entry


# ---- the restatement against itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['batch3', 'pinch2', 'crease3'])
def test_closed_form_gradient_equals_float64_autograd(name):
    verts, faces = nr.fixture(name)
    deg = 90. if name == 'pinch2' else 30.                                         # (pinch2's sharpest dihedral is 64.6 degrees)
    res = fr.penalty(verts, faces, deg)
    loss, grad = fr.autograd(verts, faces, deg)
    scale = max(np.abs(grad).max(), 1.)
    print('%s: loss %s, largest gradient %.3f, closed form off autograd by %.1e' % (name, res['loss'].tolist(), np.abs(grad).max(),
                                                                                   np.abs(res['grad'] - grad).max()))
    assert np.abs(res['loss'] - loss).max() < 1e-12 and np.abs(res['grad'] - grad).max() < 1e-11 * scale
    assert res['active'].any() and np.abs(grad).max() > 0.1


@pytest.mark.parametrize('name', sorted(GPU_FIXTURES))
def test_fixture_meets_the_conditions_of_the_gpu_comparisons(name):
    verts, faces = nr.fixture(name)
    cond = fr.conditions(verts, faces, GPU_FIXTURES[name])
    for t, c in enumerate(cond):
        print('%s frame %d: nearest theta %.3f degrees from phi or 0, worst determinant ratio %.0f, worst tie ratio %.0f'
              % (name, t, c['angle'], c['det'], c['tie']))
        assert c['angle'] > 0.25 and c['det'] > 4 and c['tie'] > 4 and c['same']
    res = fr.penalty(verts, faces, GPU_FIXTURES[name], closed=False)
    exp = nr.evaluate(verts, faces, GPU_FIXTURES[name])
    top = nr.topology(faces)
    edge = top['kind'] == nr.EDGE                                                  # charged is what the evaluation counts at that angle
    assert (res['active'][:, edge].sum(1) == exp['n_creased']).all() and (res['active'][:, ~edge].sum(1) == exp['n_pierced']).all()
    if name in ('pinch2', 'two2', 'tile257', 'flip1'):
        assert not res['loss'].any()
    if name == 'batch3':
        assert (res['loss'][0] == 0).all() and res['loss'][1, 0] > 0 and res['loss'][1, 1] == 0 and (res['loss'][2] > 0).all()


def test_copies_fixture_gives_eight_times_the_base():
    v0, f0 = nr.copies_base()
    cond = fr.conditions(v0, f0, 30.)[0]
    assert cond['angle'] > 0.25 and cond['det'] > 4 and cond['tie'] > 4
    verts, faces, _ = nr.copies_case(8)
    for dt in BOTH:
        base, whole = fr.penalty(v0, f0, 30., dt), fr.penalty(verts, faces, 30., dt)
        assert (whole['values'][0].reshape(8, -1) == base['values'][0]).all() and whole['active'].sum() == 8 * base['active'].sum() == 40
        assert np.abs(whole['loss'] - 8 * base['loss'].astype(np.float64)).max() < 1e-6
        assert np.abs(whole['grad'][:, 0].reshape(2, 8, 162, 3) - base['grad'][:, 0][:, None]).max() < 1e-6


@pytest.mark.parametrize('dt', BOTH)
def test_descent_on_the_restatement_clears_the_report(dt):
    verts, faces = nr.fixture('batch3')
    start = fr.counts(verts, faces)
    assert start[0].tolist() == [0, 2, 3] and start[1].tolist() == [0, 0, 2]
    step, x, history = fr.descend(verts, faces, dt=dt, **DESCENT)
    left = [r['n_pairs'] for r in mr.self_intersections(x, faces)]
    print('%s: all counts 0 after %s steps (cap %d); intersecting non-neighbour pairs at the end %s; moved at most %.4f'
          % (np.dtype(dt).name, step, DESCENT['steps'], left, np.abs(x - verts).max()))
    assert step is not None and step <= DESCENT['steps']
    assert not history[-1][0].any() and not history[-1][1].any() and (x[0] == verts[0]).all()           # the clean frame never moves
    # one term alone clears its own count: the crease term at the same rate, the pierce term at rate 0.01 (at 0.003 alone its two
    # pairs, which share vertices, hover at a depth of 0.004 for all 200 steps: a step of fixed length 0.003 carries the end point
    # across and the next one back; with the crease term beside it the ring opens and they leave)
    for term, rate, want in (((1., 0.), DESCENT['rate'], 0), ((0., 1.), 0.01, 1)):
        alone = fr.descend(verts, faces, dt=dt, **dict(DESCENT, weights=term, rate=rate, steps=12))[2]
        first = next((k + 1 for k, c in enumerate(alone) if not c[want].any()), None)
        print('  weights %s at rate %g: its own count is 0 after %s steps' % (term, rate, first))
        assert first is not None and not alone[-1][want].any()


def test_crease3_is_released_in_one_step():
    verts, faces = nr.fixture('crease3')
    step, _, _ = fr.descend(verts, faces, **dict(DESCENT, steps=5))
    assert step == 1


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_entry_points():
    from lasr_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    bare = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    scalar = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float}
    want = {'lasr_foldpen_scratch_bytes': ('size_t', 'N n_list'),
            'lasr_foldpen_forward': ('int', 'x faces list n_list phi values rows scratch scratch_bytes loss N V F hip_stream'),
            'lasr_foldpen_backward': ('int', 'rows vstart inc n_inc grad_loss gverts N V n_list hip_stream')}
    for name in ENTRY_POINTS:
        ret, names = want[name]
        args = [' '.join(a.split()) for a in re.search(r'\b%s %s\s*\((.*?)\);' % (ret, name), bare, re.S).group(1).split(',')]
        assert [a.replace('*', ' ').split()[-1] for a in args] == names.split()
        res, sig = _lib.SIGNATURES[name]
        assert res is scalar[ret] and sig == [ctypes.c_void_p if '*' in a else scalar[a.split()[0]] for a in args]
    assert '#define LASR_FOLDPEN_MAX_LIST %d\n' % _lib.FOLDPEN_MAX_LIST in hdr and 10 * _lib.FOLDPEN_MAX_LIST <= 0x7fffffff
    assert sorted(n for n in _lib.SIGNATURES if n.startswith('lasr_foldpen_')) == sorted(ENTRY_POINTS)
    assert _lib.ABI_VERSION == 13                                                 # new symbols only
    for word in ('derived from nothing measured on a real reconstruction', 'not of its cosine', 'the depth itself and not its square',
                 'No floating-point atomics anywhere', 'vertex pair: 0 the shared vertex'):
        assert word in ' '.join(hdr.replace(' * ', ' ').split()), word


def test_symbols_are_exported_and_the_host_checks_run_without_a_device():
    from lasr_amd import _lib
    h = _lib.lib()
    n, big = None, 1 << 40
    names = ('x', 'fa', 'li', 'va', 'ro', 'sc', 'lo')
    addr = dict(zip(names, (64, 128, 192, 256, 320, 384, 448)))                    # non-NULL addresses, never followed

    def fwd(N=1, V=3, F=1, nl=5, phi=0.5, nb=big, **kw):
        p = dict(addr, **kw)
        return h.lasr_foldpen_forward(p['x'], p['fa'], p['li'], nl, phi, p['va'], p['ro'], p['sc'], nb, p['lo'], N, V, F, n)
    none = {k: n for k in names}
    assert h.lasr_foldpen_scratch_bytes(3, 1890) == 3 * 8 * 2 * 8 and h.lasr_foldpen_scratch_bytes(1, 256) == 16
    assert h.lasr_foldpen_scratch_bytes(-1, 5) == 0 and h.lasr_foldpen_scratch_bytes(1, _lib.FOLDPEN_MAX_LIST + 1) == 0
    assert h.lasr_foldpen_scratch_bytes(65536, 1) == 0 and h.lasr_foldpen_scratch_bytes(0, 7) == 0
    assert fwd(N=0) == 0 and fwd(F=0) == 0 and fwd(nl=0) == 0 and fwd(nl=0, **none) == 0 and fwd(N=0, **none) == 0   # nothing launched
    assert fwd(N=-1) == -1 and fwd(V=-1) == -1 and fwd(F=-1) == -1 and fwd(nl=-1) == -1 and fwd(N=65536) == -1
    assert fwd(F=(1 << 20) + 1) == -1 and fwd(nl=_lib.FOLDPEN_MAX_LIST + 1, N=0) == -1 and fwd(N=4096, nl=1 << 20) == -1
    assert fwd(V=(1 << 31) // 3 + 1) == -1 and fwd(V=0) == -1
    for phi in (0., -0.1, 1.58, float('nan'), float('inf')):
        assert fwd(phi=phi) == -1 and fwd(phi=phi, nl=0) == -1
    assert fwd(phi=float(np.float32(np.pi / 2)), nb=15) == -3                      # 90 degrees is inside; it got past the pointers
    for k in names:
        assert fwd(nb=15, **{k: n}) == (-3 if k == 'ro' else -1), k                # rows may be NULL: no gradient wanted
    for a, b in (('va', 'x'), ('lo', 'va'), ('ro', 'va'), ('sc', 'lo'), ('li', 'fa'), ('ro', 'x'), ('lo', 'x')):
        assert fwd(**{a: addr[b]}) == -1, (a, b)
    assert fwd(nb=15) == -3 and fwd(N=3, nl=1890, nb=3 * 8 * 16 - 1) == -3 and fwd(nb=0) == -3         # LASR_E_WORKSPACE
    bnames = ('ro', 'vs', 'ic', 'gl', 'gv')
    baddr = dict(zip(bnames, (64, 128, 192, 256, 320)))

    def bwd(N=1, V=3, nl=5, ni=7, **kw):
        p = dict(baddr, **kw)
        return h.lasr_foldpen_backward(p['ro'], p['vs'], p['ic'], ni, p['gl'], p['gv'], N, V, nl, n)
    bnone = {k: n for k in bnames}
    assert bwd(N=0) == 0 and bwd(V=0) == 0 and bwd(N=0, **bnone) == 0             # nothing to write
    assert bwd(N=-1) == -1 and bwd(V=-1) == -1 and bwd(nl=-1) == -1 and bwd(ni=-1) == -1 and bwd(ni=26) == -1 and bwd(N=65536) == -1
    assert bwd(nl=0, ni=1) == -1 and bwd(gv=n) == -1 and bwd(nl=0, ni=0, gv=n) == -1                    # a zeroed gradient needs its buffer
    for k in bnames:
        assert bwd(**{k: n}) == -1, k
    for a, b in (('gv', 'ro'), ('gv', 'gl'), ('ic', 'vs'), ('gl', 'ro')):
        assert bwd(**{a: baddr[b]}) == -1, (a, b)
    table = [h.lasr_prof_kernel_name(i) for i in range(h.lasr_prof_kernel_count())]
    assert not any(b'foldpen' in s for s in table)                                # the kernel table is not extended


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    import torch
    fp = foldpen_guarded.fold_penalty()
    f = torch.tensor([[0, 1, 2], [1, 0, 3]])
    with pytest.raises(TypeError, match='support only cuda'):
        fp.FoldPenalty(f)
    with pytest.raises(TypeError, match='must be a tensor'):
        fp.FoldPenalty(f.numpy())
    for bad in (0., -5., 90.5, float('nan'), float('inf')):                      # before the tensors are looked at: nothing is launched
        with pytest.raises(ValueError, match=r'fold_penalty: fold_deg must be inside \(0, 90\]'):
            fp.FoldPenalty(f, bad)
        with pytest.raises(ValueError, match='fold_deg'):
            fp.fold_phi(bad)
    assert fp.fold_phi(30.) == fr.phi_of(30.) == float(np.float32(np.pi / 6)) and fp.fold_phi(90.) <= float(np.float32(1.5707964))
    assert fp.DEFAULT_FOLD_DEG == 30. == fr.FOLD_DEG and fp.SLOTS == 5
    assert 'derived from nothing measured on a real reconstruction' in ' '.join(fp.__doc__.split())
    pen = fp.FoldPenalty.__new__(fp.FoldPenalty)                                  # the checks of a call, without a device
    pen.faces, pen.keys = f.int(), torch.zeros(0, dtype=torch.int64)
    with pytest.raises(TypeError, match='must be a tensor'):
        pen(np.zeros((1, 4, 3), np.float32))
    with pytest.raises(TypeError, match='support only cuda'):
        pen(torch.zeros(1, 4, 3))
    # the inverted index is plain torch: the slots and the order of the restatement
    verts, faces = nr.fixture('ico1')
    top = nr.topology(faces)
    vstart, inc = fp.inverted_index(torch.from_numpy(top['keys']), torch.from_numpy(faces), verts.shape[1])
    sl = fr.slots(faces, top)
    want = sorted((int(v), (e * 5 + s) * 2 + int(top['kind'][e])) for e in range(len(sl)) for s, v in enumerate(sl[e]) if v >= 0)
    assert inc.dtype == torch.int32 and vstart.dtype == torch.int32 and inc.tolist() == [c for _, c in want]
    assert vstart.tolist() == [sum(1 for v, _ in want if v < k) for k in range(verts.shape[1] + 1)]
    assert len(want) == 5 * top['n_vertex'] + 4 * top['n_edge'] and vstart[-1] == len(want)
    bad = foldpen_guarded.bad_keys(torch.from_numpy(top['keys']), len(faces))     # a key that names no face, a corner code of 3
    _, inc2 = fp.inverted_index(bad, torch.from_numpy(faces), verts.shape[1])
    assert sorted(set(inc.tolist()) - set(inc2.tolist())) == sorted(c for _, c in want if c // 10 in (7, 11))
    few = fp.inverted_index(torch.from_numpy(top['keys']), torch.from_numpy(faces), 40)                # faces that name vertex 40, 41
    outside = {e for e in range(len(sl)) if (faces[top['i'][e]] >= 40).any() or (faces[top['j'][e]] >= 40).any()}
    assert {c // 10 for c in inc.tolist()} - {c // 10 for c in few[1].tolist()} == outside and few[0].numel() == 41


# ---- the optimiser's flags ------------------------------------------------------------------------------------------------------------
def test_optimize_flags_parse_and_default_to_off():
    import optimize
    d = optimize.parse_flags([])
    assert (d.fold_wt, d.pierce_wt, d.fold_deg) == (0.0, 0.0, 30.0)
    o = optimize.parse_flags('--fold_wt 0.1 --pierce_wt 0.1 --fold_deg 25'.split())
    assert (o.fold_wt, o.pierce_wt, o.fold_deg) == (0.1, 0.1, 25.0)
    src = open(os.path.join(ROOT, 'optimize.py')).read()
    assert 'derived from nothing measured on a real reconstruction' in ' '.join(src.replace('#', ' ').split())
    import extract
    assert extract.parse_flags(['--fold_wt', '0.1']).fold_wt == 0.1              # extract.py is handed the last stage's flags
    from lasr_amd.nnutils import mesh_net, train_utils
    msrc = open(mesh_net.__file__).read()
    assert 'self.fold_loss = None' in msrc and "aux['fold_loss']" in msrc
    tsrc = open(train_utils.__file__).read()
    assert 'import fold_penalty' in tsrc and "call('lasr_foldpen" not in tsrc and "call('lasr_foldpen" not in msrc


@pytest.mark.parametrize('flag, value', [('fold_wt', -0.1), ('pierce_wt', float('nan')), ('fold_wt', float('inf')), ('fold_deg', 0.),
                                         ('fold_deg', 91.)])
def test_trainer_refuses_bad_weights_and_angles(flag, value):
    import torch
    from types import SimpleNamespace
    from lasr_amd.nnutils import train_utils
    tr = train_utils.LASRTrainer.__new__(train_utils.LASRTrainer)
    tr.opts = SimpleNamespace(**{'fold_wt': 0., 'pierce_wt': 0., 'fold_deg': 30., 'ptex_method': 'alexnet', 'alexnet_weights': '',
                                 'perceptual': False, flag: value})
    tr.device, tr.rank = torch.device('cpu'), 0
    v, f = nr.fixture('ico1')
    tr.model = SimpleNamespace(get_mean_shape=lambda n: (torch.from_numpy(v), None, torch.from_numpy(f).long()[None]))
    with pytest.raises(ValueError, match='--' + flag):
        tr.define_criterion_ddp()
    tr.opts = SimpleNamespace(**dict(vars(tr.opts), **{flag: 30. if flag == 'fold_deg' else 0.}))
    tr.define_criterion_ddp()                                                      # weights of 0: no criterion, nothing loaded
    assert tr.model.fold_loss is None
    tr.opts.pierce_wt = 0.5                                                        # asked for on a CPU model: refused, no fall-back
    with pytest.raises(TypeError, match='support only cuda'):
        tr.define_criterion_ddp()


def test_reconstruct_hands_the_weights_to_every_stage_and_names_the_caveat(tmp_path):
    from lasr_amd import pipeline as pl
    from test_reconstruct_cpu import by_name, load, make_args, write_images
    plain = pl.plan(make_args(tmp_path))
    zero = pl.plan(make_args(tmp_path, '--fold_wt', '0', '--pierce_wt', '0.0'))
    assert plain == zero and not any('fold' in t or 'pierce' in t for s in plain if s.argv for t in s.argv)
    assert pl.shell_lines(plain, make_args(tmp_path)) == pl.shell_lines(zero, make_args(tmp_path, '--fold_wt', '0'))
    args = make_args(tmp_path, '--fold_wt', '0.1', '--pierce_wt', '0.2', '--schedule', 'template')
    steps = pl.plan(args)
    stages = [s for s in steps if s.name.startswith('stage-')]
    opt = load('optimize.py')
    assert len(stages) > 1
    for s in stages + [by_name(steps)['extract']]:
        argv = list(s.argv)
        assert argv[argv.index('--fold_wt') + 1] == '0.1' and argv[argv.index('--pierce_wt') + 1] == '0.2'
    for s in stages:                                                              # through the script's own parser
        o = opt.parse_flags([t for t in s.argv[2:]])
        assert (o.fold_wt, o.pierce_wt, o.fold_deg) == (0.1, 0.2, 30.)
    base = pl.plan(make_args(tmp_path, '--schedule', 'template'))
    strip = lambda argv: [t for k, t in enumerate(argv) if t not in ('--fold_wt', '--pierce_wt') and argv[k - 1] not in ('--fold_wt', '--pierce_wt')]   # noqa: E731
    assert [strip(list(s.argv)) if s.argv else None for s in steps] == [list(s.argv) if s.argv else None for s in base]
    assert [s.timeout_s for s in steps] == [s.timeout_s for s in base]
    one = pl.plan(make_args(tmp_path, '--pierce_wt', '0.5'))                      # only the weight that was asked for is named
    assert all('--pierce_wt' in s.argv and '--fold_wt' not in s.argv for s in one if s.name.startswith('stage-'))
    pieces, with_flag = pl.describe(make_args(tmp_path))['pieces'], pl.describe(args)['pieces']
    assert 'fold_penalty' not in pieces and [p for p in with_flag if p != 'fold_penalty'] == pl.describe(make_args(tmp_path, '--schedule', 'template'))['pieces']
    assert 'fold_penalty' in with_flag
    text = pl.CAVEATS['fold_penalty']
    assert 'unmeasured' in text and 'nothing measured on a real reconstruction' in text and 'unverified' in text
    again = pl.driver_argv(args)
    assert again[again.index('--fold_wt'):][:4] == ['--fold_wt', '0.1', '--pierce_wt', '0.2']
    assert '--fold_wt' not in pl.driver_argv(make_args(tmp_path)) and '--fold_wt' in load('scripts', 'reconstruct.py').__doc__
    for bad in (['--fold_wt', '-1'], ['--pierce_wt', 'nan']):
        with pytest.raises(SystemExit):
            make_args(tmp_path, *bad)
    # the command itself
    write_images(tmp_path / 'in', ['0.png', '1.png', '2.png'])
    common = ['--frames', str(tmp_path / 'in'), '--seqname', 'cat', '--workdir', str(tmp_path / 'work'), '--dry_run']
    out0, out1 = io.StringIO(), io.StringIO()
    assert pl.main(common, out=out0) == 0 and pl.main(common + ['--fold_wt', '0.1', '--pierce_wt', '0.1'], out=out1) == 0
    lines0, lines1 = out0.getvalue().splitlines(), out1.getvalue().splitlines()
    assert 'fold_wt' not in out0.getvalue() and len(lines0) == len(lines1)
    for a, b in zip(lines0, lines1):
        if 'optimize.py' in a or 'extract.py' in a:
            assert '--fold_wt 0.1 --pierce_wt 0.1' in b and b.replace(' --fold_wt 0.1 --pierce_wt 0.1', '') == a
        elif 'scripts/reconstruct.py' in a:
            assert b.replace(' --fold_wt 0.1 --pierce_wt 0.1', '') == a
        else:
            assert a == b


def test_the_demo_takes_the_weights():
    src = open(os.path.join(ROOT, 'scripts', 'reconstruct_demo.py')).read()
    assert "'--fold_wt'" in src and "'--pierce_wt'" in src and "common += ['--fold_wt'" in src


# ---- the native scan ----------------------------------------------------------------------------------------------------------------
def test_every_native_fold_penalty_launches_is_in_the_guarded_case():
    with open(os.path.join(ROOT, 'scripts', 'fold_penalty.py')) as fh:
        names, opaque = launched_in(fh.read())
    assert not opaque and sorted(set(names)) == sorted(foldpen_guarded.LAUNCHED) == sorted(n for n in ENTRY_POINTS if 'bytes' not in n)
    assert set(names) <= set(foldpen_guarded.NATIVES) == set(foldpen_guarded.CASE.natives)
    # the module reaches the topology pass through scripts/shape_neighbours.py, which tests/meshnbr_guarded.py covers as well
    assert set(foldpen_guarded.NATIVES) - set(names) == {'lasr_meshnbr_list'}
