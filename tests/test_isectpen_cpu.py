"""The intersection penalty of the optimiser without a device: closed forms of the restatement (tests/isectpen_restated.py), its
charged pairs against meshcheck_restated, its closed-form gradient against float64 autograd, the conditions the GPU comparisons of
tests/test_isectpen_gpu.py rest on, the fixed-point rules, a descent on the restatement alone, header against binding, the C ABI's
host-side checks, the Python layer's refusals, the flags of optimize.py, extract.py, scripts/reconstruct.py and
scripts/reconstruct_demo.py, and the launch site of scripts/isect_penalty.py against the guarded case (tests/isectpen_guarded.py).

Measured with this file.  On all seven fixtures the float32 and float64 restatements agree on which tests hold and which end is the
shallower, every intersecting pair has exactly two tests that hold, and nothing is dropped; the float32 sums differ from float64 by
3.3e-8 (copies_base) to 1.8e-7 (pinch2).  The closed-form gradient is off float64 autograd by at most 5.3e-15 (pinch2, largest
entry 15.9).  Descent (DESCENT below: plain, the gradient of the float64 or float32 restatement, vertices kept in float32, cap 200):
pinch2 (10 pairs) is clear after 6 steps at rate 0.003 (12, 12, 8, 8, 8, 0) and after 2 at rate 0.01 (6, 0); frame 2 of batch3
(4 pairs) after 4 steps at 0.003 (4, 1, 7, 0), in both precisions.  The overlapping frames of two2 are no part of the test (200 steps
take a minute): from 83 / 94 pairs they stand at 110 / 132 after 200 steps at rate 0.003 and at 105 / 117 at rate 0.01 (float64): the
term does not separate two bodies that overlap wholesale."""
import ctypes
import functools
import io
import os
import re

import numpy as np
import pytest

import isectpen_guarded
import isectpen_restated as ir
import meshcheck_restated as mr
import meshnbr_restated as nr
from test_guarded_alloc_cpu import launched_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = (np.float64, np.float32)
ENTRY_POINTS = ('lasr_isectpen_scratch_bytes', 'lasr_isectpen_forward')
FIXTURES = ('pinch2', 'two2', 'tile256', 'tile257', 'ico2', 'copies_base', 'batch3')
# fixture, rate -> the step after which every n_pairs is 0, and n_pairs of the charged mesh after every step
DESCENT = {('pinch2', 0.003): (6, [12, 12, 8, 8, 8, 0]), ('pinch2', 0.01): (2, [6, 0]), ('batch3', 0.003): (4, [4, 1, 7, 0])}
STEPS = 200


def fixture(name):
    if name == 'copies_base':
        return mr.copies_base()
    return nr.fixture(name) if name == 'batch3' else mr.fixture(name)


@functools.lru_cache(None)
def restated(name, dt=np.float64, variant=False):
    """The restatement of a fixture, computed once and shared."""
    return ir.penalty(*fixture(name), dt, variant)


def _one(verts, faces, dt=np.float64):
    return ir.penalty(np.asarray(verts, np.float32)[None], np.asarray(faces, np.int32), dt)


# ---- closed forms -------------------------------------------------------------------------------------------------------------------
BASE = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
# a triangle in the plane x = y whose edge 3-4 passes through the base at (1, 1, 0), its end 3 half a unit below; the base's edge 1-2
# passes through it at (2, 2, 0), both its ends 4 / sqrt(2) from that plane: a tie
THROUGH = [(1, 1, -0.5), (1, 1, 2), (5, 5, 1)]
FACES = [(0, 1, 2), (3, 4, 5)]


@pytest.mark.parametrize('dt', BOTH)
def test_two_triangles_through_each_other_at_known_depths(dt):
    r = _one(BASE + THROUGH, FACES, dt)
    f = r['frames'][0]
    assert f['pairs'].tolist() == [[0, 1]] and f['holds'].tolist() == [[False, True, False, True, False, False]]
    assert f['at_q'][0, 1] == False and f['at_q'][0, 3] == False                  # noqa: E712  the tie goes to p; end 3 is the shallower
    assert f['delta'][0, 3] == 0.5 and abs(float(f['delta'][0, 1]) - np.sqrt(8.)) < 1e-6
    assert r['n_pairs'].tolist() == [1] and r['n_dropped'].tolist() == [0]
    assert abs(float(r['loss'][0]) - (0.5 + np.sqrt(8.))) < 1e-6 and r['loss'].dtype == np.float32 and r['gunit'].dtype == np.float32
    g = r['grad'][0]
    assert np.abs(g.sum(0)).max() < 1e-6                                           # no net force
    # end 3 moves on, down, as the end of its edge; as corner a of the triangle the base's edge passes through it gets the foot's share
    unit = np.array([1., -1., 0.]) / np.sqrt(2.)                                   # sign(orient) n / |n| at vertex 1, below the plane x = y
    lam = r['grad'][0][3] - np.array([0., 0., -1.])
    assert np.allclose(g[1] - np.array([0., 0., 0.25]), unit, atol=1e-6)           # vertex 1: its own end, and corner b of the base (0.25)
    assert np.allclose(g[2], (0., 0., 0.25), atol=1e-6) and np.allclose(g[0], (0., 0., 0.5), atol=1e-6)
    assert np.allclose(lam + g[4] + g[5], -unit, atol=1e-6)                        # the three corners share minus the unit normal
    _, auto = ir.autograd(np.array(BASE + THROUGH, np.float32)[None], np.array(FACES))
    assert np.abs(auto - _one(BASE + THROUGH, FACES)['grad']).max() < 1e-12
    flipped = _one(BASE + THROUGH, [FACES[1], FACES[0]], dt)                       # the order of the rows is nothing the sums see
    assert (flipped['acc_loss'] == r['acc_loss']).all() and (flipped['acc_grad'] == r['acc_grad']).all()
    assert flipped['frames'][0]['holds'].tolist() == [[True, False, False, False, True, False]]
    one_step = np.array(BASE + THROUGH, np.float64) - 0.6 * r['grad'][0]           # linear in the depth: a step of 0.6 carries end 3 across
    assert _one(one_step, FACES, dt)['n_pairs'].tolist() == [0] and _one(one_step, FACES, dt)['loss'].tolist() == [0.]


@pytest.mark.parametrize('dt', BOTH)
def test_touching_coplanar_neighbouring_degenerate_and_distant_pairs_give_exact_zeros(dt):
    cases = {
        'touching': (BASE + [(1, 1, 0), (1, 1, 2), (5, 5, 1)], FACES),             # end 3 lies in the base's plane
        'coplanar': (BASE + [(1, 1, 0), (3, 1, 0), (1, 3, 0)], FACES),             # overlap inside the plane
        'shared': (BASE + THROUGH, [(0, 1, 2), (0, 3, 4)]),                        # a shared vertex index: never a candidate
        'repeated': (BASE + THROUGH, [(0, 1, 2), (3, 4, 4)]),                      # a repeated index: part of nothing
        'outside': (BASE + THROUGH, [(0, 1, 2), (3, 4, 6)]),                       # an index outside [0, V): part of nothing
        'distant': (BASE + [(11, 1, -0.5), (11, 1, 2), (15, 5, 1)], FACES),        # the boxes do not overlap
    }
    for name, (verts, faces) in cases.items():
        r = _one(verts, faces, dt)
        assert not r['loss'].any() and not r['gunit'].any() and not r['acc_grad'].any() and not r['grad'].any(), name
        assert r['n_pairs'].tolist() == [0] and r['n_dropped'].tolist() == [0], name
        if name in ('shared', 'repeated', 'outside', 'distant'):
            assert len(r['frames'][0]['pairs']) == 0, name
    assert _one(BASE + THROUGH, [(0, 1, 2), (3, 4, 5), (3, 4, 4), (0, 7, 9)], dt)['acc_loss'] == _one(BASE + THROUGH, FACES, dt)['acc_loss']
    assert not _one(np.zeros((6, 3)), FACES, dt)['loss'].any()                     # every face a point: nothing holds, nothing is NaN


# ---- the restatement against meshcheck_restated and against itself -------------------------------------------------------------------
@pytest.mark.parametrize('name', FIXTURES)
def test_charged_pairs_are_the_intersecting_pairs_of_the_shape_report(name):
    verts, faces = fixture(name)
    want = mr.self_intersections(verts, faces)
    for dt in BOTH:
        r = restated(name, dt)
        for t, f in enumerate(r['frames']):
            assert np.array_equal(f['pairs'][f['hit']], want[t]['pairs']) and r['n_pairs'][t] == want[t]['n_pairs']
            assert (f['holds'].sum(1)[f['hit']] == 2).all()                        # observed on every fixture, assumed nowhere
            assert (f['charged'] == f['holds']).all()
        assert not r['n_dropped'].any() and ((r['loss'] > 0) == (r['n_pairs'] > 0)).all()
    print('%s: n_pairs %s, loss %s' % (name, restated(name)['n_pairs'].tolist(), restated(name)['loss'].tolist()))
    if name == 'ico2':
        assert not restated(name)['loss'].any() and not restated(name)['gunit'].any()
    if name == 'two2':
        assert restated(name)['n_pairs'].tolist() == [0, 83, 94] and not restated(name)['gunit'][0].any()
    if name == 'pinch2':
        assert restated(name)['n_pairs'].tolist() == [10]


@pytest.mark.parametrize('name', [n for n in FIXTURES if n != 'ico2'])
def test_closed_form_gradient_equals_float64_autograd(name):
    verts, faces = fixture(name)
    r = restated(name)
    value, grad = ir.autograd(verts, faces)
    err = np.abs(r['grad'] - grad).max()
    print('%s: largest gradient entry %.3f, closed form off autograd by %.1e' % (name, np.abs(grad).max(), err))
    assert err < 1e-12 and np.abs(r['value'] - value).max() < 1e-12 and np.abs(grad).max() > 1
    # the fixed point: every one of the contributions of a vertex is off by at most 2^-41, and so is the loss per test
    n_tests = np.array([f['charged'].sum() for f in r['frames']])
    assert (np.abs(r['acc_loss'] / ir.Q - r['value']) <= n_tests * 2. ** -41).all()
    assert np.abs(r['acc_grad'] / ir.Q - r['grad']).max() <= 4 * n_tests.max() * 2. ** -41


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_meets_the_conditions_of_the_gpu_comparisons(name):
    cond = ir.conditions(*fixture(name))
    for t, c in enumerate(cond):
        print('%s frame %d: %d pairs, float32 sum off float64 by %.2e' % (name, t, c['n_pairs'], c['diff']))
        assert c['same'] and c['two']
    a, b, c = restated(name), restated(name, np.float32), restated(name, np.float32, True)
    assert (a['n_pairs'] == b['n_pairs']).all() and (b['n_pairs'] == c['n_pairs']).all()
    if a['n_pairs'].any():                                                         # the two float32 orders differ: the floor is no zero
        assert np.abs(b['gunit'].astype(np.float64) - c['gunit']).max() > 0 and np.abs(b['gunit'].astype(np.float64) - a['gunit']).max() < 4e-6


def test_copies_fixture_gives_eight_times_the_base():
    v0, f0 = mr.copies_base()
    verts, faces, exp = mr.copies_case(8)
    base = restated('copies_base', np.float32)
    sub = slice(2 * 640, 3 * 640)                                                  # one copy, as a mesh of its own on all the vertices
    part = ir.penalty(verts, faces[sub], np.float32)
    assert part['acc_loss'] == base['acc_loss'] and (part['acc_grad'][0, 2 * 324:3 * 324] == base['acc_grad'][0]).all()
    assert not part['acc_grad'][0, :2 * 324].any() and exp['n_pairs'] == 8 * base['n_pairs'][0] == 8 * 83


# ---- the fixed point ----------------------------------------------------------------------------------------------------------------
def test_fixed_point_rounds_half_to_even_and_drops_what_is_too_large():
    q = ir.quantise(np.array([2. ** -41, 3 * 2. ** -41, -3 * 2. ** -41, 0.5, 2. ** -40, 2. ** 20 - 2. ** -20], np.float64))
    assert q.tolist() == [0, 2, -2, 2 ** 39, 1, 2 ** 60 - 2 ** 20]
    assert ir.unquantise(np.array([2 ** 39, -3, 2 ** 62])).tolist() == [0.5, float(np.float32(-3 * 2. ** -40)), 4194304.0]
    assert ir.Q == 2. ** 40 and ir.LIMIT == 2. ** 20
    pts = np.array(BASE + THROUGH, np.float64)
    for dt in BOTH:
        ok = _one(pts * 2. ** 18, FACES, dt)                                       # depths 2^17 and sqrt(8) 2^18 < 2^20: charged
        assert ok['n_dropped'].tolist() == [0] and abs(float(ok['loss'][0]) - (0.5 + np.sqrt(8.)) * 2. ** 18) < 1
        assert np.abs(ok['gunit'] - _one(pts, FACES, dt)['gunit']).max() < 1e-6   # the gradient does not scale
        part = _one(pts * 2. ** 19, FACES, dt)                                     # sqrt(8) 2^19 >= 2^20: that test alone is dropped
        assert part['n_dropped'].tolist() == [1] and part['n_pairs'].tolist() == [1] and part['loss'].tolist() == [2. ** 18]
        assert part['gunit'][0, 3].tolist() == [0., 0., -1.] and part['gunit'][0, :3, 2].tolist() == [0.5, 0.25, 0.25]
        assert not part['gunit'][0, 4:].any() and not part['gunit'][0, :3, :2].any()   # nothing of the dropped test arrives anywhere
        for scale in (2. ** 21, 1e10):                                             # both depths >= 2^20; |n|^2 overflows float32 at 1e10
            big = _one(pts * scale, FACES, dt)
            assert big['n_dropped'].tolist() == [2] and big['n_pairs'].tolist() == [1]
            assert not big['loss'].any() and not big['gunit'].any() and not big['acc_grad'].any()
            assert big['frames'][0]['holds'].sum() == 2 and not big['frames'][0]['charged'].any()


# ---- descent ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, rate', sorted(DESCENT))
def test_descent_on_the_restatement_clears_shallow_pass_throughs(name, rate):
    verts, faces = fixture(name)
    mesh = int(np.argmax(restated(name)['n_pairs']))
    before = nr.evaluate(verts, faces, 20.)
    for dt in BOTH:
        step, x, history = ir.descend(verts, faces, rate, STEPS, dt)
        print('%s at rate %g in %s: clear after %s steps, n_pairs %s' % (name, rate, np.dtype(dt).name, step, [int(h[mesh]) for h in history]))
        assert (step, [int(h[mesh]) for h in history]) == DESCENT[(name, rate)]
        after = nr.evaluate(x, faces, 20.)
        if name == 'pinch2':
            assert not after['n_creased'].any() and not after['n_pierced'].any()
        else:                                                                      # batch3: no worse than at the start, clean frames unmoved
            assert (after['n_creased'] <= before['n_creased']).all() and (after['n_pierced'] <= before['n_pierced']).all()
            assert (x[:2] == verts[:2]).all()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_entry_points():
    from lasr_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    bare = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    scalar = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float}
    want = {'lasr_isectpen_scratch_bytes': ('size_t', 'N V'),
            'lasr_isectpen_forward': ('int', 'x faces scratch scratch_bytes loss gunit n_pairs n_dropped N V F hip_stream')}
    for name in ENTRY_POINTS:
        ret, names = want[name]
        args = [' '.join(a.split()) for a in re.search(r'\b%s %s\s*\((.*?)\);' % (ret, name), bare, re.S).group(1).split(',')]
        assert [a.replace('*', ' ').split()[-1] for a in args] == names.split()
        res, sig = _lib.SIGNATURES[name]
        assert res is scalar[ret] and sig == [ctypes.c_void_p if '*' in a else scalar[a.split()[0]] for a in args]
    assert sorted(n for n in _lib.SIGNATURES if n.startswith('lasr_isectpen_')) == sorted(ENTRY_POINTS)
    assert _lib.ABI_VERSION == 13                                                 # new symbols only
    flat = ' '.join(hdr.replace(' * ', ' ').split())
    for word in ('FIXED POINT with Q = 2^40', 'llrint((double)c Q)', 'derived from nothing measured', 'unverified', 'is not checked',
                 'There is no backward entry point', 'same bits on every run and under any permutation'):
        assert word in flat, word


def test_symbols_are_exported_and_the_host_checks_run_without_a_device():
    from lasr_amd import _lib
    h = _lib.lib()
    n, big = None, 1 << 40
    names = ('x', 'fa', 'sc', 'lo', 'gu', 'np', 'nd')
    addr = dict(zip(names, (64, 128, 192, 256, 320, 384, 448)))                    # non-NULL addresses, never followed

    def fwd(N=1, V=3, F=1, nb=big, **kw):
        p = dict(addr, **kw)
        return h.lasr_isectpen_forward(p['x'], p['fa'], p['sc'], nb, p['lo'], p['gu'], p['np'], p['nd'], N, V, F, n)
    none = {k: n for k in names}
    assert h.lasr_isectpen_scratch_bytes(3, 162) == 8 * (3 + 3 * 162 * 3) and h.lasr_isectpen_scratch_bytes(1, 0) == 8
    assert h.lasr_isectpen_scratch_bytes(-1, 5) == 0 and h.lasr_isectpen_scratch_bytes(1, -1) == 0 and h.lasr_isectpen_scratch_bytes(0, 7) == 0
    assert h.lasr_isectpen_scratch_bytes(65536, 1) == 0 and h.lasr_isectpen_scratch_bytes(4, (1 << 31) // 12 + 1) == 0
    assert fwd(N=0) == 0 and fwd(F=0) == 0 and fwd(N=0, **none) == 0 and fwd(F=0, **none) == 0                  # nothing launched
    assert fwd(N=-1) == -1 and fwd(V=-1) == -1 and fwd(F=-1) == -1 and fwd(N=65536) == -1 and fwd(F=(1 << 20) + 1) == -1
    assert fwd(N=4096, F=1 << 20) == -1 and fwd(N=4, V=(1 << 31) // 12 + 1) == -1 and fwd(V=0) == -1 and fwd(N=-1, F=0) == -1
    for k in names:
        assert fwd(nb=7, **{k: n}) == (-3 if k == 'gu' else -1), k                # gunit may be NULL: no gradient wanted
    for a, b in (('lo', 'x'), ('gu', 'lo'), ('sc', 'lo'), ('np', 'nd'), ('fa', 'x'), ('gu', 'x'), ('nd', 'sc')):
        assert fwd(**{a: addr[b]}) == -1, (a, b)
    assert fwd(nb=8 * 10 - 1) == -3 and fwd(N=3, V=162, nb=8 * (3 + 3 * 162 * 3) - 1) == -3 and fwd(nb=0) == -3   # LASR_E_WORKSPACE
    table = [h.lasr_prof_kernel_name(i) for i in range(h.lasr_prof_kernel_count())]
    assert not any(b'isectpen' in s for s in table)                               # the kernel table is not extended


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    import torch
    ip = isectpen_guarded.isect_penalty()
    f = torch.tensor([[0, 1, 2], [3, 4, 5]])
    with pytest.raises(TypeError, match='support only cuda'):
        ip.IsectPenalty(f)
    with pytest.raises(TypeError, match='must be a tensor'):
        ip.IsectPenalty(f.numpy())
    assert 'derived from nothing measured' in ' '.join(ip.__doc__.split()) and 'unverified' in ip.__doc__
    assert 'does not separate two bodies that overlap wholesale' in ' '.join(ip.__doc__.split())
    pen = ip.IsectPenalty.__new__(ip.IsectPenalty)                                # the checks of a call, without a device
    pen.faces, pen.n_verts = f.int(), None
    with pytest.raises(TypeError, match='must be a tensor'):
        pen(np.zeros((1, 6, 3), np.float32))
    with pytest.raises(TypeError, match='support only cuda'):
        pen(torch.zeros(1, 6, 3))
    with pytest.raises(TypeError, match='support only cuda'):
        pen.counts(torch.zeros(1, 6, 3))


# ---- the optimiser's flags ------------------------------------------------------------------------------------------------------------
def test_optimize_and_extract_flags_parse_and_default_to_off():
    import optimize
    assert optimize.parse_flags([]).isect_wt == 0.0 and optimize.parse_flags('--isect_wt 0.1'.split()).isect_wt == 0.1
    src = ' '.join(open(os.path.join(ROOT, 'optimize.py')).read().replace('#', ' ').split())
    assert 'derived from nothing measured' in src and 'does not separate two bodies that overlap wholesale' in src
    import extract
    assert extract.parse_flags(['--isect_wt', '0.1']).isect_wt == 0.1            # extract.py is handed the last stage's flags
    from lasr_amd.nnutils import mesh_net, train_utils
    msrc = open(mesh_net.__file__).read()
    assert 'self.isect_loss = None' in msrc and "aux['isect_loss']" in msrc and 'MEANS_MAX_TERMS' in msrc
    tsrc = open(train_utils.__file__).read()
    assert 'import isect_penalty' in tsrc and "call('lasr_isectpen" not in tsrc and "call('lasr_isectpen" not in msrc


@pytest.mark.parametrize('value', [-0.1, float('nan'), float('inf')])
def test_trainer_refuses_bad_weights(value):
    import torch
    from types import SimpleNamespace
    from lasr_amd.nnutils import train_utils
    tr = train_utils.LASRTrainer.__new__(train_utils.LASRTrainer)
    tr.opts = SimpleNamespace(fold_wt=0., pierce_wt=0., fold_deg=30., isect_wt=value, ptex_method='alexnet', alexnet_weights='', perceptual=False)
    tr.device, tr.rank = torch.device('cpu'), 0
    v, f = nr.fixture('ico1')
    tr.model = SimpleNamespace(get_mean_shape=lambda n: (torch.from_numpy(v), None, torch.from_numpy(f).long()[None]))
    with pytest.raises(ValueError, match='--isect_wt'):
        tr.define_criterion_ddp()
    tr.opts.isect_wt = 0.
    tr.define_criterion_ddp()                                                      # a weight of 0: no criterion, nothing loaded
    assert tr.model.isect_loss is None and tr.model.fold_loss is None
    tr.opts.isect_wt = 0.5                                                         # asked for on a CPU model: refused, no fall-back
    with pytest.raises(TypeError, match='support only cuda'):
        tr.define_criterion_ddp()


def test_reconstruct_hands_the_weight_to_every_stage_and_names_the_caveat(tmp_path):
    from lasr_amd import pipeline as pl
    from test_reconstruct_cpu import by_name, load, make_args, write_images
    plain = pl.plan(make_args(tmp_path))
    zero = pl.plan(make_args(tmp_path, '--isect_wt', '0'))
    assert plain == zero and not any('isect' in t for s in plain if s.argv for t in s.argv)
    assert pl.shell_lines(plain, make_args(tmp_path)) == pl.shell_lines(zero, make_args(tmp_path, '--isect_wt', '0.0'))
    args = make_args(tmp_path, '--isect_wt', '0.1', '--schedule', 'template')
    steps = pl.plan(args)
    stages = [s for s in steps if s.name.startswith('stage-')]
    opt = load('optimize.py')
    assert len(stages) > 1
    for s in stages + [by_name(steps)['extract']]:
        argv = list(s.argv)
        assert argv[argv.index('--isect_wt') + 1] == '0.1' and '--fold_wt' not in argv
    for s in stages:                                                              # through the script's own parser
        o = opt.parse_flags([t for t in s.argv[2:]])
        assert (o.isect_wt, o.fold_wt, o.pierce_wt) == (0.1, 0., 0.)
    base = pl.plan(make_args(tmp_path, '--schedule', 'template'))
    strip = lambda argv: [t for k, t in enumerate(argv) if t != '--isect_wt' and argv[k - 1] != '--isect_wt']   # noqa: E731
    assert [strip(list(s.argv)) if s.argv else None for s in steps] == [list(s.argv) if s.argv else None for s in base]
    assert [s.timeout_s for s in steps] == [s.timeout_s for s in base]
    pieces, with_flag = pl.describe(make_args(tmp_path))['pieces'], pl.describe(args)['pieces']
    assert 'isect_penalty' not in pieces and [p for p in with_flag if p != 'isect_penalty'] == pl.describe(make_args(tmp_path, '--schedule', 'template'))['pieces']
    assert 'isect_penalty' in with_flag and 'fold_penalty' not in with_flag
    both = pl.describe(make_args(tmp_path, '--isect_wt', '0.1', '--fold_wt', '0.1'))['pieces']
    assert both.index('isect_penalty') == both.index('fold_penalty') + 1
    text = pl.CAVEATS['isect_penalty']
    assert 'unmeasured' in text and 'derived from nothing measured' in text and 'unverified' in text and 'overlap wholesale' in text
    again = pl.driver_argv(args)
    assert again[again.index('--isect_wt'):][:2] == ['--isect_wt', '0.1']
    assert '--isect_wt' not in pl.driver_argv(make_args(tmp_path)) and '--isect_wt' in load('scripts', 'reconstruct.py').__doc__
    for bad in (['--isect_wt', '-1'], ['--isect_wt', 'nan']):
        with pytest.raises(SystemExit):
            make_args(tmp_path, *bad)
    # the command itself: without the flag every line keeps its bytes
    write_images(tmp_path / 'in', ['0.png', '1.png', '2.png'])
    common = ['--frames', str(tmp_path / 'in'), '--seqname', 'cat', '--workdir', str(tmp_path / 'work'), '--dry_run']
    out0, out1, out2 = io.StringIO(), io.StringIO(), io.StringIO()
    assert pl.main(common, out=out0) == 0 and pl.main(common + ['--isect_wt', '0.1'], out=out1) == 0
    assert pl.main(common + ['--isect_wt', '0'], out=out2) == 0 and out2.getvalue() == out0.getvalue()
    lines0, lines1 = out0.getvalue().splitlines(), out1.getvalue().splitlines()
    assert 'isect_wt' not in out0.getvalue() and len(lines0) == len(lines1)
    for a, b in zip(lines0, lines1):
        if 'optimize.py' in a or 'extract.py' in a or 'scripts/reconstruct.py' in a:
            assert ' --isect_wt 0.1' in b and b.replace(' --isect_wt 0.1', '') == a
        else:
            assert a == b


def test_the_demo_takes_the_weight():
    src = open(os.path.join(ROOT, 'scripts', 'reconstruct_demo.py')).read()
    assert "'--isect_wt'" in src and "common += ['--isect_wt'" in src and "'n_pairs'" in src
    bench = open(os.path.join(ROOT, 'tools', 'isectpen_bench.py')).read()
    assert 'meshcheck._records' in bench and 'meshcheck._pairs' in bench and 'no test asserts a time' in bench


# ---- the native scan ----------------------------------------------------------------------------------------------------------------
def test_the_native_isect_penalty_launches_is_in_the_guarded_case():
    with open(os.path.join(ROOT, 'scripts', 'isect_penalty.py')) as fh:
        names, opaque = launched_in(fh.read())
    assert not opaque and sorted(set(names)) == sorted(isectpen_guarded.NATIVES) == sorted(n for n in ENTRY_POINTS if 'bytes' not in n)
    assert set(isectpen_guarded.NATIVES) == set(isectpen_guarded.CASE.natives)
