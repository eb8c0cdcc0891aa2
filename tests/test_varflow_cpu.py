"""Variational optical flow without a device: the restatement (tests/varflow_restated.py) on closed forms and on the seeded
fixtures, the C ABI's host-side checks, the two scripts' argument handling, and the share of pixels the GPU comparison
(tests/test_varflow_gpu.py) leaves out.

Bounds.  The GPU tests compare a kernel with the float64 restatement under bound(f32, f64) = max(4 x max |float32 restatement -
float64 restatement|, one float32 ulp of the largest magnitude), computed from the restatement alone on the inputs of the
comparison.  For the whole pipeline at the default parameters the restatement measures (float64 EPE over the scored region, zero-flow
EPE, max |float32 - float64|): trans 0.0030 px / 3.71 / 8.0e-6; big 0.0025 / 9.63 / 1.7e-5; affine 0.0452 / 2.22 / 9.2e-6; ellipse
(eroded object) 0.0214 / 5.94 / 1.9e-5; odd 0.0034 / 2.73 / 5.9e-6; seam 0.0060 / 2.72 / 4.7e-6; tiny 0.498 / 0.72 / 1.1e-6 (9 x 7
pixels on one level: a plumbing case, not a motion case).  The largest pipeline bound is 4 x 1.9e-5 = 7.5e-5 px, below the 1e-3 px
at which a fixture counts as ill-conditioned.
"""
import os
import re
import sys

import numpy as np
import pytest

import varflow_restated as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'preprocess'))

ILL_CONDITIONED = 1e-3              # px: a pipeline bound above this disqualifies the fixture
LEFT_OUT_CAP = 0.01                 # share of a fixture's pixels the GPU comparison may leave out


def bound(r32, r64):
    """4 x the float32 / float64 spread of the restatement, at least one float32 ulp of the largest magnitude."""
    r64 = np.asarray(r64, np.float64)
    return max(4 * float(np.abs(np.asarray(r32, np.float64) - r64).max()), float(np.spacing(np.float32(np.abs(r64).max()))))


def pipeline_bound(name):
    return bound(vr.restated(name, 'float32')[0], vr.restated(name)[0])


def left_out(name):
    """bool [H,W]: the pixels the whole-pipeline GPU comparison of fixture `name` leaves out."""
    p = vr.fixture(name)
    return vr.near_edge(vr.restated(name)[1], (p.H, p.W), pipeline_bound(name))


# ---- closed forms -----------------------------------------------------------------------------------------------------------------

def test_levels():
    assert vr.level_shapes(64, 80) == [(64, 80), (32, 40), (16, 20)]
    assert vr.level_shapes(37, 53) == [(37, 53), (19, 27)]
    assert vr.level_shapes(9, 7) == [(9, 7)] and vr.level_shapes(31, 500) == [(31, 500)]
    assert vr.level_shapes(32, 32) == [(32, 32), (16, 16)]
    assert vr.level_shapes(1080, 1920)[-1] == (17, 30)
    for H, W in ((64, 80), (1080, 1920), (480, 854), (33, 65)):
        assert 16 <= min(vr.level_shapes(H, W)[-1]) <= 31


def test_reduce_of_a_constant_and_of_a_ramp():
    c = vr.reduce(np.full((11, 14), 0.3))
    assert c.shape == (6, 7) and np.abs(c - 0.3).max() <= 1e-15
    ys, xs = np.mgrid[0:21, 0:18].astype(np.float64)
    r = vr.reduce(3 * xs + 2 * ys + 1)
    assert r.shape == (11, 9)
    want = 3 * (2 * np.arange(9))[None] + 2 * (2 * np.arange(11))[:, None] + 1
    assert np.abs(r - want)[1:-1, 1:-1].max() <= 1e-12                            # the symmetric kernel keeps a linear field
    assert np.abs(r - want)[0].max() > 0.1                                        # and the clamped border does not
    img = np.random.default_rng(0).integers(0, 256, (9, 7, 3), dtype=np.uint8)
    assert vr.reduce(vr.to_unit(img)).shape == (5, 4, 3)
    assert vr.reduce(vr.to_unit(img), np.float32).dtype == np.float32 and vr.to_unit(img, np.float32).dtype == np.float32


def test_expand_of_a_constant_flow_doubles_it():
    uv = np.stack([np.full((5, 4), 1.25), np.full((5, 4), -0.5)])
    for h, w in ((10, 8), (9, 7), (10, 7)):
        e = vr.expand(uv, h, w)
        assert e.shape == (2, h, w) and np.abs(e[0] - 2.5).max() <= 1e-15 and np.abs(e[1] + 1.).max() <= 1e-15
    ramp = np.stack([np.arange(4.)[None].repeat(5, 0), np.zeros((5, 4))])
    e = vr.expand(ramp, 10, 8)
    assert np.abs(e[0][3] - np.array([0, 1, 2, 3, 4, 5, 6, 6])).max() <= 1e-15    # 2 * bilinear at x / 2, the last tap clamped


def test_identical_frames_give_exactly_zero_flow_at_every_level():
    for name in ('trans', 'odd', 'tiny'):
        p = vr.fixture(name)
        for dt in (np.float64, np.float32):
            trace = []
            f = vr.flow(p.imgA, p.imgA, dt, trace)
            assert f.dtype == dt and not f.any()
            assert len(trace) == 5 * len(vr.level_shapes(p.H, p.W)) and not any(t['d'].any() or t['uv'].any() for t in trace)


def test_a_ramp_shifted_by_one_pixel_recovers_u_equal_one():
    xs = np.arange(24)
    A = np.repeat((40 + 6 * xs)[None, :, None], 20, 0).repeat(3, 2).astype(np.uint8)
    B = (A.astype(int) - 6).astype(np.uint8)                                      # B(x) = A(x - 1): A(p) = B(p + (1, 0))
    assert len(vr.level_shapes(20, 24)) == 1
    f = vr.flow(A, B)
    # Inside, the linearisation of a ramp is exact and u = 1 solves it.  The first column sees half the gradient (replicated
    # border), the last one leaves the frame and carries no data; both reach the interior only through the smoothness term, and
    # 450 SOR iterations are not convergence.  The bar is a tenth of the feature's accuracy bar of 0.1 px.
    assert np.abs(f[2:-2, 2:-2, 0] - 1).max() < 0.01 and np.abs(f[..., 1]).max() == 0


def test_occlusion_map_closed_forms():
    H, W = 6, 8
    z = np.zeros((H, W, 2))
    occ, e = vr.occlusion(z, z)
    assert occ.dtype == np.float32 and (occ == -2).all() and (e == 0).all()       # e = 0: (0 - 1) / 0.5
    out = z.copy()
    out[2, 3] = (5., 0.)                                                          # 3 + 5 = 8 > W - 1
    out[4, 1] = (-1.5, 0.)
    out[0, 0] = (0., -0.25)
    occ, e = vr.occlusion(out, z)
    assert occ[2, 3] == 6 and occ[4, 1] == 6 and occ[0, 0] == 6 and np.isnan(e[2, 3])
    edge = z.copy()
    edge[2, 3] = (4., 0.)                                                         # exactly W - 1: inside
    assert vr.occlusion(edge, z)[0][2, 3] == 6 and vr.occlusion(edge, z)[1][2, 3] == 4      # e = 4: clamped to +6
    back = z.copy()
    back[..., 0] = 1.                                                             # e = tau exactly: occ = 0 -> the smallest normal
    occ, e = vr.occlusion(z, back)
    assert (e == 1).all() and (occ == vr.TINY).all() and (occ != 0).all() and vr.TINY == np.finfo(np.float32).tiny
    back[..., 0] = 1.25
    assert (vr.occlusion(z, back)[0] == 0.5).all()
    back[..., 0] = 100.
    assert (vr.occlusion(z, back)[0] == 6).all()
    f = np.zeros((H, W, 2))
    f[..., 0] = 2.                                                                # consistent pair: e = 0 wherever the target is inside
    occ, _ = vr.occlusion(f, -f)
    assert (occ[:, :W - 2] == -2).all() and (occ[:, W - 2:] == 6).all()


# ---- accuracy of the restatement ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', vr.MOTION)
def test_restatement_accuracy(name):
    p = vr.fixture(name)
    f, _ = vr.restated(name)
    region = vr.score_region(p)
    got, zero = vr.epe(f, p.truth_ab, region), vr.epe(np.zeros_like(f), p.truth_ab, region)
    print(name, 'EPE %.4f px, zero flow %.3f px, region %d px' % (got, zero, int(region.sum())))
    assert region.sum() > 200
    assert got < 0.1
    assert got * 20 <= zero


def test_the_large_translation_is_about_a_ninth_of_the_width_and_the_ellipse_has_two_layers():
    big, ell = vr.fixture('big'), vr.fixture('ellipse')
    assert abs(big.truth_ab[0, 0, 0] / big.W - 0.11) < 1e-9
    assert ell.maskA.sum() > 400 and (ell.truth_ab[ell.maskA] == (5.5, -2.25)).all() and (ell.truth_ab[~ell.maskA] == (0.75, -0.5)).all()
    assert (ell.truth_ba[ell.maskB] == (-5.5, 2.25)).all() and (ell.truth_ba[~ell.maskB] == (-0.75, 0.5)).all()
    for name in vr.FIXTURES:
        p = vr.fixture(name)
        assert p.imgA.dtype == np.uint8 and p.imgA.shape == p.imgB.shape == (p.H, p.W, 3)
    assert (vr.fixture('seam').H, vr.fixture('seam').W) == (4 * 8 + 1, 64 + 1)    # one pixel past a 64 x 8 solver tile each way


def test_the_ellipse_consistency_map_marks_the_covered_background():
    p = vr.fixture('ellipse')
    occ, e = vr.occlusion(vr.restated('ellipse')[0], vr.restated_back('ellipse'))
    covered, obj, far = occlusion_regions(p)
    print('covered %d px, occ > 0 on %.3f of them, median e %.2f px' % (covered.sum(), (occ[covered] > 0).mean(), np.nanmedian(e[covered])))
    assert covered.sum() > 50 and (occ[covered] > 0).mean() > 0.5
    assert not (occ[obj] > 0).any() and not (occ[far] > 0).any()


def occlusion_regions(p):
    """(covered background, eroded object, far from both silhouettes) of the two-layer fixture.  Covered: background pixels of A
    whose true target lies at least 1 px inside the object of B.  Far: further than 3 px from both silhouettes and, since the
    definition writes +6 where p + f(p) leaves the frame and this background moves, at least 4 px from the frame's border."""
    ys, xs = np.mgrid[0:p.H, 0:p.W]
    qx = np.clip(np.rint(xs + p.truth_ab[..., 0]).astype(int), 0, p.W - 1)
    qy = np.clip(np.rint(ys + p.truth_ab[..., 1]).astype(int), 0, p.H - 1)
    covered = ~p.maskA & vr.erode(p.maskB, 1)[qy, qx]
    inner = (xs >= 4) & (xs < p.W - 4) & (ys >= 4) & (ys < p.H - 4)
    far = ~vr.dilate(p.maskA, 3) & ~vr.dilate(p.maskB, 3) & inner
    return covered, vr.erode(p.maskA, 3), far


# ---- what the GPU comparison leaves out ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', vr.FIXTURES)
def test_pipeline_bound_and_left_out_share(name):
    b = pipeline_bound(name)
    out = left_out(name)
    f32, f64 = vr.restated(name, 'float32')[0], vr.restated(name)[0]
    print(name, 'bound %.3g px, left out %d of %d px' % (b, int(out.sum()), out.size))
    assert b <= ILL_CONDITIONED
    assert out.mean() <= LEFT_OUT_CAP
    assert np.abs(f32.astype(np.float64) - f64)[~out].max() <= b / 4 + 1e-12     # the float32 restatement stays inside its own spread


def test_near_edge_counts_positions_next_to_the_border_but_not_on_it():
    uv, d = np.zeros((2, 5, 6)), np.zeros((2, 5, 6))
    tr = [dict(level=0, uv=uv, d=d)]
    assert not vr.near_edge(tr, (5, 6), 1e-4).any()                               # exactly on the border: the same in any precision
    d2 = d.copy()
    d2[0, 2, 5] = 5e-5
    d2[1, 0, 1] = -5e-5
    d2[0, 3, 3] = 2.                                                              # 3 + 2 = W - 1 exactly
    m = vr.near_edge([dict(level=0, uv=uv, d=d2)], (5, 6), 1e-4)
    assert m.sum() == 2 and m[2, 5] and m[0, 1]
    m = vr.near_edge([dict(level=1, uv=uv[:, :3, :3], d=d2[:, :3, :3])], (5, 6), 1e-4)      # a coarse pixel covers its 2 x 2 block
    assert m.sum() == 4 and m[0:2, 2:4].all()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------

ENTRY_POINTS = ('lasr_varflow_reduce', 'lasr_varflow_expand', 'lasr_varflow_tensor', 'lasr_varflow_weights', 'lasr_varflow_sor',
                'lasr_varflow_occ')


def test_header_and_binding_agree_on_the_six_entry_points():
    from lasr_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    kinds = {'int': _lib._i, 'float': _lib._f}
    for name in ENTRY_POINTS:
        args = re.search(r'int\s+%s\s*\((.*?)\)\s*;' % name, hdr, re.S).group(1)
        want = [_lib._p if '*' in a else kinds[a.split()[0]] for a in args.split(',')]
        res, got = _lib.SIGNATURES[name]
        assert res is _lib._i and got == want, name
    for name, value in (('MIN_SIZE', 2), ('MAX_SIZE', 16384)):
        assert '#define LASR_VARFLOW_%s %d\n' % (name, value) in hdr and getattr(_lib, 'VARFLOW_' + name) == value
    assert sorted(n for n in _lib.SIGNATURES if n.startswith('lasr_varflow_')) == sorted(ENTRY_POINTS)
    assert _lib.ABI_VERSION == 13                                                 # new symbols only


def test_symbols_are_exported_and_the_host_checks_run_without_a_device():
    from lasr_amd import _lib
    h = _lib.lib()
    n, a, b = None, 1 << 20, 1 << 21                                              # a, b: non-null addresses; no launch reads them
    BAD = -1
    sizes = ((1, 8), (8, 1), (0, 0), (-1, 8), (16385, 8), (8, 16385))

    def reduce(u8=n, inp=n, l0=n, out=n, H=8, W=9):
        return h.lasr_varflow_reduce(u8, inp, l0, out, H, W, n)
    assert reduce() == BAD and reduce(u8=a, inp=a, l0=b, out=b) == BAD            # no input form; both
    assert reduce(u8=a) == BAD and reduce(inp=a) == BAD and reduce(inp=a, l0=b, out=b) == BAD and reduce(inp=a, out=a) == BAD
    assert reduce(u8=a, l0=b, out=b) == BAD
    for H, W in sizes:
        assert reduce(u8=a, l0=b, H=H, W=W) == BAD and reduce(inp=a, out=b, H=H, W=W) == BAD

    def expand(c=a, f=b, hc=4, wc=5, hh=8, w=9):
        return h.lasr_varflow_expand(c, f, hc, wc, hh, w, n)
    assert expand(c=n) == BAD and expand(f=n) == BAD and expand(f=a) == BAD
    assert expand(hc=5) == BAD and expand(wc=4) == BAD and expand(hh=1, hc=1) == BAD and expand(w=16386, wc=8193) == BAD

    def tensor(p=a, H=8, W=9):
        return h.lasr_varflow_tensor(p, p, p, p, H, W, n)
    assert tensor(p=n) == BAD and h.lasr_varflow_tensor(a, a, a, n, 8, 9, n) == BAD and h.lasr_varflow_tensor(a, n, a, a, 8, 9, n) == BAD

    def weights(p=a, H=8, W=9, eps=1e-3):
        return h.lasr_varflow_weights(p, p, p, p, H, W, eps, n)
    assert weights(p=n) == BAD and weights(eps=0.) == BAD and weights(eps=-1.) == BAD and weights(eps=float('nan')) == BAD
    assert weights(eps=float('inf')) == BAD

    def sor(p=a, d=a, s=b, H=8, W=9, alpha=0.03, omega=1.8, iters=1):
        return h.lasr_varflow_sor(p, p, p, d, s, H, W, alpha, omega, iters, n)
    assert sor(p=n) == BAD and sor(d=n) == BAD and sor(s=n) == BAD and sor(s=a) == BAD          # d == scratch
    assert sor(alpha=0.) == BAD and sor(alpha=float('nan')) == BAD and sor(omega=0.) == BAD and sor(omega=2.) == BAD
    assert sor(omega=float('nan')) == BAD and sor(iters=-1) == BAD

    def occ(p=a, o=b, H=8, W=9, tau=1., s=0.5):
        return h.lasr_varflow_occ(p, p, o, H, W, tau, s, n)
    assert occ(p=n) == BAD and occ(o=n) == BAD and occ(tau=-1.) == BAD and occ(tau=float('nan')) == BAD and occ(s=0.) == BAD
    assert occ(s=float('inf')) == BAD
    for H, W in sizes:
        assert tensor(H=H, W=W) == BAD and weights(H=H, W=W) == BAD and sor(H=H, W=W) == BAD and occ(H=H, W=W) == BAD
    names = [h.lasr_prof_kernel_name(i) for i in range(h.lasr_prof_kernel_count())]
    assert not any(b'varflow' in x for x in names)                                # the kernel-name table is not extended


def test_python_layer_refuses_cpu_tensors_and_bad_parameters():
    import torch
    from lasr_amd.nnutils import varflow
    img, uv = torch.zeros(8, 9, 3, dtype=torch.uint8), torch.zeros(2, 8, 9)
    I, J = torch.zeros(8, 9, 3), torch.zeros(6, 8, 9)
    for call in (lambda: varflow.reduce(img), lambda: varflow.reduce(I), lambda: varflow.pyramid(img), lambda: varflow.expand(uv, 16, 18),
                 lambda: varflow.tensor(I, I, uv), lambda: varflow.weights(J, uv, uv), lambda: varflow.sor(J, uv, uv, uv.clone()),
                 lambda: varflow.occlusion(torch.zeros(8, 9, 2), torch.zeros(8, 9, 2)), lambda: varflow.flow(img, img),
                 lambda: varflow.flow_pair(img, img)):
        with pytest.raises(TypeError, match='only cuda'):
            call()
    with pytest.raises(TypeError):
        varflow.flow(img.numpy(), img.numpy())
    with pytest.raises(TypeError, match='unknown parameters'):
        varflow.params(sigma=3.)
    with pytest.raises(TypeError, match='unknown parameters'):
        varflow.make_flow_fn(K=5)
    for bad in (dict(alpha=0.), dict(omega=2.), dict(eps=-1.), dict(NW=0), dict(NI=0)):
        with pytest.raises(ValueError):
            varflow.params(**bad)
    assert varflow.params() == vr.params() == varflow.DEFAULTS and varflow.params(NI=4)['NI'] == 4
    assert (varflow.OCC_TAU, varflow.OCC_S) == (vr.OCC_TAU, vr.OCC_S)
    for H, W in ((64, 80), (37, 53), (9, 7), (1080, 1920), (32, 32)):
        assert varflow.level_shapes(H, W) == vr.level_shapes(H, W)


def test_flow_fn_computes_a_pair_once_and_serves_the_reverse_call_from_its_cache(monkeypatch):
    import torch
    from lasr_amd.nnutils import varflow
    calls = []

    def fake_pair(a, b, **over):
        calls.append((int(a[0, 0, 0]), int(b[0, 0, 0]), over))
        H, W = a.shape[:2]
        ab = torch.full((H, W, 2), float(a[0, 0, 0]) - float(b[0, 0, 0]))
        return ab, torch.full((H, W), 1.), -ab, torch.full((H, W), 2.)
    monkeypatch.setattr(varflow, 'flow_pair', fake_pair)
    fn = varflow.make_flow_fn(device='cpu', NI=4)
    A, B, C = (np.full((5, 6, 3), v, np.uint8) for v in (10, 20, 30))
    f, o = fn(A, B)
    assert f.dtype == o.dtype == np.float32 and f.shape == (5, 6, 3) and o.shape == (5, 6)
    assert (f[..., :2] == -10).all() and (f[..., 2] == 1).all() and (o == 1).all()
    f, o = fn(B, A)
    assert (f[..., :2] == 10).all() and (f[..., 2] == 1).all() and (o == 2).all() and calls == [(10, 20, dict(NI=4))]
    assert fn.stats == dict(computed=1, cached=1)
    fn(B, A)                                                                      # served once: the next call computes
    fn(A, C)                                                                      # another pair drops the cached reverse of (B, A)
    fn(A, B)
    assert [c[:2] for c in calls] == [(10, 20), (20, 10), (10, 30), (10, 20)] and fn.stats == dict(computed=4, cached=1)
    g = fn(A[..., 0], C[..., 0])[0]                                               # grey frames are tiled to three channels
    assert g.shape == (5, 6, 3)
    with pytest.raises(ValueError):
        fn(A, np.zeros((5, 7, 3), np.uint8))
    with pytest.raises(ValueError):
        fn(A.astype(np.float32), B.astype(np.float32))


# ---- the scripts ------------------------------------------------------------------------------------------------------------------

def test_both_scripts_parse_the_flag_default_to_vcn_and_refuse_a_checkpoint_with_it(capsys):
    import auto_gen
    import propagate_mask as pm
    base = {auto_gen: ['--datapath', 'd/JPEGImages/x/'], pm: ['--datapath', 'd/JPEGImages/x/', '--key', '0:a.png']}
    for mod, argv in base.items():
        a = mod.parse_args(argv)
        assert a.flow_method == 'vcn' and a.loadmodel is None
        assert mod.parse_args(argv + ['--loadmodel', 'vcn_rob.pth']).loadmodel == 'vcn_rob.pth'            # as before
        assert {n: getattr(a, 'vf_' + n) for n in vr.DEFAULTS} == vr.DEFAULTS
        a = mod.parse_args(argv + '--flow_method variational --vf_alpha 0.05 --vf_eps 1e-2 --vf_omega 1.5 --vf_NW 3 --vf_NO 2 --vf_NI 8 '
                                  '--testres 0.5'.split())
        assert a.flow_method == 'variational' and a.testres == 0.5
        assert {n: getattr(a, 'vf_' + n) for n in vr.DEFAULTS} == dict(alpha=0.05, eps=1e-2, omega=1.5, NW=3, NO=2, NI=8)
        with pytest.raises(SystemExit):
            mod.parse_args(argv + ['--flow_method', 'variational', '--loadmodel', 'vcn_rob.pth'])
        assert 'uses no network' in capsys.readouterr().err
        with pytest.raises(SystemExit):
            mod.parse_args(argv + ['--flow_method', 'farneback'])
    assert [n for n, _, _, _ in auto_gen.FLOW_TUNING] == list(vr.DEFAULTS) and {n: d for n, _, d, _ in auto_gen.FLOW_TUNING} == vr.DEFAULTS
    a = pm.parse_args(base[pm] + ['--eps', '1e-2', '--vf_eps', '1e-4'])            # the two eps are different parameters
    assert pm.tuning_of(a)['eps'] == 1e-2 and a.vf_eps == 1e-4


def test_variational_flow_fn_passes_the_flags_on_and_scales_the_frames_by_testres():
    import auto_gen
    seen = []

    def make(**over):
        seen.append(over)

        def inner(a, b):
            seen.append((a.shape, a.dtype))
            f = np.zeros(a.shape[:2] + (3,), np.float32)
            f[..., 0], f[..., 1], f[..., 2] = 2., -1., 1.
            return f, np.full(a.shape[:2], 3., np.float32)
        return inner
    args = auto_gen.parse_args(['--flow_method', 'variational', '--vf_NI', '6'])
    fn = auto_gen.variational_flow_fn(args, make)
    assert seen == [dict(vr.DEFAULTS, NI=6)]
    img = np.zeros((20, 30, 3), np.uint8)
    f, o = fn(img, img)
    assert seen[-1] == ((20, 30, 3), np.uint8) and f.shape == (20, 30, 3) and (f[..., 0] == 2).all()
    args = auto_gen.parse_args(['--flow_method', 'variational', '--testres', '0.5'])
    f, o = auto_gen.variational_flow_fn(args, make)(img, img)
    assert seen[-1] == ((10, 15, 3), np.uint8)                                    # the flow ran at half the size
    assert f.shape == (20, 30, 3) and f.dtype == np.float32 and o.shape == (20, 30) and o.dtype == np.float32
    assert np.allclose(f[..., 0], 4.) and np.allclose(f[..., 1], -2.) and (f[..., 2] == 1).all() and np.allclose(o, 3.)
