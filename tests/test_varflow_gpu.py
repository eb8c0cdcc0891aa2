"""Variational optical flow on the device (lasr_amd/nnutils/varflow.py, csrc/varflow.hip) against the float64 restatement
(tests/varflow_restated.py).  The flow is this project's own addition: the restatement is the only parity there is.

Every comparison is made under test_varflow_cpu.bound: 4 x max |float32 restatement - float64 restatement| on the very inputs of the
comparison, at least one float32 ulp of the largest magnitude; no figure of it comes from a kernel.  The per-stage inputs are those
of the last warp of every level of the float64 run of every fixture, rounded to float32, so each kernel is run at every level's
shape of every fixture (64 x 80, 32 x 40, 16 x 20, 37 x 53, 19 x 27, 9 x 7, 33 x 65, 17 x 33).  Where `valid` of the linearisation
could differ between precisions (a warped position within one float32 ulp of the frame's size of the frame edge without being on
it) the pixel is left out of the tensor comparison; the whole-pipeline comparison leaves out test_varflow_cpu.left_out, which that
file caps at 1 % and measures as 0 pixels on every fixture.  Each test prints its figures before it asserts.

Measured on an MI355X: every stage at every level of every fixture, the consistency map and the whole flow() equal the float32
restatement bit for bit (|kernel - float32 restatement| = 0), so |kernel - float64| is a quarter of its bound throughout: whole
flow 8.0e-6 px (trans), 1.7e-5 (big), 9.2e-6 (affine), 1.9e-5 (ellipse), 5.9e-6 (odd), 1.1e-6 (tiny), 4.7e-6 (seam); SOR after ten
iterations at most 1.4e-5 px (big, level 0), psi at most 0.088 of values up to 500 (big, level 0).  EPE against the truth
0.0030 / 0.0025 / 0.0452 / 0.0214 px on trans / big / affine / ellipse; 96 % of the 67 covered background pixels of the ellipse have
occ > 0; the mask propagation along this flow reaches IoU 1.000 on all eight frames.
"""
import os
import sys

import numpy as np
import pytest
import torch

import maskprop_restated as br
import varflow_restated as vr
from test_maskprop_cpu import write_video
from test_varflow_cpu import bound, left_out, occlusion_regions, pipeline_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _vf():
    from lasr_amd.nnutils import varflow
    return varflow


def _dev(cuda, *arrays):
    out = [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]
    return out[0] if len(out) == 1 else out


def _f32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


@pytest.fixture(scope='module')
def stages():
    """name -> list over the levels (finest first) of the float32-rounded inputs of that level's last warp in the float64 run, and
    `coarse`, the flow the level below handed up; computed once, shared, left unchanged."""
    out = {}
    for name in vr.FIXTURES:
        p = vr.fixture(name)
        _, trace = vr.restated(name)
        n = len(vr.level_shapes(p.H, p.W))
        levels = []
        for lev in range(n):
            t = [e for e in trace if e['level'] == lev][-1]
            entry = {k: _f32(t[k]) for k in ('I1', 'I2', 'uv', 'J', 'psi', 'd_in')}
            if lev + 1 < n:
                below = [e for e in trace if e['level'] == lev + 1][-1]
                entry['coarse'] = _f32(below['uv'] + below['d'])
            levels.append(entry)
        out[name] = levels
    return out


def _check(what, got, r32, r64, keep=None):
    got, r32, r64 = (np.asarray(a, np.float64) for a in (got, r32, r64))
    if keep is not None:
        got, r32, r64 = got[..., keep], r32[..., keep], r64[..., keep]
    b = bound(r32, r64)
    err = float(np.abs(got - r64).max())
    print('%s: |kernel - float64| %.3g, bound %.3g, |kernel - float32 restatement| %.3g' % (what, err, b, float(np.abs(got - r32).max())))
    assert err <= b, what


@pytest.mark.parametrize('name', vr.FIXTURES)
def test_every_stage_against_the_restatement_at_every_level(cuda, stages, name):
    vf = _vf()
    p = vr.fixture(name)
    par = vr.params()
    for lev, s in enumerate(stages[name]):
        h, w = s['uv'].shape[1:]
        tag = '%s level %d (%d x %d)' % (name, lev, h, w)
        # REDUCE of this level (the uint8 form on level 0), whether or not the pyramid goes on below it
        if lev == 0:
            level0, red = vf.reduce(_dev(cuda, p.imgA))
            _check(tag + ' unit', level0.cpu().numpy(), vr.to_unit(p.imgA, np.float32), vr.to_unit(p.imgA))
            src = vr.to_unit(p.imgA, np.float32)
        else:
            src = s['I1']
            red = vf.reduce(_dev(cuda, src))
        assert tuple(red.shape) == ((h + 1) // 2, (w + 1) // 2, 3)
        _check(tag + ' reduce', red.cpu().numpy(), vr.reduce(src, np.float32), vr.reduce(src))
        if 'coarse' in s:
            _check(tag + ' expand', vf.expand(_dev(cuda, s['coarse']), h, w).cpu().numpy(), vr.expand(s['coarse'], h, w, np.float32),
                   vr.expand(s['coarse'], h, w))
        I1, I2, uv, J, psi, d_in = _dev(cuda, s['I1'], s['I2'], s['uv'], s['J'], s['psi'], s['d_in'])
        X, Y, _ = vr.warp_positions(s['uv'].astype(np.float64))
        near = np.zeros((h, w), bool)
        for P, hi in ((X, w - 1), (Y, h - 1)):
            for edge in (0., float(hi)):
                near |= (np.abs(P - edge) <= float(np.spacing(np.float32(max(h, w))))) & (P != edge)
        assert near.mean() <= 0.01
        _check(tag + ' tensor', vf.tensor(I1, I2, uv).cpu().numpy(), vr.tensor(s['I1'], s['I2'], s['uv'], np.float32),
               vr.tensor(s['I1'], s['I2'], s['uv']), keep=~near)
        _check(tag + ' weights', vf.weights(J, uv, d_in, par['eps']).cpu().numpy(), vr.weights(s['J'], s['uv'], s['d_in'], par['eps'], np.float32),
               vr.weights(s['J'], s['uv'], s['d_in'], par['eps']))
        d = d_in.clone()
        assert vf.sor(J, psi, uv, d, par['alpha'], par['omega'], par['NI']) is d
        _check(tag + ' sor', d.cpu().numpy(), vr.sor(s['J'], s['psi'], s['uv'], s['d_in'], par['alpha'], par['omega'], par['NI'], np.float32),
               vr.sor(s['J'], s['psi'], s['uv'], s['d_in'], par['alpha'], par['omega'], par['NI']))


def test_tensor_is_zero_where_the_warp_leaves_the_frame_and_on_identical_frames(cuda):
    vf = _vf()
    p = vr.fixture('odd')
    I = _dev(cuda, vr.to_unit(p.imgA, np.float32))
    uv = np.zeros((2, p.H, p.W), np.float32)
    same = vf.tensor(I, I, _dev(cuda, uv))
    assert not same[3:].any() and same[0].any() and same[2].any()                 # It = 0 exactly: only J11, J12, J22 are left
    uv[0, :, -3:] = 3.5                                                           # leaves on the right
    uv[1, :2] = -2.5                                                              # leaves at the top
    uv[0, 10, 10] = np.nan
    J = vf.tensor(I, _dev(cuda, vr.to_unit(p.imgB, np.float32)), _dev(cuda, uv)).cpu().numpy()
    a, b = vr.to_unit(p.imgA, np.float32), vr.to_unit(p.imgB, np.float32)
    gone = np.zeros((p.H, p.W), bool)
    gone[:, -3:] = gone[:2] = gone[10, 10] = True
    assert not J[:, gone].any() and np.isfinite(J).all() and J[:, ~gone].any()
    _check('odd tensor, part of the warp outside', J, vr.tensor(a, b, np.nan_to_num(uv), np.float32), vr.tensor(a, b, np.nan_to_num(uv)), keep=~gone)


@pytest.mark.parametrize('name', ['seam', 'odd', 'tiny'])
def test_sor_iterations_compose_bit_for_bit_and_repeat(cuda, stages, name):
    vf = _vf()
    for lev, s in enumerate(stages[name]):
        J, psi, uv, d_in = _dev(cuda, s['J'], s['psi'], s['uv'], s['d_in'])
        rng = np.random.default_rng(5)
        rough = _dev(cuda, (s['d_in'] + rng.uniform(-0.5, 0.5, s['d_in'].shape)).astype(np.float32))      # a start far from the fixed point
        for start in (d_in, rough):
            for n in (1, 2, 3, 10):
                once = vf.sor(J, psi, uv, start.clone(), iters=n)
                step = start.clone()
                for _ in range(n):
                    vf.sor(J, psi, uv, step, iters=1)
                again = vf.sor(J, psi, uv, start.clone(), iters=n, scratch=torch.full_like(start, 7.))
                assert torch.equal(once, step) and torch.equal(once, again), (name, lev, n)
            assert torch.equal(vf.sor(J, psi, uv, start.clone(), iters=0), start)
        # against the restatement from the rough start too: one iteration, where the colours' order and the tile borders show
        _check('%s level %d sor x1' % (name, lev), vf.sor(J, psi, uv, rough.clone(), iters=1).cpu().numpy(),
               vr.sor(s['J'], s['psi'], s['uv'], rough.cpu().numpy(), iters=1, dt=np.float32),
               vr.sor(s['J'], s['psi'], s['uv'], rough.cpu().numpy(), iters=1))


@pytest.fixture(scope='module')
def device_flows(cuda):
    """name -> flow() of the fixture on the device, computed once."""
    vf = _vf()
    out = {}
    for name in vr.FIXTURES:
        p = vr.fixture(name)
        A, B = _dev(cuda, p.imgA, p.imgB)
        out[name] = vf.flow(A, B)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('name', vr.FIXTURES)
def test_flow_matches_the_restatement_and_the_truth(cuda, device_flows, name):
    p = vr.fixture(name)
    f = device_flows[name]
    assert f.dtype == torch.float32 and tuple(f.shape) == (p.H, p.W, 2) and f.is_contiguous()
    f = f.cpu().numpy().astype(np.float64)
    f64, f32 = vr.restated(name)[0], vr.restated(name, 'float32')[0]
    out = left_out(name)
    b = pipeline_bound(name)
    err = np.abs(f - f64).max(-1)
    print('%s: |flow - float64| %.3g px, bound %.3g px, |flow - float32 restatement| %.3g px, left out %d px'
          % (name, err[~out].max(), b, np.abs(f - f32).max(), int(out.sum())))
    assert err[~out].max() <= b
    if name in vr.MOTION:
        got = vr.epe(f, p.truth_ab, vr.score_region(p))
        print('%s: EPE %.4f px' % (name, got))
        assert got < 0.1
    A, B = _dev(cuda, p.imgA, p.imgB)
    assert torch.equal(_vf().flow(A, B), device_flows[name])                      # two runs, the same bits


def test_flow_pair_marks_the_covered_background_of_the_ellipse(cuda, device_flows):
    vf = _vf()
    p = vr.fixture('ellipse')
    A, B = _dev(cuda, p.imgA, p.imgB)
    f_ab, occ_ab, f_ba, occ_ba = vf.flow_pair(A, B)
    assert torch.equal(f_ab, device_flows['ellipse']) and torch.equal(f_ba, vf.flow(B, A))
    assert tuple(occ_ab.shape) == tuple(occ_ba.shape) == (p.H, p.W) and occ_ab.dtype == torch.float32
    want, _ = vr.occlusion(f_ab.cpu().numpy(), f_ba.cpu().numpy())                # the map of these very flows, in float64
    w32, _ = vr.occlusion(f_ab.cpu().numpy(), f_ba.cpu().numpy(), np.float32)
    occ = occ_ab.cpu().numpy()
    _check('ellipse occ', occ, w32, want)
    assert (occ != 0).all() and occ.min() >= -6 and occ.max() <= 6
    covered, obj, far = occlusion_regions(p)
    print('covered background: occ > 0 on %.3f of %d px' % ((occ[covered] > 0).mean(), covered.sum()))
    assert (occ[covered] > 0).mean() > 0.5
    assert not (occ[obj] > 0).any() and not (occ[far] > 0).any()


def test_occlusion_closed_forms_on_the_device(cuda):
    vf = _vf()
    H, W = 6, 8
    z = np.zeros((H, W, 2), np.float32)
    out, back = z.copy(), z.copy()
    out[2, 3], out[4, 1], out[0, 0], out[5, 7] = (5., 0.), (-1.5, 0.), (0., -0.25), (np.nan, 0.)
    back[..., 0] = 1.
    occ = vf.occlusion(_dev(cuda, out), _dev(cuda, z)).cpu().numpy()
    assert occ[2, 3] == occ[4, 1] == occ[0, 0] == occ[5, 7] == 6 and occ[1, 1] == -2
    occ = vf.occlusion(_dev(cuda, z), _dev(cuda, back)).cpu().numpy()             # e = tau: an exact 0 becomes the smallest normal
    assert (occ == vr.TINY).all() and (occ != 0).all()
    assert np.array_equal(occ, vr.occlusion(z, back)[0])


def test_scripts_run_on_the_variational_flow(cuda, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'preprocess'))
    import auto_gen
    import propagate_mask as pm
    seq = br.fixture('ellipse')
    datapath, key = write_video(seq, tmp_path)
    args = pm.parse_args(['--datapath', datapath, '--key', '0:' + key, '--min_area', '100', '--flow_method', 'variational'])
    fn = auto_gen.variational_flow_fn(args)
    pm.run(args, fn)
    out = pm.annotations_dir(datapath)
    ious = [br.iou(auto_gen.read_mask(os.path.join(out, '%05d.png' % t)), seq.masks[t]) for t in range(seq.T)]
    print('IoU along the variational flow', ['%.3f' % v for v in ious], fn.stats)
    assert min(ious) >= 0.95
    assert fn.stats == dict(computed=seq.T - 1, cached=seq.T - 1)                 # every pair once, every reverse call from the cache
    # auto_gen.run writes the same files as with the sequence's closed-form flow_fn
    listing = {}
    for tag, flow_fn in (('truth', seq.flow_fn), ('variational', auto_gen.variational_flow_fn(auto_gen.parse_args(['--flow_method', 'variational'])))):
        root = tmp_path / tag
        kept = auto_gen.run(auto_gen.parse_args(['--datapath', datapath, '--outdir', str(root)]), flow_fn)
        assert kept == [(t, t + 1) for t in range(seq.T - 1)]
        listing[tag] = sorted(os.path.relpath(os.path.join(d, f), str(root)) for d, _, files in os.walk(str(root)) for f in files)
        if tag == 'variational':
            assert flow_fn.stats == dict(computed=seq.T - 1, cached=seq.T - 1)
    assert listing['truth'] == listing['variational'] and len(listing['truth']) == 4 * (seq.T - 1) + 2 * seq.T
    from lasr_amd.ext_utils.util_flow import readPFM
    flo, _ = readPFM(str(tmp_path / 'variational' / 'FlowFW' / 'flo-00000.pfm'))
    occ, _ = readPFM(str(tmp_path / 'variational' / 'FlowFW' / 'occ-00000.pfm'))
    assert flo.shape == (seq.H, seq.W, 3) and (flo[..., 2] == 1).all() and occ.shape == (seq.H, seq.W) and (occ != 0).all()
    # what is on disk is the flow_fn's answer with the rows flipped before write_pfm, as the reference does
    want = auto_gen.variational_flow_fn(args)(seq.frames[0], seq.frames[1])
    assert np.array_equal(flo[::-1], want[0]) and np.array_equal(occ[::-1], want[1])
