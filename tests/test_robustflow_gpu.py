"""The gradient-constancy term of the variational flow on the device (preprocess/robust_flow.py, lasr_amd/csrc/robustflow.hip)
against the float64 restatement (tests/robustflow_restated.py): the only parity there is, as for the flow it extends.

Every comparison is made under test_varflow_cpu.bound: 4 x max |float32 restatement - float64 restatement| on the very inputs of the
comparison, at least one float32 ulp of the largest magnitude; no figure of it comes from a kernel.  The per-stage inputs are those
of the last warp of every level of the float64 run of trans, odd, tiny and seam, rounded to float32 (64 x 80, 32 x 40, 16 x 20,
37 x 53, 19 x 27, 9 x 7, 33 x 65, 17 x 33: more than one tile, no multiple of the 32 x 8 tile, smaller than the double stencil).
Where `valid` could differ between precisions (a warped position within one float32 ulp of the frame's size of the frame edge
without being on it) the pixel is left out of the tensor comparison, and the whole-flow comparison leaves out
varflow_restated.near_edge of the float64 trace; both are capped at 1 %.  Each test prints its figures before it asserts.

Measured on an MI355X: every new stage at every level of the four fixtures, the 2 x 2 record and the whole flow() equal the float32
restatement bit for bit (|kernel - float32 restatement| = 0), so |kernel - float64| is a quarter of its bound throughout: whole
flow 6.3e-6 px against 2.5e-5 (trans, 16 of 5120 pixels left out), 4.0e-6 against 1.6e-5 (odd, none left out), 1.3e-5 against
5.1e-5 (2 x 2); Jg at most 5.3e-10, the combined J at most 2.2e-7, psi_s at most 0.022 of values up to 500.  EPE against the truth,
varflow.flow -> robust_flow.flow: trans 1.6569 -> 0.4038 (gain), 2.3037 -> 0.3733 (ramp), 4.9665 -> 0.8225 (shadow); affine
1.5995 -> 0.6199, 2.3509 -> 0.5973, 6.3625 -> 1.0254; unchanged trans / affine / ellipse 0.0043 / 0.0703 / 0.0128 px.  The ellipse
sequence of maskprop_restated with every second frame relit (gain) propagates at minimum IoU 1.000 along the plain variational flow
and 1.000 with --vf_gamma 5: on this fixture the relighting does not break the propagation, and the test shows no more than that
the flag does no harm there.
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

import guarded
import maskprop_restated as br
import robustflow_guarded
import robustflow_restated as rr
import varflow_restated as vr
from test_maskprop_cpu import write_video
from test_varflow_cpu import LEFT_OUT_CAP, bound
from test_varflow_gpu import _check, _dev, _f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
STAGED = ('trans', 'odd', 'tiny', 'seam')


def _rf():
    return robustflow_guarded.robust_flow()


def _vf():
    from lasr_amd.nnutils import varflow
    return varflow


@pytest.fixture(scope='module')
def stages():
    """name -> list over the levels (finest first) of the float32-rounded inputs of that level's last warp in the float64 run;
    computed once, shared, left unchanged."""
    out = {}
    for name in STAGED:
        _, trace = rr.restated(name)
        n = len(vr.level_shapes(*trace[-1]['uv'].shape[1:]))
        out[name] = [{k: _f32([e for e in trace if e['level'] == lev][-1][k]) for k in ('I1', 'I2', 'R1', 'R2', 'uv', 'Jb', 'Jg', 'd_in')}
                     for lev in range(n)]
    return out


@pytest.mark.parametrize('name', STAGED)
def test_every_new_stage_against_the_restatement_at_every_level(cuda, stages, name):
    rf = _rf()
    eps = vr.params()['eps']
    for lev, s in enumerate(stages[name]):
        h, w = s['uv'].shape[1:]
        tag = '%s level %d (%d x %d)' % (name, lev, h, w)
        for k in ('I1', 'I2'):
            rec = rf.derivs(_dev(cuda, s[k]))
            assert tuple(rec.shape) == (h, w, 3, 6) and rec.is_contiguous()
            _check('%s derivs of %s' % (tag, k), rec.cpu().numpy(), rr.derivs(s[k], np.float32), rr.derivs(s[k]))
        R1, R2, uv, Jb, Jg, d_in = _dev(cuda, s['R1'], s['R2'], s['uv'], s['Jb'], s['Jg'], s['d_in'])
        X, Y, _ = vr.warp_positions(s['uv'].astype(np.float64))
        near = np.zeros((h, w), bool)
        for P, hi in ((X, w - 1), (Y, h - 1)):
            for edge in (0., float(hi)):
                near |= (np.abs(P - edge) <= float(np.spacing(np.float32(max(h, w))))) & (P != edge)
        assert near.mean() <= LEFT_OUT_CAP
        got = rf.tensor(R1, R2, uv)
        r32, r64 = rr.tensor(s['R1'], s['R2'], s['uv'], np.float32), rr.tensor(s['R1'], s['R2'], s['uv'])
        for q, what in enumerate(('Jb', 'Jg')):
            _check('%s tensor %s' % (tag, what), got[q].cpu().numpy(), r32[q], r64[q], keep=~near)
        got = rf.weights(Jb, Jg, uv, d_in, eps, rr.BETA, rr.GAMMA)
        r32 = rr.weights(s['Jb'], s['Jg'], s['uv'], s['d_in'], eps, rr.BETA, rr.GAMMA, np.float32)
        r64 = rr.weights(s['Jb'], s['Jg'], s['uv'], s['d_in'], eps, rr.BETA, rr.GAMMA)
        for q, what in enumerate(('J', 'psi')):
            _check('%s weights %s' % (tag, what), got[q].cpu().numpy(), r32[q], r64[q])
        assert bool((got[1][0] == 1).all())


def test_the_brightness_tensor_is_the_one_of_varflow(cuda, stages):
    rf, vf = _rf(), _vf()
    for name in ('odd', 'seam'):
        s = stages[name][0]
        I1, I2, uv = _dev(cuda, s['I1'], s['I2'], s['uv'])
        assert torch.equal(rf.tensor(rf.derivs(I1), rf.derivs(I2), uv)[0], vf.tensor(I1, I2, uv))


def test_tensors_are_zero_where_the_warp_leaves_the_frame_or_the_flow_is_nan(cuda):
    rf = _rf()
    p = vr.fixture('odd')
    a, b = vr.to_unit(p.imgA, np.float32), vr.to_unit(p.imgB, np.float32)
    uv = np.zeros((2, p.H, p.W), np.float32)
    uv[0, :, -3:] = 3.5                                                           # leaves on the right
    uv[1, :2] = -2.5                                                              # leaves at the top
    uv[0, 10, 10] = np.nan
    R1, R2 = rf.derivs(_dev(cuda, a)), rf.derivs(_dev(cuda, b))
    Jb, Jg = (t.cpu().numpy() for t in rf.tensor(R1, R2, _dev(cuda, uv)))
    gone = np.zeros((p.H, p.W), bool)
    gone[:, -3:] = gone[:2] = gone[10, 10] = True
    for J in (Jb, Jg):
        assert not J[:, gone].any() and np.isfinite(J).all() and J[:, ~gone].any()
    clean = np.nan_to_num(uv)
    r32, r64 = rr.tensor(rr.derivs(a, np.float32), rr.derivs(b, np.float32), clean, np.float32), rr.tensor(rr.derivs(a, np.float32), rr.derivs(b, np.float32), clean)
    _check('odd Jb, part of the warp outside', Jb, r32[0], r64[0], keep=~gone)
    _check('odd Jg, part of the warp outside', Jg, r32[1], r64[1], keep=~gone)
    J, psi = rf.weights(_dev(cuda, Jb), _dev(cuda, Jg), _dev(cuda, clean), torch.zeros(2, p.H, p.W, device=cuda))
    assert bool(torch.isfinite(J).all()) and bool(torch.isfinite(psi).all())


@pytest.fixture(scope='module')
def device_flows(cuda):
    """(name, kind) -> (robust_flow.flow, varflow.flow) of the pair on the device, computed once."""
    rf, vf = _rf(), _vf()
    out = {}
    for name in ('trans', 'affine', 'ellipse', 'odd'):
        for kind in (None,) + (rr.RELIGHTINGS if name in ('trans', 'affine') else ()):
            p = rr.fixture(name, kind)
            A, B = _dev(cuda, p.imgA, p.imgB)
            out[name, kind] = (rf.flow(A, B), vf.flow(A, B))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('name', ['trans', 'odd'])
def test_flow_matches_the_restatement_and_repeats(cuda, device_flows, name):
    p = vr.fixture(name)
    f = device_flows[name, None][0]
    assert f.dtype == torch.float32 and tuple(f.shape) == (p.H, p.W, 2) and f.is_contiguous()
    f = f.cpu().numpy().astype(np.float64)
    (f64, trace), f32 = rr.restated(name), rr.restated(name, None, 'float32')[0]
    b = bound(f32, f64)
    out = vr.near_edge(trace, (p.H, p.W), b)
    err = np.abs(f - f64).max(-1)
    print('%s: |flow - float64| %.3g px, bound %.3g px, |flow - float32 restatement| %.3g px, left out %d px'
          % (name, err[~out].max(), b, np.abs(f - f32).max(), int(out.sum())))
    assert out.mean() <= LEFT_OUT_CAP
    assert err[~out].max() <= b
    A, B = _dev(cuda, p.imgA, p.imgB)
    assert torch.equal(_rf().flow(A, B), device_flows[name, None][0])             # two runs, the same bits


def test_gamma_zero_through_the_script_is_the_brightness_flow(cuda, device_flows):
    sys.path.insert(0, os.path.join(ROOT, 'preprocess'))
    import auto_gen
    p = vr.fixture('odd')
    fn = auto_gen.variational_flow_fn(auto_gen.parse_args(['--flow_method', 'variational', '--vf_gamma', '0']))
    f, _ = fn(p.imgA, p.imgB)
    assert torch.equal(torch.from_numpy(np.ascontiguousarray(f[..., :2])), device_flows['odd', None][1].cpu())
    fn5 = auto_gen.variational_flow_fn(auto_gen.parse_args(['--flow_method', 'variational', '--vf_gamma', '5']))
    f5, occ = fn5(p.imgA, p.imgB)
    assert torch.equal(torch.from_numpy(np.ascontiguousarray(f5[..., :2])), device_flows['odd', None][0].cpu())
    assert (f5[..., 2] == 1).all() and occ.shape == (p.H, p.W) and (occ != 0).all()
    fn5(p.imgB, p.imgA)
    assert fn5.stats == dict(computed=1, cached=1)


@pytest.mark.parametrize('name', ['trans', 'affine'])
@pytest.mark.parametrize('kind', rr.RELIGHTINGS)
def test_the_term_halves_the_error_on_a_relit_pair_on_the_device(device_flows, name, kind):
    p = rr.fixture(name, kind)
    region = vr.score_region(p)
    robust, plain = (vr.epe(f.cpu().numpy(), p.truth_ab, region) for f in device_flows[name, kind])
    print('%s / %s: varflow.flow %.4f px, robust_flow.flow %.4f px, ratio %.3f' % (name, kind, plain, robust, robust / plain))
    assert robust <= 0.5 * plain


@pytest.mark.parametrize('name', ['trans', 'affine', 'ellipse'])
def test_the_unchanged_pairs_stay_under_the_bar_on_the_device(device_flows, name):
    p = vr.fixture(name)
    got = vr.epe(device_flows[name, None][0].cpu().numpy(), p.truth_ab, vr.score_region(p))
    print('%s: EPE %.4f px' % (name, got))
    assert got < 0.1


def test_a_two_by_two_pair(cuda):
    rf = _rf()
    g = np.random.default_rng(9)
    A, B = (g.integers(0, 256, (2, 2, 3), dtype=np.uint8) for _ in range(2))
    f = rf.flow(_dev(cuda, A), _dev(cuda, B))
    assert tuple(f.shape) == (2, 2, 2) and bool(torch.isfinite(f).all())
    b = bound(rr.flow(A, B, np.float32), rr.flow(A, B))
    err = float(np.abs(f.cpu().numpy() - rr.flow(A, B)).max())
    print('2 x 2: |flow - float64| %.3g px, bound %.3g px' % (err, b))
    assert err <= b
    unit = vr.to_unit(A, np.float32)
    _check('2 x 2 derivs', rf.derivs(_dev(cuda, unit)).cpu().numpy(), rr.derivs(unit, np.float32), rr.derivs(unit))


def test_the_three_natives_with_guard_bands_and_poison(cuda):
    rf = _rf()
    guarded.run_case(robustflow_guarded.CASE, cuda, modules=[rf] + guarded._product_modules())


def test_the_three_natives_with_relocated_inputs(cuda):
    rf = _rf()
    record = guarded.run_relocated(robustflow_guarded.CASE, cuda, modules=[rf] + guarded._product_modules())
    assert sorted(record) == sorted(robustflow_guarded.NATIVES)


def test_propagate_mask_on_a_relit_sequence(cuda, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'preprocess'))
    import auto_gen
    import propagate_mask as pm
    seq = br.fixture('ellipse')
    frames = np.stack([rr.relight(f, 'gain') if t % 2 else f for t, f in enumerate(seq.frames)])
    lowest = {}
    for tag, extra in (('plain', []), ('robust', ['--vf_gamma', '5'])):
        datapath, key = write_video(types.SimpleNamespace(frames=frames, masks=seq.masks), tmp_path / tag)
        args = pm.parse_args(['--datapath', datapath, '--key', '0:' + key, '--min_area', '100', '--flow_method', 'variational'] + extra)
        fn = auto_gen.variational_flow_fn(args)
        pm.run(args, fn)
        out = pm.annotations_dir(datapath)
        ious = [br.iou(auto_gen.read_mask(os.path.join(out, '%05d.png' % t)), seq.masks[t]) for t in range(seq.T)]
        print('%s: IoU along the flow' % tag, ['%.3f' % v for v in ious], fn.stats)
        lowest[tag] = min(ious)
    print('minimum IoU, every second frame relit (gain): plain %.3f, --vf_gamma 5 %.3f' % (lowest['plain'], lowest['robust']))
    assert lowest['robust'] >= lowest['plain']
