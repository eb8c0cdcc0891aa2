"""Silhouette propagation on the device (lasr_amd/nnutils/maskprop.py, csrc/maskprop.hip) against the float64 restatement
(tests/maskprop_restated.py).  The propagation is this project's own addition: the restatement is the only parity there is.

Tolerance on the soft field.  The restatement itself, run in float32 and in float64 on the CPU on the first step of the four
fixtures (ellipse, odd, tiny, border), differs after K = 5 iterations by at most 8.34e-8 (ellipse 6.87e-8, odd 8.34e-8, tiny
7.66e-8, border 8.28e-8); the kernel's operation order and expf differ from numpy's, so 8 times that is allowed:
Q_TOL = 8 * 8.4e-8 = 6.7e-7.  The earlier stages are compared under the same rule with their own float32 / float64 spread of the
restatement (largest of the four fixtures): u 2.46e-5 (the logit's slope is 1000 at the clamp of the prior), q0 1.55e-6,
iteration 1 5.2e-7, iteration 2 9.4e-8, iteration 3 1.09e-7, iteration 4 8.6e-8.  None of these figures comes from the kernel.
Binary masks must agree everywhere but at the pixels test_maskprop_cpu.py counts as undecided (float64 q within Q_TOL of 0.5;
there are none on these fixtures).

Measured on an MI355X (each test prints its figures before it asserts): |q - float64| after 5 iterations 6.87e-8 (ellipse), 8.34e-8
(odd), 7.66e-8 (tiny), 8.28e-8 (border), bound 6.7e-7; u at most 2.46e-5 (odd), bound 2e-4; q0 at most 1.65e-6 (tiny), bound 1.28e-5;
histograms equal.  Full propagation: soft differs from the restatement by at most 1.1e-7 (ellipse), 2.9e-7 (noisy), 8.3e-8 (border),
no mask pixel differs, IoU against the truth >= 0.998.
lasr_amd.synth_data.SyntheticSequence(image_size=64, n_frames=6) is not a case: its mesh turns 60 degrees a frame and the float64
restatement reaches IoU 0.99, 0.95, 0.80, 0.76, 0.70 on frames 1-5 (the device 0.97, 0.86, 0.70, 0.65, 0.60), below the 0.85 at which
the case was to be kept.
"""
import os
import sys

import numpy as np
import pytest
import torch

import maskprop_restated as br
from test_maskprop_cpu import GPU_Q_TOL as Q_TOL, undecided, write_video

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# float32 / float64 spread of the restatement per stage (header); the bound is 8 x
SPREAD = {'u': 2.5e-5, 'q0': 1.6e-6, 1: 5.2e-7, 2: 9.4e-8, 3: 1.1e-7, 4: 8.7e-8, 5: 8.4e-8}
assert 8 * SPREAD[5] == Q_TOL


def _mp():
    from lasr_amd.nnutils import maskprop
    return maskprop


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _hist32(h):
    return torch.from_numpy(h.astype(np.int32))


HIST_CASES = [('ellipse', (0, 0, 80, 64)),            # the whole image
              ('ellipse', (0, 10, 80, 33)),           # cuts the left and right border
              ('ellipse', (61, 0, 80, 64)),           # cuts the top, bottom and right border
              ('ellipse', (0, 0, 41, 52)),            # cuts the top and left border
              ('ellipse', (13, 7, 54, 58)),           # inside
              ('ellipse', (30, 20, 30, 40)),          # empty
              ('ellipse', (30, 20, 50, 20)),          # empty
              ('odd', (3, 0, 53, 37)),
              ('tiny', (0, 0, 7, 9)),
              ('tiny', (2, 3, 3, 4))]                 # one pixel


@pytest.mark.parametrize('name,window', HIST_CASES)
def test_histogram_counts_are_the_restatement_s(cuda, name, window):
    seq = br.fixture(name)
    rng = np.random.default_rng(3)
    P = seq.masks[0].astype(np.float32)
    soft = np.clip(P * 0.9 + rng.uniform(0, 0.1, P.shape), 0, 1).astype(np.float32)      # values on both sides of hi and lo
    soft[::5, ::3] = np.float32(0.9)                                                  # and exactly on the thresholds
    soft[1::5, ::3] = np.float32(0.1)
    for field in (P, soft):
        img, Pd = _dev(cuda, seq.frames[0], field)
        got = _mp().histogram(img, Pd, window)
        want = br.hist(seq.frames[0], field, window)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), _hist32(want))
        # the kernel adds to what the output holds
        again = _mp().histogram(img, Pd, window, got)
        assert again is got and torch.equal(got.cpu(), _hist32(2 * want))
    if window[2] > window[0] and window[3] > window[1]:
        assert want.sum() > 0


@pytest.fixture(scope='module')
def first_steps():
    """name -> (inputs, trace of the float64 restatement): computed once, shared, left unchanged."""
    out = {}
    for name in br.FIXTURES:
        f = br.first_step(name)
        tr = {}
        br.step(f['img_s'], f['img_t'], f['P_s'], f['flow_ts'], f['flow_st'], f['key_hist'], br.params(), trace=tr)
        out[name] = (f, tr)
    return out


@pytest.mark.parametrize('name', br.FIXTURES)
def test_unary_and_every_meanfield_iteration_against_the_restatement(cuda, first_steps, name):
    f, tr = first_steps[name]
    p = br.params()
    mp = _mp()
    img_s, img_t, P_s, fts, fst = _dev(cuda, f['img_s'], f['img_t'], f['P_s'], f['flow_ts'], f['flow_st'])
    hist = _hist32(f['key_hist']).to(cuda)
    mp.histogram(img_s, P_s, tr['window'], hist, p['hi'], p['lo'])
    assert torch.equal(hist.cpu(), _hist32(tr['hist']))
    u, q0 = mp.unary(img_t, P_s, fts, fst, hist, p['tau'], p['w_p'], p['w_a'], p['eps'], p['U'])
    qs = mp.meanfield(img_t, u, q0, p['K'], p['R'], p['sigma_i'], p['sigma_s'], p['w_s'], every=True)
    torch.cuda.synchronize()
    errs = {'u': np.abs(u.cpu().numpy() - tr['u']).max(), 'q0': np.abs(q0.cpu().numpy() - tr['q'][0]).max()}
    for k, q in enumerate(qs, 1):
        errs[k] = np.abs(q.cpu().numpy() - tr['q'][k]).max()
    print(name, {k: '%.3g (bound %.3g)' % (v, 8 * SPREAD[k]) for k, v in errs.items()})
    assert len(qs) == 5
    for k, v in errs.items():
        assert v <= 8 * SPREAD[k], (name, k, v)
    und = undecided(name)
    assert (((qs[-1].cpu().numpy() > 0.5) == (tr['q'][-1] > 0.5)) | und).all()
    # the step of the host layer is these launches
    q = mp.step(img_s, img_t, P_s, fts, fst, _hist32(f['key_hist']).to(cuda), p)
    assert torch.equal(q, qs[-1])
    # a radius of 0 has no neighbours, K = 0 launches nothing
    q_r0 = mp.meanfield(img_t, u, q0, 1, 0)
    assert np.abs(q_r0.cpu().numpy() - tr['q'][0]).max() <= 8 * SPREAD['q0']
    assert torch.equal(mp.meanfield(img_t, u, q0, 0), q0)


@pytest.mark.parametrize('R', [1, 8])
def test_meanfield_other_radii_on_cut_tiles(cuda, first_steps, R):
    # odd: 37 x 53 against 32 x 8 tiles; R = 8 is the largest halo, wider than tiny itself.  One iteration of the restatement in
    # float32 and in float64 from the same float32 u and q0 differs by at most 8.5e-8 (odd R 1; 8.1e-8 odd R 8, 6.9e-8 tiny): 8 x.
    for name in ('odd', 'tiny'):
        f, tr = first_steps[name]
        p = br.params(R=R)
        img, u, q0 = _dev(cuda, f['img_t'], tr['u'].astype(np.float32), tr['q'][0].astype(np.float32))
        got = _mp().meanfield(img, u, q0, 1, R).cpu().numpy()
        want = br.meanfield(f['img_t'], tr['u'].astype(np.float32), tr['q'][0].astype(np.float32), p)
        err = np.abs(got - want).max()
        print(name, R, err)
        assert err <= 8 * 8.5e-8


@pytest.fixture(scope='module')
def restated_full():
    out = {}
    for name in ('ellipse', 'ellipse_noisy', 'border'):
        seq, k = br.fixture(name), br.KEYS[name]
        out[name] = br.propagate(seq.frames, {k: seq.masks[k]}, seq.flow)
    return out


@pytest.mark.parametrize('name', ['ellipse', 'ellipse_noisy', 'border'])
def test_full_propagation_matches_the_restatement_and_the_truth(cuda, restated_full, name):
    seq, k = br.fixture(name), br.KEYS[name]
    want_masks, want_soft = restated_full[name]
    masks, soft, report = _mp().propagate(seq.frames, {k: seq.masks[k]}, seq.flow_fn)
    assert masks.dtype == bool and soft.dtype == np.float32 and masks.shape == soft.shape == seq.masks.shape
    und = np.abs(want_soft - 0.5) <= Q_TOL
    ious = [br.iou(masks[t], seq.masks[t]) for t in range(seq.T)]
    print(name, 'max |soft - restated| %.3g' % np.abs(soft - want_soft).max(), 'undecided', int(und.sum()), ['%.3f' % v for v in ious])
    assert ((masks == want_masks) | und).all()
    assert min(ious) >= 0.95
    assert (masks[k] == seq.masks[k]).all() and report['areas'] == [int(m.sum()) for m in masks] and report['keys'] == [k]
    assert report['flow_pairs'] == 2 * (seq.T - 1)                                    # every ordered pair once


def test_two_calls_give_the_same_bits_and_two_keys_blend(cuda):
    seq = br.fixture('ellipse_noisy')
    a = _mp().propagate(seq.frames, {0: seq.masks[0]}, seq.flow_fn)
    b = _mp().propagate(seq.frames, {0: seq.masks[0]}, seq.flow_fn)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
    seq = br.fixture('ellipse')
    masks, soft, _ = _mp().propagate(list(seq.frames), {0: seq.masks[0], 7: seq.masks[7]}, seq.flow_fn)
    want_masks, want_soft = br.propagate(seq.frames, {0: seq.masks[0], 7: seq.masks[7]}, seq.flow)
    und = np.abs(want_soft - 0.5) <= Q_TOL
    assert ((masks == want_masks) | und).all() and (masks[0] == seq.masks[0]).all() and (masks[7] == seq.masks[7]).all()
    assert min(br.iou(masks[t], seq.masks[t]) for t in range(8)) >= 0.95
    assert _mp().roundtrip(seq.frames, 0, seq.masks[0], seq.flow_fn) >= 0.95


def test_an_empty_propagated_mask_is_a_named_error(cuda):
    seq = br.fixture('ellipse')
    away = lambda a, b: (np.full((seq.H, seq.W, 2), 1000., np.float32), None)         # noqa: E731
    with pytest.raises(_mp().EmptyPropagation, match='frame 1') as e:
        _mp().propagate(seq.frames, {0: seq.masks[0]}, away, w_a=0.)
    assert e.value.frame == 1


def test_script_end_to_end_then_auto_gen(cuda, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'preprocess'))
    import auto_gen
    import propagate_mask as pm
    seq = br.fixture('ellipse')
    datapath, key = write_video(seq, tmp_path)
    args = pm.parse_args(['--datapath', datapath, '--key', '0:' + key, '--min_area', '100', '--roundtrip'])
    report = pm.run(args, seq.flow_fn)
    out = pm.annotations_dir(datapath)
    assert sorted(os.listdir(out)) == ['%05d.png' % t for t in range(8)] + ['maskprop.json']
    assert report['roundtrip_iou'] >= 0.95
    for t in range(8):
        assert br.iou(auto_gen.read_mask(os.path.join(out, '%05d.png' % t)), seq.masks[t]) >= 0.95
    kept = auto_gen.run(auto_gen.parse_args(['--datapath', datapath, '--outdir', str(tmp_path / 'out')]), seq.flow_fn)
    assert kept == [(t, t + 1) for t in range(7)]
