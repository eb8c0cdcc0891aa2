"""Motion segmentation on the device (lasr_amd/nnutils/motionseg.py, csrc/motionseg.hip) against the float64 restatement
(tests/motionseg_restated.py).  The segmentation is this project's own addition: the restatement is the only parity there is.

Tolerances follow the rule of tests/test_maskprop_gpu.py: for each compared quantity the restatement itself is run with float32
and with float64 per-pixel arithmetic on the CPU (tests/test_motionseg_cpu.py: restated, sequence_restated; computed when the tests
run, and printed), and 8 x the largest difference is allowed, because the kernel's expf differs from numpy's.  Two bounds cannot
come from that spread alone, and come from the number formats instead:
  - a float64 sum of n terms taken in another order (lanes, waves, workgroups against numpy's pairwise sum) differs by up to
    n 2^-53 sum |term|; that is added to every moment's bound, and is the whole bound from the initial state, where w = conf in
    both precisions and the spread is exactly 0;
  - theta solves an 8 x 8 system whose matrix carries that rounding: cond(A) n 2^-53 max |theta| is added to theta's bound.
No figure comes from the kernel.  Spreads of the restatement on the CPU (float32 against float64):
  conf 2.9e-6 (holes; odd 1.8e-6, tiny 2.0e-7); evidence 1.0e-6 (odd; tiny and holes 2.4e-7); moments from the mid-fit state at
  most 1.3e-8 of sum |term| on pan, odd, large and holes and 4.9e-8 on tiny (largest absolute 2.3e-3, large); theta after 8
  iterations 6.6e-13 (pan), 1.0e-8 (odd), 1.9e-11 (tiny), 5.9e-9 (large), 6.3e-14 (holes), sigma equal; q after the mean field
  3.1e-7 (pan) and 3.7e-7 (pan_noisy), no pixel of either within 8 x that of 0.5.
Histogram pixels whose float64 16 r lies within 1e-5 of an integer >= 1: 0 to 2 per fixture and state (test_motionseg_cpu.py).
The restatement alone, on the CPU: thresholded-evidence IoU 1.000 on every pair of pan and pan_noisy, theta of pan 1.2e-5 px from
the truth; on the PanSequence fixtures the key masks and every propagated mask have IoU 1.000 against the truth.

Measured on an MI355X (every test prints its figures before it asserts): the kernels round as the float32 restatement does.
conf 1.8e-6 (odd, bound 1.4e-5), 1.4e-7 (tiny, bound 1.6e-6), 3.0e-6 (holes, bound 2.3e-5); evidence 1.0e-6 / 2.4e-7 / 2.4e-7
(bounds 8.3e-6 / 1.9e-6 / 1.9e-6); moments from the initial state at most 3.4 % of their rounding bound (tiny; largest absolute
error 4.7e-10, large), from the mid-fit state exactly the float32 spread, an eighth of the bound; histograms equal to the float32
restatement's, no count moved; theta after 8 iterations 6.6e-13 (pan, bound 2.2e-11), 1.0e-8 (odd, 8.3e-8), 1.9e-11 (tiny,
1.5e-10), 5.9e-9 (large, 4.8e-8), 6.3e-14 (holes, 1.7e-11), sigma and n equal, pan theta 1.1e-5 px from the truth; segment: q within
3.1e-7 (pan) and 3.7e-7 (pan_noisy) of the restatement, no mask pixel differs, keys 6 and 1 as the restatement's, every written
mask of the end-to-end runs IoU 1.000, 14 flow calls each.  The 21 tests take 7 s.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import maskprop_restated as mr
import motionseg_restated as ms
from test_motionseg_cpu import KERNEL_CASES, moment_bounds, restated, sequence_restated, sequence_spread, write_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def _ms():
    from lasr_amd.nnutils import motionseg
    return motionseg


def _dev(cuda, *arrays):
    out = [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]
    return out[0] if len(out) == 1 else out


@pytest.mark.parametrize('name', ['odd', 'tiny', 'holes'])
def test_conf_and_evidence_against_the_restatement(cuda, name):
    r = restated(name)
    f, fb = _dev(cuda, r['flow'], r['back'])
    conf = _ms().confidence(f, fb).cpu().numpy()
    c_spread = np.abs(r['conf32'] - r['conf64']).max()
    c_err = np.abs(conf - r['conf64']).max()
    S = r['fit'][F64]
    e = _ms().evidence(f, _dev(cuda, r['conf32']), _dev(cuda, S)).cpu().numpy()
    e_spread = np.abs(r['evidence'][F32] - r['evidence'][F64]).max()
    e_err = np.abs(e - r['evidence'][F64]).max()
    print(name, 'conf %.3g (bound %.3g), evidence %.3g (bound %.3g)' % (c_err, 8 * c_spread, e_err, 8 * e_spread))
    assert conf.dtype == np.float32 and np.isfinite(conf).all() and np.isfinite(e).all()
    assert c_err <= 8 * c_spread and e_err <= 8 * e_spread
    assert ((conf == 0) == (r['conf64'] == 0)).all()
    # accumulate = 1 adds to what the output holds
    twice = _ms().evidence(f, _dev(cuda, r['conf32']), _dev(cuda, S), out=torch.from_numpy(e).to(cuda))
    assert np.array_equal(twice.cpu().numpy(), e + e)


@pytest.mark.parametrize('name', KERNEL_CASES)
def test_moments_and_histogram_from_the_initial_and_a_mid_fit_state(cuda, name):
    from lasr_amd import _lib
    r = restated(name)
    f, conf = _dev(cuda, r['flow'], r['conf32'])
    H, W = r['flow'].shape[:2]
    blocks = min(_lib.MOTIONSEG_BLOCKS, (H * W + 255) // 256)
    for key in ('initial', 'mid'):
        S = r['states'][key]
        partials = torch.full((_lib.MOTIONSEG_BLOCKS, _lib.MOTIONSEG_MOMENTS), float('nan'), dtype=torch.float64, device=cuda)
        partials, hist = _ms().moments(f, conf, _dev(cuda, S), partials=partials)
        P = partials.cpu().numpy()
        M = np.zeros(ms.MOMENTS)
        for row in P:                                       # the fold of lasr_motionseg_solve: rows in index order
            M = M + row
        bound, spread = moment_bounds(name, key)
        err = np.abs(M - r[key][F64][0])
        h = hist.cpu().numpy().astype(np.int64)
        near = ms.near_integer(r['flow'], r['conf32'], S)
        moved = int(np.abs(h - r[key][F32][1]).sum())
        print(name, key, 'moments: worst error / bound %.3g (largest error %.3g, largest spread %.3g); histogram: %d counts moved, %d '
              'pixels near an integer, n %d' % ((err / np.maximum(bound, 1e-300)).max(), err.max(), spread.max(), moved, near, h.sum()))
        assert np.isfinite(P).all() and (P[blocks:] == 0).all()                   # the rows of workgroups that do not exist
        assert (err <= bound).all()
        assert h.sum() == r[key][F32][1].sum() and moved <= 2 * near and near <= 0.001 * h.sum()
        # the histogram is added to: a second launch on the same buffer doubles it
        _lib.call('lasr_motionseg_moments', f, conf, _dev(cuda, S), partials, hist, H, W)
        assert np.array_equal(hist.cpu().numpy(), 2 * h) and np.array_equal(partials.cpu().numpy(), P)


def _theta_bound(name, **over):
    """8 x the float32 / float64 spread of theta + cond(A) n 2^-53 max |theta| (header), from the restatement's last iteration.
    A is the full 8 x 8 matrix: a model that switches parameters off solves a principal block of it, whose condition is no worse."""
    r = restated(name)
    S32, S64 = (ms.fit(r['flow'], r['conf32'], ms.params(**over), dt) for dt in (F32, F64)) if over else (r['fit'][F32], r['fit'][F64])
    states = []
    ms.fit(r['flow'], r['conf32'], ms.params(iters=7, **over), states=states)
    A, _ = ms.assemble(ms.moments(r['flow'], r['conf32'], states[-1])[0])
    n = r['flow'].shape[0] * r['flow'].shape[1]
    return 8 * np.abs(S32[ms.TH] - S64[ms.TH]).max() + np.linalg.cond(A) * n * 2. ** -53 * np.abs(S64[ms.TH]).max()


@pytest.mark.parametrize('name', KERNEL_CASES)
def test_whole_fit_theta_sigma_status_and_two_calls_give_the_same_bits(cuda, name):
    r = restated(name)
    f, conf = _dev(cuda, r['flow'], r['conf32'])
    S = _ms().fit(f, conf)
    again = _ms().fit(f, conf)
    e, e2 = _ms().evidence(f, conf, S), _ms().evidence(f, conf, again)
    got, want = S.cpu().numpy(), r['fit'][F64]
    bound = _theta_bound(name)
    err = np.abs(got[ms.TH] - want[ms.TH]).max()
    print(name, 'theta %.3g (bound %.3g), sigma %g / %g, n %d / %d, status %d' % (err, bound, got[ms.SIGMA], want[ms.SIGMA], got[ms.N],
                                                                                 want[ms.N], got[ms.STATUS]))
    assert S.dtype == torch.float64 and tuple(S.shape) == (12,) and np.isfinite(got).all()
    assert err <= bound and got[ms.STATUS] == want[ms.STATUS] == 0 and got[ms.N] == want[ms.N]
    assert abs(got[ms.SIGMA] - want[ms.SIGMA]) <= 8 * abs(r['fit'][F32][ms.SIGMA] - want[ms.SIGMA])
    assert abs(got[ms.MED] - want[ms.MED]) <= 8 * abs(r['fit'][F32][ms.MED] - want[ms.MED])
    assert torch.equal(S, again) and torch.equal(e, e2)
    if name == 'pan':
        truth = np.abs(got[ms.TH] - ms.flow_case('pan').theta).max()
        print('pan: |theta - truth| %.3g px' % truth)
        assert truth <= 1e-4
    # the fit is the launches it is made of, continued from a state
    half = _ms().fit(f, conf, iters=3)
    assert torch.equal(_ms().fit(f, conf, iters=5, state=half), S)


@pytest.mark.parametrize('model', ['translation', 'affine'])
def test_model_switch_on_the_device(cuda, model):
    r = restated('odd')
    f, conf = _dev(cuda, r['flow'], r['conf32'])
    got = _ms().fit(f, conf, model=model).cpu().numpy()
    want = ms.fit(r['flow'], r['conf32'], ms.params(model=model))
    off = [k for k in range(8) if k not in ms.ENABLED[ms.MODELS[model]]]
    err, bound = np.abs(got[ms.TH] - want[ms.TH]).max(), _theta_bound('odd', model=model)
    print(model, 'theta %.3g (bound %.3g)' % (err, bound))
    assert all(got[k] == 0 for k in off) and got[ms.STATUS] == 0 and err <= bound


def test_holes_are_skipped_not_weighted_and_all_skipped_is_degenerate(cuda):
    f_np, fb_np, bad = ms.holes()
    clean_np = ms.flow_case('pan').pair(0, 1)[0]
    f, fb, clean = _dev(cuda, f_np, fb_np, clean_np)
    conf = _ms().confidence(f, fb)
    assert (conf.cpu().numpy()[bad] == 0).all()
    # the bad pixels' conf is 0: the same bits as the clean field with that conf
    a, b = _ms().fit(f, conf), _ms().fit(clean, conf)
    pa, ha = _ms().moments(f, conf, a)
    pb, hb = _ms().moments(clean, conf, a)
    assert torch.equal(a, b) and torch.equal(pa, pb) and torch.equal(ha, hb)
    assert torch.isfinite(a).all() and torch.isfinite(pa).all() and torch.isfinite(_ms().evidence(f, conf, a)).all()
    # a flow that is not finite is skipped whatever its conf: conf 1 everywhere against conf 0 on those pixels of a finite field
    ones = torch.ones_like(conf)
    finite = np.isfinite(f_np).all(-1)
    zeroed = _dev(cuda, np.where(finite[..., None], f_np, np.float32(0)))
    c, d = _ms().fit(f, ones), _ms().fit(zeroed, _dev(cuda, finite.astype(np.float32)))
    e = _ms().evidence(f, ones, c)
    assert torch.equal(c, d) and torch.isfinite(c).all() and torch.isfinite(e).all() and (e.cpu().numpy()[~finite] == 0).all()
    print('holes: theta', a.cpu().numpy()[:8], 'n', int(a[10]))
    f_all, fb_all, _ = ms.holes('all')
    f_all, fb_all = _dev(cuda, f_all, fb_all)
    conf = _ms().confidence(f_all, fb_all)
    S = _ms().fit(f_all, conf).cpu().numpy()
    print('all skipped: state', S)
    assert (conf == 0).all() and S[ms.STATUS] == 1 and S[ms.N] == 0 and (S[ms.TH] == 0).all() and np.isinf(S[ms.SIGMA])
    assert (_ms().evidence(f_all, conf, _dev(cuda, S)) == 0).all()


@pytest.fixture(scope='module')
def segmented(cuda):
    """name -> segment's result on the device, computed once, shared, left unchanged."""
    out = {}
    for name in ('pan', 'pan_noisy'):
        seq = ms.sequence(name)
        seq.calls.clear()
        out[name] = _ms().segment(seq.frames, seq.flow_fn) + (list(seq.calls),)
    return out


@pytest.mark.parametrize('name', ['pan', 'pan_noisy'])
def test_segment_matches_the_restatement_and_the_truth(cuda, segmented, name):
    seq = ms.sequence(name)
    masks, soft, scores, report, calls = segmented[name]
    want_masks, want_soft, want_scores, want_rep = sequence_restated(name)[F64]
    spread, _ = sequence_spread(name)
    und = np.abs(want_soft - 0.5) <= 8 * spread
    keys, want_keys = _ms().select_keys(list(scores), report['params']), ms.select_keys(list(want_scores), want_rep['params'])
    ious = [mr.iou(masks[t], seq.masks[t]) for t in range(seq.T)]
    print(name, 'max |soft - restated| %.3g (mean-field bound %.3g), undecided %d, max |score - restated| %.3g, keys %s / %s, IoU %s' % (
        np.abs(soft - want_soft).max(), 8 * spread, int(und.sum()), np.abs(scores - want_scores).max(), keys, want_keys,
        ['%.3f' % v for v in ious]))
    assert masks.dtype == bool and soft.dtype == np.float32 and masks.shape == soft.shape == seq.masks.shape
    q_agree = ((soft > 0.5) == (want_soft > 0.5)) | und
    assert q_agree.all()
    assert all((masks[t] == want_masks[t]).all() for t in range(seq.T) if not und[t].any())
    assert keys == want_keys and mr.iou(masks[keys[0]], seq.masks[keys[0]]) >= 0.95
    assert len(report['pairs']) == 14 and all(p['status'] == 0 for p in report['pairs']) and report['flow_pairs'] == 14
    assert sorted(calls) == sorted(set(calls)) and len(calls) == 14                 # every ordered pair once
    again = _ms().segment(seq.frames, seq.flow_fn)
    assert np.array_equal(again[0], masks) and np.array_equal(again[1], soft) and np.array_equal(again[2], scores)
    assert {t: m.tolist() for t, m in _ms().auto_keys(seq.frames, seq.flow_fn).items()} == {keys[0]: masks[keys[0]].tolist()}


def test_nothing_moves_is_a_named_error(cuda):
    seq = ms.sequence('pan')
    still = lambda a, b: (np.zeros(a.shape[:2] + (2,), np.float32), None)         # noqa: E731
    with pytest.raises(_ms().NoMovingObject):
        _ms().auto_keys(seq.frames, still)


@pytest.mark.parametrize('name', ['pan', 'pan_noisy'])
def test_script_end_to_end_then_auto_gen_and_the_flows_are_not_computed_twice(cuda, tmp_path, name):
    sys.path.insert(0, os.path.join(ROOT, 'preprocess'))
    import auto_gen
    import auto_mask as am
    import propagate_mask as pm
    seq = ms.sequence(name)
    datapath = write_frames(seq, tmp_path, name)
    seq.calls.clear()
    block = am.run(am.parse_args(['--datapath', datapath, '--min_area', '100']), seq.flow_fn)
    calls = list(seq.calls)
    out = pm.annotations_dir(datapath)
    ious = [mr.iou(auto_gen.read_mask(os.path.join(out, '%05d.png' % t)), seq.masks[t]) for t in range(seq.T)]
    print(name, 'keys', block['keys'], 'IoU of the written masks', ['%.3f' % v for v in ious], 'flow calls', len(calls))
    assert sorted(os.listdir(out)) == ['%05d.png' % t for t in range(8)] + ['maskprop.json']
    assert sorted(os.listdir(out + '.autokeys')) == ['key-%05d.png' % t for t in block['keys']]
    assert min(ious) >= 0.90
    assert sorted(calls) == sorted(set(calls)) and len(calls) == 14 == block['flow_calls']      # not doubled by the hand-over
    saved = json.load(open(os.path.join(out, 'maskprop.json')))
    assert saved['motion'] == json.loads(json.dumps(block)) and saved['keys'] == block['keys'] and len(saved['motion']['pairs']) == 14
    kept = auto_gen.run(auto_gen.parse_args(['--datapath', datapath, '--outdir', str(tmp_path / 'out')]), seq.flow_fn)
    assert kept == [(t, t + 1) for t in range(7)]
