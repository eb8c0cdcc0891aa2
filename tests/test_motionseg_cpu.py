"""Motion segmentation without a device: the float64 restatement (tests/motionseg_restated.py) on its analytic fixtures and on
closed forms, the C ABI's host-side checks, the python layer's refusals, and the argument handling and file layout of
preprocess/auto_mask.py driven with stand-ins for the device passes."""
import json
import os
import re
import sys

import numpy as np
import pytest

import maskprop_restated as mr
import motionseg_restated as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'preprocess'))


def _fit(case, a, b, dtype=np.float32, **over):
    f, fb = case.pair(a, b, dtype)
    conf = ms.confidence(f, fb)
    S = ms.fit(f, conf, ms.params(**over))
    return f, conf, S


# ---- known answers of the restatement ---------------------------------------------------------------------------------------------

def test_plain_recovers_theta_to_rounding():
    case = ms.flow_case('plain')
    _, conf, S = _fit(case, 0, 1, np.float64)
    err = np.abs(S[ms.TH] - case.theta).max()
    print('plain: max |theta - truth| %.3g, sigma %g, n %d' % (err, S[ms.SIGMA], S[ms.N]))     # measured: 3.1e-16
    assert err <= 1e-9 and S[ms.STATUS] == 0 and S[ms.SIGMA] == 0.25


@pytest.mark.parametrize('name', ['pan', 'pan_noisy'])
def test_thresholded_evidence_is_the_object_on_every_pair(name):
    case = ms.flow_case(name)
    worst_iou, worst_th = 1., 0.
    for a in range(case.T):
        for b in (a - 1, a + 1):
            if not 0 <= b < case.T:
                continue
            f, conf, S = _fit(case, a, b)
            e = ms.evidence(f, conf, S)
            worst_iou = min(worst_iou, mr.iou(e > 0, case.masks[a]))
            if b > a:                                       # the flow back is the model's inverse, not the model: 0.06 px off
                worst_th = max(worst_th, np.abs(S[ms.TH] - case.theta).max())
            assert S[ms.STATUS] == 0
    print(name, 'worst IoU %.4f, worst |theta - truth| forward %.3g' % (worst_iou, worst_th))
    # measured: pan 1.0000 and 1.2e-5 px; pan_noisy 1.0000 and 0.27 px (the noise is smooth, 0.5 px in amplitude)
    assert worst_iou >= 0.95
    if name == 'pan':
        assert worst_th <= 1e-4


def test_all_skipped_is_degenerate_with_zero_evidence_and_holes_change_nothing_else():
    f, fb, bad = ms.holes('all')
    conf = ms.confidence(f, fb)
    assert (conf == 0).all()
    S = ms.fit(f, conf)
    assert S[ms.STATUS] == 1 and S[ms.N] == 0 and (S[ms.TH] == 0).all() and np.isinf(S[ms.SIGMA])
    assert (ms.evidence(f, conf, S) == 0).all()
    f, fb, bad = ms.holes()
    conf = ms.confidence(f, fb)
    assert (conf[bad] == 0).all() and (conf[~bad] > 0).mean() > 0.9
    S = ms.fit(f, conf)
    e = ms.evidence(f, conf, S)
    assert np.isfinite(S).all() and np.isfinite(e).all() and (e[bad] == 0).all()
    assert np.abs(S[ms.TH] - ms.flow_case('pan').theta).max() <= 1e-4
    # the same sums as with the bad pixels' conf set to 0 by hand on a clean field
    clean = np.where(bad[..., None], np.float32(0), f)
    M0, h0 = ms.moments(f, conf, S)
    M1, h1 = ms.moments(clean, np.where(bad, 0, conf), S)
    assert (M0 == M1).all() and (h0 == h1).all()


@pytest.mark.parametrize('model,off', [('translation', (1, 2, 4, 5, 6, 7)), ('affine', (6, 7)), ('quadratic', ())])
def test_a_switched_off_parameter_stays_zero(model, off):
    case = ms.flow_case('pan')
    _, _, S = _fit(case, 0, 1, model=model)
    assert S[ms.STATUS] == 0 and all(S[k] == 0 for k in off) and all(S[k] != 0 for k in range(8) if k not in off)


def test_moments_and_solve_closed_forms():
    # a constant flow (3, -2) with conf 1: theta = (3, 0, 0, -2, 0, ...), residual 0 afterwards, med = half a bin
    H, W = 6, 9
    f = np.zeros((H, W, 2))
    f[..., 0], f[..., 1] = 3., -2.
    conf = np.ones((H, W))
    S0 = ms.initial_state()
    M, h = ms.moments(f, conf, S0)
    X, Y = ms.coords(H, W)
    assert M[0] == H * W and abs(M[1]) < 1e-12 and abs(M[2]) < 1e-12 and abs(M[3] - (X * X).sum()) < 1e-12
    assert abs(M[14] - (Y ** 4).sum()) < 1e-12 and M[15] == 3 * H * W and M[21] == -2 * H * W and M[27] == 13 * H * W
    assert h.sum() == H * W and h[int(16 * np.sqrt(13.))] == H * W
    S1 = ms.solve(M, h, S0)
    # the first step carries the ridge's bias, ridge * trace / 8 against the smallest eigenvalue; the second removes it
    assert np.abs(S1[ms.TH] - [3, 0, 0, -2, 0, 0, 0, 0]).max() < 1e-7 and S1[ms.N] == H * W and S1[ms.STATUS] == 0
    assert S1[ms.MED] == (int(16 * np.sqrt(13.)) + 0.5) / 16 and S1[ms.SIGMA] == 3 * S1[ms.MED]      # the scale is lagged
    M, h = ms.moments(f, conf, S1)
    S2 = ms.solve(M, h, S1)
    assert h[0] == H * W and S2[ms.MED] == 0.5 / 16 and S2[ms.SIGMA] == 0.25
    assert np.abs(S2[ms.TH] - [3, 0, 0, -2, 0, 0, 0, 0]).max() < 1e-12
    # the median bin: counts 3, 0, 4 -> ceil(7 / 2) = 4 is reached in bin 2
    hh = np.zeros(ms.BINS, np.int64)
    hh[0], hh[2] = 3, 4
    assert ms.solve(M, hh, S1)[ms.MED] == 2.5 / 16
    hh[0] = 4
    assert ms.solve(M, hh, S1)[ms.MED] == 0.5 / 16
    # conf outside the frame, and exp(-2) where the flows disagree by 2 px
    fb = np.zeros((H, W, 2))
    fb[..., 0], fb[..., 1] = -1., 2.
    c = ms.confidence(f, fb)
    inside = (np.arange(W)[None] + 3 <= W - 1) & (np.arange(H)[:, None] - 2 >= 0)
    assert np.abs(c[inside] - np.exp(-2.)).max() < 1e-15 and (c[~inside] == 0).all()
    # evidence: residual 0 gives -kappa conf, a large one +U conf
    e = ms.evidence(f, conf * 0.5, S2)
    assert np.abs(e + 2.).max() < 1e-9
    assert (ms.evidence(f + 5., conf * 0.5, S2) == 3.).all()


def test_key_selection_spacing_ties_min_score_and_no_moving_object():
    p = ms.params(n_keys=3, min_spacing=3, min_score=1.)
    assert ms.select_keys([0, 5, 9, 8, 2, 2, 7, 0.5], p) == [2, 6]                 # 3 is within 3 of 2; then 1, 4, 5 likewise
    assert ms.select_keys([0, 5, 9, 8, 2, 2, 7, 0.5], ms.params(n_keys=3, min_spacing=2)) == [2, 4, 6]   # the tie 4 / 5 goes to 4
    assert ms.select_keys([3, 3, 3], ms.params(n_keys=1)) == [0]
    assert ms.select_keys([3, 3, 3, 3], ms.params(n_keys=2, min_spacing=1)) == [0, 1]
    assert ms.select_keys([0.5, 4, 0.9], ms.params(n_keys=3, min_spacing=0)) == [1]                      # stops at min_score
    with pytest.raises(ms.NoMovingObject):
        ms.select_keys([0.2, 0.99, 0.], ms.params())
    with pytest.raises(ms.NoMovingObject):
        ms.select_keys([], ms.params())
    from lasr_amd.nnutils import motionseg
    for scores, over in (([0, 5, 9, 8, 2, 2, 7, 0.5], dict(n_keys=3, min_spacing=3)), ([3, 3, 3, 3], dict(n_keys=2, min_spacing=1))):
        assert motionseg.select_keys(scores, motionseg.params(**over)) == ms.select_keys(scores, ms.params(**over))
    with pytest.raises(motionseg.NoMovingObject):
        motionseg.select_keys([0.2], motionseg.params())
    assert issubclass(motionseg.NoMovingObject, ValueError)
    # the score: a blob away from the rim, one on it, one too large
    u = -np.ones((20, 30))
    P = np.zeros((20, 30), bool)
    P[5:10, 5:12] = True
    u[P] = 4.
    assert ms.score(u, P, True, ms.params()) == motionseg.score(u, P, True, motionseg.params()) == 5.
    assert ms.score(u, P, False, ms.params()) == 0.
    Q = np.zeros((20, 30), bool)
    Q[0:5, 5:12] = True                                                             # 7 of its 20 boundary pixels are on the rim
    assert abs(ms.score(u * 0 + Q * 5 - 1, Q, True, ms.params()) - 5 * (1 - 7 / 20)) < 1e-12
    assert motionseg.score(u * 0 + Q * 5 - 1, Q, True, motionseg.params()) == ms.score(u * 0 + Q * 5 - 1, Q, True, ms.params())
    big = np.ones((20, 30), bool)
    big[:, :10] = False
    assert ms.score(u, big, True, ms.params()) == 0. and ms.score(u, big & False, True, ms.params()) == 0.
    q = np.zeros((8, 8), bool)
    q[0:2, 0:2], q[4:7, 4:7], q[7, 7] = True, True, True                           # 8-connected: the speck joins the 3 x 3 block
    assert ms.largest_component(q).sum() == 10 and (motionseg.largest_component(q) == ms.largest_component(q)).all()
    assert not motionseg.largest_component(q & False).any()


@pytest.mark.parametrize('name', ['pan', 'pan_noisy'])
def test_restatement_segments_the_pan_sequence_and_the_propagation_follows(name):
    seq = ms.sequence(name)
    masks, soft, scores, rep = ms.segment(seq.frames, seq.flow)
    ious = [mr.iou(masks[t], seq.masks[t]) for t in range(seq.T)]
    keys = ms.select_keys(list(scores), rep['params'])
    print(name, 'scores', np.round(scores, 2), 'IoU', ['%.3f' % v for v in ious], 'keys', keys)
    # measured: IoU 1.000 on every frame of both; scores 19.0-19.2 inside, 9.5 on the two end frames (one pair); keys [6] and [1]
    assert len(keys) == 1 and ious[keys[0]] >= 0.95 and scores.min() > 1
    got, _ = mr.propagate(seq.frames, {k: masks[k] for k in keys}, seq.flow)
    assert min(mr.iou(got[t], seq.masks[t]) for t in range(seq.T)) >= 0.90       # measured: 1.000
    # the background flow is closed form and inside the affine model
    bg = seq.background_flow(2, 3)
    X, Y = ms.coords(seq.H, seq.W)
    A = np.stack([np.ones_like(X), X, Y], -1).reshape(-1, 3)
    for ch in range(2):
        coef = np.linalg.lstsq(A, bg[..., ch].ravel(), rcond=None)[0]
        assert np.abs(A @ coef - bg[..., ch].ravel()).max() < 1e-10


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

NAMES = ('lasr_motionseg_conf', 'lasr_motionseg_moments', 'lasr_motionseg_solve', 'lasr_motionseg_evidence')


def test_header_and_binding_agree_on_the_four_entry_points():
    from lasr_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    kinds = {'int': _lib._i, 'float': _lib._f}
    for name in NAMES:
        args = re.search(r'int\s+%s\s*\((.*?)\)\s*;' % name, hdr, re.S).group(1)
        want = [_lib._p if '*' in a else kinds[a.split()[0]] for a in args.split(',')]
        res, got = _lib.SIGNATURES[name]
        assert res is _lib._i and got == want and want[-1] is _lib._p, name
    for name, value in (('MAX_SIZE', 16384), ('BLOCKS', 256), ('MOMENTS', 28), ('BINS', 1024), ('STATE', 12)):
        assert '#define LASR_MOTIONSEG_%s %d\n' % (name, value) in hdr and getattr(_lib, 'MOTIONSEG_' + name) == value
    assert (ms.MOMENTS, ms.BINS, ms.STATE) == (_lib.MOTIONSEG_MOMENTS, _lib.MOTIONSEG_BINS, _lib.MOTIONSEG_STATE)
    assert _lib.ABI_VERSION == 13
    assert 'lasr_motionseg' in open(os.path.join(ROOT, 'lasr_amd', 'csrc', 'GNUmakefile')).read().replace('motionseg.o', 'lasr_motionseg')


def test_symbols_are_exported_and_the_host_checks_run_without_a_device():
    from lasr_amd import _lib
    h = _lib.lib()
    assert h.lasr_abi_version() == 13
    n, a, b, c, d, e = None, 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20          # any non-null addresses; no launch reads them
    nan, inf = float('nan'), float('inf')

    def conf(H=8, W=9, tau=1., p=(n, n, n)):
        return h.lasr_motionseg_conf(p[0], p[1], p[2], H, W, tau, n)
    assert conf() == -1 and conf(H=0) == 0 and conf(W=0) == 0 and conf(H=0, W=0) == 0 and conf(H=-1) == -1 and conf(W=-2) == -1
    assert conf(H=16385, W=0) == -1 and conf(H=0, W=16385) == -1 and conf(H=16384, W=0) == 0
    assert conf(H=0, tau=0.) == -1 and conf(H=0, tau=-1.) == -1 and conf(H=0, tau=nan) == -1 and conf(H=0, tau=inf) == -1
    assert conf(p=(a, b, a)) == -1 and conf(p=(a, b, b)) == -1 and conf(p=(a, n, c)) == -1 and conf(tau=0., p=(a, b, c)) == -1

    def mom(H=8, W=9, p=(n, n, n, n, n)):
        return h.lasr_motionseg_moments(p[0], p[1], p[2], p[3], p[4], H, W, n)
    assert mom() == -1 and mom(H=0) == 0 and mom(W=0) == 0 and mom(H=-1) == -1 and mom(W=16385, H=0) == -1
    assert mom(p=(a, b, c, d, n)) == -1 and mom(p=(a, b, c, c, e)) == -1 and mom(p=(a, b, c, d, a)) == -1
    assert mom(p=(a, b, c, d, d)) == -1 and mom(p=(a, b, c, b, e)) == -1

    def sol(H=8, W=9, model=2, ks=3., smin=0.25, ridge=1e-9, p=(n, n, n)):
        return h.lasr_motionseg_solve(p[0], p[1], p[2], H, W, model, ks, smin, ridge, n)
    assert sol() == -1 and sol(H=0) == 0 and sol(W=0) == 0 and sol(H=-1) == -1 and sol(H=0, W=16385) == -1
    assert sol(H=0, model=-1) == -1 and sol(H=0, model=3) == -1 and all(sol(H=0, model=m) == 0 for m in (0, 1, 2))
    assert sol(H=0, ks=0.) == -1 and sol(H=0, ks=nan) == -1 and sol(H=0, smin=0.) == -1 and sol(H=0, smin=inf) == -1
    assert sol(H=0, ridge=-1e-9) == -1 and sol(H=0, ridge=nan) == -1 and sol(H=0, ridge=inf) == -1 and sol(H=0, ridge=0.) == 0
    assert sol(p=(a, b, a)) == -1 and sol(p=(a, b, b)) == -1 and sol(p=(a, b, n)) == -1 and sol(model=3, p=(a, b, c)) == -1

    def evi(H=8, W=9, kappa=4., U=6., acc=0, p=(n, n, n, n)):
        return h.lasr_motionseg_evidence(p[0], p[1], p[2], p[3], H, W, kappa, U, acc, n)
    assert evi() == -1 and evi(H=0) == 0 and evi(W=0) == 0 and evi(H=0, acc=1) == 0 and evi(H=-1) == -1 and evi(H=16385, W=0) == -1
    assert evi(H=0, acc=2) == -1 and evi(H=0, acc=-1) == -1 and evi(H=0, kappa=0.) == -1 and evi(H=0, kappa=nan) == -1
    assert evi(H=0, U=0.) == -1 and evi(H=0, U=inf) == -1 and evi(H=0, U=-6.) == -1
    assert evi(p=(a, b, c, a)) == -1 and evi(p=(a, b, c, b)) == -1 and evi(p=(a, b, c, c)) == -1 and evi(p=(a, b, c, n)) == -1
    assert evi(acc=2, p=(a, b, c, d)) == -1
    names = [h.lasr_prof_kernel_name(i) for i in range(h.lasr_prof_kernel_count())]
    assert not any(b'motionseg' in x for x in names)                              # the kernel-name table is not extended


def test_python_layer_refuses_cpu_tensors_and_unknown_parameters():
    import torch
    from lasr_amd.nnutils import motionseg
    f, c, S = torch.zeros(4, 5, 2), torch.zeros(4, 5), torch.zeros(12, dtype=torch.float64)
    with pytest.raises(TypeError):
        motionseg.confidence(f, f)
    with pytest.raises(TypeError):
        motionseg.fit(f, c)
    with pytest.raises(TypeError):
        motionseg.moments(f, c, S)
    with pytest.raises(TypeError):
        motionseg.evidence(f, c, S)
    with pytest.raises(TypeError):
        motionseg.confidence(np.zeros((4, 5, 2)), f)
    with pytest.raises(TypeError, match='unknown parameters'):
        motionseg.params(sigma=3.)
    with pytest.raises(ValueError):
        motionseg.params(model='homography')
    with pytest.raises(ValueError):
        motionseg.params(gap=0)
    assert motionseg.params() == ms.params() == motionseg.DEFAULTS and motionseg.params(gap=3)['gap'] == 3
    assert motionseg.MODELS == ms.MODELS
    calls = []

    def flow_fn(x, y):
        calls.append(1)
        return x.astype(np.float32) - y, None
    cached = motionseg.caching_flow_fn(flow_fn)
    x, y = np.arange(6, dtype=np.uint8).reshape(1, 2, 3), np.ones((1, 2, 3), np.uint8)
    r = cached(x, y)
    assert cached(x.copy(), y.copy())[0] is r[0] and len(calls) == 1 and cached.calls == 1
    cached(y, x)
    assert len(calls) == 2 and cached.calls == 2


# ---- the script -------------------------------------------------------------------------------------------------------------------

def test_script_arguments_are_the_defaults_of_the_two_layers():
    import auto_mask as am
    import propagate_mask as pm
    from lasr_amd.nnutils import motionseg
    d = 'database/DAVIS/JPEGImages/Full-Resolution/mine/'
    a = am.parse_args(['--datapath', d])
    assert am.motion_of(a) == motionseg.DEFAULTS and [m[0] for m in am.MOTION] == list(motionseg.DEFAULTS)
    assert pm.tuning_of(a) == mr.params() and a.flow_method == 'vcn' and a.loadmodel is None
    assert (a.testres, a.maxdisp, a.fac, a.min_area) == (1, 256, 1, 1000) and not (a.keys_only or a.roundtrip or a.force)
    assert am.key_dir(a) == 'database/DAVIS/Annotations/Full-Resolution/mine.autokeys'
    a = am.parse_args(('--datapath %s --flow_method variational --n_keys 2 --ms_gap 3 --ms_model affine --keys_only --roundtrip --min_area 10 '
                       '--force --ms_tau 2 --ms_iters 4 --ms_k_sigma 2.5 --ms_sigma_min 0.5 --ms_ridge 1e-6 --ms_kappa 3 --ms_U 5 '
                       '--ms_min_share 0.02 --ms_max_share 0.4 --ms_min_spacing 5 --ms_min_score 2 --K 3 --w_a 1 --keydir kk --vf_NW 3' % d).split())
    assert am.motion_of(a) == dict(tau=2., model='affine', iters=4, k_sigma=2.5, sigma_min=0.5, ridge=1e-6, kappa=3., U=5., gap=3,
                                   min_share=0.02, max_share=0.4, min_spacing=5, min_score=2., n_keys=2)
    assert a.keys_only and a.roundtrip and a.force and a.min_area == 10 and a.K == 3 and a.w_a == 1. and am.key_dir(a) == 'kk'
    assert a.flow_method == 'variational' and a.vf_NW == 3
    assert am.parse_args(['--datapath', d, '--ms_n_keys', '3']).ms_n_keys == 3
    # the printed command line is one propagate_mask.py accepts, with the same tuning
    pa = pm.parse_args(am.propagate_argv(a, {4: 'kk/key-00004.png', 17: 'kk/key-00017.png'}))
    assert pa.key == [(4, 'kk/key-00004.png'), (17, 'kk/key-00017.png')] and pm.tuning_of(pa) == pm.tuning_of(a)
    assert pa.flow_method == 'variational' and pa.vf_NW == 3 and pa.roundtrip and pa.force and pa.min_area == 10
    for bad in (['--ms_model', 'homography'], ['--flow_method', 'variational', '--loadmodel', 'x.pth'], ['--ms_sigma', '3']):
        with pytest.raises(SystemExit):
            am.parse_args(['--datapath', d] + bad)
    with pytest.raises(SystemExit):
        am.parse_args([])


def _restated_segment(seq):
    def segment(frames, flow_fn, **over):
        flow_of = lambda a, b: flow_fn(frames[a], frames[b])[0][..., :2]          # noqa: E731
        masks, soft, scores, rep = ms.segment(frames, flow_of, **over)
        pairs = [dict(frame=t, to=s, theta=list(S[ms.TH]), sigma=S[ms.SIGMA]) for (t, s), S in rep['states'].items()]
        return masks, soft.astype(np.float32), scores, dict(params=rep['params'], pairs=pairs)
    return segment


def _restated_propagate(frames, keys, flow_fn, **tuning):
    flow_of = lambda a, b: flow_fn(frames[a], frames[b])[0][..., :2]              # noqa: E731
    masks, soft = mr.propagate(frames, keys, flow_of, **tuning)
    return masks, soft.astype(np.float32), {}


def write_frames(seq, root, name='pan'):
    """The fixture as a DAVIS-layout folder of lossless frames.  -> datapath."""
    from PIL import Image
    d = os.path.join(str(root), 'DAVIS', 'JPEGImages', 'Full-Resolution', name)
    os.makedirs(d)
    for t, f in enumerate(seq.frames):
        Image.fromarray(f).save(os.path.join(d, '%05d.png' % t))
    return d + '/'


def test_script_writes_keys_annotations_and_the_motion_block(tmp_path, capsys):
    import auto_gen
    import auto_mask as am
    import propagate_mask as pm
    from PIL import Image
    seq = ms.sequence('pan')
    seq.calls.clear()
    datapath = write_frames(seq, tmp_path)
    out = pm.annotations_dir(datapath)
    args = am.parse_args(['--datapath', datapath, '--min_area', '100', '--keys_only'])
    block = am.run(args, seq.flow_fn, segment=_restated_segment(seq))
    want_key = block['keys'][0]
    assert block['keys'] == [6] and sorted(os.listdir(out + '.autokeys')) == ['key-%05d.png' % want_key]
    assert not os.path.exists(out)                                                # --keys_only writes no Annotations
    key = auto_gen.read_mask(os.path.join(out + '.autokeys', 'key-%05d.png' % want_key))
    assert mr.iou(key, seq.masks[want_key]) >= 0.95
    enc = np.asarray(Image.open(block['key_paths'][0]).convert('RGB'))
    assert set(np.unique(enc[..., 0])) == {0, 128} and not enc[..., 1:].any()     # the reference's encoding
    text = capsys.readouterr().out
    assert 'propagate_mask.py --datapath' in text and '--key %d:%s' % (want_key, block['key_paths'][0]) in text
    with pytest.raises(pm.AnnotationsExist, match='--force'):                     # the key folder is not overwritten unasked
        am.run(args, seq.flow_fn, segment=_restated_segment(seq))
    # the whole run: keys, propagation with the flows already computed, the motion block, and auto_gen.py next
    seq.calls.clear()
    args = am.parse_args(['--datapath', datapath, '--min_area', '100', '--force'])
    block = am.run(args, seq.flow_fn, segment=_restated_segment(seq), propagate=_restated_propagate)
    assert sorted(os.listdir(out)) == ['%05d.png' % t for t in range(8)] + ['maskprop.json']
    for t in range(8):
        assert mr.iou(auto_gen.read_mask(os.path.join(out, '%05d.png' % t)), seq.masks[t]) >= 0.90
    saved = json.load(open(os.path.join(out, 'maskprop.json')))
    assert saved['keys'] == [want_key] and saved['params'] == mr.params() and saved['motion'] == json.loads(json.dumps(block))
    m = saved['motion']
    assert m['params'] == ms.params() and len(m['scores']) == 8 and m['keys'] == [want_key] and len(m['pairs']) == 14
    assert all(len(p['theta']) == 8 and p['sigma'] >= 0.25 for p in m['pairs'])
    assert sorted(seq.calls) == sorted(set(seq.calls)) and len(seq.calls) == 14 == m['flow_calls']     # every ordered pair once
    kept = auto_gen.run(auto_gen.parse_args(['--datapath', datapath, '--outdir', str(tmp_path / 'out')]), seq.flow_fn)
    assert kept == [(t, t + 1) for t in range(7)]
    # a second run refuses the Annotations folder before it computes anything
    seq.calls.clear()
    args.force = False
    with pytest.raises(pm.AnnotationsExist):
        am.run(args, seq.flow_fn, segment=_restated_segment(seq), propagate=_restated_propagate)
    assert not seq.calls


def test_no_moving_object_is_a_named_error_and_main_explains(tmp_path, monkeypatch):
    import auto_mask as am
    seq = ms.sequence('pan')
    datapath = write_frames(seq, tmp_path)
    still = lambda a, b: (np.zeros(a.shape[:2] + (2,), np.float32), None)         # noqa: E731
    args = am.parse_args(['--datapath', datapath, '--keys_only'])
    from lasr_amd.nnutils import motionseg
    with pytest.raises(motionseg.NoMovingObject):
        am.run(args, still, segment=_restated_segment(seq))
    monkeypatch.setattr(am.auto_gen, 'build_model', lambda a: None)
    monkeypatch.setattr(am, 'run', lambda a, f: (_ for _ in ()).throw(motionseg.NoMovingObject('nothing moves')))
    with pytest.raises(SystemExit) as e:
        am.main(['--datapath', datapath])
    assert all(word in str(e.value) for word in ('--ms_gap', '--ms_model', 'paint', 'nothing moves'))


# ---- what the GPU comparison may excuse --------------------------------------------------------------------------------------------

HIST_CASES = ('pan', 'odd', 'tiny', 'large', 'holes')


def kernel_case(name):
    """-> (flow, flow back) float32 of the pair the kernel comparisons run on a fixture."""
    if name == 'holes':
        return ms.holes()[:2]
    return ms.flow_case(name).pair(0, 1)


def mid_state(name):
    """The float64 restatement's state after 3 iterations: the mid-fit state the moments are compared from."""
    f, fb = kernel_case(name)
    states = []
    ms.fit(f, ms.confidence(f, fb), ms.params(iters=3), states=states)
    return states[-1]


@pytest.mark.parametrize('name', HIST_CASES)
def test_near_integer_share_of_the_histogram_comparison(name):
    f, fb = kernel_case(name)
    conf = ms.confidence(f, fb).astype(np.float32)
    for S in (ms.initial_state(), mid_state(name)):
        near, n = ms.near_integer(f, conf, S), int((conf >= 0.5).sum())
        print(name, 'near an integer: %d of %d' % (near, n))
        assert near <= 0.001 * n


# ---- the float32 / float64 spread of the restatement: what the GPU tolerances are derived from ------------------------------------------

KERNEL_CASES = ('pan', 'odd', 'tiny', 'large', 'holes')
_cache = {}


def restated(name):
    """Everything the kernel comparisons need of a fixture, from the restatement alone, computed once: the pair's flows, conf in
    float32 (the kernels' input) and in both precisions, the initial and the mid-fit state, the moments and histograms from both
    states in both precisions, the scale sum |w| |term| of every moment, the fits and the evidence in both precisions."""
    if name in _cache:
        return _cache[name]
    f, fb = kernel_case(name)
    r = dict(flow=f, back=fb, conf64=ms.confidence(f, fb), conf32=ms.confidence(f, fb, 1., np.float32))
    conf = r['conf32']
    r['states'] = {'initial': ms.initial_state(), 'mid': mid_state(name)}
    for key, S in r['states'].items():
        r[key] = {dt: ms.moments(f, conf, S, dt) for dt in (np.float32, np.float64)}
        r[key]['scale'] = _scales(f, conf, S)
    r['fit'] = {dt: ms.fit(f, conf, None, dt) for dt in (np.float32, np.float64)}
    r['evidence'] = {dt: ms.evidence(f, conf, r['fit'][np.float64], 4., 6., dt) for dt in (np.float32, np.float64)}
    _cache[name] = r
    return r


def _scales(flow, conf, S):
    """sum w |term| per moment in float64: the size against which the rounding of a float64 sum of n terms is bounded."""
    keep = ~ms._skipped(flow, conf)
    w = ms.weights(ms.residual2(flow, S), conf.astype(np.float64), S)[keep]
    X, Y = ms.coords(*flow.shape[:2])
    X, Y, u, v = np.abs(X[keep]), np.abs(Y[keep]), np.abs(flow[..., 0][keep]).astype(np.float64), np.abs(flow[..., 1][keep]).astype(np.float64)
    mono = [X ** i * Y ** j for i, j in ms.EXPONENTS]
    return np.array([(w * m).sum() for m in mono] + [(w * u * m).sum() for m in mono[:6]] + [(w * v * m).sum() for m in mono[:6]]
                    + [(w * (u * u + v * v)).sum()])


def moment_bounds(name, key):
    """Per moment: 8 x the float32 / float64 spread of the restatement, plus the rounding of a float64 sum of n terms in another
    order, n 2^-53 sum |term| (the kernel folds lanes, waves and workgroups; numpy sums pairwise)."""
    r = restated(name)
    spread = np.abs(r[key][np.float32][0] - r[key][np.float64][0])
    n = r['flow'].shape[0] * r['flow'].shape[1]
    return 8 * spread + n * 2. ** -53 * r[key]['scale'], spread


@pytest.mark.parametrize('name', KERNEL_CASES)
def test_spread_of_the_restatement_on_the_kernel_fixtures(name):
    r = restated(name)
    print(name, 'conf spread %.3g' % np.abs(r['conf32'] - r['conf64']).max(),
          'evidence spread %.3g' % np.abs(r['evidence'][np.float32] - r['evidence'][np.float64]).max(),
          'theta spread %.3g' % np.abs(r['fit'][np.float32][ms.TH] - r['fit'][np.float64][ms.TH]).max(),
          'sigma', r['fit'][np.float32][ms.SIGMA], r['fit'][np.float64][ms.SIGMA])
    for key in ('initial', 'mid'):
        bound, spread = moment_bounds(name, key)
        rel = spread / np.maximum(r[key]['scale'], 1e-300)
        print('  %s: largest moment spread %.3g (relative to sum |term| %.3g), histograms differ in %d bins' % (
            key, spread.max(), rel.max(), int((r[key][np.float32][1] != r[key][np.float64][1]).sum())))
        assert (rel <= 1e-5).all() and np.isfinite(bound).all()
    assert r['fit'][np.float32][ms.STATUS] == r['fit'][np.float64][ms.STATUS] == 0


@pytest.mark.parametrize('name', ['pan', 'pan_noisy'])
def test_spread_of_the_restatement_on_the_sequences(name):
    print(name, 'q spread %.3g, undecided %d' % sequence_spread(name))


def sequence_restated(name):
    if ('seq', name) not in _cache:
        seq = ms.sequence(name)
        _cache[('seq', name)] = {dt: ms.segment(seq.frames, seq.flow, dt) for dt in (np.float32, np.float64)}
    return _cache[('seq', name)]


def sequence_spread(name):
    """-> (the float32 / float64 spread of q after the mean field, the number of pixels whose float64 q is within 8 x that of 0.5)."""
    r = sequence_restated(name)
    spread = float(np.abs(r[np.float32][1] - r[np.float64][1]).max())
    return spread, int((np.abs(r[np.float64][1] - 0.5) <= 8 * spread).sum())
