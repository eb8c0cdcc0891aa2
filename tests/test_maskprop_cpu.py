"""Silhouette propagation without a device: the float64 restatement (tests/maskprop_restated.py) on the analytic fixtures and on
closed forms, the C ABI's host-side checks, the script's argument handling and file layout, and the undecided share of the
fixtures tests/test_maskprop_gpu.py compares on."""
import argparse
import json
import os
import re
import sys

import numpy as np
import pytest

import maskprop_restated as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'preprocess'))

# The GPU comparison's tolerance on q after K = 5 (derived in test_maskprop_gpu.py's header): 8 x the float32 / float64 spread of
# the restatement itself on the four fixtures.
GPU_Q_TOL = 8 * 8.4e-8


def _ious(seq, masks):
    return [br.iou(masks[t], seq.masks[t]) for t in range(seq.T)]


@pytest.mark.parametrize('name', ['ellipse', 'ellipse_noisy', 'ellipse_distractor'])
def test_restatement_tracks_the_ellipse(name):
    seq = br.fixture(name)
    masks, soft = br.propagate(seq.frames, {0: seq.masks[0]}, seq.flow)
    ious = _ious(seq, masks)
    print(name, ['%.3f' % v for v in ious])                                       # measured: >= 0.998 on every frame
    assert min(ious) >= 0.95
    assert soft.shape == (8, 64, 80) and (soft >= 0).all() and (soft <= 1).all()


def test_the_fixture_tells_the_feature_from_a_plain_warp():
    seq = br.fixture('ellipse')
    masks, _ = br.propagate(seq.frames, {0: seq.masks[0]}, seq.flow, w_a=0., K=0)
    ious = _ious(seq, masks)
    print(['%.3f' % v for v in ious])                                             # measured: 0.81 on frame 1, 0.39 on frame 7
    assert ious[-1] < 0.7 and ious[0] == 1.


def test_round_trip_returns_to_the_annotation():
    seq = br.fixture('ellipse')
    assert br.roundtrip(seq.frames, 0, seq.masks[0], seq.flow) >= 0.95            # measured: 1.0


def test_two_keys_keep_their_annotation_and_blend_between():
    seq = br.fixture('ellipse')
    masks, soft = br.propagate(seq.frames, {0: seq.masks[0], 7: seq.masks[7]}, seq.flow)
    assert (masks[0] == seq.masks[0]).all() and (masks[7] == seq.masks[7]).all()
    assert set(np.unique(soft[0])) <= {0., 1.} and set(np.unique(soft[7])) <= {0., 1.}
    assert min(_ious(seq, masks)) >= 0.95


def test_an_empty_propagated_mask_is_an_error_that_names_the_frame():
    seq = br.fixture('ellipse')
    away = lambda a, b: np.full((seq.H, seq.W, 2), 1000., np.float32)             # noqa: E731  every q outside: prior 0 everywhere
    with pytest.raises(br.EmptyPropagation, match='frame 1'):
        br.propagate(seq.frames, {0: seq.masks[0]}, away, w_a=0.)


# ---- closed forms -----------------------------------------------------------------------------------------------------------------

def _flat(H, W, colour):
    return np.broadcast_to(np.array(colour, np.uint8), (H, W, 3)).copy()


def test_zero_flow_and_an_uninformative_histogram_return_the_source_mask():
    H, W = 20, 24
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    P = np.zeros((H, W))
    P[5:14, 6:17] = 1
    zero = np.zeros((H, W, 2))
    h = np.zeros((2, br.BINS), np.int64)                                          # empty histograms: app = log(eps / eps) = 0
    p = br.params()
    u, q0, conf, prior = br.unary(img, P, zero, zero, h, p)
    assert (conf == 1).all() and (prior == P).all()
    assert np.abs(u - np.where(P > 0, 1, -1) * min(np.log(0.999 / 0.001), p['U'])).max() < 1e-12
    assert ((q0 > 0.5) == (P > 0.5)).all()
    # the same when both histograms are equal (every colour as likely on either side)
    h2 = np.stack([np.bincount(br.bins(img).ravel(), minlength=br.BINS)] * 2)
    assert np.abs(br.unary(img, P, zero, zero, h2, p)[0] - u).max() < 1e-12
    q = br.step(img, img, P, zero, zero, h, p)
    assert ((q > 0.5) == (P > 0.5)).all()


def test_an_integer_translation_of_a_flat_square_is_reproduced_exactly():
    H, W, d = 32, 40, (5, -3)
    frames, masks = [], []
    for t in range(3):
        m = np.zeros((H, W), bool)
        m[12 + t * d[1]:22 + t * d[1], 6 + t * d[0]:18 + t * d[0]] = True
        frames.append(np.where(m[..., None], np.uint8([210, 40, 40]), np.uint8([30, 90, 160])).astype(np.uint8))
        masks.append(m)

    def flow_of(a, b):
        return masks[a][..., None] * (np.array(d, float) * (b - a))
    got, _ = br.propagate(frames, {0: masks[0]}, flow_of)
    assert all((got[t] == masks[t]).all() for t in range(3))
    got, _ = br.propagate(frames, {2: masks[2]}, flow_of)
    assert all((got[t] == masks[t]).all() for t in range(3))


def test_conf_is_exp_minus_two_where_the_flows_disagree_by_two_pixels():
    H, W = 12, 16
    img = _flat(H, W, (9, 9, 9))
    fts = np.zeros((H, W, 2))
    fts[..., 0] = 3.
    fst = np.zeros((H, W, 2))
    fst[..., 0] = -1.                                                              # 3 + (-1) = 2 px of disagreement
    _, _, conf, _ = br.unary(img, np.ones((H, W)), fts, fst, np.zeros((2, br.BINS), np.int64), br.params(tau=1.))
    inside = np.arange(W)[None] + 3 <= W - 1
    assert np.abs(conf[:, inside[0]] - np.exp(-2.)).max() < 1e-15 and (conf[:, ~inside[0]] == 0).all()


def test_histogram_counts_and_window():
    seq = br.fixture('ellipse')
    P = seq.masks[0].astype(np.float32)
    win = br.window_of(P)
    ys, xs = np.nonzero(seq.masks[0])
    w, h = xs.max() - xs.min() + 1, ys.max() - ys.min() + 1
    assert win == (max(0, xs.min() - w // 2 - 8), max(0, ys.min() - h // 2 - 8), min(80, xs.max() + 1 + w // 2 + 8),
                   min(64, ys.max() + 1 + h // 2 + 8))
    hh = br.hist(seq.frames[0], P, win)
    x0, y0, x1, y1 = win
    assert hh[1].sum() == seq.masks[0].sum() and hh[0].sum() == (y1 - y0) * (x1 - x0) - seq.masks[0].sum()
    assert br.hist(seq.frames[0], P, (5, 5, 5, 9)).sum() == 0 and br.window_of(P * 0) is None
    half = np.full_like(P, 0.5)
    assert br.hist(seq.frames[0], half, win).sum() == 0                           # neither side claims an undecided pixel


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

def test_header_and_binding_agree_on_the_three_entry_points():
    from lasr_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    kinds = {'int': _lib._i, 'float': _lib._f}
    for name in ('lasr_maskprop_hist', 'lasr_maskprop_unary', 'lasr_maskprop_meanfield'):
        args = re.search(r'int\s+%s\s*\((.*?)\)\s*;' % name, hdr, re.S).group(1)
        want = [_lib._p if '*' in a else kinds[a.split()[0]] for a in args.split(',')]
        res, got = _lib.SIGNATURES[name]
        assert res is _lib._i and got == want, name
    for name, value in (('BINS', 4096), ('MAX_SIZE', 16384), ('MAX_RADIUS', 8)):
        assert '#define LASR_MASKPROP_%s %d\n' % (name, value) in hdr and getattr(_lib, 'MASKPROP_' + name) == value
    assert br.BINS == _lib.MASKPROP_BINS


def test_symbols_are_exported_and_the_host_checks_run_without_a_device():
    from lasr_amd import _lib
    h = _lib.lib()
    n, a = None, 1 << 20                                                          # a: any non-null address; no launch reads it
    hist = lambda H=8, W=9, x0=0, y0=0, x1=9, y1=8, hi=0.9, lo=0.1, p=n: h.lasr_maskprop_hist(p, p, p, H, W, x0, y0, x1, y1,   # noqa: E731
                                                                                               hi, lo, n)
    assert hist() == -1                                                           # null buffers
    assert hist(x1=0) == 0 and hist(y1=0) == 0 and hist(x0=4, x1=4) == 0 and hist(x0=5, x1=3) == 0      # empty window
    assert hist(H=0, W=0, x1=0, y1=0) == 0 and hist(H=0, y1=0) == 0               # empty image
    assert hist(H=-1) == -1 and hist(W=-1) == -1 and hist(x0=-1) == -1 and hist(y0=-1) == -1
    assert hist(x1=10) == -1 and hist(y1=9) == -1 and hist(x1=10, p=a) == -1
    assert hist(hi=0.1, lo=0.9, x1=0) == -1 and hist(hi=0.5, lo=0.5, x1=0) == -1 and hist(hi=float('nan'), x1=0) == -1
    assert hist(H=16385, W=1, x1=0, y1=0) == -1 and hist(H=16384, W=1, x1=0, y1=0) == 0
    assert hist(H=16384, W=16384, x1=0, y1=0) == 0 and hist(H=16384 * 2, W=16384 * 2, x1=0) == -1
    assert hist(H=30000 // 1, W=30000, x1=0) == -1                                # sides above LASR_MASKPROP_MAX_SIZE

    def unary(H=8, W=9, tau=1., w_p=1., w_a=0.5, eps=1e-3, U=6., p=n):
        return h.lasr_maskprop_unary(p, p, p, p, p, p, p, p, H, W, tau, w_p, w_a, eps, U, n)
    assert unary() == -1 and unary(H=0) == 0 and unary(W=0) == 0 and unary(H=-1) == -1 and unary(W=-3) == -1
    assert unary(H=0, tau=0.) == -1 and unary(H=0, tau=-1.) == -1 and unary(H=0, tau=float('nan')) == -1
    assert unary(H=0, eps=0.) == -1 and unary(H=0, U=0.) == -1 and unary(H=0, U=float('inf')) == -1
    assert unary(H=0, w_p=-1.) == -1 and unary(H=0, w_a=-0.5) == -1 and unary(H=0, w_p=0., w_a=0.) == 0
    assert unary(H=16385, W=0) == -1 and unary(tau=0., p=a) == -1

    def mf(H=8, W=9, R=4, si=12., ss=3., ws=0.3, p=n):
        return h.lasr_maskprop_meanfield(p, p, p, p, H, W, R, si, ss, ws, n)
    assert mf() == -1 and mf(H=0) == 0 and mf(W=0) == 0 and mf(H=-1) == -1
    assert mf(H=0, R=-1) == -1 and mf(H=0, R=9) == -1 and mf(H=0, R=8) == 0 and mf(H=0, R=0) == 0 and mf(R=9, p=a) == -1
    assert mf(H=0, si=0.) == -1 and mf(H=0, ss=0.) == -1 and mf(H=0, ss=float('nan')) == -1 and mf(H=0, ws=-1.) == -1
    assert mf(H=0, ws=0.) == 0 and mf(W=16385, H=0) == -1
    assert h.lasr_maskprop_meanfield(a, a, a, a, 8, 9, 4, 12., 3., 0.3, n) == -1  # q_in == q_out: the iteration is not in place
    names = [h.lasr_prof_kernel_name(i) for i in range(h.lasr_prof_kernel_count())]
    assert not any(b'maskprop' in x for x in names)                               # the kernel-name table is not extended


def test_python_layer_refuses_cpu_tensors_and_unknown_parameters():
    import torch
    from lasr_amd.nnutils import maskprop
    img, f = torch.zeros(4, 5, 3, dtype=torch.uint8), torch.zeros(4, 5)
    with pytest.raises(TypeError):
        maskprop.histogram(img, f, (0, 0, 5, 4))
    with pytest.raises(TypeError):
        maskprop.unary(img, f, torch.zeros(4, 5, 2), torch.zeros(4, 5, 2), torch.zeros(2, 4096, dtype=torch.int32))
    with pytest.raises(TypeError):
        maskprop.meanfield(img, f, f)
    with pytest.raises(TypeError, match='unknown parameters'):
        maskprop.params(sigma=3.)
    with pytest.raises(ValueError):
        maskprop.params(R=9)
    assert maskprop.params() == br.params() and maskprop.params(K=2)['K'] == 2
    P = np.zeros((60, 90), np.float32)
    P[30:40, 40:60] = 1
    assert maskprop.window_of(P) == br.window_of(P) == (22, 17, 78, 53)
    assert maskprop.window_of(P[:45, :70]) == br.window_of(P[:45, :70]) == (22, 17, 70, 45)
    assert maskprop.window_of(P * 0) is None
    q = np.zeros((12, 12))
    q[1:7, 1:7] = 0.9
    q[10, 10] = 0.8                                                               # a speck of 1 px against 36: dropped
    q[8:10, 0:1] = 0.7                                                            # 2 px >= 0.05 * 36 = 1.8: kept
    got = maskprop.component_filter(q, 0.05)
    assert got[10, 10] == 0 and got[8, 0] == 0.7 and got[3, 3] == 0.9 and (got == br.component_filter(q, 0.05)).all()


# ---- the script -------------------------------------------------------------------------------------------------------------------

def test_script_arguments():
    import propagate_mask as pm
    a = pm.parse_args(['--datapath', 'database/DAVIS/JPEGImages/Full-Resolution/camel/', '--key', '0:first.png'])
    assert a.key == [(0, 'first.png')] and a.loadmodel is None and not a.roundtrip and not a.force and a.min_area == 1000
    assert pm.tuning_of(a) == br.params()
    assert (a.testres, a.maxdisp, a.fac) == (1, 256, 1)                           # what auto_gen.build_model / flow_inference read
    a = pm.parse_args('--datapath d/JPEGImages/x --key 0:a.png --key 40:dir/b:c.png --loadmodel vcn_rob.pth --roundtrip --min_area 10 '
                      '--force --tau 2 --w_p 0.5 --w_a 1 --eps 1e-2 --U 4 --R 3 --sigma_i 8 --sigma_s 2 --w_s 0.2 --K 3 --hi 0.8 '
                      '--lo 0.2 --min_component 0.1'.split())
    assert a.key == [(0, 'a.png'), (40, 'dir/b:c.png')] and a.roundtrip and a.force and a.min_area == 10 and a.loadmodel == 'vcn_rob.pth'
    assert pm.tuning_of(a) == dict(hi=0.8, lo=0.2, tau=2., w_p=0.5, w_a=1., eps=1e-2, U=4., R=3, sigma_i=8., sigma_s=2., w_s=0.2, K=3,
                                   min_component=0.1)
    for bad in (['--key', 'first.png'], ['--key', 'x:first.png'], ['--key', '0:'], ['--key', '0:a.png', '--key', '0:b.png'], []):
        with pytest.raises(SystemExit):
            pm.parse_args(['--datapath', 'd'] + bad)
    with pytest.raises(argparse.ArgumentTypeError):
        pm.parse_key('-1:a.png')


def test_annotations_path_is_auto_gen_s_substitution():
    import propagate_mask as pm
    d = 'database/DAVIS/JPEGImages/Full-Resolution/camel/'
    assert pm.annotations_dir(d) == os.path.normpath(d).replace('JPEGImages', 'Annotations') == \
        'database/DAVIS/Annotations/Full-Resolution/camel'
    with pytest.raises(ValueError, match='JPEGImages'):
        pm.annotations_dir('somewhere/frames/camel')


def test_masks_are_written_128_in_red_and_read_back_by_auto_gen(tmp_path):
    import auto_gen
    import propagate_mask as pm
    from PIL import Image
    m = np.zeros((6, 7), bool)
    m[2:4, 1:5] = True
    enc = pm.encode_mask(m)
    assert enc.dtype == np.uint8 and (enc[..., 0] == m * 128).all() and not enc[..., 1:].any()
    path = str(tmp_path / '00000.png')
    Image.fromarray(enc).save(path)
    assert (auto_gen.read_mask(path) == m).all()
    # a key PNG of any non-zero encoding is accepted
    for arr in (m.astype(np.uint8), m.astype(np.uint8) * 255, enc, np.stack([m * 0, m * 0, m * 7], -1).astype(np.uint8)):
        Image.fromarray(arr).save(path)
        assert (pm.read_key(path, m.shape) == m).all()
    with pytest.raises(ValueError, match='6 x 7'):
        pm.read_key(path, (6, 8))
    Image.fromarray(np.zeros((6, 7), np.uint8)).save(path)
    with pytest.raises(ValueError, match='empty'):
        pm.read_key(path, m.shape)


def _restated_propagate(frames, keys, flow_fn, **tuning):
    flow_of = lambda a, b: flow_fn(frames[a], frames[b])[0][..., :2]              # noqa: E731
    masks, soft = br.propagate(frames, keys, flow_of, **tuning)
    return masks, soft.astype(np.float32), {}


def _restated_roundtrip(frames, key, mask, flow_fn, **tuning):
    return br.roundtrip(frames, key, mask, lambda a, b: flow_fn(frames[a], frames[b])[0][..., :2], **tuning)


def write_video(seq, root):
    """The fixture as a DAVIS-layout folder of lossless frames + the annotation of frame 0.  -> (datapath, key path)."""
    from PIL import Image
    d = os.path.join(str(root), 'DAVIS', 'JPEGImages', 'Full-Resolution', 'ellipse')
    os.makedirs(d)
    for t, f in enumerate(seq.frames):
        Image.fromarray(f).save(os.path.join(d, '%05d.png' % t))
    key = os.path.join(str(root), 'first.png')
    Image.fromarray(seq.masks[0].astype(np.uint8) * 255).save(key)
    return d + '/', key


def test_script_layout_overwrite_refusal_min_area_and_auto_gen_runs_next(tmp_path, capsys):
    import auto_gen
    import propagate_mask as pm
    seq = br.fixture('ellipse')
    datapath, key = write_video(seq, tmp_path)
    args = pm.parse_args(['--datapath', datapath, '--key', '0:' + key, '--min_area', '100', '--roundtrip'])
    report = pm.run(args, seq.flow_fn, propagate=_restated_propagate, roundtrip=_restated_roundtrip)
    out = pm.annotations_dir(datapath)
    assert sorted(os.listdir(out)) == ['%05d.png' % t for t in range(8)] + ['maskprop.json']
    for t in range(8):
        assert br.iou(auto_gen.read_mask(os.path.join(out, '%05d.png' % t)), seq.masks[t]) >= 0.95
    saved = json.load(open(os.path.join(out, 'maskprop.json')))
    assert saved == json.loads(json.dumps(report | dict(min_area=100, skipped=[])))
    assert saved['params'] == br.params() and saved['areas'] == [int(m.sum()) for m in seq.masks] and saved['keys'] == [0]
    assert saved['roundtrip_iou'] >= 0.95 and 'IoU' in capsys.readouterr().out
    # a second run refuses the folder unless forced
    with pytest.raises(pm.AnnotationsExist, match='--force'):
        pm.run(args, seq.flow_fn, propagate=_restated_propagate, roundtrip=_restated_roundtrip)
    args.force, args.roundtrip = True, False
    assert pm.run(args, seq.flow_fn, propagate=_restated_propagate)['roundtrip_iou'] is None
    # auto_gen.py runs next, unchanged, on what was written
    ag = auto_gen.parse_args(['--datapath', datapath, '--outdir', str(tmp_path / 'out')])
    kept = auto_gen.run(ag, seq.flow_fn)
    assert kept == [(t, t + 1) for t in range(7)]
    assert len(os.listdir(str(tmp_path / 'out' / 'FlowFW'))) == 14
    # --min_area: the small frames are reported, not written, and nothing is renumbered
    args.min_area = int(max(m.sum() for m in seq.masks[:4])) + 1
    capsys.readouterr()
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    rep = pm.run(args, seq.flow_fn, propagate=_restated_propagate)
    small = [t for t in range(8) if seq.masks[t].sum() < args.min_area]
    text = capsys.readouterr().out
    assert small and len(small) < 8 and 'renumber' in text and str(small) in text and 'NOT written' in text
    assert sorted(os.listdir(out)) == ['%05d.png' % t for t in range(8) if t not in small] + ['maskprop.json']
    assert json.load(open(os.path.join(out, 'maskprop.json')))['skipped'] == small and rep['areas'][0] == int(seq.masks[0].sum())


# ---- what the GPU comparison may leave undecided ----------------------------------------------------------------------------------------

def undecided(name, tol=GPU_Q_TOL):
    """bool [H,W]: the pixels of the fixture's first step whose float64 q after the K iterations lies within tol of 0.5.  (Before
    the iterations a pixel can sit at 0.5 exactly: tiny has one whose prior is the half-pixel sample 0.5 and whose colour no
    histogram has seen, so u = 0 in any precision; the masks are compared on the final q.)"""
    f = br.first_step(name)
    q = br.step(f['img_s'], f['img_t'], f['P_s'], f['flow_ts'], f['flow_st'], f['key_hist'], br.params())
    return np.abs(q - 0.5) <= tol


@pytest.mark.parametrize('name', br.FIXTURES)
def test_undecided_share_of_the_gpu_comparison(name):
    und = undecided(name)
    print(name, int(und.sum()), 'of', und.size)                                   # measured: 0 on every fixture (nearest: 0.2 away)
    assert und.mean() <= 0.005


@pytest.mark.parametrize('name', ['ellipse', 'ellipse_noisy', 'border'])
def test_undecided_share_of_the_full_propagation(name):
    seq = br.fixture(name)
    _, soft = br.propagate(seq.frames, {br.KEYS[name]: seq.masks[br.KEYS[name]]}, seq.flow)
    und = np.abs(soft - 0.5) <= GPU_Q_TOL
    assert und.mean() <= 0.005                                                     # measured: 0
