"""Reprojection scores on the device (lasr_amd/nnutils/reproj.py, csrc/reproj.hip) against the float64 restatement
(tests/reproj_restated.py) and closed forms.  The scores are this project's own addition: the restatement is the only parity
there is.

Bit maps and the integer counts are compared exactly.  The tolerances of the two means are derived in tests/test_reproj_cpu.py from
the float32 / float64 spread of the restatement itself (8 x 1.5e-5 px on the mean epe, 8 x 0.31 on the mean squared colour
difference), not from what the kernel gives; n_le1 / n_le3 may differ by the pixels whose float64 epe lies within that tolerance
of the threshold.  The closed-form case is bounded by PX = 1e-3 px, the position bound of tests/test_tracks_gpu.py.  Every test
prints its figures before it asserts.

Measured on an MI355X:
  bit maps, boundary maps and the counts 0-7 equal the restatement on the six mask pairs at every radius (64 x 80: n_pb 175, n_gb
    176, pm 54 / 86 / 143 / 170 at radius 0 / 1 / 3 / 7, gm 176 at radius 7 and 12).
  flow prediction against lasr_track_project: 1100 / 1052 / 1087 / 919 pixel centres of frames 0-3, sum of epe exactly 0 in every
    frame: the same bits.
  flow fixture: n_flow 864 / 813 / 857 / 775 / 0 and n_rgb 1100 / 1052 / 1087 / 919 / 804 exact, n_le1 and n_le3 equal to the
    restatement's (no undecided pixel), mean epe error 1.1e-7 px (bound 1.2e-4), mean sq error 3.9e-4 (bound 2.48).
  translating quad: mean epe against the analytic displacement 1.9e-6 / 2.1e-6 / 2.2e-6 px (bound 1e-3), J = F = 1.
  script: J 0.8835, F 0.8653, epe 0.354 px (the fixture adds 0.25 px to both flow components), worst frame the shifted one.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import reproj_restated as rr
import tracks_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
H, W, IS = tc.H, tc.W, tc.IS
PX = 1e-3
SIZES = [(9, 7), (37, 53), (64, 64), (64, 80), (70, 130), (33, 129)]


def _rp():
    from lasr_amd.nnutils import reproj
    return reproj


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _planes(cuda, verts, faces, K, size=IS):
    from lasr_amd.nnutils import bake
    tv, tf, tK = _dev(cuda, verts, faces, K)
    return bake.face_index_raster(tv, tf.int(), tK, size)[:, 1].cpu().numpy()


def _words(t):
    return t.cpu().numpy().view(np.uint64)


def _hand_raster(cuda, preds):
    """aggrs_info [T,2,IS,IS] whose plane 1 names face 0 on the True pixels of preds [T,h,w] and -1 elsewhere."""
    T, h, w = preds.shape
    size = max(h, w)
    r = -np.ones((T, 2, size, size), np.float32)
    r[:, 1, :h, :w] = np.where(preds, 0., -1.)
    return torch.from_numpy(r).to(cuda)


@pytest.mark.parametrize('size', SIZES)
def test_bit_maps_and_silhouette_counts_equal_the_restatement(cuda, size):
    rp = _rp()
    h, w = size
    pred, gt = rr.pair(h, w)
    preds, gts = np.stack([pred, gt]), np.stack([gt, pred])                  # frame 1 swaps the roles
    verts = torch.tensor([[[0., 0., 2.], [1., 0., 2.], [0., 1., 2.]]], device=cuda).repeat(2, 1, 1)
    faces = torch.tensor([[0, 1, 2]], device=cuda)
    K = torch.tensor([[50., 50., 1., 1.]], device=cuda).repeat(2, 1)
    raster = _hand_raster(cuda, preds)
    masks = torch.from_numpy(gts.astype(np.uint8) * 7).to(cuda)
    ww = (w + 63) // 64
    radii = [0, 1, 3, 7, 12] + ([96] if size == (70, 130) else []) + [0.008]
    for bound_th in radii:
        out = rp.evaluate(verts, faces, K, masks, bound_th=bound_th, raster=raster)
        rho = rr.radius_of(bound_th, h, w)
        assert (out['radius'] == rho).all() and out['bits'].shape == (2, 2, h, ww)
        bits, bbits = _words(out['bits']), _words(out['boundary_bits'])
        for t in range(2):
            want = rr.silhouette_counts(preds[t], gts[t], rho)
            got = {k: int(out[k][t]) for k in want}
            assert got == want, (size, bound_th, t, got, want)
            assert np.array_equal(bits[t, 0], rr.pack_bits(preds[t])) and np.array_equal(bits[t, 1], rr.pack_bits(gts[t]))
            assert np.array_equal(bbits[t, 0], rr.pack_bits(rr.boundary(preds[t])))
            assert np.array_equal(bbits[t, 1], rr.pack_bits(rr.boundary(gts[t])))
            sc = rr.scores(want)
            for k in ('J', 'precision', 'recall', 'F'):
                assert out[k][t] == sc[k], (k, out[k][t], sc[k])
            for k in ('n_flow', 'n_le1', 'n_le3', 'n_rgb'):
                assert out[k][t] == 0
            assert np.isnan(out['epe'][t]) and np.isnan(out['psnr'][t])
        if w % 64:                                                            # bits at or beyond W are zero
            beyond = ~np.uint64((1 << (w % 64)) - 1)
            assert not (bits[..., -1] & beyond).any() and not (bbits[..., -1] & beyond).any()
        assert np.array_equal(rp.unpack_bits(out['bits'].cpu().numpy(), w), np.stack([preds, gts], 1))
    c = rr.silhouette_counts(pred, gt, 7)
    print('pair %d x %d: n_pb %d, n_gb %d, pm %d, gm %d at radius 7; default radius %d' % (h, w, c['n_pb'], c['n_gb'], c['pm'], c['gm'],
                                                                                         rr.radius_of(0.008, h, w)))
    if size == (64, 80):
        assert [rr.silhouette_counts(pred, gt, r)['pm'] for r in (0, 1, 3, 7)] == [54, 86, 143, 170]


@pytest.fixture(scope='module')
def sphere(cuda):
    """The flow / colour fixture on the device raster's own planes, and the restatement's answer (computed once)."""
    fx = rr.flow_fixture()
    planes = _planes(cuda, fx['verts'], fx['faces'], fx['K'])
    masks, flows, occs = rr.observed_flow(fx, planes)
    want = rr.evaluate(fx['verts'], fx['faces'], fx['K'], planes, masks, flows, occs, fx['frames'], fx['colors'])
    tensors = _dev(cuda, fx['verts'], fx['faces'], fx['K'], masks, flows, occs, fx['frames'], fx['colors'])
    return dict(fx=fx, planes=planes, masks=masks, flows=flows, occs=occs, want=want, tensors=tensors)


def test_flow_prediction_is_the_tracks_kernel_s(cuda, sphere):
    """The rendered flow of every covered pixel centre equals, bit for bit, what lasr_track_project gives for the same centre: the
    tracks kernel's own answer is handed back as the observed flow, and a difference of exactly 0 in every counted pixel is the only
    way to a sum of exactly 0.  (The comparison goes through the counters' inputs; the ABI has no per-pixel output.)"""
    from lasr_amd.nnutils import tracks as tk
    rp = _rp()
    fx, planes = sphere['fx'], sphere['planes']
    tv, tf, tK = sphere['tensors'][:3]
    T = fx['verts'].shape[0]
    flows = torch.zeros(T - 1, H, W, 3, device=cuda)
    finite = []
    for i in range(T - 1):
        q = torch.from_numpy(tc.centres(planes[i, :H, :W] >= 0, i).astype(np.float32)).to(cuda)
        tracks, state, _ = tk.track_points(tv, tf, tK, q, H, W)
        nxt = tracks[:, i + 1]                                                # (u, v) in frame i + 1
        ok = ~torch.isnan(nxt).any(1)
        r, c = q[ok, 1].long(), q[ok, 2].long()
        flows[i, r, c, 0] = nxt[ok, 0] - q[ok, 2]                            # float32, the kernel's own subtraction
        flows[i, r, c, 1] = nxt[ok, 1] - q[ok, 1]
        flows[i, r, c, 2] = 1.
        finite.append(int(ok.sum()))
        assert (state[:, i] == 1).all()
    masks = torch.ones(T, H, W, dtype=torch.uint8, device=cuda)
    out = rp.evaluate(tv, tf, tK, masks, flows=flows)
    print('flow prediction against lasr_track_project: %s pixels per frame, sum of epe %s' % (finite, out['sums'][:, 0].tolist()))
    assert min(finite) >= 400
    assert out['n_flow'][:-1].tolist() == finite and out['n_le1'][:-1].tolist() == finite and out['n_flow'][-1] == 0
    assert torch.equal(out['sums'][:, 0], torch.zeros(T, dtype=torch.float64, device=cuda))


def test_flow_and_colour_counts_and_sums(cuda, sphere):
    rp = _rp()
    want = sphere['want']
    tv, tf, tK, tm, tfl, toc, tfr, tco = sphere['tensors']
    out = rp.evaluate(tv, tf, tK, tm, flows=tfl, occs=toc, frames=tfr, colors=tco)
    tol, sq_tol = 8 * rr.EPE_SPREAD, 8 * rr.SQ_SPREAD
    T = len(want['n_flow'])
    psnr_tol = 10. / np.log(10.) * sq_tol / (want['sum_sq'] / want['n_rgb']).min() * 1.01      # d psnr = 10 / ln 10 * d sq / sq
    for k in rr.COUNTS[:8]:
        assert (out[k] == want[k]).all(), k
    und1 = np.array([int((np.abs(e - 1.) <= tol).sum()) for e in want['epe_px']])
    und3 = np.array([int((np.abs(e - 3.) <= tol).sum()) for e in want['epe_px']])
    epe_err = np.abs(out['epe'][:-1] - want['epe'][:-1]).max()
    sq_err = np.abs(out['sums'][:, 1].cpu().numpy() / out['n_rgb'] - want['sum_sq'] / want['n_rgb']).max()
    print('flow fixture on the device raster: n_flow %s, n_rgb %s, n_le1 %s (restatement %s, undecided %s), n_le3 %s (restatement %s, '
          'undecided %s), mean epe error %.3e px (bound %.1e), mean sq error %.3e (bound %.2f), psnr %s'
          % (out['n_flow'].tolist(), out['n_rgb'].tolist(), out['n_le1'].tolist(), want['n_le1'].tolist(), und1.tolist(),
             out['n_le3'].tolist(), want['n_le3'].tolist(), und3.tolist(), epe_err, tol, sq_err, sq_tol, np.round(out['psnr'], 3).tolist()))
    assert (out['n_flow'] == want['n_flow']).all() and (out['n_rgb'] == want['n_rgb']).all()
    assert (want['n_flow'][:-1] > 500).all() and (want['n_rgb'] > want['n_flow']).all()
    assert (np.abs(out['n_le1'] - want['n_le1']) <= und1).all() and (np.abs(out['n_le3'] - want['n_le3']) <= und3).all()
    assert max(und1.sum(), und3.sum()) <= 0.005 * want['n_flow'].sum()
    assert epe_err <= tol and sq_err <= sq_tol
    assert out['n_flow'][-1] == 0 and np.isnan(out['epe'][-1]) and np.isnan(out['pck1'][-1]) and not np.isnan(out['psnr']).any()
    assert np.allclose(out['pck1'][:-1], out['n_le1'][:-1] / out['n_flow'][:-1]) and np.abs(out['psnr'] - want['psnr']).max() <= psnr_tol
    assert out['counts'].shape == (T, 12) and out['sums'].dtype == torch.float64
    # without occs the occluded band counts again; without flows and colours their counters stay 0
    more = rp.evaluate(tv, tf, tK, tm, flows=tfl)
    assert (more['n_flow'][:-1] > out['n_flow'][:-1]).all() and (more['n_rgb'] == 0).all() and np.isnan(more['psnr']).all()


def test_determinism_and_chunking(cuda, sphere, monkeypatch):
    rp = _rp()
    tv, tf, tK, tm, tfl, toc, tfr, tco = sphere['tensors']
    assert rp.CHUNK_FRAMES >= 5
    a = rp.evaluate(tv, tf, tK, tm, flows=tfl, occs=toc, frames=tfr, colors=tco)
    b = rp.evaluate(tv, tf, tK, tm, flows=tfl, occs=toc, frames=tfr, colors=tco)
    monkeypatch.setattr(rp, 'CHUNK_FRAMES', 2)                               # chunks of 2, 2 and 1 frames: frames 1 and 3 look ahead
    c = rp.evaluate(tv, tf, tK, tm, flows=tfl, occs=toc, frames=tfr, colors=tco)
    for other in (b, c):
        for k in ('counts', 'sums', 'bits', 'boundary_bits'):
            assert torch.equal(a[k], other[k]), k
    assert (a['n_flow'][[1, 3]] > 500).all()


def test_translating_quad_closed_form(cuda):
    rp = _rp()
    verts, faces, K = tc.quad_case()
    T = len(verts)
    planes = _planes(cuda, verts, faces, K)[:, :H, :W]
    masks = (planes >= 0).astype(np.uint8)                                    # the device raster's own silhouette: J = F = 1
    fx, fy, px, py = tc.QUAD_K
    r, c = np.mgrid[:H, :W] + 0.5
    flows = np.zeros((T - 1, H, W, 3), np.float32)
    for i in range(T - 1):                                                    # the quad of frame i lies in the plane z = z_i
        z = tc.QUAD_Z0 + i * tc.QUAD_STEP[2]
        P = np.stack([(c - px) / fx * z, (r - py) / fy * z, np.full_like(c, z)], -1) + tc.QUAD_STEP
        flows[i, ..., 0] = fx * P[..., 0] / P[..., 2] + px - c
        flows[i, ..., 1] = fy * P[..., 1] / P[..., 2] + py - r
        flows[i, ..., 2] = 1.
    tv, tf, tK, tm, tfl = _dev(cuda, verts, faces, K, masks, flows)
    out = rp.evaluate(tv, tf, tK, tm, flows=tfl, bound_th=0)
    print('translating quad: n_flow %s, mean epe against the analytic displacement %s px (bound %.0e), J %s, F %s'
          % (out['n_flow'].tolist(), out['epe'][:-1].tolist(), PX, out['J'].tolist(), out['F'].tolist()))
    assert (out['J'] == 1.).all() and (out['F'] == 1.).all() and (out['n_pb'] == out['pm']).all() and (out['n_pb'] > 50).all()
    assert (out['n_flow'][:-1] == out['n_pred'][:-1]).all() and (out['n_flow'][:-1] > 500).all()
    assert np.abs(flows[..., :2]).max() > 5.                                  # the displacement is of several pixels
    assert (out['epe'][:-1] <= PX).all() and (out['n_le1'] == out['n_flow']).all()


def test_python_layer_validates_its_arguments(cuda):
    rp = _rp()
    verts, faces, K = tc.quad_case()
    T = len(verts)
    tv, tf, tK = _dev(cuda, verts, faces, K)
    tm = torch.ones(T, H, W, dtype=torch.uint8, device=cuda)
    fl = torch.zeros(T - 1, H, W, 3, device=cuda)
    with pytest.raises(TypeError):
        rp.evaluate(tv, tf, tK, tm.cpu())
    with pytest.raises(TypeError):
        rp.evaluate(tv, tf, tK, tm, flows=fl.cpu())
    bad = tf.clone()
    bad[1, 1] = 4
    with pytest.raises(ValueError, match='must index the 4 vertices'):
        rp.evaluate(tv, bad, tK, tm)
    with pytest.raises(ValueError, match=r'K must be \[T = 4, 4\]'):
        rp.evaluate(tv, tf, tK[:3], tm)
    with pytest.raises(ValueError, match=r'masks must be \[T = 4, H, W\]'):
        rp.evaluate(tv, tf, tK, tm[:3])
    with pytest.raises(ValueError, match=r'flows must be floating point \[T - 1 = 3'):
        rp.evaluate(tv, tf, tK, tm, flows=torch.zeros(T, H, W, 3, device=cuda))
    with pytest.raises(ValueError, match='occs comes with flows'):
        rp.evaluate(tv, tf, tK, tm, occs=torch.zeros(T - 1, H, W, device=cuda))
    with pytest.raises(ValueError, match='frames and colors come together'):
        rp.evaluate(tv, tf, tK, tm, frames=torch.zeros(T, H, W, 3, dtype=torch.uint8, device=cuda))
    with pytest.raises(ValueError, match='colors must be uint8'):
        rp.evaluate(tv, tf, tK, tm, frames=torch.zeros(T, H, W, 3, dtype=torch.uint8, device=cuda), colors=torch.zeros(T, 4, 3, device=cuda))
    with pytest.raises(ValueError, match='bound_th must be at least 0'):
        rp.evaluate(tv, tf, tK, tm, bound_th=-0.01)
    with pytest.raises(ValueError, match='exceeds the limit of 96'):
        rp.evaluate(tv, tf, tK, tm, bound_th=97)
    out = rp.evaluate(tv[:0], tf, tK[:0], tm[:0])                            # no frames: empty outputs, nothing launched
    assert out['J'].shape == (0,) and out['bits'].shape == (0, 2, H, 1)


def test_script_end_to_end(cuda, tmp_path, monkeypatch):
    rp = _rp()
    root = str(tmp_path)
    verts, faces, K = tc.sphere_case()
    T = len(verts)
    rng = np.random.default_rng(4)
    frames = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    colors = rng.integers(0, 256, (T, verts.shape[1], 3), dtype=np.uint8)
    centre = verts.mean(1, keepdims=True)
    grown = ((verts - centre) * 1.04 + centre).astype(np.float32)            # annotations: the raster of a slightly scaled mesh
    masks = (_planes(cuda, grown, faces, K)[:, :H, :W] >= 0).astype(np.uint8) * 255
    masks[2] = np.roll(masks[2], 6, axis=1)                                   # frame 2's annotation is shifted by 6 px
    planes = _planes(cuda, verts, faces, K)
    flows = np.zeros((T - 1, H, W, 3), np.float32)
    base = rr.evaluate(verts, faces, K, planes, np.ones((T, H, W), np.uint8), flows=flows)
    for t in range(T - 1):
        r, c, fp = base['flow_px'][t]
        flows[t, r, c, :2] = fp + 0.25
        flows[t, r, c, 2] = 1.
    test = rr.write_sequence(root, 'ball', verts, faces, K, frames, masks, flows, np.zeros((T - 1, H, W), np.float32), colors)
    out = os.path.join(root, 'scores', 'reproj.json')
    rc = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'eval_reproj.py'), '--testdir', test, '--seqname', 'ball',
                         '--outpath', out, '--worst', '2', '--bound_th', '2'], cwd=root, timeout=600, capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    print(rc.stdout.strip())
    doc = json.load(open(out))
    # the same files through the same loaders, scored in this process
    monkeypatch.chdir(root)
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import eval_reproj
    import render_vis
    loaded = [render_vis.load_mesh(test, i) for i in range(T)]
    tv = torch.stack([m[0] for m in loaded]).to(cuda)
    tco = torch.stack([m[2] for m in loaded]).to(cuda)
    tf, tK, tm, tfl, tfr = _dev(cuda, faces, K, (masks != 0).astype(np.uint8), flows, frames)
    res = rp.evaluate(tv, tf, tK, tm, flows=tfl, occs=torch.zeros(T - 1, H, W, device=cuda), frames=tfr, colors=tco, bound_th=2)
    assert doc['frame_ids'] == list(range(T)) and doc['radius'] == 2 and doc['params']['flow_pairs'] == T - 1 and doc['params']['colours']
    for k in ('J', 'F', 'epe', 'psnr'):
        x = res[k][np.isfinite(res[k])]
        assert doc['means'][k] == float(x.mean()), k
    assert doc['means']['JF'] == float(((res['J'] + res['F']) / 2).mean()) and doc['nan_frames']['epe'] == 1
    assert doc['per_frame']['n_flow'] == res['n_flow'].tolist() and doc['per_frame']['J'] == res['J'].tolist()
    assert 0.2 < doc['means']['epe'] < 0.5 and 0.8 < doc['means']['J'] < 1. and min(doc['per_frame']['n_rgb']) > 500
    lines = rc.stdout.splitlines()
    assert lines[0] == eval_reproj.summary_line(doc) and len(lines) == 3
    assert lines[1].startswith('worst: frame 2 (position 2) ') and int(np.argmin(doc['per_frame']['JF'])) == 2
