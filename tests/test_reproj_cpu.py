"""Reprojection scores without a device: closed forms of the float64 restatement (tests/reproj_restated.py), the flow fixture
tests/test_reproj_gpu.py compares on and the tolerances derived from it, the header against the binding, the C ABI's host-side
checks and scripts/eval_reproj.py with the restated evaluate injected.

Flow fixture (tracks_cases.sphere_case(), 5 frames of 48 x 64, hand-made raster planes; test_flow_fixture_and_its_tolerances prints
the figures): 3309 flow pixels and 4962 colour pixels; the restatement in float32 differs from float64 by at most 1.494e-5 px in a
pixel's epe and 0.3091 in its squared colour difference (reproj_restated.EPE_SPREAD = 1.5e-5, SQ_SPREAD = 0.31).  The GPU
tolerances are 8 x these, the project's rule: 1.2e-4 px on the mean epe, 2.48 on the mean squared colour difference (of about
2.4e4).  No pixel has a float64 epe within 1.2e-4 px of 1 or 3 (cap 0.5 %); 407 / 2902 pixels lie below / above 1 px, 2258 / 1051
below / above 3 px.
"""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

import reproj_restated as rr
import tracks_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADII = (0, 1, 3, 7, 12, 96)


def _square(H, W, r0, r1, c0, c1):
    m = np.zeros((H, W), bool)
    m[r0:r1, c0:c1] = True
    return m


def _score(pred, gt, rho):
    c = rr.silhouette_counts(pred, gt, rho)
    return c, rr.scores(c)


@pytest.mark.parametrize('rho', RADII)
def test_identical_and_empty_masks(rho):
    pred, gt = rr.pair(37, 53)
    c, s = _score(gt, gt, rho)
    assert s['J'] == 1. and s['F'] == 1. and c['pm'] == c['n_pb'] == c['n_gb'] == c['gm'] > 0
    empty = np.zeros((37, 53), bool)
    c, s = _score(empty, empty, rho)
    assert c['union'] == 0 and c['n_pb'] == 0 and s == dict(J=1., precision=1., recall=1., F=1.)
    c, s = _score(empty, _square(37, 53, 10, 20, 10, 20), rho)
    assert s == dict(J=0., precision=1., recall=0., F=0.) and c['n_gb'] > 0
    c, s = _score(_square(37, 53, 10, 20, 10, 20), empty, rho)
    assert s == dict(J=0., precision=0., recall=1., F=0.)


@pytest.mark.parametrize('d', [1, 3, 5])
def test_shifted_square(d):
    H, W, w = 40, 60, 16
    gt = _square(H, W, 10, 26, 12, 12 + w)
    pred = _square(H, W, 10, 26, 12 + d, 12 + d + w)
    for rho in (0, 1, 2, 3, 4, 5, 7):
        c, s = _score(pred, gt, rho)
        assert c['inter'] * (w + d) == c['union'] * (w - d) and abs(s['J'] - (w - d) / (w + d)) < 1e-15
        bp, bg = rr.boundary(pred), rr.boundary(gt)
        hit = bp & rr.dilate(bg, rho)
        # the vertical edges of pred lie d columns from those of gt: six rows or more from the corners they match only at rho >= d
        left, right = hit[16:20, 12 + d - 1], hit[16:20, 12 + d + w - 1]
        assert bp[16:20, 12 + d - 1].all() and bp[16:20, 12 + d + w - 1].all()
        assert left.all() == right.all() == (rho >= d) and left.any() == (rho >= d)
        assert hit[9, 12 + d:12 + w].all()                                    # the top edge coincides over the shared columns


def test_border_rule_of_the_boundary_map():
    H, W = 6, 9
    for r, c, want in ((H - 1, 3, [(H - 2, 2), (H - 2, 3), (H - 1, 2), (H - 1, 3)]),      # last row
                       (2, W - 1, [(1, W - 2), (1, W - 1), (2, W - 2), (2, W - 1)]),      # last column
                       (H - 1, W - 1, [(H - 2, W - 2), (H - 2, W - 1), (H - 1, W - 2)])):  # the last pixel itself is 0
        m = np.zeros((H, W), bool)
        m[r, c] = True
        assert sorted(zip(*np.nonzero(rr.boundary(m)))) == sorted(want), (r, c)
    full = np.ones((H, W), bool)
    assert not rr.boundary(full).any()                                        # nothing differs inside, and the border rule adds nothing


@pytest.mark.parametrize('size', [(9, 7), (37, 53), (64, 80), (70, 130)])
def test_row_run_form_equals_disk_dilation(size):
    pred, gt = rr.pair(*size)
    for rho in RADII:
        for m in (rr.boundary(pred), rr.boundary(gt), pred):
            assert np.array_equal(rr.dilate_rows(m, rho), rr.dilate(m, rho)), (size, rho)
    assert rr.disk(0).shape == (1, 1) and rr.disk(3).sum() == 29 and rr.disk(96).shape == (193, 193)


def test_mask_pairs_tell_the_radii_apart():
    pred, gt = rr.pair(64, 80)
    got = {rho: rr.silhouette_counts(pred, gt, rho) for rho in (0, 1, 3, 7, 12)}
    assert [got[r]['pm'] for r in (0, 1, 3, 7)] == [54, 86, 143, 170]
    assert all(c['n_pb'] == 175 and c['n_gb'] == 176 for c in got.values())
    assert got[7]['gm'] == got[12]['gm'] == 176 and got[7]['pm'] == got[12]['pm'] == 170     # the speck stays out of reach
    assert pred[:2, -3:].all() and not gt[:2, -3:].any()
    assert np.array_equal(rr.pack_bits(pred)[3], np.array([sum(1 << c for c in range(64) if pred[3, c]),
                                                           sum(1 << (c - 64) for c in range(64, 80) if pred[3, c])], np.uint64))
    assert rr.radius_of(0.008, 1080, 1920) == 18 and rr.radius_of(0.008, 8192, 8192) == 93 and rr.radius_of(0, 5, 5) == 0
    assert rr.radius_of(7, 5, 5) == 7


def test_flow_fixture_and_its_tolerances():
    fx = rr.flow_fixture()
    planes = tc.face_index(fx['verts'], fx['faces'], fx['K'])
    masks, flows, occs = rr.observed_flow(fx, planes)
    args = (fx['verts'], fx['faces'], fx['K'], planes, masks, flows, occs, fx['frames'], fx['colors'])
    a, b = rr.evaluate(*args), rr.evaluate(*args, dtype=np.float32)
    assert (a['n_flow'] == b['n_flow']).all() and (a['n_rgb'] == b['n_rgb']).all()
    e64, e32 = np.concatenate(a['epe_px']), np.concatenate(b['epe_px'])
    s64, s32 = np.concatenate(a['sq_px']), np.concatenate(b['sq_px'])
    spread, sq_spread = np.abs(e64 - e32).max(), np.abs(s64 - s32).max()
    tol = 8 * rr.EPE_SPREAD
    near = [int((np.abs(e64 - th) <= tol).sum()) for th in (1., 3.)]
    sides = [(int((e64 < th).sum()), int((e64 > th).sum())) for th in (1., 3.)]
    print('flow fixture: %d flow pixels, %d colour pixels, float32 / float64 spread %.3e px in epe and %.4f in sq (largest sq %.3e); '
          'within %.1e px of 1 / 3: %s; below / above: %s; epe %.3f .. %.3f'
          % (len(e64), len(s64), spread, sq_spread, s64.max(), tol, near, sides, e64.min(), e64.max()))
    assert rr.EPE_SPREAD / 2 <= spread <= rr.EPE_SPREAD and rr.SQ_SPREAD / 2 <= sq_spread <= rr.SQ_SPREAD
    assert max(near) <= 0.005 * len(e64)
    assert min(min(s) for s in sides) >= 50
    assert e64.min() < 0.1 and 4.5 < e64.max() < 5.5                          # the smooth field spreads epe over 0 .. 5 px
    assert a['n_flow'][-1] == 0 and np.isnan(a['epe'][-1]) and (a['n_flow'][:-1] > 500).all()
    # the invalid column band and the occluded row band are really left out
    covered = (planes[:, :fx['H'], :fx['W']] >= 0)
    for t in range(4):
        valid = covered[t].copy()
        valid[:, 30:34] = False
        valid[20:23] = False
        assert a['n_flow'][t] == valid.sum() < covered[t].sum() == a['n_rgb'][t]
    # an observed flow equal to the rendered one scores 0
    zero = flows.copy()
    for t in range(4):
        r, c, fp = a['flow_px'][t]
        zero[t, r, c, :2] = fp
    z = rr.evaluate(fx['verts'], fx['faces'], fx['K'], planes, masks, zero, occs)
    assert np.nanmax(z['epe']) <= 1e-6 and (z['n_le1'] == z['n_flow']).all()


def _header():
    return open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()


def test_header_against_the_binding():
    from lasr_amd import _lib
    hdr = _header()
    assert '#define LASR_REPROJ_MAX_RADIUS 96\n' in hdr and _lib.REPROJ_MAX_RADIUS == 96 == rr.MAX_RADIUS
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    ctype = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t}
    for name in ('lasr_reproj_workspace_bytes', 'lasr_reproj_pixels', 'lasr_reproj_boundary'):
        m = re.search(r'(\w+)\s+%s\((.*?)\);' % name, code, re.S)
        assert m, name
        params = [' '.join(p.split()) for p in m.group(2).split(',')]
        want = [ctypes.c_void_p if '*' in p else ctype[p.split()[0]] for p in params]
        res, args = _lib.SIGNATURES[name]
        assert res is ctype[m.group(1)] and args == want, name
    assert len(_lib.SIGNATURES['lasr_reproj_pixels'][1]) == 22 and len(_lib.SIGNATURES['lasr_reproj_boundary'][1]) == 8
    from lasr_amd.nnutils import reproj
    assert reproj.COUNTS == rr.COUNTS and len(reproj.COUNTS) == 12
    slots = re.search(r'counts uint64 \[n,12\].*?n_rgb', hdr, re.S).group(0)
    assert [k for k in re.findall(r'\b(inter|union|n_pred|n_gt|n_pb|n_gb|pm|gm|n_flow|n_le1|n_le3|n_rgb)\b', slots)][:12] == list(rr.COUNTS)


def test_host_checks_run_without_a_device():
    from lasr_amd import _lib
    h = _lib.lib()
    n, x = None, 8                                                           # x: a non-NULL pointer no launch ever sees

    def pix(nf=1, V=3, F=1, IS=64, H=48, W=64, base=x, nxt=(n, n, n, n), rgb=(n, n)):
        vn, kn, fl, oc = nxt
        return h.lasr_reproj_pixels(base, vn, base, base, kn, base, base, fl, oc, rgb[0], rgb[1], base, base, base, base, nf, V, F, IS,
                                    H, W, n)
    assert pix(nf=0) == 0 and pix(nf=0, base=n) == 0                          # empty work: nothing launched, nothing checked
    assert pix(base=n) == -1                                                  # null buffers
    assert pix(nf=-1) == -1 and pix(nf=0, V=0) == -1 and pix(nf=0, F=-1) == -1 and pix(nf=0, F=0) == 0
    assert pix(nf=0, H=0) == -1 and pix(nf=0, W=0) == -1 and pix(nf=0, H=65) == -1 and pix(nf=0, W=65) == -1   # H, W > IS
    assert pix(nf=0, IS=8193, H=1, W=8193) == -1 and pix(nf=0, IS=8192, H=1, W=8192) == 0
    assert pix(nf=0, F=(1 << 24) + 1) == -1
    for half in ((x, n, n, n), (n, x, n, n), (n, n, x, n), (x, x, n, n), (x, n, x, n), (n, x, x, n), (n, n, n, x), (x, x, n, x)):
        assert pix(nf=0, nxt=half) == -1, half                                # the flow group given in part
    assert pix(nf=0, nxt=(x, x, x, n)) == 0 and pix(nf=0, nxt=(x, x, x, x)) == 0
    assert pix(nf=0, rgb=(x, n)) == -1 and pix(nf=0, rgb=(n, x)) == -1 and pix(nf=0, rgb=(x, x)) == 0

    bnd = lambda nf=1, H=48, W=64, r=3, p=n: h.lasr_reproj_boundary(p, p, p, nf, H, W, r, n)                     # noqa: E731
    assert bnd(nf=0) == 0 and bnd() == -1 and bnd(nf=-1) == -1
    assert bnd(nf=0, r=-1) == -1 and bnd(nf=0, r=97) == -1 and bnd(nf=0, r=96) == 0 and bnd(nf=0, r=0) == 0
    assert bnd(nf=0, H=0) == -1 and bnd(nf=0, W=0) == -1 and bnd(nf=0, W=8193) == -1 and bnd(nf=0, H=8192, W=8192) == 0
    ws = h.lasr_reproj_workspace_bytes
    assert ws(-1, 48, 64) == 0 and ws(1, 0, 64) == 0 and ws(1, 48, 8193) == 0 and ws(0, 48, 64) == 0
    assert ws(1, 48, 64) == 3 * 16 and ws(3, 49, 65) == 3 * 4 * 2 * 16 and ws(2, 1, 1) == 2 * 16        # a workgroup: 16 rows of 64 columns
    names = [h.lasr_prof_kernel_name(i) for i in range(h.lasr_prof_kernel_count())]
    assert not any(b'reproj_' in k for k in names)                            # these launches stay out of the kernel-name table


def test_python_layer_refuses_cpu_tensors_and_derives_the_radius():
    import torch
    from lasr_amd.nnutils import reproj
    v, f, K, m = torch.zeros(1, 3, 3), torch.tensor([[0, 1, 2]]), torch.ones(1, 4), torch.zeros(1, 4, 4)
    with pytest.raises(TypeError):
        reproj.evaluate(v, f, K, m)
    with pytest.raises(TypeError, match='masks must be a tensor'):
        reproj.evaluate(v, f, K, m.numpy())
    assert reproj.radius_of(0.008, 1080, 1920) == 18 and reproj.radius_of(0, 48, 64) == 0 and reproj.radius_of(12, 48, 64) == 12
    assert reproj.radius_of(0.008, 48, 64) == rr.radius_of(0.008, 48, 64) == 1 and reproj.radius_of(96, 9, 9) == 96
    for bad in (-0.1, 97, 2.5, float('nan')):
        with pytest.raises(ValueError):
            reproj.radius_of(bad, 48, 64)
    # the host's share of the definition: precision, recall and F from the counts, NaN where nothing was counted
    c = np.zeros((4, 12), np.int64)
    c[0, 4:8] = (0, 5, 0, 0)
    c[1, 4:8] = (5, 0, 0, 0)
    c[3, :] = (30, 40, 35, 35, 10, 8, 5, 6, 4, 1, 3, 2)
    got = reproj.metrics(c, np.array([[0., 0.], [0., 0.], [0., 0.], [6., 2. * 3 * 255. ** 2 / 100]]))
    assert got['precision'].tolist() == [1., 0., 1., .5] and got['recall'].tolist() == [0., 1., 1., .75]
    assert got['F'].tolist() == [0., 0., 1., 2 * .5 * .75 / 1.25] and got['J'].tolist() == [1., 1., 1., .75]
    assert np.isnan(got['epe'][:3]).all() and np.isnan(got['psnr'][:3]).all() and got['epe'][3] == 1.5
    assert got['pck1'][3] == .25 and got['pck3'][3] == .75 and abs(got['psnr'][3] - 20.) < 1e-12
    words = rr.pack_bits(rr.pair(33, 129)[0])
    assert np.array_equal(reproj.unpack_bits(words, 129), rr.pair(33, 129)[0]) and words.shape == (33, 3)


# ---- the script ---------------------------------------------------------------------------------------------------------------------------
def _script():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import eval_reproj
    return eval_reproj


def _restated_evaluate(seen):
    def evaluate(verts, faces, K, masks, flows=None, occs=None, frames=None, colors=None, bound_th=0.008):
        planes = tc.face_index(verts, faces, K, masks.shape[1], masks.shape[2])
        res = rr.evaluate(verts, faces, K, planes, masks, flows, occs, frames, colors, bound_th)
        pred = (planes >= 0)
        res['boundary'] = np.stack([np.stack([rr.boundary(p), rr.boundary(m != 0)]) for p, m in zip(pred, masks)])
        seen.update(res=res, flows=flows, occs=occs, frames=frames, colors=colors, masks=masks, verts=verts)
        return res
    return evaluate


def test_script_arguments_and_path_substitution():
    er = _script()
    a = er.parse_args(['--testdir', 'log/camel-5/', '--seqname', 'camel'])
    assert (a.bound_th, a.outpath, a.vis, a.worst) == (0.008, '', '', 5)
    a = er.parse_args('--testdir t --seqname s --bound_th 3 --outpath o/r.json --vis v --worst 2'.split())
    assert (a.testdir, a.seqname, a.bound_th, a.outpath, a.vis, a.worst) == ('t', 's', 3., 'o/r.json', 'v', 2)
    name = 'database/DAVIS/JPEGImages/Full-Resolution/camel/00004.jpg'
    assert er.annotation_path(name) == 'database/DAVIS/Annotations/Full-Resolution/camel/00004.png'
    assert er.flow_paths(name, 1) == ('database/DAVIS/FlowFW/Full-Resolution/camel/flo-00004.pfm',
                                      'database/DAVIS/FlowFW/Full-Resolution/camel/occ-00004.pfm')
    assert er.flow_paths(name, 2) == ('database/DAVIS/FlowFW/Full-Resolution/camel_02/flo-00004.pfm',
                                      'database/DAVIS/FlowFW/Full-Resolution/camel_02/occ-00004.pfm')
    # the loader's own lists (lasr_amd/dataloader/vid.py) name the same files
    import types
    from lasr_amd.dataloader.vid import VidDataset
    for dframe in (1, 2):
        imgs = ['database/DAVIS/JPEGImages/Full-Resolution/camel/%05d.jpg' % i for i in range(6)]
        ds = VidDataset(types.SimpleNamespace(sil_path='none', batch_size=1, ngpu=1, img_size=8), imglist=imgs, dframe=dframe)
        assert [er.annotation_path(i) for i in imgs] == ds.masklist
        assert [er.flow_paths(i, dframe)[0] for i in imgs] == ds.flowfwlist
    f = np.array([[0, 1, 2], [0, 2, 3]])
    with pytest.raises(ValueError, match='pred7 does not share the topology of pred5'):
        er.check_topology([f, f, f[:, ::-1]], [5, 6, 7])


def _sequence(tmp_path, monkeypatch, **kw):
    verts, faces, K = tc.quad_case()
    T = len(verts)
    rng = np.random.default_rng(2)
    frames = rng.integers(0, 256, (T, tc.H, tc.W, 3), dtype=np.uint8)
    planes = tc.face_index(verts, faces, K)
    masks = (planes >= 0).astype(np.uint8) * 255
    masks[1] = np.roll(masks[1], 6, axis=1)                                   # frame 1's annotation sits 6 px to the right
    flows = np.zeros((T - 1, tc.H, tc.W, 3), np.float32)
    flows[..., 2] = 1.
    flows[2, ..., 2] = 0.                                                      # a pair whose flow is all invalid: epe NaN there too
    colors = rng.integers(0, 256, (T, 4, 3), dtype=np.uint8)
    test = rr.write_sequence(str(tmp_path), 'quad', verts, faces, K, frames, masks, flows, None, colors, **kw)
    monkeypatch.chdir(tmp_path)
    return test, dict(verts=verts, faces=faces, K=K, frames=frames, masks=masks, flows=flows, colors=colors)


def test_script_json_means_and_overlays(tmp_path, monkeypatch, capsys):
    er = _script()
    test, data = _sequence(tmp_path, monkeypatch, dframe=2)
    seen = {}
    vis = str(tmp_path / 'vis')
    doc = er.main(['--testdir', test, '--seqname', 'quad', '--bound_th', '2', '--vis', vis, '--worst', '2'], evaluate=_restated_evaluate(seen))
    res = seen['res']
    assert np.array_equal(seen['masks'], (data['masks'] != 0).astype(np.uint8)) and np.array_equal(seen['frames'], data['frames'])
    assert np.array_equal(seen['flows'], data['flows']) and np.array_equal(seen['colors'], data['colors'])
    assert not seen['occs'].any()                                              # no occ-*.pfm: nothing counts as occluded
    on_disk = json.load(open(os.path.join(test, 'reproj.json')))
    assert on_disk == json.loads(json.dumps(doc))
    assert sorted(doc) == ['frame_ids', 'means', 'nan_frames', 'params', 'per_frame', 'radius']
    assert doc['frame_ids'] == [0, 2, 4, 6] and doc['radius'] == 2
    assert doc['params'] == dict(testdir=test, seqname='quad', bound_th=2., dframe=2, size=[tc.H, tc.W], flow_pairs=3, colours=True)
    assert sorted(doc['per_frame']) == sorted(er.PER_FRAME + er.COUNTS + ('JF',))
    assert doc['per_frame']['epe'][2] is None and doc['per_frame']['epe'][3] is None and doc['per_frame']['epe'][0] is not None
    assert doc['nan_frames'] == dict(J=0, F=0, JF=0, epe=2, psnr=0)
    assert doc['means']['epe'] == float(np.mean(res['epe'][:2])) and doc['means']['J'] == float(res['J'].mean())
    assert doc['means']['JF'] == float(((res['J'] + res['F']) / 2).mean()) and doc['means']['psnr'] == float(res['psnr'].mean())
    assert doc['per_frame']['n_flow'] == [int(x) for x in res['n_flow']] and doc['per_frame']['J'][0] == 1.
    lines = capsys.readouterr().out.splitlines()
    assert lines[-4] == er.summary_line(doc) and lines[-4].startswith('reproj: 4 frames, J ')
    assert lines[-3].startswith('worst: frame 2 (position 1) J ') and lines[-2].startswith('worst: frame ')
    assert lines[-1] == 'wrote 4 overlays to %s' % vis
    from PIL import Image
    assert sorted(os.listdir(vis)) == ['reproj-%05d.png' % i for i in (0, 2, 4, 6)]
    for pos, fr in ((0, 0), (1, 2)):
        img = np.asarray(Image.open(os.path.join(vis, 'reproj-%05d.png' % fr)))
        bp, bg = res['boundary'][pos]
        assert (img[bp & bg] == er.YELLOW).all() and (img[bp & ~bg] == er.RED).all() and (img[bg & ~bp] == er.GREEN).all()
        rest = ~(bp | bg)
        assert (img[rest] == data['frames'][pos][rest]).all()
    b0, b1 = res['boundary'][0], res['boundary'][1]
    assert (b0[0] == b0[1]).all() and b0[0].sum() > 50 and (b1[0] & ~b1[1]).sum() > 20 and (b1[1] & ~b1[0]).sum() > 20


def test_script_without_flow_and_its_refusals(tmp_path, monkeypatch, capsys):
    er = _script()
    from PIL import Image
    verts, faces, K = tc.quad_case()
    T = len(verts)
    frames = np.full((T, tc.H, tc.W, 3), 102, np.uint8)
    masks = (tc.face_index(verts, faces, K) >= 0).astype(np.uint8)
    test = rr.write_sequence(str(tmp_path), 'bare', verts, faces, K, frames, masks)      # .obj meshes, no FlowFW
    monkeypatch.chdir(tmp_path)
    seen = {}
    out = str(tmp_path / 'deep' / 'r.json')
    doc = er.main(['--testdir', test, '--seqname', 'bare', '--outpath', out, '--worst', '0'], evaluate=_restated_evaluate(seen))
    text = capsys.readouterr().out
    assert 'no FlowFW maps for bare: scored on silhouettes alone' in text and 'worst:' not in text
    assert seen['flows'] is None and seen['frames'] is None and seen['colors'] is None      # the .obj fallback's grey is not scored
    assert doc['means']['epe'] is None and doc['means']['psnr'] is None and doc['nan_frames']['epe'] == T and doc['means']['J'] == 1.
    assert os.path.exists(out) and doc['params']['flow_pairs'] == 0 and doc['params']['colours'] is False
    # an annotation of another size is an error, not a resize
    ann = os.path.join(str(tmp_path), 'database', 'DAVIS', 'Annotations', 'Full-Resolution', 'bare', '00002.png')
    Image.fromarray(np.zeros((tc.H, tc.W + 2), np.uint8)).save(ann)
    with pytest.raises(SystemExit, match=r'00002.png is 66 x 48, the frames are 64 x 48'):
        er.main(['--testdir', test, '--seqname', 'bare'], evaluate=_restated_evaluate({}))
    Image.fromarray(masks[2]).save(ann)
    from lasr_amd.soft_renderer.functional import save_obj
    import torch
    save_obj(os.path.join(test, 'pred3.obj'), torch.from_numpy(verts[3]), torch.from_numpy(faces[:, ::-1].copy()))
    with pytest.raises(SystemExit, match='pred3 does not share the topology of pred0'):
        er.main(['--testdir', test, '--seqname', 'bare'], evaluate=_restated_evaluate({}))
    with pytest.raises(SystemExit, match='no config for sequence nosuch'):
        er.main(['--testdir', test, '--seqname', 'nosuch'], evaluate=_restated_evaluate({}))
