"""Texture bake on the device (lasr_amd/nnutils/bake.py, csrc/bake.hip) against closed forms and the float64 restatement
(tests/bake_restated.py).  The bake is this project's own addition: the restatement is the only parity there is.

Measured on an MI355X (each test prints its figures before it asserts):
  case 4, undecided share: 0.000 % (R 3), 0.278 % (R 3, masks), 0.195 % (R 8), 0.391 % (R 8, masks); cap 2 %.  Weight error
    at most 2.8e-6 relative (bound 1e-4), texture error at most 3.4e-7 (bound 1.08e-4 with G = 0.098).
  case 6, worst error / bound: 0.459 (R 3), 0.410 (R 8) over 316 pixels.
  case 7 (256 x 256, 5 frames, 1280 faces, R 8): seen 57.6 %; mean absolute colour error inside the eroded silhouette, 0-255:
    baked preview 8.32, flat mean foreground colour 74.08.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bake_restated as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
H, W, IS = br.H, br.W, br.IS
RAMP = (1., 3., 10.)                       # a, b, c of the uint8-exact ramp: a != b, so a row / column swap shows


def _bake():
    from lasr_amd.nnutils import bake
    return bake


def _dev(cuda, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _run(cuda, verts, faces, K, frames, masks=None, R=4, power=2, fallback=None):
    tv, tf, tK, tfr, tm, tfb = _dev(cuda, verts, faces, K, frames, masks, fallback)
    tex, w = _bake().bake_texture(tv, tf, tK, tfr, tm, texture_res=R, power=power, fallback=tfb)
    torch.cuda.synchronize()
    return tex.cpu().numpy(), w.cpu().numpy()


def _plane(cuda, verts, faces, K):
    """The device raster's own face-index plane [T,IS,IS]."""
    tv, tf, tK = _dev(cuda, verts, faces, K)
    return _bake().face_index_raster(tv, tf.int(), tK, IS)[:, 1].cpu().numpy()


def _away_from(x, offset):
    y = x - offset
    return np.abs(y - np.round(y)) >= br.UNDECIDED_PX


TRI_V = np.array([[[-0.55, -0.4, 2.], [0.6, -0.3, 2.], [-0.1, 0.5, 2.]]], np.float32)     # fronto-parallel, z constant
TRI_K = np.array([[40., 38., 32.25, 24.5]], np.float32)


def test_convention_closed_form(cuda):
    a, b, c = RAMP
    frames = br.ramp_image(a, b, c)[None]
    R = 4
    faces = np.array([[0, 1, 2]])
    tex, w = _run(cuda, TRI_V, faces, TRI_K, frames, R=R)
    _, u, v = br.project(TRI_V, faces, TRI_K, R)
    assert (w > 0).all()                                             # every centroid lies a texel's third inside the triangle
    assert u.min() > 1 and u.max() < W - 1 and v.min() > 1 and v.max() < H - 1
    for ch in range(3):
        want = (a * u[0] + b * v[0] + c + ch) / 255.
        err = np.abs(tex[..., ch] - want).max()
        print('channel %d: max error %.3e' % (ch, err))
        assert err <= 1e-5 + 0.5 / 255
    # corners 1 and 2 swapped: texel j now samples the point the texel of (c0, c2) sampled
    tex_sw, w_sw = _run(cuda, TRI_V, faces[:, [0, 2, 1]], TRI_K, frames, R=R)
    c0, c1, c2 = br.centroids(R)
    perm = np.array([br.surface_texel(float(p), float(q), R) for p, q in zip(c0, c2)])
    assert sorted(perm) == list(range(R * R)) and (perm != np.arange(R * R)).any()
    # the same 3-D point up to float32 rounding of the centroid (1e-7 of 64 px) under a gradient of 3/255 per pixel
    assert np.abs(tex_sw[0] - tex[0][perm]).max() <= 1e-5
    assert np.abs(w_sw[0] - w[0][perm]).max() <= 1e-5


def test_occlusion(cuda):
    # face 0 in front (z = 2) covers part of face 1 behind it (z = 3, parallel); two frames, same geometry, other colours
    front = TRI_V[0] * np.array([0.7, 0.7, 1.], np.float32) + np.array([0.25, 0.05, 0.], np.float32)
    back = TRI_V[0] * np.array([1.5, 1.5, 1.5], np.float32)
    verts = np.repeat(np.concatenate([front, back])[None], 2, 0)
    faces = np.array([[0, 1, 2], [3, 4, 5]])
    K = np.repeat(TRI_K, 2, 0)
    frames = np.stack([np.full((H, W, 3), 51, np.uint8), np.full((H, W, 3), 153, np.uint8)])
    fallback = np.random.default_rng(0).uniform(0, 1, (6, 3)).astype(np.float32)
    R = 4
    tex, w = _run(cuda, verts, faces, K, frames, R=R, fallback=fallback)
    plane = _plane(cuda, verts, faces, K)
    _, u, v = br.project(verts, faces, K, R)
    clear = _away_from(u[0], 0.) & _away_from(v[0], 0.)              # the nearest pixel is not a matter of rounding
    owner = plane[0][np.floor(v[0]).astype(int), np.floor(u[0]).astype(int)]            # [2, R*R]
    hidden = (owner[1] == 0) & clear[1]
    shown = (owner[1] == 1) & clear[1]
    print('back face: %d texels hidden by the front face, %d seen; front face: %d seen'
          % (hidden.sum(), shown.sum(), ((owner[0] == 0) & clear[0]).sum()))
    assert hidden.sum() >= 2 and shown.sum() >= 2 and ((owner[0] == 0) & clear[0]).sum() >= 2
    for f in (0, 1):                                                 # seen exactly where the raster names the face itself
        assert (w[f][(owner[f] == f) & clear[f]] > 0).all() and (w[f][(owner[f] != f) & clear[f]] == 0).all()
    c0, c1, c2 = br.centroids(R)
    fb = c0[:, None] * fallback[3] + c1[:, None] * fallback[4] + c2[:, None] * fallback[5]
    assert np.abs(tex[1][hidden] - fb[hidden]).max() <= 1e-6
    seen = w > 0
    assert np.abs(tex[seen] - 0.4).max() <= 1e-6                     # equal weights in both frames: (51 + 153) / 2 / 255


def test_masks(cuda):
    a, b, c = RAMP
    frames = br.ramp_image(a, b, c)[None]
    masks = np.zeros((1, H, W), np.uint8)
    masks[:, :, :30] = 128                                           # a half plane: columns 0 .. 29
    R = 4
    faces = np.array([[0, 1, 2]])
    tex, w = _run(cuda, TRI_V, faces, TRI_K, frames, masks, R=R)
    _, u, v = br.project(TRI_V, faces, TRI_K, R)
    clear = _away_from(u[0, 0], 0.5)
    x1 = np.floor(u[0, 0] - 0.5).astype(int) + 1                     # the right-hand taps' column
    inside = x1 <= 29
    print('%d texels with all four taps inside the mask, %d without' % ((inside & clear).sum(), (~inside & clear).sum()))
    assert (inside & clear).sum() >= 2 and (~inside & clear).sum() >= 2
    assert (w[0][~inside & clear] == 0).all() and (w[0][inside & clear] > 0).all()
    assert (tex[0][~inside & clear] == 0.5).all()                    # no fallback given: grey
    for ch in range(3):
        want = (a * u[0, 0] + b * v[0, 0] + c + ch) / 255.
        assert np.abs(tex[0, :, ch] - want)[inside & clear].max() <= 1e-5 + 0.5 / 255


@pytest.fixture(scope='module')
def sphere(cuda):
    verts, faces, K, frames, masks = br.icosphere_case()
    return dict(verts=verts, faces=faces, K=K, frames=frames, masks=masks, plane=_plane(cuda, verts, faces, K),
                G=br.max_gradient(frames))


@pytest.mark.parametrize('use_masks', [False, True])
@pytest.mark.parametrize('power', [0, 2])
@pytest.mark.parametrize('R', [3, 8])
def test_against_the_restatement(cuda, sphere, R, power, use_masks):
    s = sphere
    masks = s['masks'] if use_masks else None
    fallback = np.random.default_rng(1).uniform(0, 1, (42, 3)).astype(np.float32)
    tex, w = _run(cuda, s['verts'], s['faces'], s['K'], s['frames'], masks, R=R, power=power, fallback=fallback)
    rtex, rw, undecided = br.bake(s['verts'], s['faces'], s['K'], s['plane'], s['frames'], masks, R=R, power=power, fallback=fallback)
    share = undecided.mean()
    ok = ~undecided
    werr = (np.abs(w - rw) / np.maximum(rw, 1e-300))[ok & (rw > 0)].max()
    terr = np.abs(tex - rtex)[ok].max()
    bound = s['G'] * 1e-3 + 1e-5
    print('R %d power %d masks %s: undecided %.3f %%, seen %.1f %%, weight rel err %.3e, texture err %.3e (bound %.3e, G %.4f)'
          % (R, power, use_masks, 100 * share, 100 * (rw > 0).mean(), werr, terr, bound, s['G']))
    assert share <= 0.02
    assert (rw > 0).mean() > 0.5
    assert ((w > 0) == (rw > 0))[ok].all()
    assert werr <= 1e-4
    assert terr <= bound


def test_determinism_and_chunking(cuda, monkeypatch):
    bake = _bake()
    verts, faces, K, frames, masks = br.icosphere_case(T=5)
    assert bake.CHUNK_FRAMES >= 5
    one = _run(cuda, verts, faces, K, frames, masks, R=5)
    again = _run(cuda, verts, faces, K, frames, masks, R=5)
    assert np.array_equal(one[0], again[0]) and np.array_equal(one[1], again[1])
    tv, tf, tK, tfr, tm = _dev(cuda, verts, faces, K, frames, masks)
    a = bake.bake_texture(tv, tf, tK, tfr, tm, texture_res=5)
    monkeypatch.setattr(bake, 'CHUNK_FRAMES', 2)                     # chunks of 2, 2 and 1 frames
    b = bake.bake_texture(tv, tf, tK, tfr, tm, texture_res=5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert (a[1] > 0).float().mean() > 0.5


def test_python_layer_validates_its_arguments(cuda):
    bake = _bake()
    verts, faces, K, frames, masks = br.icosphere_case(T=1)
    tv, tf, tK, tfr, tm = _dev(cuda, verts, faces, K, frames, masks)
    bad = tf.clone()
    bad[3, 1] = 42
    with pytest.raises(ValueError, match='must index the 42 vertices'):
        bake.bake_texture(tv, bad, tK, tfr)
    with pytest.raises(ValueError, match='frames must be uint8'):
        bake.bake_texture(tv, tf, tK, tfr.float())
    with pytest.raises(ValueError, match='masks must be'):
        bake.bake_texture(tv, tf, tK, tfr, tm[:, :-1])
    with pytest.raises(ValueError, match='texture_res'):
        bake.bake_texture(tv, tf, tK, tfr, texture_res=33)
    with pytest.raises(ValueError, match='power'):
        bake.bake_texture(tv, tf, tK, tfr, power=17)
    with pytest.raises(TypeError):
        bake.bake_texture(tv.cpu(), tf, tK, tfr)


@pytest.mark.parametrize('R', [3, 8])
def test_round_trip_through_the_renderer(cuda, sphere, R):
    bake = _bake()
    s = sphere
    a, b, c = RAMP
    frame = br.ramp_image(a, b, c)
    verts, K = s['verts'][:1], s['K'][:1]
    tv, tf, tK, tfr = _dev(cuda, verts, s['faces'], K, frame[None])
    tex, w = bake.bake_texture(tv, tf, tK, tfr, texture_res=R)
    img = bake.render_baked(tv, tf, tK, tex, H, W)[0].permute(1, 2, 0).cpu().numpy()      # H,W,4
    plane = s['plane'][0][:H, :W]
    g = np.hypot(a, b) / 255.                                        # the ramp's gradient per pixel, 0-1 units
    u = K[0, 0] * verts[0, :, 0] / verts[0, :, 2] + K[0, 2]
    v = K[0, 1] * verts[0, :, 1] / verts[0, :, 2] + K[0, 3]
    tri = np.stack([u, v], 1).astype(np.float64)[s['faces']]                              # F,3,2
    edge = np.linalg.norm(tri - np.roll(tri, 1, axis=1), axis=2).max(1)                   # longest projected edge, pixels
    checked, worst = 0, 0.
    for r in range(1, H - 1):
        for col in range(1, W - 1):
            f = plane[r, col]
            if f < 0 or not (plane[r - 1:r + 2, col - 1:col + 2] == f).all():
                continue
            bound = g * edge[int(f)] / R + 1. / 255
            err = np.abs(img[r, col, :3] - frame[r, col] / 255.).max()
            checked += 1
            worst = max(worst, err / bound)
            assert img[r, col, 3] > 0.5 and err <= bound, (r, col, int(f), err, bound)
    print('R %d: %d pixels checked, worst error / bound %.3f' % (R, checked, worst))
    assert checked >= 200


def _iou(a, b):
    return float((a & b).sum()) / max(float((a | b).sum()), 1.)


def _erode(m, n):
    for _ in range(n):
        p = np.pad(m, 1)
        m = p[1:-1, 1:-1] & p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return m


def test_script_end_to_end(cuda, tmp_path):
    from PIL import Image, ImageSequence
    from lasr_amd.nnutils.mesh_net import quaternion_to_rotation_matrix
    from lasr_amd.soft_renderer.functional import load_obj, save_obj
    root, n, size, focal, R = str(tmp_path), 5, 256, 10., 8
    rc = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'render_syn.py'), '--outdir', 'bake5', '--nframes', str(n),
                         '--img_size', str(size), '--root', root, '--surface_tex'], cwd=root, timeout=600, capture_output=True,
                        text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    base = os.path.join(root, 'database', 'DAVIS')
    test = os.path.join(root, 'bake-out')
    os.makedirs(test)
    for i in range(n):                                               # the ground truth stands in for extract.py's output
        v, f = load_obj(os.path.join(base, 'Meshes', 'Full-Resolution', 'bake5', '%05d.obj' % i))
        save_obj(os.path.join(test, 'pred%d.obj' % i), v.cpu(), f.cpu())
        cam = np.loadtxt(os.path.join(base, 'Camera', 'Full-Resolution', 'bake5', '%05d.txt' % i))
        rtk = np.zeros((4, 4))
        rtk[:3, :3] = quaternion_to_rotation_matrix(torch.tensor(np.r_[cam[4:7], cam[3]]).float()).numpy()
        rtk[:3, 3] = (0, 0, cam[7])
        rtk[3] = (focal * size / 2, focal * size / 2, size / 2, size / 2)
        np.savetxt(os.path.join(test, 'cam%d.txt' % i), rtk)
    F = f.shape[0]
    out, gif = os.path.join(root, 'atlas', 'baked'), os.path.join(root, 'preview.gif')
    rc = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'bake_texture.py'), '--testdir', test, '--seqname', 'bake5',
                         '--texture_res', str(R), '--outpath', out, '--preview', gif], cwd=root, timeout=600, capture_output=True,
                        text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    print(rc.stdout.strip())
    lines = open(out + '.obj').read().splitlines()
    assert sum(l.startswith('vt ') for l in lines) == 3 * F
    fl = [l.split() for l in lines if l.startswith('f ')]
    assert len(fl) == F and all(len(t) == 4 and all(x.count('/') == 1 for x in t[1:]) for t in fl)
    tile_w = int((F - 1.) ** 0.5) + 1
    tile_h = int((F - 1.) / tile_w) + 1
    assert Image.open(out + '.png').size == (tile_w * R, tile_h * R)
    assert 'map_Kd baked.png' in open(out + '.mtl').read()
    weight = np.load(out + '_weight.npy')
    assert weight.shape == (F, R * R)
    seen = 100. * float((weight > 0).mean())
    line = [l for l in rc.stdout.splitlines() if l.startswith('baked ')]
    assert line == ['baked %d faces x %d texels, seen %.1f %%' % (F, R * R, seen)] and seen > 0

    g = Image.open(gif)
    assert g.n_frames == n and g.size == (2 * size, size)
    frames = np.stack([np.asarray(fr.convert('RGB')) for fr in ImageSequence.Iterator(g)]).astype(np.float64)
    preview = frames[:, :, size:]
    jpg = np.stack([np.asarray(Image.open(os.path.join(base, 'JPEGImages', 'Full-Resolution', 'bake5', '%05d.jpg' % i)).convert('RGB'))
                    for i in range(n)]).astype(np.float64)
    sil = np.stack([np.asarray(Image.open(os.path.join(base, 'Annotations', 'Full-Resolution', 'bake5', '%05d.png' % i)))
                    for i in range(n)]) > 0
    for i in range(n):
        got = preview[i].sum(2) > 24                                 # the render's background is black, the object never is
        assert _iou(got, sil[i]) >= 0.99, (i, _iou(got, sil[i]))
    inner = np.stack([_erode(m, 2) for m in sil])
    mean_fg = jpg[sil].mean(0)
    err_bake = np.abs(preview - jpg)[inner].mean()
    err_flat = np.abs(mean_fg[None, None, None] - jpg)[inner].mean()
    print('mean absolute colour error inside the eroded silhouette (0-255): baked preview %.2f, flat mean colour %.2f' % (err_bake, err_flat))
    assert err_bake < err_flat
