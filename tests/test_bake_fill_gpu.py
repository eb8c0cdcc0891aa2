"""Atlas completion on the device (lasr_amd/nnutils/bake.py, csrc/bake_fill.hip) against the numpy restatement
(tests/bake_fill_restated.py) and closed forms.  The fill is this project's own addition: the restatement is the only parity
there is.  The blend must equal the float32 restatement bit for bit; the mirror must equal it exactly on the symmetric sphere
and is held to a membership test on the two asymmetric fixtures (every test prints its figures before it asserts).

bound = 4 x max |d2_f32 - d2_f64| + one float32 ulp of the largest d2, from the two restatements (test_bake_fill_cpu.py prints
the same figures): jittered sphere 2.907e-08 (R 3), 3.385e-08 (R 8); swollen sphere 1.434e-07 (R 3), 1.725e-07 (R 8).

Measured on an MI355X:
  blend: 0 differing bits in every case.  Affine field, border fixed, 7 iterations: largest change 1.19e-07 (bound 1e-6).
  symmetric sphere: 348 (R 3) / 2402 (R 8) texels listed, all filled, src equal to both restatements, largest d2 3.0e-14,
    colour error 0.
  |d2 - d2_f64| at most: jittered 7.24e-09 (R 3), 8.43e-09 (R 8); swollen 3.54e-08 (R 3), 4.27e-08 (R 8): a quarter of the bound.
    On the jittered sphere no closest point leaves the interior of a face (the texel centroids lie a third of a cell inside, and
    +-3 % moves the projection by less), so the device names the float64 face and texel everywhere; on the swollen sphere at
    R 8 it names another face than float64 for 8 of 2430 texels, each at most 2.8e-10 farther, and a touching texel always.
  script: 80 faces x 16 texels, seen 51.6 %, mirrored 38.4 %, blended 10.1 %; 634 of 1296 atlas pixels differ, all inside the 46
    tiles with a filled texel.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bake_fill_restated as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bake():
    from lasr_amd.nnutils import bake
    return bake


def _dev(cuda, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _meshes():
    grid_v, grid_f = fr.grid_case()
    sph_v, sph_f = fr.sphere_case()
    return {'grid': (grid_v, grid_f), 'sphere': (sph_v, sph_f)}


def _blend_raw(cuda, tex, fixed, nbr, R, iters):
    """lasr_bake_blend itself, ping-pong, with the restatement's nbr: the kernel apart from the torch adjacency."""
    from lasr_amd import _lib
    cur, tfixed, tnbr = _dev(cuda, tex.astype(np.float32), fixed.astype(np.uint8), nbr.astype(np.int32))
    bufs = [torch.empty_like(cur), torch.empty_like(cur)]
    for k in range(iters):
        _lib.call('lasr_bake_blend', cur, bufs[k & 1], tfixed, tnbr, nbr.shape[0], R)
        cur = bufs[k & 1]
    torch.cuda.synchronize()
    return cur.cpu().numpy()


@pytest.mark.parametrize('mesh,R', [('grid', 1), ('grid', 2), ('grid', 5), ('sphere', 3)])
def test_blend_equals_the_float32_restatement_bit_for_bit(cuda, mesh, R):
    bake = _bake()
    verts, faces = _meshes()[mesh]
    F = faces.shape[0]
    rng = np.random.default_rng(5 + R)
    tex = rng.uniform(0, 1, (F, R * R, 3)).astype(np.float32)
    fixed = (rng.uniform(0, 1, (F, R * R)) < 0.3).astype(np.uint8)
    nbr = fr.face_neighbours(faces, verts.shape[0])
    tf, = _dev(cuda, faces)
    got_nbr = bake.face_neighbours(tf, verts.shape[0]).cpu().numpy()
    assert got_nbr.dtype == np.int32 and (got_nbr == nbr).all()                    # the torch adjacency is the restatement's
    assert (bake.face_neighbours(tf).cpu().numpy() == nbr).all()
    for K in (1, 7):
        want = fr.blend(tex, fixed, nbr, R, K)
        raw = _blend_raw(cuda, tex, fixed, nbr, R, K)
        source = torch.from_numpy(np.where(fixed, 0, 2).astype(np.uint8)).to(cuda)
        got = bake.blend_fill(torch.from_numpy(tex).to(cuda), source, tf, iters=K).cpu().numpy()
        moved = (want != tex).any(2)
        print('%s R %d K %d: %d of %d texels moved, max |device - restatement| %.1e' % (mesh, R, K, moved.sum(), moved.size,
                                                                                     np.abs(raw - want).max()))
        assert want.dtype == np.float32 and moved.sum() > 0.5 * (fixed == 0).sum() and not moved[fixed != 0].any()
        assert np.array_equal(raw.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_blend_guards_and_the_affine_field(cuda):
    bake = _bake()
    verts, faces = _meshes()['grid']
    F, R = faces.shape[0], 5
    nbr = fr.face_neighbours(faces, verts.shape[0])
    # an nbr code that names a face outside [0, F) counts as no neighbour
    bad = nbr.copy()
    f, k = [(f, k) for f, k in zip(*np.nonzero(nbr >= 0))][3]
    bad[f, k] = (F * 3 + 1) * 2
    rng = np.random.default_rng(2)
    tex = rng.uniform(0, 1, (F, R * R, 3)).astype(np.float32)
    fixed = np.zeros((F, R * R), np.uint8)
    want = fr.blend(tex, fixed, bad, R, 2)
    assert (want != fr.blend(tex, fixed, nbr, R, 2)).any()
    assert np.array_equal(_blend_raw(cuda, tex, fixed, bad, R, 2).view(np.uint32), want.view(np.uint32))
    # an affine colour field with the border texels fixed stays where it is
    pts = fr.sample_points(verts, faces, np.arange(F * R * R), R, np.float64)
    field = (pts @ np.array([[0.1, -0.05, 0.02], [0.03, 0.1, -0.08], [0., 0., 0.]]) + np.array([0.2, 0.3, 0.6])).astype(np.float32)
    tn = fr.texel_neighbours(nbr, R)
    border = ~(tn >= 0).all(1)
    tf, = _dev(cuda, faces)
    source = torch.from_numpy(np.where(border, 0, 2).astype(np.uint8).reshape(F, R * R)).to(cuda)
    got = bake.blend_fill(torch.from_numpy(field.reshape(F, R * R, 3)).to(cuda), source, tf, iters=7).cpu().numpy()
    err = np.abs(got.reshape(-1, 3) - field).max()
    print('affine field, %d border texels fixed, 7 iterations: max change %.2e' % (border.sum(), err))
    assert 0 < border.sum() < border.size and err <= 1e-6
    assert np.array_equal(got.reshape(-1, 3)[border], field[border])


def _colour(points):
    """A colour that is a function of (|x|, y, z): float32 [..., 3]."""
    x, y, z = np.abs(points[..., 0]), points[..., 1], points[..., 2]
    return np.stack([0.2 + 0.5 * x, 0.5 + 0.4 * y, 0.5 + 0.3 * z * x], -1).astype(np.float32)


def _mirror(cuda, rest, faces, tex, weight, axis=0, tol=fr.JITTER_TOL):
    out, source, info = _bake().mirror_fill(*_dev(cuda, rest, faces, tex, weight), axis=axis, tol=tol)
    torch.cuda.synchronize()
    return (out.cpu().numpy(), source.cpu().numpy(), info['texels'].cpu().numpy(), info['src'].cpu().numpy(),
            info['d2'].cpu().numpy(), info['max_d2'])


def _membership(src, m64, bound, R, weight):
    """Every device answer must be one the float64 restatement allows within `bound`: filled from a candidate (a face whose d2 is
    within the bound of the smallest, a texel of it whose region comes within 1e-4 cell widths of the closest point) that a frame
    saw; or the restatement's own refusal; or refused as unseen because a candidate is unseen.  -> figures for the print."""
    RR = R * R
    st = dict(worst_face=0., worst_texel=0., other_face=0, other_texel=0)
    for i in range(len(src)):
        if m64['g'][i] < 0:
            assert src[i] == -1 - fr.NO_FACE, (i, src[i])
            continue
        near = np.nonzero(m64['all_d2'][i] <= m64['d2'][i] + bound)[0]
        cands = {(int(g), j): fr.region_violation(m64['all_w'][i, g, 0], m64['all_w'][i, g, 1], j, R) for g in near for j in range(RR)}
        cands = {k: v for k, v in cands.items() if v <= 1e-4}
        assert (int(m64['all_d2'][i].argmin()), fr.source_texel(*m64['all_w'][i, m64['g'][i]], R)) in cands
        if src[i] >= 0:
            g, j = int(src[i]) // RR, int(src[i]) % RR
            assert (g, j) in cands and weight[g, j] > 0, (i, g, j, sorted(cands))
            st['worst_face'] = max(st['worst_face'], m64['all_d2'][i, g] - m64['d2'][i])
            st['worst_texel'] = max(st['worst_texel'], cands[(g, j)])
            st['other_face'] += int(g != m64['g'][i])
            st['other_texel'] += int(g == m64['g'][i] and src[i] != m64['src'][i])
        elif src[i] != m64['src'][i]:
            assert src[i] == -1 - fr.UNSEEN and any(not weight[g, j] > 0 for g, j in cands), (i, src[i], m64['src'][i])
    return st


@pytest.mark.parametrize('R', [3, 8])
def test_mirror_on_the_symmetric_sphere_equals_the_restatement(cuda, R):
    rest, faces = fr.sphere_case()
    F, RR = faces.shape[0], R * R
    weight, points = fr.unseen_by_x(rest, faces, R)
    truth = _colour(points)
    tex = np.where(weight[..., None] > 0, truth, np.float32(0.5)).astype(np.float32)
    out, source, texels, src, d2, max_d2 = _mirror(cuda, rest, faces, tex, weight)
    assert (texels == np.nonzero(weight.reshape(-1) == 0)[0]).all() and texels.dtype == np.int32
    m32 = fr.mirror(rest, faces, texels, weight, R, 0, max_d2, np.float32)
    m64 = fr.mirror(rest, faces, texels, weight, R, 0, max_d2, np.float64)
    filled = src >= 0
    err = np.abs(out.reshape(-1, 3)[texels[filled]] - truth.reshape(-1, 3)[texels[filled]]).max()
    print('R %d: %d texels listed, %d filled, largest d2 %.2e, max colour error %.2e' % (R, len(texels), filled.sum(), d2.max(), err))
    assert (src == m32['src']).all() and (src == m64['src']).all()
    assert filled.all() and len(texels) > 0.3 * F * RR                            # every mirror image lies in x > 0.05: seen
    assert d2.max() < 1e-11
    flat_in, flat_out = tex.reshape(-1, 3), out.reshape(-1, 3)
    assert np.array_equal(flat_out[texels].view(np.uint32), flat_in[src].view(np.uint32))       # a bitwise copy of the source
    seen = weight.reshape(-1) > 0
    assert np.array_equal(flat_out[seen].view(np.uint32), flat_in[seen].view(np.uint32))        # and nothing else is written
    assert err <= 1e-6
    want_source = np.zeros(F * RR, np.uint8)
    want_source[texels] = 1
    assert source.dtype == np.uint8 and (source.reshape(-1) == want_source).all()


def test_mirror_refusals(cuda):
    from lasr_amd import _lib
    bake = _bake()
    rest, faces = fr.sphere_case()
    V, F, R = rest.shape[0], faces.shape[0], 3
    RR = R * R
    weight, points = fr.unseen_by_x(rest, faces, R)
    tex = _colour(points)
    # list entries out of range are skipped, the others are served
    listed = np.array([-1, F * RR, 5, -2 ** 31, 2 ** 31 - 1, F * RR - 1], np.int32)
    w1 = np.ones_like(weight)
    trest, tfaces, ttex, tw, tlist = _dev(cuda, rest, faces.astype(np.int32), tex, w1, listed)
    out, src, d2 = ttex.clone(), torch.zeros(6, dtype=torch.int32, device=cuda), torch.zeros(6, device=cuda)
    _lib.call('lasr_bake_mirror', trest, tfaces, tlist, ttex, tw, out, src, d2, V, F, R, 6, 0, 1e-3)
    torch.cuda.synchronize()
    src, d2 = src.cpu().numpy(), d2.cpu().numpy()
    want = fr.mirror(rest, faces, listed, w1, R, 0, 1e-3, np.float32)
    print('out-of-range entries: src %s, d2 %s' % (src, d2))
    assert (src == want['src']).all() and (src[[0, 1, 3, 4]] == -1 - fr.NO_FACE).all() and (src[[2, 5]] >= 0).all()
    assert np.isinf(d2[[0, 1, 3, 4]]).all() and (d2[[2, 5]] < 1e-11).all()
    # a face with a bad index anchors nothing: its own texels stay, and no texel takes it as a source
    badf = faces.copy()
    victim = int(np.nonzero(weight.min(1) > 0)[0][0])                              # a seen face, so that it is somebody's mirror
    badf[victim, 1] = V
    lost = int(np.nonzero(weight.min(1) == 0)[0][0])                               # and an unseen face
    badf[lost, 2] = -1
    o, source, texels, src, d2, max_d2 = _mirror(cuda, rest, badf, tex, weight)
    m64 = fr.mirror(rest, badf, texels, weight, R, 0, max_d2, np.float64)
    m32 = fr.mirror(rest, badf, texels, weight, R, 0, max_d2, np.float32)
    both = np.isfinite(m64['d2'])
    bound = 4. * float(np.abs(m32['d2'].astype(np.float64)[both] - m64['d2'][both]).max()) + float(np.spacing(np.float32(m64['d2'][both].max())))
    own = texels // RR == lost
    st = _membership(src, m64, bound, R, weight)                                   # mirror images on the bad face go to the face
    print('bad faces: %d texels of the unseen bad face, %d filled, bound %.3e, another face than float64 for %d, another texel '
          'for %d' % (own.sum(), (src >= 0).sum(), bound, st['other_face'], st['other_texel']))   # across its nearest edge
    assert own.sum() > 0 and (src[own] == -1 - fr.NO_FACE).all() and np.isinf(d2[own]).all()
    assert not (src[src >= 0] // RR == victim).any() and not (src[src >= 0] // RR == lost).any()
    assert np.abs(d2.astype(np.float64)[both] - m64['d2'][both]).max() <= bound
    # all texels unseen: nothing is a source; the blend then smooths the resolve's fallback, as the restatement does
    w0 = np.zeros_like(weight)
    o, source, texels, src, d2, max_d2 = _mirror(cuda, rest, faces, tex, w0)
    assert len(texels) == F * RR and (src == -1 - fr.UNSEEN).all() and (source == 2).all()
    assert np.array_equal(o.view(np.uint32), tex.view(np.uint32))
    tr, tf, tt, tw0 = _dev(cuda, rest, faces, tex, w0)
    got, source, info = bake.complete_texture(tf, tt, tw0, fill='mirror', rest_verts=tr, iters=3)
    want = fr.blend(tex, np.zeros((F, RR), np.uint8), fr.face_neighbours(faces, V), R, 3)
    assert (source == 2).all() and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    got, source, info = bake.complete_texture(tf, tt, tw0, fill='blend', iters=3)
    assert info is None and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # nothing unseen: M = 0, nothing launched, nothing changed
    o, source, texels, src, d2, max_d2 = _mirror(cuda, rest, faces, tex, w1)
    assert len(texels) == 0 and len(src) == 0 and (source == 0).all() and np.array_equal(o.view(np.uint32), tex.view(np.uint32))
    # argument checks of the python layer
    with pytest.raises(ValueError, match='axis'):
        bake.mirror_fill(tr, tf, tt, tw0, axis=3)
    with pytest.raises(ValueError, match='tol'):
        bake.mirror_fill(tr, tf, tt, tw0, tol=-1.)
    with pytest.raises(ValueError, match='weight must be'):
        bake.mirror_fill(tr, tf, tt, tw0[:, :-1])
    with pytest.raises(ValueError, match='not R\\*R'):
        bake.mirror_fill(tr, tf, tt[:, :-1], tw0[:, :-1])
    with pytest.raises(ValueError, match='iters'):
        bake.blend_fill(tt, torch.zeros(F, RR, dtype=torch.uint8, device=cuda), tf, iters=-1)


@pytest.mark.parametrize('R', [3, 8])
@pytest.mark.parametrize('name', sorted(fr.MIRROR_FIXTURES))
def test_mirror_membership_on_the_asymmetric_fixtures(cuda, name, R):
    m = fr.mirror_margins(name, R)
    rest, faces, weight, bound, m64 = m['rest'], m['faces'], m['weight'], m['bound'], m['m64']
    RR = R * R
    tex = _colour(m['points'])
    out, source, texels, src, d2, max_d2 = _mirror(cuda, rest, faces, tex, weight)
    assert (texels == m['texels']).all()
    assert abs(max_d2 - m['max_d2']) <= 1e-6 * max_d2                             # the diagonal in float32 on either side
    derr = np.abs(d2.astype(np.float64) - m64['d2']).max()
    assert derr <= bound, (derr, bound)
    filled = src >= 0
    # distance and normal verdicts do not hang on rounding in these fixtures (test_bake_fill_cpu.py asserts the margins)
    assert not np.isin(src, (-1 - fr.FAR, -1 - fr.NORMAL, -1 - fr.NO_FACE)).any()
    st = _membership(src, m64, bound, R, weight)
    print('%s R %d: %d listed, %d filled; |d2 - d2_f64| at most %.3e (bound %.3e); chosen face at most %.3e farther than the '
          'nearest, another face than float64 for %d, another texel of the same face for %d; worst texel distance %.2e cells'
          % (name, R, len(texels), filled.sum(), derr, bound, st['worst_face'], st['other_face'], st['other_texel'], st['worst_texel']))
    assert filled.mean() > 0.5
    assert np.array_equal(out.reshape(-1, 3)[texels[filled]].view(np.uint32), tex.reshape(-1, 3)[src[filled]].view(np.uint32))
    # max_d2 = 0 refuses every texel whose distance is not a matter of rounding
    out0, source0, texels0, src0, d20, max0 = _mirror(cuda, rest, faces, tex, weight, tol=0.)
    far = m64['d2'] > bound
    assert max0 == 0. and (src0[far] == -1 - fr.FAR).all() and far.mean() > 0.95
    assert np.array_equal(d20.view(np.uint32), d2.view(np.uint32))


def test_determinism(cuda):
    bake = _bake()
    m = fr.mirror_margins('swollen', 8)
    tex = _colour(m['points'])
    weight = m['weight'].copy()
    weight[m['points'][..., 0] > 0.6] = 0                                          # a cap of the seen side too: nobody's source
    tr, tf, tt, tw = _dev(cuda, m['rest'], m['faces'], tex, weight)
    runs = []
    for _ in range(2):
        out, source, info = bake.complete_texture(tf, tt, tw, fill='mirror', rest_verts=tr, iters=9)
        runs.append([t.cpu().numpy() for t in (out, source, info['src'], info['d2'])])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert (runs[0][1] == 1).any() and (runs[0][1] == 2).any() and (runs[0][1] == 0).any()


def test_script_end_to_end(cuda, tmp_path):
    from PIL import Image
    from lasr_amd.nnutils.mesh_net import quaternion_to_rotation_matrix
    from lasr_amd.soft_renderer.functional import load_obj, save_obj
    root, n, size, focal, R = str(tmp_path), 3, 128, 10., 4
    sv, sf = fr.sphere_case()
    rest = (sv * np.float32(0.6)).astype(np.float32)                               # symmetric about x = 0, well inside the frame
    save_obj(os.path.join(root, 'ball.obj'), torch.from_numpy(rest), torch.from_numpy(sf))
    rc = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'render_syn.py'), '--outdir', 'ball3', '--nframes', str(n),
                         '--img_size', str(size), '--root', root, '--surface_tex', '--obj', os.path.join(root, 'ball.obj'),
                         '--alpha', '0.15'], cwd=root, timeout=600, capture_output=True, text=True)   # a twentieth of a turn per frame
    assert rc.returncode == 0, rc.stderr[-2000:]
    base = os.path.join(root, 'database', 'DAVIS')
    test = os.path.join(root, 'bake-out')
    os.makedirs(test)
    for i in range(n):                                                             # the ground truth stands in for extract.py's output
        v, f = load_obj(os.path.join(base, 'Meshes', 'Full-Resolution', 'ball3', '%05d.obj' % i))
        save_obj(os.path.join(test, 'pred%d.obj' % i), v.cpu(), f.cpu())
        cam = np.loadtxt(os.path.join(base, 'Camera', 'Full-Resolution', 'ball3', '%05d.txt' % i))
        rtk = np.zeros((4, 4))
        rtk[:3, :3] = quaternion_to_rotation_matrix(torch.tensor(np.r_[cam[4:7], cam[3]]).float()).numpy()
        rtk[:3, 3] = (0, 0, cam[7])
        rtk[3] = (focal * size / 2, focal * size / 2, size / 2, size / 2)
        np.savetxt(os.path.join(test, 'cam%d.txt' % i), rtk)
    faces = f.cpu().numpy()
    assert (faces == sf).all()
    F = faces.shape[0]

    def run(out, *extra):
        return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'bake_texture.py'), '--testdir', test, '--seqname', 'ball3',
                               '--texture_res', str(R), '--outpath', out] + list(extra), cwd=root, timeout=600, capture_output=True,
                              text=True)
    plain, none, mirr = (os.path.join(root, d, 'baked') for d in ('plain', 'none', 'mirror'))
    np.savez(os.path.join(test, 'rig.npz'), rest_verts=rest, faces=faces.astype(np.int32))
    stdout = {}
    for out, extra in ((plain, ()), (none, ('--fill', 'none')), (mirr, ('--fill', 'mirror', '--fill_iters', '5'))):
        rc = run(out, *extra)
        assert rc.returncode == 0, rc.stderr[-2000:]
        stdout[out] = rc.stdout
        print(rc.stdout.strip())
    for ext in ('.obj', '.mtl', '.png', '_weight.npy'):                            # --fill none: the bytes of a run without the flag
        assert open(plain + ext, 'rb').read() == open(none + ext, 'rb').read(), ext
    assert not os.path.exists(none + '_source.npy') and stdout[none] == stdout[plain] and 'filled' not in stdout[none]
    weight = np.load(mirr + '_weight.npy')
    assert np.array_equal(weight, np.load(plain + '_weight.npy'))
    source = np.load(mirr + '_source.npy')
    assert source.shape == (F, R * R) and source.dtype == np.uint8
    assert ((source == 0) == (weight > 0)).all()
    seen = (weight > 0).mean()
    assert 0.1 < seen < 0.9                                                        # one side only
    texels = np.nonzero(weight.reshape(-1) == 0)[0]
    want = fr.mirror(rest, faces, texels, weight, R, 0, fr.max_d2_of(rest, 0.05), np.float32)
    want64 = fr.mirror(rest, faces, texels, weight, R, 0, fr.max_d2_of(rest, 0.05), np.float64)
    assert (want['src'] == want64['src']).all()
    code1 = np.zeros(F * R * R, bool)
    code1[texels[want['src'] >= 0]] = True
    assert ((source.reshape(-1) == 1) == code1).all() and code1.sum() > 0 and (source == 2).sum() > 0   # the rim is unseen on both sides
    line = [l for l in stdout[mirr].splitlines() if l.startswith('filled: ')]
    assert line == ['filled: mirrored %.1f %%, blended %.1f %%' % (100. * (source == 1).mean(), 100. * (source == 2).mean())]
    a, b = np.asarray(Image.open(plain + '.png')), np.asarray(Image.open(mirr + '.png'))
    tile_w = int((F - 1.) ** 0.5) + 1
    assert a.shape == b.shape == ((int((F - 1.) / tile_w) + 1) * R, tile_w * R, 3)
    touched = np.zeros(a.shape[:2], bool)
    for fn in np.nonzero((source != 0).any(1))[0]:                                 # face fn owns tile (fn % tile_w, fn // tile_w),
        col, row = fn % tile_w, fn // tile_w                                       # counted from the bottom row of the picture
        touched[a.shape[0] - (row + 1) * R:a.shape[0] - row * R, col * R:(col + 1) * R] = True
    differ = (a != b).any(2)
    print('atlas: %d of %d pixels differ, all inside the %d tiles with a filled texel' % (differ.sum(), differ.size,
                                                                                      (source != 0).any(1).sum()))
    assert differ.sum() > 0 and not (differ & ~touched).any()
