"""Atlas completion without a device: the texel adjacency and the mirror map of the restatement (tests/bake_fill_restated.py) on
the fixtures tests/test_bake_fill_gpu.py uses, header against binding, the C ABI's host-side checks, the script's arguments, and
the margins of the jittered fixture.  The fill is this project's own addition: the restatement is the only parity there is."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import bake_fill_restated as fr
import bake_restated as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _texel_points(verts, faces, R):
    F = faces.shape[0]
    return fr.sample_points(verts, faces, np.arange(F * R * R), R, np.float64)


@pytest.mark.parametrize('R', [1, 2, 3, 5, 8])
def test_grid_adjacency_is_symmetric_and_keeps_an_affine_field(R):
    verts, faces = fr.grid_case()
    assert faces.shape == (32, 3)
    nbr = fr.face_neighbours(faces, verts.shape[0])
    assert (nbr < 0).sum() == 16                                                  # the border of the 4 x 4 grid
    same = nbr[nbr >= 0] & 1
    assert (same == 0).any() and (same == 1).any()
    for f, k in zip(*np.nonzero(nbr >= 0)):                                       # the face adjacency points back
        g, k2 = nbr[f, k] // 6, (nbr[f, k] // 2) % 3
        assert nbr[g, k2] == (f * 3 + k) * 2 + (nbr[f, k] & 1)
    tn = fr.texel_neighbours(nbr, R)
    for i, row in enumerate(tn):
        for j in row[row >= 0]:
            assert i in tn[j], (i, j)
        assert len(set(row[row >= 0])) == (row >= 0).sum() and i not in row
    pts = _texel_points(verts, faces, R)
    field = pts @ np.array([[0.3, -0.2, 0.1], [0.05, 0.4, -0.3], [0., 0., 0.]]) + np.array([0.2, 0.5, 0.7])
    out = fr.blend(field.reshape(32, R * R, 3), np.zeros((32, R * R), np.uint8), nbr, R, 1, np.float64).reshape(-1, 3)
    three = (tn >= 0).all(1)
    err = np.abs(out - field)[three].max()
    print('R %d: %d texels with three neighbours, affine fixed-point error %.2e' % (R, three.sum(), err))
    assert three.sum() >= 16 and err <= 1e-12


def test_closed_sphere_has_no_open_edge_and_no_same_direction_pair():
    verts, faces = fr.sphere_case()
    nbr = fr.face_neighbours(faces, verts.shape[0])
    assert nbr.shape == (80, 3) and (nbr >= 0).all() and ((nbr & 1) == 0).all()
    tn = fr.texel_neighbours(nbr, 3)
    assert (tn >= 0).all()
    for i, row in enumerate(tn):
        assert all(i in tn[j] for j in row)


def test_non_manifold_edge_and_bad_faces_have_no_neighbour():
    faces = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [2, 1, 5], [5, 1, 5], [0, 2, 9]])
    nbr = fr.face_neighbours(faces, 9)
    assert (nbr[:3, 2] == -1).all()                                               # edge 0-1 has three faces
    assert nbr[0, 0] == (3 * 3 + 2) * 2 + 0 and nbr[3, 2] == (0 * 3 + 0) * 2 + 0  # edge 1-2: opposite directions
    assert (nbr[4] == -1).all() and (nbr[5] == -1).all()                          # a repeated index; an index out of range
    assert nbr[0, 1] == -1 and nbr[3, 1] == -1 and nbr[3, 0] == -1                # their edges anchor nothing


@pytest.mark.parametrize('R', [3, 4, 8])
def test_mirror_on_the_sphere_is_one_to_one_in_both_precisions(R):
    verts, faces = fr.sphere_case()
    F, RR = faces.shape[0], R * R
    texels = np.arange(F * RR)
    weight = np.ones((F, RR), np.float32)
    for axis in (0, 1, 2):
        m64 = fr.mirror(verts, faces, texels, weight, R, axis, 1e-6, np.float64)
        m32 = fr.mirror(verts, faces, texels, weight, R, axis, 1e-6, np.float32)
        gap = np.sort(m64['all_d2'], 1)
        print('R %d axis %d: d2 at most %.1e (float32 %.1e), second-nearest face at least %.1e farther'
              % (R, axis, m64['d2'].max(), m32['d2'].max(), (gap[:, 1] - gap[:, 0]).min()))
        assert (m64['src'] >= 0).all() and sorted(m64['src']) == list(range(F * RR))
        assert m64['d2'].max() < 1e-30 and m32['d2'].max() < 1e-11
        assert (m32['src'] == m64['src']).all()
        assert (m64['dots'] > 1e-3).all()
        # the closest point sits a third of a cell from every texel boundary: float32 cannot choose another texel
        g = m64['g']
        b = m64['all_w'][texels, g]
        viol = [fr.region_violation(b[i, 0], b[i, 1], m64['src'][i] % RR, R) for i in range(0, F * RR, 7)]
        assert max(viol) == 0.


def test_source_texel_on_edges_and_corners_touches_the_closest_point():
    # a closest point on an edge or at a corner of the source face: surface_texel alone names a texel elsewhere on the face
    # (b0 = 1 -> ix = R; b0 + b1 rounded above 1 on the last diagonal -> the transposed cell); the pull towards the centroid mends it
    for R in (1, 2, 3, 5, 8, 32):
        for dt in (np.float32, np.float64):
            ts = np.linspace(0, 1, 257).astype(dt)
            for t in ts:
                for b0, b1 in ((dt(1) - t, t), (t, dt(0)), (dt(0), t), (dt(1) - t, dt(0)), (dt(0), dt(1) - t)):
                    j = fr.source_texel(dt(b0), dt(b1), R)
                    assert 0 <= j < R * R
                    assert fr.region_violation(float(b0), float(b1), j, R) <= 1e-4, (R, dt, b0, b1, j)
    assert br.surface_texel(np.float32(1), np.float32(0), 3) == 3                # the texel of (ix, iy) = (0, 1): away from corner 0


def _prototype(name):
    hdr = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'\bint %s\s*\((.*?)\);' % name, hdr, re.S)
    assert m, name
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def test_header_and_binding_agree_on_both_entry_points():
    from lasr_amd import _lib
    ctype = lambda a: (ctypes.c_void_p if '*' in a else {'int': ctypes.c_int, 'float': ctypes.c_float}[a.split()[0]])   # noqa: E731
    for name, params in (('lasr_bake_mirror', 'rest_verts faces texels textures weight out_textures src d2 V F R M axis max_d2 '
                                              'hip_stream'),
                         ('lasr_bake_blend', 'in out fixed nbr F R hip_stream')):
        args = _prototype(name)
        assert [a.replace('*', ' ').split()[-1] for a in args] == params.split()
        res, sig = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and sig == [ctype(a) for a in args]
    hdr = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    assert '#define LASR_BAKE_FILL_TILE 256\n' in hdr
    for k, reason in enumerate(('FAR', 'NORMAL', 'UNSEEN', 'NO_FACE')):
        assert '#define LASR_BAKE_MIRROR_%s %d\n' % (reason, k) in hdr
    assert (fr.FAR, fr.NORMAL, fr.UNSEEN, fr.NO_FACE) == (0, 1, 2, 3)
    assert _lib.ABI_VERSION == 13                                                 # new symbols only


def test_symbols_are_exported_and_the_host_checks_run_without_a_device():
    from lasr_amd import _lib
    h = _lib.lib()
    n, x, y = None, 64, 128                                                       # x, y: two non-NULL addresses, never followed
    mir = lambda V=3, F=1, R=4, M=5, axis=0, max_d2=1., p=n, out=n: h.lasr_bake_mirror(p, p, p, p, p, out, p, p, V, F, R, M, axis,   # noqa: E731
                                                                                       max_d2, n)
    assert mir(M=0) == 0 and mir(F=0) == 0                                        # nothing to do
    assert mir() == -1                                                            # null buffers
    assert mir(p=x, out=x) == -1                                                  # out_textures == textures
    assert mir(M=-1) == -1 and mir(M=0, F=-1) == -1 and mir(M=0, V=0) == -1
    assert mir(M=0, R=0) == -1 and mir(M=0, R=33) == -1 and mir(M=0, R=32) == 0
    assert mir(M=0, axis=-1) == -1 and mir(M=0, axis=3) == -1 and mir(M=0, axis=2) == 0
    assert mir(M=0, max_d2=-1e-9) == -1 and mir(M=0, max_d2=float('inf')) == -1 and mir(M=0, max_d2=float('nan')) == -1
    assert mir(M=0, max_d2=0.) == 0
    assert mir(M=0, F=(1 << 31) // (4 * 16), R=4) == -1 and mir(M=0, F=(1 << 31) // (4 * 16) - 1, R=4) == 0
    ble = lambda F=1, R=4, a=n, b=n, c=n, d=n: h.lasr_bake_blend(a, b, c, d, F, R, n)   # noqa: E731
    assert ble(F=0) == 0 and ble() == -1
    assert ble(a=x, b=x, c=x, d=x) == -1                                          # in == out
    assert ble(a=x, b=y, c=x, d=n) == -1 and ble(a=x, b=y, c=n, d=x) == -1 and ble(a=n, b=y, c=x, d=x) == -1
    assert ble(F=-1) == -1 and ble(F=0, R=0) == -1 and ble(F=0, R=33) == -1
    assert ble(F=(1 << 31) // (4 * 16), R=4) == -1
    assert ble(F=(1 << 31) // 6, R=1) == -1                                       # 6 F + 5 past int32: the range of an nbr code
    names = [h.lasr_prof_kernel_name(i) for i in range(h.lasr_prof_kernel_count())]
    assert not any(b'mirror' in s or b'blend' in s for s in names)                # the kernel table is not extended


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from lasr_amd.nnutils import bake
    v, f = torch.zeros(3, 3), torch.tensor([[0, 1, 2]])
    tex, w = torch.zeros(1, 4, 3), torch.zeros(1, 4)
    with pytest.raises(TypeError):
        bake.mirror_fill(v, f, tex, w)
    with pytest.raises(TypeError):
        bake.blend_fill(tex, w.to(torch.uint8), f)
    with pytest.raises(TypeError):
        bake.face_neighbours(f)
    with pytest.raises(TypeError):
        bake.complete_texture(f, tex, w, fill='blend')
    with pytest.raises(TypeError):
        bake.mirror_fill(v.numpy(), f, tex, w)
    with pytest.raises(ValueError, match='fill must be'):
        bake.complete_texture(f, tex, w, fill='none')
    with pytest.raises(ValueError, match='rest_verts'):
        bake.complete_texture(f, tex, w, fill='mirror')
    assert (bake.SEEN, bake.MIRRORED, bake.BLENDED) == (0, 1, 2) and len(bake.MIRROR_REASONS) == 4


def test_script_arguments_and_rig_refusals(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import bake_texture
    a = bake_texture.parse_args(['--testdir', 'log/camel-5/', '--seqname', 'camel'])
    assert (a.texture_res, a.power, a.pose_frame, a.mask, a.outpath, a.preview) == (8, 2, 0, True, '', '')      # as they were
    assert (a.fill, a.rig, a.symidx, a.sym_tol, a.fill_iters) == ('none', '', 0, 0.05, 64)
    a = bake_texture.parse_args('--fill mirror --rig r/rig.npz --symidx 2 --sym_tol 0.1 --fill_iters 8'.split())
    assert (a.fill, a.rig, a.symidx, a.sym_tol, a.fill_iters) == ('mirror', 'r/rig.npz', 2, 0.1, 8)
    assert bake_texture.parse_args(['--fill', 'blend']).fill == 'blend'
    with pytest.raises(SystemExit):
        bake_texture.parse_args(['--fill', 'inpaint'])
    face = np.array([[0, 1, 2], [0, 2, 3]])
    rest = np.arange(12, dtype=np.float32).reshape(4, 3)
    missing = str(tmp_path / 'none' / 'rig.npz')
    with pytest.raises(ValueError, match=r'does not exist \(write it with extract.py --rig\)'):
        bake_texture.load_rest_shape(missing, face)
    path = str(tmp_path / 'rig.npz')
    np.savez(path, rest_verts=rest, faces=face.astype(np.int32))
    got = bake_texture.load_rest_shape(path, face)
    assert got.dtype == np.float32 and (got == rest).all()
    np.savez(path, rest_verts=rest, faces=face[:, ::-1].astype(np.int32))
    with pytest.raises(ValueError, match=r'differ from the topology of the pred<i> meshes.*extract.py --rig'):
        bake_texture.load_rest_shape(path, face)
    np.savez(path, rest_verts=rest, faces=face[:1].astype(np.int32))
    with pytest.raises(ValueError, match='differ from the topology'):
        bake_texture.load_rest_shape(path, face)
    np.savez(path, rest_verts=rest[:3], faces=face.astype(np.int32))
    with pytest.raises(ValueError, match='hold every vertex'):
        bake_texture.load_rest_shape(path, face)
    np.savez(path, verts=rest)
    with pytest.raises(ValueError, match='not what extract.py --rig writes'):
        bake_texture.load_rest_shape(path, face)
    for flag in ('--fill', '--rig', '--symidx', '--sym_tol', '--fill_iters'):
        assert flag in bake_texture.__doc__
    with pytest.raises(SystemExit):
        bake_texture.parse_args(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert text.count('a default nobody has measured on a real reconstruction') == 2      # --sym_tol and --fill_iters say so


@pytest.mark.parametrize('R', [3, 8])
@pytest.mark.parametrize('name', sorted(fr.MIRROR_FIXTURES))
def test_margins_of_the_asymmetric_fixtures(name, R):
    m = fr.mirror_margins(name, R)
    m64, m32, bound, max_d2, texels = m['m64'], m['m32'], m['bound'], m['max_d2'], m['texels']
    gap = np.sort(m64['all_d2'], 1)
    ties = int(((gap[:, 1] - gap[:, 0]) <= bound).sum())
    b = m64['all_w'][np.arange(len(texels)), m64['g']]
    border = int(((b.min(1) <= 0) | (b.sum(1) >= 1)).sum())
    print('%s R %d: %d texels listed, d2 in %.3e .. %.3e, max_d2 %.3e, bound %.3e, |dot| at least %.3e; %d closest points on an '
          'edge or a corner, %d texels with a second face within the bound, float32 and float64 name another source for %d'
          % (name, R, len(texels), m64['d2'].min(), m64['d2'].max(), max_d2, bound, np.abs(m64['dots']).min(), border, ties,
             int((m32['src'] != m64['src']).sum())))
    assert len(texels) > 0.3 * m['weight'].size
    assert (np.abs(m64['d2'] - max_d2) > bound).all()                             # no texel's d2 within the bound of max_d2
    assert (m64['d2'] > bound).mean() > 0.95                                      # max_d2 = 0 must refuse all of these
    assert (np.abs(m64['dots']) > 1e-3).all()                                     # no normal dot near zero
    assert (m64['src'] >= 0).mean() > 0.5                                         # and most texels find a seen source
    if name == 'swollen' and R == 8:
        assert border > 0.02 * len(texels) and ties > 0.02 * len(texels)          # edges, corners and their ties are exercised
