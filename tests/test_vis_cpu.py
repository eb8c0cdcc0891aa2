"""render_vis.py without a GPU: the .ply files extract.py writes for it, the bones' Gaussian spheres, the label colormap, the
command line, and the host-side argument checks of lasr_vis_shade."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ['--testdir', '--seqname', '--watertight', '--outpath', '--cam_type', '--append_img', '--append_render', '--nosmooth',
         '--gray', '--overlay', '--vis_bones', '--freeze']          # the reference's render_vis.py:38-62


def test_ply_round_trip(tmp_path):
    from lasr_amd.ext_utils.ply import read_ply, write_ply
    rng = np.random.default_rng(0)
    v = rng.standard_normal((50, 3)) * 3
    f = rng.integers(0, 50, (80, 3))
    c = rng.integers(0, 256, (50, 3))
    p = str(tmp_path / 'm.ply')
    write_ply(p, v, f, colors=c)
    m = read_ply(p)
    np.testing.assert_allclose(m['verts'], v, atol=5e-7)                       # '%f': six decimals
    assert (m['colors'] == c).all() and m['colors'].dtype == np.uint8
    assert (m['faces'] == f).all()
    assert (m['normals'] == 0).all()


def test_reader_parses_fusion_meshwrite_layout(tmp_path):
    from lasr_amd.ext_utils.ply import read_ply
    text = ('ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n'
            'property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n'
            'property uchar blue\nelement face 2\nproperty list uchar int vertex_index\nend_header\n'
            '0.000000 0.000000 0.000000 0.000000 0.000000 0.000000 255 0 0\n'
            '1.000000 0.000000 0.000000 0.000000 0.000000 0.000000 0 255 0\n'
            '1.000000 1.000000 0.500000 0.000000 0.000000 0.000000 0 0 255\n'
            '0.000000 1.000000 -0.250000 0.000000 0.000000 0.000000 12 34 56\n'
            '3 0 1 2\n3 0 2 3\n')
    p = tmp_path / 'f.ply'
    p.write_text(text)
    m = read_ply(str(p))
    assert m['verts'].shape == (4, 3) and m['verts'][2, 2] == 0.5 and m['verts'][3, 2] == -0.25
    assert m['colors'].tolist() == [[255, 0, 0], [0, 255, 0], [0, 0, 255], [12, 34, 56]]
    assert m['faces'].tolist() == [[0, 1, 2], [0, 2, 3]]


def test_label_colormap_closed_form():
    from lasr_amd.vis import label_colormap
    cm = label_colormap(9)
    # index bits (b2 b1 b0) -> (r, g, b) = 128 * (b0, b1, b2); the next three bits land on bit 6
    assert cm.tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128], [128, 0, 128], [0, 128, 128],
                           [128, 128, 128], [64, 0, 0]]
    assert label_colormap(256)[255].tolist() == [224, 224, 192]


def test_gaussian_spheres_match_the_formula():
    from lasr_amd import vis
    from lasr_amd.nnutils.mesh_net import quaternion_to_rotation_matrix
    g = torch.Generator().manual_seed(0)
    J = 4
    ctl_ts, log_ctl = torch.randn(J, 3, generator=g), 3 * torch.randn(J, 3, generator=g)
    ctl_rs = torch.randn(J, 4, generator=g)
    Rmat = torch.linalg.qr(torch.randn(J + 1, 3, 3, generator=g, dtype=torch.float64))[0].float()
    Tmat = torch.randn(J + 1, 3, generator=g)
    verts, faces, colors = vis.gaussian_spheres(ctl_ts, ctl_rs, log_ctl, Rmat, Tmat)
    sv, sf = vis.uv_sphere(0.05)
    Vs = len(sv)
    assert verts.shape == (J * Vs, 3) and faces.shape == (J * len(sf), 3) and colors.shape == (J * Vs, 3)
    for k in range(J):
        q = ctl_rs[k].double() / ctl_rs[k].double().norm()
        R = quaternion_to_rotation_matrix(q).double()
        p = torch.from_numpy(sv) / torch.exp(0.5 * log_ctl[k].double().clamp(-2, 2))
        p = p @ R.T + ctl_ts[k].double()
        p = p @ Rmat[k + 1].double() + Tmat[k + 1].double()                    # the bone's own transform (identity skin)
        p = p @ Rmat[0].double() + Tmat[0].double()                            # then the body
        np.testing.assert_allclose(verts[k * Vs:(k + 1) * Vs].double().numpy(), p.numpy(), atol=2e-5)
        assert (colors[k * Vs:(k + 1) * Vs] == vis.label_colormap(J)[k]).all()
    assert (faces[len(sf):2 * len(sf)] == sf + Vs).all()
    assert vis.signed_volume(sv, sf) > 0


def test_fix_inversion_and_floor():
    from lasr_amd import vis
    sv, sf = vis.uv_sphere(1.0)
    inv = torch.from_numpy(sf[:, [0, 2, 1]])
    assert vis.signed_volume(sv, inv) < 0 and vis.signed_volume(sv, vis.fix_inversion(torch.from_numpy(sv), inv)) > 0
    assert (vis.fix_inversion(torch.from_numpy(sv), torch.from_numpy(sf)) == torch.from_numpy(sf)).all()
    fv, ff, fc = vis.floor_quad(torch.tensor([[-1., -2., 4.], [2., 1., 6.]]))
    assert fv[:, 1].tolist() == [1.] * 4 and sorted(set(fv[:, 0].tolist())) == [-10., 20.]
    assert sorted(set(fv[:, 2].tolist())) == [2., 60.] and ff.shape == (2, 3) and (fc == 1).all()


def _script(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'render_vis.py')] + list(args), capture_output=True, text=True,
                          timeout=300, cwd=ROOT)


def test_command_line():
    out = _script('--help')
    assert out.returncode == 0
    for f in FLAGS:
        assert f in out.stdout, f
    r = _script('--cam_type', 'orthographic')
    assert r.returncode != 0 and 'perspective' in r.stderr
    r = _script('--watertight', 'yes')
    assert r.returncode != 0 and 'Manifold' in r.stderr
    r = _script('--append_render', 'no')                       # nothing to write
    assert r.returncode != 0 and '--append_img yes' in r.stderr


def test_vis_shade_rejects_bad_arguments_on_the_host():
    from lasr_amd import _lib
    h = _lib.lib()
    d = 16                                                   # never dereferenced: every call below fails before a launch
    p = _lib.VisParams()
    import ctypes
    P = ctypes.byref(p)
    ok = dict(vert_rec=d, faces=d, face_rec=d, r0=d, r1=None, sh=d, xf=d, fr=None, out=d, N=2, V=10, F=8, F0=8, IS=64, S=128,
              H=48, W=64, params=P)

    def call(**kw):
        a = dict(ok, **kw)
        return h.lasr_vis_shade(a['vert_rec'], a['faces'], a['face_rec'], a['r0'], a['r1'], a['sh'], a['xf'], a['fr'], a['out'],
                                a['N'], a['V'], a['F'], a['F0'], a['IS'], a['S'], a['H'], a['W'], a['params'], None)
    assert call(N=0) == 0                                    # empty batch
    for k in ('vert_rec', 'faces', 'face_rec', 'r0', 'sh', 'xf', 'out'):
        assert call(**{k: None}) == -1, k
    assert call(params=None) == -1
    for k, bad in (('N', -1), ('V', 0), ('V', -3), ('F', 0), ('F0', 0), ('F0', 9), ('IS', 0), ('IS', -64), ('IS', 1 << 20),
                   ('S', 0), ('S', 1 << 20), ('H', 0), ('H', 65), ('W', -1), ('W', 65), ('V', 1 << 30), ('N', 1 << 20)):
        assert call(**{k: bad}) == -1, (k, bad)
    assert call(r1=d) == -1                                  # two layers need F0 < F
    assert call(F0=5) == -1                                  # one layer needs F0 == F
    p.overlay = 1
    assert call() == -1                                      # overlay without frames
