"""Known answers of the Phong pass's float64 restatement (tests/phong_restated.py), the host-side checks of
lasr_phong_shade, and the command-line surface of extract.py / scripts/eval_mesh.py --render.  No device needed."""
import math
import os
import sys

import numpy as np
import pytest

import phong_restated as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _quad(z, half=2.):
    """Camera-facing quad at depth z (normal (0, 0, -1), toward the camera at the origin): verts [4,3], faces [2,3]."""
    v = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], np.float64)
    f = np.array([[0, 2, 1], [0, 3, 2]])
    return v, f


def test_pixel_centres_follow_pytorch3d_ndc():
    x, y = pr.pixel_ndc(4)
    assert np.allclose(x[0], [0.75, 0.25, -0.25, -0.75]) and np.allclose(y[:, 0], [0.75, 0.25, -0.25, -0.75])


def test_camera_facing_quad_has_the_closed_form_diffuse_and_specular():
    z0, S = 2., 5
    v, f = _quad(z0)
    n = pr.vertex_normals(v, f)
    assert np.allclose(n, [0., 0., -1.])                                     # outward winding points at the camera
    fm = np.zeros((S, S), np.int64)
    tex = np.full((4, 3), 0.25)
    img = pr.shade(v, f, tex, fm)
    # the centre pixel sits at (0, 0, z0): l = (0, 1, -z0)/L, n.l = z0/L, r = (0, -1, -z0)/L, v = (0, 0, -1), v.r = z0/L
    c = z0 / math.sqrt(1 + z0 * z0)
    want = (1 + c) * 0.25 + c ** 64
    assert np.allclose(img[2, 2, :3], want, rtol=0, atol=1e-7), (img[2, 2], want)   # (pytorch3d's 1e-8 in the area)
    assert img[2, 2, 3] == 0.5                                               # on the interior diagonal: d2 = 0, the seam
    assert img[2, 1, 3] == 1.0                                               # 0.4 / sqrt(2) from the diagonal: sigmoid(800) = 1
    # off-centre pixel (x = 0.4, y = -0.4): general closed form
    p = np.array([0.4, -0.4, z0])
    l = (np.array([0., 1., 0.]) - p) / np.linalg.norm(np.array([0., 1., 0.]) - p)
    ndl = -l[2]
    r = 2 * ndl * np.array([0., 0., -1.]) - l
    s = max(float(np.dot(-p / np.linalg.norm(p), r)), 0.) ** 64
    assert np.allclose(img[3, 1, :3], (1 + ndl) * 0.25 + s, atol=1e-7)


def test_turned_away_normal_gets_ambient_only():
    col = pr.phong_colour(np.array([[0., -2., 2.]]), np.array([[0., -1., 0.]]), np.full((1, 3), 0.3))
    assert np.allclose(col, 0.3)                                             # n.l < 0: no diffuse, no specular


def test_blend_weight_at_z_inv_1e_4_is_e_to_the_minus_one():
    z = 100. - 1e-4 * 99.                                                    # z_inv = 1e-4 = m
    rgb, alpha = pr.blend(np.array([[0.2, 0.4, 0.6]]), np.array([1.]), np.array([z]), (1., 0., 0.5))
    d = math.exp((1e-10 - 1e-4) / 1e-4)
    assert abs(d - math.exp(-1)) < 1.01e-6 * math.exp(-1)                   # exp(-1 + 1e-6)
    want = (np.array([0.2, 0.4, 0.6]) + d * np.array([1., 0., 0.5])) / (1 + d)
    assert np.allclose(rgb[0], want, atol=1e-12) and alpha[0] == 1.0


def test_surface_beyond_zfar_shows_the_background():
    v, f = _quad(150.)
    img = pr.shade(v, f, np.full((4, 3), 0.7), np.zeros((6, 6), np.int64), background=(0.1, 0.2, 0.3))
    assert np.allclose(img[..., :3], [0.1, 0.2, 0.3], atol=1e-12) and np.all(img[..., 3] >= 0.5)   # 0.5 on the diagonal seam


def test_uncovered_pixels_are_background_with_zero_alpha_and_edges_half_alpha():
    v = np.array([[0., 0., 2.], [0., 1., 2.], [1., 0., 2.]])
    f = np.array([[0, 1, 2]])
    S = 8
    x, y = pr.pixel_ndc(S)
    fm = np.where((x >= 0) & (y >= 0) & (x + y <= 1), 0, -1)                  # the face's pixels (world x is NDC x)
    img = pr.shade(v, f, np.full((3, 3), 0.5), fm, background=(1., 1., 1.))
    assert np.all(img[fm < 0, 3] == 0) and np.all(img[fm < 0, :3] == 1)
    d2 = np.minimum(np.minimum(x, y) ** 2, ((1 - x - y) / math.sqrt(2)) ** 2)[fm == 0]
    assert np.allclose(img[fm == 0, 3], 1 / (1 + np.exp(-d2 / 1e-4)), rtol=0, atol=1e-12)
    assert np.isclose(img[fm == 0, 3].min(), 0.5)                            # pixel centres on the edges


def test_entry_point_checks_sizes_and_pointers_without_a_device():
    from lasr_amd import _lib
    h = _lib.lib()
    bg = (_lib.ctypes.c_float * 3)(1., 1., 1.)
    p = 16                                                                   # never dereferenced: rejected on the host first
    assert h.lasr_phong_shade(None, None, None, None, None, 0, 3, 1, 8, None) == 0        # empty batch
    assert h.lasr_phong_shade(None, None, None, bg, None, 1, 3, 1, 8, None) == -1          # null buffers
    assert h.lasr_phong_shade(p, p, p, None, p, 1, 3, 1, 8, None) == -1                    # null background
    for N, V, F, S in ((-1, 3, 1, 8), (1, 0, 1, 8), (1, 3, 0, 8), (1, 3, 1, 0), (1, 3, 1, 8193), (65536, 3, 1, 8)):
        assert h.lasr_phong_shade(p, p, p, bg, p, N, V, F, S, None) == -1, (N, V, F, S)


def test_render_flag_defaults_off_and_keeps_optimize_defaults():
    sys.path.insert(0, ROOT)
    import extract
    import optimize
    before = dict(optimize.DEFAULTS)
    opts = extract.parse_flags(['--model_path', 'x.pth'])
    assert opts.render is False and 'render' not in optimize.DEFAULTS and optimize.DEFAULTS == before
    assert extract.parse_flags(['--render']).render is True


def test_overlay_restates_the_reference_arithmetic():
    sys.path.insert(0, ROOT)
    import extract
    img = np.array([[[0.5, 0.2, 1.0]]]).transpose(2, 0, 1)                # [3,1,1] in 0-1
    out = extract.mask_overlay(img, np.array([[0.6]]))
    # red = (0, 0, 255) * 0.6*255/255 -> uint8 (0, 0, 153); addWeighted(red, .5, 255 img (uint8), 1, 0) rounds and saturates
    base = (255 * np.array([0.5, 0.2, 1.0])).astype(np.uint8)
    want = np.clip(np.round(0.5 * np.array([0, 0, 153]) + base), 0, 255)
    assert out.dtype == np.uint8 and np.array_equal(out[0, 0], want.astype(np.uint8)), out


def test_eval_mesh_render_flags():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import eval_mesh
    a = eval_mesh.parse_args(['--testdir', 't', '--gtdir', 'g'])
    assert a.render is False and a.gif == os.path.join('tmp', 'output.gif')
    assert eval_mesh.parse_args(['--testdir', 't', '--gtdir', 'g', '--render', '--gif', 'x.gif']).gif == 'x.gif'


def test_error_colour_is_plasma_of_twice_the_squared_distance():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import eval_mesh
    import matplotlib
    d2 = np.array([0., 0.1, 0.3, 2.])
    assert np.allclose(eval_mesh.error_colors(d2), matplotlib.colormaps['plasma'](2 * d2)[:, :3])
