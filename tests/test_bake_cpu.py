"""Texture bake without a device: the texel layout, closed forms of the float64 restatement (tests/bake_restated.py), the C ABI's
host-side checks, the script's argument handling, and the undecided share of the fixture tests/test_bake_gpu.py compares on."""
import os
import sys

import numpy as np
import pytest

import bake_restated as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('R', [1, 2, 3, 5, 8])
def test_every_centroid_maps_to_its_own_texel(R):
    c0, c1, c2 = br.centroids(R)
    got = [br.surface_texel(float(a), float(b), R) for a, b in zip(c0, c1)]
    assert got == list(range(R * R))
    assert (c0 > 0).all() and (c1 > 0).all() and (c2 > 0).all()                  # strictly inside the face
    # the same through float32, the kernel's arithmetic
    c0f, c1f = c0.astype(np.float32), c1.astype(np.float32)
    assert [br.surface_texel(np.float32(a), np.float32(b), R) for a, b in zip(c0f, c1f)] == list(range(R * R))


def _fronto_triangle():
    """One triangle at z = 2 that projects well inside the 48 x 64 frame, and a face-index plane that names it everywhere."""
    verts = np.array([[[-0.5, -0.4, 2.], [0.6, -0.3, 2.], [-0.1, 0.5, 2.]]])
    K = np.array([[40., 40., 32., 24.]])
    return verts, np.array([[0, 1, 2]]), K, np.zeros((1, br.H, br.W))


def test_restatement_affine_image_closed_form():
    verts, faces, K, plane = _fronto_triangle()
    a, b, c = 2., 2., 10.
    frames = br.ramp_image(a, b, c)[None]
    for R in (1, 4, 5):
        tex, weight, _ = br.bake(verts, faces, K, plane, frames, R=R, power=2)
        _, u, v = br.project(verts, faces, K, R)
        assert (weight > 0).all()
        for ch in range(3):
            want = (a * u[0] + b * v[0] + c + ch) / 255.
            assert np.abs(tex[..., ch] - want).max() <= 1e-12


def test_restatement_constant_frames_and_plain_mean():
    verts, faces, K, plane = _fronto_triangle()
    verts2, K2, plane2 = np.repeat(verts, 2, 0), np.repeat(K, 2, 0), np.repeat(plane, 2, 0)
    const = np.full((2, br.H, br.W, 3), 51, np.uint8)
    tex, weight, _ = br.bake(verts2, faces, K2, plane2, const, R=3, power=2)
    assert np.abs(tex - 0.2).max() <= 1e-12 and (weight > 0).all()
    two = np.stack([np.full((br.H, br.W, 3), 51, np.uint8), np.full((br.H, br.W, 3), 153, np.uint8)])
    verts2[1, :, 2] = 3.                                                          # another depth, so other view weights for p > 0
    verts2[1, 0, 2] = 2.5
    tex, weight, _ = br.bake(verts2, faces, K2, plane2, two, R=3, power=0)
    assert np.abs(tex - 0.4).max() <= 1e-12 and np.abs(weight - 2.).max() == 0
    # an unseen face takes the fallback's interpolation, or grey
    none = -np.ones_like(plane)
    fb = np.array([[1., 0., 0.], [0., 1., 0.], [0., 0., 1.]])
    tex, weight, _ = br.bake(verts, faces, K, none, const[:1], R=2, power=2, fallback=fb)
    c0, c1, c2 = br.centroids(2)
    assert (weight == 0).all() and np.abs(tex[0] - np.stack([c0, c1, c2], 1)).max() <= 1e-15
    assert (br.bake(verts, faces, K, none, const[:1], R=2)[0] == 0.5).all()


def test_symbols_are_exported_and_the_host_checks_run_without_a_device():
    from lasr_amd import _lib
    h = _lib.lib()
    n = None
    acc = lambda T=1, V=3, F=1, R=4, IS=64, H=48, W=64, power=2: h.lasr_bake_accumulate(n, n, n, n, n, n, n, T, V, F, R, IS, H, W,   # noqa: E731
                                                                                         power, n)
    assert acc(T=0) == 0 and acc(F=0) == 0                                        # nothing to do
    assert acc() == -1                                                            # null buffers
    assert acc(R=0) == -1 and acc(R=33) == -1 and acc(T=0, R=32) == 0
    assert acc(T=0, H=0) == -1 and acc(T=0, W=0) == -1 and acc(T=0, H=65) == -1 and acc(T=0, W=65) == -1
    assert acc(T=0, IS=8193, H=8193, W=1) == -1 and acc(T=0, IS=8192, H=8192, W=1) == 0
    assert acc(T=0, power=-1) == -1 and acc(T=0, power=17) == -1 and acc(T=0, power=16) == 0 and acc(T=0, power=0) == 0
    assert acc(T=0, F=(1 << 31) // (4 * 16), R=4) == -1 and acc(T=0, F=(1 << 31) // (4 * 16) - 1, R=4) == 0   # 4 F R R in int32
    assert acc(T=-1) == -1 and acc(T=0, F=-1) == -1 and acc(T=0, V=0) == -1
    res = lambda V=3, F=1, R=4: h.lasr_bake_resolve(n, n, n, n, n, V, F, R, n)    # noqa: E731
    assert res(F=0) == 0 and res() == -1 and res(F=0, R=0) == -1 and res(F=0, R=33) == -1 and res(F=0, V=0) == -1
    assert res(F=(1 << 31) // 64, R=4) == -1
    names = [h.lasr_prof_kernel_name(i) for i in range(h.lasr_prof_kernel_count())]
    assert names[-2:] == [b'bake_accumulate_kernel', b'bake_resolve_kernel']      # appended: earlier ids keep their numbers
    assert (_lib.BAKE_MAX_RES, _lib.BAKE_MAX_SIZE, _lib.BAKE_MAX_POWER) == (32, 8192, 16)
    hdr = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    for name, value in (('RES', 32), ('SIZE', 8192), ('POWER', 16)):
        assert '#define LASR_BAKE_MAX_%s %d\n' % (name, value) in hdr


def test_python_layer_refuses_cpu_tensors():
    import torch
    from lasr_amd.nnutils import bake
    v, f, K = torch.zeros(1, 3, 3), torch.tensor([[0, 1, 2]]), torch.ones(1, 4)
    with pytest.raises(TypeError):
        bake.bake_texture(v, f, K, torch.zeros(1, 4, 4, 3, dtype=torch.uint8))


def test_script_arguments_and_topology_check():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import bake_texture
    a = bake_texture.parse_args(['--testdir', 'log/camel-5/', '--seqname', 'camel'])
    assert (a.texture_res, a.power, a.pose_frame, a.mask, a.outpath, a.preview) == (8, 2, 0, True, '', '')
    a = bake_texture.parse_args('--testdir t --seqname s --texture_res 4 --power 0 --pose_frame 3 --no_mask --outpath o/baked '
                                '--preview p.gif'.split())
    assert (a.texture_res, a.power, a.pose_frame, a.mask, a.outpath, a.preview) == (4, 0, 3, False, 'o/baked', 'p.gif')
    f = np.array([[0, 1, 2], [0, 2, 3]])
    assert (bake_texture.check_topology([f, f.copy()], [0, 1]) == f).all()
    with pytest.raises(ValueError, match='pred7 does not share the topology of pred5'):
        bake_texture.check_topology([f, f, f[:, ::-1]], [5, 6, 7])
    with pytest.raises(ValueError, match='pred6 does not share'):
        bake_texture.check_topology([f, f[:1]], [5, 6])
    assert bake_texture.silhouette_path('d/JPEGImages/Full-Resolution/s/00003.jpg') == 'd/Annotations/Full-Resolution/s/00003.png'


def test_undecided_share_of_the_gpu_fixture_is_small():
    verts, faces, K, frames, masks = br.icosphere_case()
    assert verts.shape == (4, 42, 3) and faces.shape == (80, 3) and frames.shape == (4, br.H, br.W, 3)
    plane = br.numpy_face_index(verts, faces, K)
    assert (plane[:, br.H:] == -1).all() and ((plane >= 0).reshape(4, -1).mean(1) > 0.15).all()   # inside the frame, a fair share
    for R in (3, 8):
        for m in (None, masks):
            tex, weight, undecided = br.bake(verts, faces, K, plane, frames, m, R=R, power=2)
            print('R %d masks %s: undecided %.3f %%, seen %.1f %%' % (R, m is not None, 100 * undecided.mean(), 100 * (weight > 0).mean()))
            assert undecided.mean() <= 0.02
            assert (weight > 0).mean() > 0.5                                      # four views a quarter turn apart see most of a sphere
