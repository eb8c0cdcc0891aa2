"""Export side of soft_renderer without a GPU: the reference's names and signatures, host-side argument checks of the two C
entry points, and known answers of the numpy restatement (tests/export_restated.py) that the GPU tests hold the kernels to."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import export_restated as xr                     # noqa: E402


def test_signatures_match_the_reference():
    import lasr_amd.soft_renderer as sr
    import lasr_amd.soft_renderer.functional as srf
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    # third_party/softras/soft_renderer/functional/save_obj.py:9,90, voxelization.py:41, mesh.py:177
    assert sig(srf.create_texture_image) == [('textures', E), ('texture_res', 16)]
    assert sig(srf.save_voxel) == [('filename', E), ('voxel', E)]
    assert sig(srf.voxelization) == [('faces', E), ('size', E), ('normalize', False)]
    assert sig(sr.Mesh.voxelize) == [('self', E), ('voxel_size', 32)]


def test_entry_points_reject_bad_arguments_on_the_host():
    from lasr_amd import _lib
    h = _lib.lib()
    dummy = 16                                    # never dereferenced: every call below fails before a launch
    for vox in (h.lasr_voxelize, h.lasr_voxelize_f64):
        assert vox(dummy, dummy, None, dummy, 1 << 30, 1, 4, 257, None) == -1          # S > LASR_VOXEL_MAX_SIZE
        assert vox(dummy, dummy, None, dummy, 1 << 30, 1, 4, 0, None) == -1            # S < 1
        assert vox(dummy, dummy, None, dummy, 1 << 30, -1, 4, 8, None) == -1
        assert vox(dummy, dummy, None, dummy, 1 << 30, 1, -4, 8, None) == -1
        assert vox(None, dummy, None, dummy, 1 << 30, 1, 4, 8, None) == -1             # faces
        assert vox(dummy, None, None, dummy, 1 << 30, 1, 4, 8, None) == -1             # voxels
        assert vox(dummy, dummy, None, None, 1 << 30, 1, 4, 8, None) == -3             # workspace
        assert vox(dummy, dummy, None, dummy, 7, 1, 4, 8, None) == -3
        assert vox(dummy, dummy, None, dummy, 1 << 30, 1 << 20, 1 << 10, 8, None) == -1  # B * F * 9 overflows int
        assert vox(None, None, None, None, 0, 0, 4, 8, None) == 0                       # empty batch
    assert h.lasr_voxelize_workspace_bytes(2, 64) == 2 * 64 * 64 * 8
    assert h.lasr_voxelize_workspace_bytes(1, 65) == 65 * 65 * 2 * 8 * 3
    assert h.lasr_voxelize_workspace_bytes(1, 257) == 0 and h.lasr_voxelize_workspace_bytes(1, 0) == 0
    for tex in (h.lasr_create_texture_image, h.lasr_create_texture_image_f64):
        assert tex(None, None, None, 0, 2, 4, 1e-5, None) == 0                           # no faces
        assert tex(None, dummy, dummy, 3, 2, 4, 1e-5, None) == -1
        assert tex(dummy, None, dummy, 3, 2, 4, 1e-5, None) == -1
        assert tex(dummy, dummy, None, 3, 2, 4, 1e-5, None) == -1
        assert tex(dummy, dummy, dummy, 3, 0, 4, 1e-5, None) == -1
        assert tex(dummy, dummy, dummy, 3, 2, 0, 1e-5, None) == -1
        assert tex(dummy, dummy, dummy, -3, 2, 4, 1e-5, None) == -1
        assert tex(dummy, dummy, dummy, 1 << 20, 2, 1 << 10, 1e-5, None) == -1         # image larger than int indexing


def cube(lo, hi):
    """Closed axis-aligned box, 12 outward triangles: [12,3,3]."""
    c = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [[q[0], q[1], q[2]] for q in quads] + [[q[0], q[2], q[3]] for q in quads]
    return c[np.asarray(f)]


def sphere(r, centre, nu=6):
    from lasr_amd import synth
    v, f = synth.geodesic_sphere(nu)
    return (v.astype(np.float64) * r + centre)[f]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_restated_cube_is_a_solid_block(dtype):
    S = 16
    vox = xr.voxelization(cube(4.5, 10.5)[None].astype(dtype), S, normalize=True)[0]
    want = np.zeros((S, S, S), np.int32)
    want[4:11, 4:11, 4:11] = 1                      # faces at 4.5 / 10.5 mark voxels 4 and 10; the inside is filled
    assert (vox == want).all() and vox.sum() == 7 ** 3


def test_restated_single_triangle_is_only_its_surface():
    S = 16
    tri = np.array([[[2.2, 2.3, 5.5], [12.7, 2.4, 5.5], [2.1, 12.8, 5.5]]])
    vox = xr.voxelization(tri[None], S, normalize=True)[0]
    occ = xr.surface(tri, S)
    assert (vox == occ).all()                       # an open mesh encloses nothing
    assert vox.sum() > 0 and set(np.unique(np.nonzero(vox)[2])) == {5}
    assert vox[:, :, 4].sum() == 0 and vox[:, :, 6].sum() == 0


def test_restated_nested_spheres_fill_the_outer_volume():
    S = 32
    outer, inner = sphere(12.0, 16.0), sphere(6.0, 16.0)
    both = xr.voxelization(np.concatenate([outer, inner])[None], S, normalize=True)[0]
    alone = xr.voxelization(outer[None], S, normalize=True)[0]
    assert (both == alone).all()                    # the inner surface and the cavity lie inside the filled outer one
    c = np.stack(np.meshgrid(*[np.arange(S) + 0.5] * 3, indexing='ij'), -1)
    r = np.linalg.norm(c - 16.0, axis=-1)
    assert both[r < 10].all() and not both[r > 14].any()


def test_restated_fill_matches_the_reference_sweeps_and_the_box_margin_is_wide_enough():
    S = 20
    rng = np.random.default_rng(3)
    faces = np.concatenate([sphere(7.0, 10.0, 4), sphere(3.0, 9.0, 3), rng.uniform(-2, 22, (40, 3, 3))])
    occ_full = xr.surface(faces, S, margin=None)     # every column of the grid, as the reference scans
    assert (xr.surface(faces, S, margin=2) == occ_full).all() and (xr.surface(faces, S, margin=1) == occ_full).all()
    assert (xr.fill(occ_full) == xr.fill_sweeps(occ_full)).all()


def test_restated_two_face_atlas_layout():
    tex = np.zeros((2, 4, 3), np.float32)            # R_in = 2: texel t of face f has colour (f, t, 0.5)
    tex[:, :, 0] = np.arange(2)[:, None]
    tex[:, :, 1] = np.arange(4)[None, :]
    tex[:, :, 2] = 0.5
    image, vt = xr.texture_image(tex, 4)
    tw, th, v = xr.atlas_layout(2, 4)
    assert (tw, th) == (2, 1) and image.shape == (4, 8, 3)
    # corners: (c*R + R/2, r*R + 1), (c*R + 1, (r+1)*R - 2), ((c+1)*R - 2, (r+1)*R - 2)
    assert (v == np.array([[[2, 1], [1, 2], [2, 2]], [[6, 1], [5, 2], [6, 2]]], np.float32)).all()
    assert np.allclose(vt, v / np.array([7, 3], np.float32)) and vt.dtype == np.float32
    img = image[::-1]                                 # back to row 0 = y 0
    assert (img[:, :4, 0] == 0).all() and (img[:, 4:, 0] == 1).all()   # each tile holds only its own face's texels
    assert (img[..., 2] == 0.5).all()
    # face 0 by hand: the triangle (2,1) (1,2) (2,2) has w = (2-y, 2-x, x+y-3), clamped to [0,1] and normalised; e.g. pixel
    # (0,0): (1/2, 1/2, 0) -> w_x = w_y = 0 and (w0+w1)R - 0 - 0 = 2 > 1 -> mirrored texel (1,1) = 3; pixel (2,1): (1, 0, 0) ->
    # w_x = 1 (1/(1+eps) * 2), lower texel 1
    want = np.array([[3, 3, 1, 1],
                     [3, 3, 1, 0],
                     [2, 2, 0, 0],
                     [2, 0, 0, 0]])
    assert (img[:, :4, 1] == want).all(), img[:, :4, 1]


def test_restated_atlas_pixels_past_the_last_face_are_one():
    tex = np.random.default_rng(0).uniform(0, 0.9, (7, 1, 3)).astype(np.float32)
    image, _ = xr.texture_image(tex, 2)
    img = image[::-1]
    assert img.shape == (6, 6, 3)
    assert (img[4:, 2:] == 1).all() and (img[:4] < 1).all() and (img[4:, :2] < 1).all()
