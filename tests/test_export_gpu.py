"""Export side of soft_renderer on the GPU (csrc/export.hip): voxelisation and texture atlases bit for bit against the numpy
restatement of the reference (tests/export_restated.py), and the .obj / .mtl / .png round trip of save_obj."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import export_restated as xr                     # noqa: E402
from test_export_cpu import cube, sphere          # noqa: E402

SPOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'spot', 'spot_triangulated.obj')
SIZES = [16, 32, 64, 65, 100, 128]


def _fit(f, lo=0.05, hi=0.95):
    """Scale a face array [F,3,3] uniformly into [lo, hi]^3 (unit voxelisation coordinates)."""
    mn, mx = f.reshape(-1, 3).min(0), f.reshape(-1, 3).max(0)
    return (f - (mn + mx) / 2) / (mx - mn).max() * (hi - lo) + 0.5


def _spot_faces():
    from lasr_amd.soft_renderer import functional as srf
    v, f = srf.load_obj(SPOT, device='cpu')
    return v.numpy().astype(np.float64)[f.numpy()]


def meshes():
    from lasr_amd import synth
    v, f = synth.geodesic_sphere(8)
    bv, bf, _ = synth.blobby_mesh(11)                 # M2: 2,420 faces
    hemi = sphere(0.35, 0.5, 8)
    return {
        'cube': cube(0.2, 0.8),
        'sphere': _fit(v.astype(np.float64)[f]),
        'blobby_m2': _fit(bv.astype(np.float64)[bf]),
        'spot': _fit(_spot_faces()),
        'nested': np.concatenate([sphere(0.4, 0.5, 6), sphere(0.25, 0.5, 5)[:, ::-1]]),
        'hemisphere': hemi[hemi.mean(1)[:, 2] > 0.5],
        'crossing': sphere(0.35, np.array([0.85, 0.3, 0.6]), 6),
    }


@pytest.fixture(scope='module')
def mesh_set():
    return meshes()


def _gpu(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('S', SIZES)
def test_voxelization_matches_the_restatement(cuda, mesh_set, S, dtype):
    from lasr_amd.soft_renderer import functional as srf
    bad = []
    for name, f in mesh_set.items():
        faces = np.ascontiguousarray(f[None], dtype=dtype)
        got = srf.voxelization(_gpu(faces, dtype, cuda), S)
        assert got.dtype == torch.int32 and got.shape == (1, S, S, S)
        want = torch.from_numpy(xr.voxelization(faces, S))
        if not torch.equal(got.cpu(), want):
            bad.append('%s: %d voxels differ' % (name, int((got.cpu() != want).sum())))
        elif name in ('cube', 'sphere', 'nested'):
            surf = xr.surface(faces[0] * dtype(S), S)
            assert want.sum() > surf.sum(), name           # closed meshes: the fill added an interior
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('S', [32, 100])
def test_voxelization_batch_of_different_meshes(cuda, mesh_set, S, dtype):
    from lasr_amd.soft_renderer import functional as srf
    F = 2000
    picks = [mesh_set['blobby_m2'], mesh_set['nested'], mesh_set['crossing']]
    batch = np.zeros((3, F, 3, 3), dtype)              # padding: degenerate faces at the origin (a single vertex voxel)
    for i, f in enumerate(picks):
        f = f[:F]
        batch[i, :len(f)] = f
    faces = _gpu(batch, dtype, cuda)
    torch.cuda.synchronize()
    with torch.cuda.device(cuda):
        torch.cuda.set_sync_debug_mode('error')          # the call chain must not synchronise with the host
        try:
            got = srf.voxelization(faces, S)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    want = torch.from_numpy(xr.voxelization(batch, S))
    assert torch.equal(got.cpu(), want)


@pytest.mark.gpu
def test_mesh_voxelize_default_size(cuda):
    import lasr_amd.soft_renderer as sr
    from lasr_amd import synth
    v, f, _ = synth.blobby_mesh(11)
    v = v / np.abs(v).max() * 0.49
    mesh = sr.Mesh(torch.from_numpy(v).to(cuda)[None], torch.from_numpy(f.astype(np.int32)).to(cuda)[None])
    got = mesh.voxelize()
    S = 32
    fv = mesh.face_vertices.cpu().numpy()
    norm = fv * np.float32(S) / np.float32(S - 1) + np.float32(0.5)
    assert got.shape == (1, S, S, S)
    assert torch.equal(got.cpu(), torch.from_numpy(xr.voxelization(norm, S)))
    assert got.sum() > 1000


@pytest.mark.gpu
def test_voxelization_rejects_sizes_past_the_limit(cuda):
    from lasr_amd.soft_renderer import functional as srf
    with pytest.raises(ValueError):
        srf.voxelization(torch.zeros(1, 1, 3, 3, device=cuda), 257)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('F', [1, 2, 7, 2420, 5856])
def test_texture_atlas_matches_the_restatement(cuda, F, dtype):
    from lasr_amd.soft_renderer import functional as srf
    rng = np.random.default_rng(F)
    for R_in in (1, 2, 4, 6):
        tex = rng.uniform(0, 1, (F, R_in * R_in, 3)).astype(dtype)
        for R_out in (2, 4, 16):
            image, vt = srf.create_texture_image(_gpu(tex, dtype, cuda), R_out)
            want_image, want_vt = xr.texture_image(tex, R_out)
            assert image.dtype == dtype and vt.dtype == dtype
            assert image.shape == want_image.shape and vt.shape == (F, 3, 2)
            assert np.array_equal(image, want_image), (R_in, R_out, int((image != want_image).sum()))
            assert np.array_equal(vt, want_vt), (R_in, R_out)


def _read_obj(path):
    v, vt, f, mtl = 0, 0, [], None
    for line in open(path):
        tok = line.split()
        if not tok:
            continue
        if tok[0] == 'v':
            v += 1
        elif tok[0] == 'vt':
            vt += 1
        elif tok[0] == 'f':
            f.append(tok[1:])
        elif tok[0] == 'mtllib':
            mtl = tok[1]
    return v, vt, f, mtl


@pytest.mark.gpu
def test_textured_round_trip_through_files(cuda, tmp_path):
    import lasr_amd.soft_renderer as sr
    from lasr_amd.soft_renderer import functional as srf
    from PIL import Image
    mesh = sr.Mesh.from_obj(SPOT, load_texture=True, texture_res=1)
    F = mesh.num_faces
    out = str(tmp_path / 'spot_out.obj')
    mesh.save_obj(out, save_texture=True, texture_res_out=8)
    v, vt, f, mtl = _read_obj(out)
    assert (v, vt, len(f), mtl) == (mesh.num_vertices, 3 * F, F, 'spot_out.mtl')
    assert f[1] == ['%d/4' % (mesh.faces[0, 1, 0].item() + 1), '%d/5' % (mesh.faces[0, 1, 1].item() + 1),
                    '%d/6' % (mesh.faces[0, 1, 2].item() + 1)]
    assert open(str(tmp_path / 'spot_out.mtl')).read().split() == ['newmtl', 'material_1', 'map_Kd', 'spot_out.png']
    verts, faces, tex = srf.load_obj(out, load_texture=True, texture_res=1)
    assert torch.equal(faces, mesh.faces[0]) and torch.allclose(verts, mesh.vertices[0], atol=1e-6)
    err = (tex - mesh.textures[0]).abs().amax(dim=(1, 2))
    assert float(err.max()) <= 1 / 255 + 1e-6, (int((err > 1 / 255 + 1e-6).sum()), float(err.max()))
    # R_in > 1: the files only (bilinear re-sampling makes the round trip inexact)
    tex4 = torch.rand(F, 16, 3, device=cuda)
    out4 = str(tmp_path / 'spot4.obj')
    srf.save_obj(out4, mesh.vertices[0], mesh.faces[0], tex4, texture_res=16)
    v, vt, f, mtl = _read_obj(out4)
    assert vt == 3 * F and mtl == 'spot4.mtl'
    assert 'map_Kd spot4.png' in open(str(tmp_path / 'spot4.mtl')).read()
    tw = int((F - 1.) ** 0.5) + 1
    th = int((F - 1.) / tw) + 1
    png = Image.open(str(tmp_path / 'spot4.png'))
    assert png.size == (tw * 16, th * 16) and png.mode == 'RGB'


@pytest.mark.gpu
def test_save_voxel_writes_one_vertex_per_set_voxel(cuda, tmp_path):
    from lasr_amd.soft_renderer import functional as srf
    vox = srf.voxelization(_gpu(sphere(0.3, 0.5, 4)[None], np.float32, cuda), 16)[0]
    path = str(tmp_path / 'vox.obj')
    srf.save_voxel(path, vox)
    lines = [l.split() for l in open(path) if l.startswith('v ')]
    assert len(lines) == int(vox.sum()) > 0
    assert not any(l.startswith('f ') for l in open(path))
    got = np.asarray([[float(t) for t in l[1:]] for l in lines])
    idx = np.argwhere(vox.cpu().numpy() == 1)
    want = (idx / 16.).astype(np.float32)
    assert np.array_equal(got, np.asarray([[float('%.8f' % c) for c in p] for p in want]))
