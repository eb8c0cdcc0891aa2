"""Watertight re-meshing on the GPU (csrc/manifold.hip, lasr_amd/nnutils/manifold.py): the repair, refill and extraction bit for
bit against the numpy restatement, the topology and geometry of watertight() on closed, open, overlapping, nested and inverted
inputs, the guard, determinism, and the two scripts end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manifold_restated as mr                    # noqa: E402

pytestmark = pytest.mark.gpu
SPOT = os.path.join(ROOT, 'tests', 'golden', 'spot', 'spot_triangulated.obj')
DEV = torch.device('cuda', 0)


def spot():
    from lasr_amd.soft_renderer.functional import load_obj
    v, f = load_obj(SPOT, device=DEV)[:2]
    return v.float(), f.long()


def icosphere(centre=(0., 0., 0.), radius=1.):
    d = np.load(os.path.join(ROOT, 'tests', 'golden', 'meshzoo_icosphere.npz'))
    v = d['v3'] / np.linalg.norm(d['v3'], axis=1, keepdims=True) * radius + np.asarray(centre)
    f = d['f3'].astype(np.int64)
    if mr.signed_volume(v, f) < 0:
        f = f[:, ::-1].copy()
    return v, f


def torus(R=1., r=0.4, n=48, m=24):
    u, w = np.meshgrid(np.arange(n) * 2 * np.pi / n, np.arange(m) * 2 * np.pi / m, indexing='ij')
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing='ij')
    a, b = i * m + j, ((i + 1) % n) * m + j
    c, d = ((i + 1) % n) * m + (j + 1) % m, i * m + (j + 1) % m
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    if mr.signed_volume(v, f) < 0:
        f = f[:, ::-1].copy()
    return v, f


def disk(n=64):
    t = np.arange(n) * 2 * np.pi / n
    v = np.concatenate([[[0., 0., 0.]], np.stack([np.cos(t), np.sin(t), 0 * t], 1)])
    f = np.stack([np.zeros(n, int), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], 1)
    return v, f


def gpu(v, f):
    return torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32, device=DEV), torch.as_tensor(np.ascontiguousarray(f),
                                                                                                      dtype=torch.int64, device=DEV)


def check_closed_manifold(verts, faces):
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    assert len(f) % 2 == 0 and len(f) > 0
    assert mr.closed_oriented(f), 'a directed edge is missing its reverse or appears twice'
    assert mr.vertex_links_are_cycles(f, len(v)), 'a vertex link is not one cycle'
    assert mr.signed_volume(v, f) > 0
    return mr.euler(f, len(v)), mr.components(f, len(v))


# ---- bit for bit against the restatement -------------------------------------------------------------------------------------
CASES = [(16, 0.35, 0, 1), (48, 0.5, 0, 2), (64, 0.3, 0, 3), (100, 0.6, 0, 4), (128, 0.5, 3, 5), (256, 0.5, 8, 6)]


@pytest.mark.parametrize('S,density,smooth,seed', CASES)
def test_repair_refill_extract_match_the_restatement(S, density, smooth, seed):
    from lasr_amd.nnutils import manifold
    solid = mr.random_solid(S, density, seed, smooth=smooth)
    if S == 128:                                          # a closed cavity the refill must fill
        solid[60:70, 60:70, 60:70] = True
        solid[62:68, 62:68, 62:68] = False
    want, sweeps, wv, wf = mr.pipeline(solid)
    vox = torch.from_numpy(solid.astype(np.int32)).to(DEV)
    verts, faces, host = manifold.boundary(vox)
    assert host[0] == sweeps
    np.testing.assert_array_equal(vox.cpu().numpy(), want.astype(np.int32))
    assert host[3:] == [len(wv), len(wf)]
    np.testing.assert_array_equal(verts.cpu().numpy(), wv.astype(np.float32))
    np.testing.assert_array_equal(faces.cpu().numpy(), wf)
    assert mr.closed_oriented(wf)
    if S <= 64:
        assert mr.vertex_links_are_cycles(wf, len(wv))
    assert mr.signed_volume(wv, wf) == pytest.approx(float(want.sum()))


def test_a_solid_on_the_outer_layer_is_refused():
    from lasr_amd.nnutils import manifold
    s = np.zeros((16, 16, 16), np.int32)
    s[5:9, 5:9, 5:9] = 1
    s[5, 5, 15] = 1
    with pytest.raises(ValueError, match='outer voxel layer'):
        manifold.boundary(torch.from_numpy(s).to(DEV))


# ---- watertight() on inputs ----------------------------------------------------------------------------------------------------
def test_spot_is_one_sphere():
    from lasr_amd.nnutils import manifold
    v, f = spot()
    r = manifold.remesh(v, f, 10000)
    assert r['S'] == 128 and r['surface_voxels'] >= 10000
    assert check_closed_manifold(r['verts'], r['faces']) == (2, 1)


def test_torus_has_genus_one():
    from lasr_amd.nnutils.manifold import watertight
    assert check_closed_manifold(*watertight(*gpu(*torus()), 5000)) == (0, 1)


def test_overlapping_spheres_become_one():
    from lasr_amd.nnutils.manifold import watertight
    a, fa = icosphere((0., 0., 0.))
    b, fb = icosphere((0.8, 0.3, 0.))
    v, f = np.concatenate([a, b]), np.concatenate([fa, fb + len(a)])
    assert check_closed_manifold(*watertight(*gpu(v, f), 5000)) == (2, 1)


def test_nested_reversed_sphere_is_filled():
    from lasr_amd.nnutils.manifold import watertight
    a, fa = icosphere()
    b, fb = icosphere(radius=0.5)
    v, f = np.concatenate([a, b]), np.concatenate([fa, fb[:, ::-1] + len(a)])
    assert check_closed_manifold(*watertight(*gpu(v, f), 5000)) == (2, 1)


def test_spot_with_holes_comes_out_closed():
    from lasr_amd.nnutils.manifold import watertight
    v, f = spot()
    keep = torch.from_numpy(np.random.default_rng(0).random(f.shape[0]) >= 0.05).to(DEV)
    check_closed_manifold(*watertight(v, f[keep], 10000))


def test_open_disk_comes_out_a_closed_sphere():
    from lasr_amd.nnutils.manifold import watertight
    assert check_closed_manifold(*watertight(*gpu(*disk()), 2000)) == (2, 1)


def test_inverted_input_comes_out_with_positive_volume():
    from lasr_amd.nnutils.manifold import watertight
    v, f = spot()
    ov, of = watertight(v, f.flip(1), 10000)
    check_closed_manifold(ov, of)


# ---- geometry, guard, determinism ------------------------------------------------------------------------------------------
def distance_to(points, verts, faces):
    from lasr_amd.nnutils import manifold
    q = manifold.project(points.contiguous(), verts.contiguous(), faces.contiguous())
    return (points - q).norm(dim=1)


def test_geometry_bounds_and_guard_on_spot():
    from lasr_amd.nnutils import manifold
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import eval_mesh
    v, f = spot()
    r = manifold.remesh(v, f, 10000)
    h = r['h']
    bound = 2 * 3 ** 0.5 * h
    out, of = r['verts'], r['faces']
    assert float(distance_to(out, v, f).max()) <= bound                       # every output vertex near the input
    gen = torch.Generator(device=DEV).manual_seed(0)
    pts = eval_mesh.sample_points(v, f, 50000, gen)
    assert float(distance_to(pts, out, of).max()) <= bound                    # every input sample near the output
    moved = (r['moved'] != r['lattice']).any(1)
    assert bool(moved.any())
    diam = float((v.max(0).values - v.min(0).values).norm())
    assert float(distance_to(out[moved], v, f).max()) <= 1e-5 * diam          # moved vertices lie on the input
    # no face of the output fails the guard (lattice units, as the guard ran)
    m, lat = r['moved'][of], r['lattice'][of]
    n = torch.linalg.cross(m[:, 1] - m[:, 0], m[:, 2] - m[:, 0])
    nl = torch.linalg.cross(lat[:, 1] - lat[:, 0], lat[:, 2] - lat[:, 0])
    assert bool(((n * nl).sum(1) > 0).all())
    assert float(0.5 * n.norm(dim=1).min()) >= manifold.MIN_AREA
    assert r['rounds'] >= 0 and r['repair_sweeps'] >= 1


def test_two_calls_are_byte_identical():
    from lasr_amd.nnutils.manifold import watertight
    v, f = spot()
    a = watertight(v, f, 10000)
    b = watertight(v, f, 10000)
    assert a[1].dtype == torch.int64 and a[0].dtype == torch.float32 and a[0].device == v.device
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_bad_inputs_raise():
    from lasr_amd.nnutils.manifold import watertight
    v, f = spot()
    for args in ((v[:0], f), (v, f[:0]), (v, f, 0), (v, f, -5)):
        with pytest.raises(ValueError):
            watertight(*args)
    bad = v.clone()
    bad[3, 1] = float('nan')
    with pytest.raises(ValueError):
        watertight(bad, f)


# ---- scripts -------------------------------------------------------------------------------------------------------------------
def run(args, timeout=600):
    p = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


def test_manifold_script_writes_a_closed_mesh(tmp_path):
    from lasr_amd.soft_renderer.functional import load_obj
    out = str(tmp_path / 'spot_wt.obj')
    run([os.path.join('scripts', 'manifold.py'), SPOT, out])
    v, f = load_obj(out, device=DEV)[:2]
    assert check_closed_manifold(v, f.long()) == (2, 1)


def test_eval_mesh_remesh_scores_spot_against_itself(tmp_path):
    import shutil
    (tmp_path / 'pred').mkdir()
    (tmp_path / 'gt').mkdir()
    shutil.copy(SPOT, str(tmp_path / 'pred' / 'pred0.obj'))
    shutil.copy(SPOT, str(tmp_path / 'gt' / 'spot.obj'))
    out = run([os.path.join('scripts', 'eval_mesh.py'), '--testdir', str(tmp_path / 'pred'), '--gtdir', str(tmp_path / 'gt'),
               '--remesh', '10000'])
    cd = float(out.strip().splitlines()[-1].split()[1].rstrip(','))
    assert cd < 0.15, out
