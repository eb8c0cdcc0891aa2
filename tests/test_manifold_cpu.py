"""Watertight re-meshing without a GPU: known answers of the numpy restatement (tests/manifold_restated.py) that the GPU tests hold
csrc/manifold.hip to, the command lines of scripts/manifold.py and eval_mesh.py --remesh, and the host-side checks of the
lasr_manifold_* entry points."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manifold_restated as mr                    # noqa: E402


def grid(S=8):
    return np.zeros((S, S, S), bool)


def closed(solid, repair=True):
    s, sweeps, v, f = mr.pipeline(solid) if repair else (mr.fill(solid), 0) + mr.extract(mr.fill(solid))
    return sweeps, v, f, mr.is_closed_manifold(f, len(v))


def test_one_voxel_is_a_cube():
    s = grid()
    s[3, 4, 2] = True
    sweeps, v, f, ok = closed(s)
    assert sweeps == 1 and ok and (len(v), len(f)) == (8, 12)
    assert mr.euler(f, len(v)) == 2 and mr.signed_volume(v, f) == 1.0
    assert v.tolist() == [[3, 4, 2], [3, 4, 3], [3, 5, 2], [3, 5, 3], [4, 4, 2], [4, 4, 3], [4, 5, 2], [4, 5, 3]]   # lattice order
    # voxel order, then -c0, +c0, -c1, +c1, -c2, +c2; two triangles per quad, counter-clockwise from outside
    normals = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert normals[::2].tolist() == [[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]]
    assert (normals[1::2] == normals[::2]).all()


@pytest.mark.parametrize('second', [(4, 5, 2), (4, 4, 3), (3, 5, 3)])
def test_voxels_sharing_only_an_edge_are_repaired(second):
    s = grid()
    s[3, 4, 2] = True
    s[second] = True
    assert not closed(s, repair=False)[3]
    sweeps, v, f, ok = closed(s)
    assert ok and sweeps == 2 and mr.euler(f, len(v)) == 2 and mr.components(f, len(v)) == 1


def test_voxels_sharing_only_a_vertex_are_repaired():
    s = grid()
    s[3, 3, 3] = s[4, 4, 4] = True
    assert not closed(s, repair=False)[3]
    sweeps, v, f, ok = closed(s)
    assert ok and sweeps == 2 and mr.euler(f, len(v)) == 2 and mr.components(f, len(v)) == 1


def test_an_empty_antipodal_pair_is_filled():
    s = grid()
    s[3:5, 3:5, 3:5] = True
    s[3, 3, 3] = s[4, 4, 4] = False
    s[4, 4, 4] = False
    rep, sweeps = mr.repair(s)
    assert sweeps == 2 and rep[3:5, 3:5, 3:5].all() and rep.sum() == 8


def test_a_ring_is_a_torus():
    s = grid()
    s[2:5, 2:5, 3] = True
    s[3, 3, 3] = False
    sweeps, v, f, ok = closed(s)
    assert ok and sweeps == 1 and mr.euler(f, len(v)) == 0 and mr.signed_volume(v, f) == 8.0


def test_a_cavity_is_filled():
    s = grid()
    s[2:6, 2:6, 2:6] = True
    s[3:5, 3:5, 3:5] = False
    sweeps, v, f, ok = closed(s)
    assert ok and mr.euler(f, len(v)) == 2 and mr.signed_volume(v, f) == 64.0


def test_random_solids_are_manifold_after_the_repair_only():
    broken = 0
    for seed, density in enumerate((0.2, 0.3, 0.45, 0.55, 0.7)):
        s = mr.random_solid(14, density, seed)
        rep, sweeps, v, f = mr.pipeline(s)
        assert mr.is_closed_manifold(f, len(v)), seed
        assert (rep >= s).all() and not rep[0].any() and not rep[-1].any()
        assert mr.signed_volume(v, f) == float(rep.sum())
        fv, ff = mr.extract(mr.fill(s))
        broken += not mr.is_closed_manifold(ff, len(fv))
    assert broken >= 1


def test_repair_never_grows_past_the_bounding_box():
    s = mr.random_solid(16, 0.4, 7, margin=5)
    rep, _ = mr.repair(s)
    assert not rep[:5].any() and not rep[-5:].any() and not rep[:, :5].any() and not rep[:, :, -5:].any()


# ---- command lines -------------------------------------------------------------------------------------------------------------
def _help(script):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', script), '--help'], capture_output=True, text=True,
                          timeout=120)


def test_manifold_script_takes_the_binary_arguments():
    r = _help('manifold.py')
    assert r.returncode == 0
    for word in ('input', 'output', 'resolution', '10000'):
        assert word in r.stdout, word


def test_eval_mesh_lists_remesh():
    r = _help('eval_mesh.py')
    assert r.returncode == 0 and '--remesh' in r.stdout and '--testdir' in r.stdout


# ---- host-side checks of the C ABI -----------------------------------------------------------------------------------------
def test_manifold_entry_points_reject_bad_arguments_on_the_host():
    from lasr_amd import _lib
    h = _lib.lib()
    d = 16                                                   # never dereferenced: every call below fails before a launch
    assert h.lasr_manifold_workspace_bytes(3) == 0 and h.lasr_manifold_workspace_bytes(257) == 0
    need = h.lasr_manifold_workspace_bytes(32)
    assert need > 4 * 32 * 32 * 8 and h.lasr_manifold_workspace_bytes(256) > need
    for S in (3, 0, -4, 257, 1 << 20):
        assert h.lasr_manifold_repair(d, d, d, 1 << 40, S, None) == -1, S
        assert h.lasr_manifold_count(d, d, d, 1 << 40, S, None) == -1, S
        assert h.lasr_manifold_extract(d, d, d, 8, 12, d, 1 << 40, S, None) == -1, S
    assert h.lasr_manifold_repair(None, d, d, need, 32, None) == -1
    assert h.lasr_manifold_repair(d, None, d, need, 32, None) == -1
    assert h.lasr_manifold_repair(d, d, None, need, 32, None) == -3
    assert h.lasr_manifold_repair(d, d, d, need - 1, 32, None) == -3
    assert h.lasr_manifold_count(None, d, d, need, 32, None) == -1
    assert h.lasr_manifold_count(d, None, d, need, 32, None) == -1
    assert h.lasr_manifold_count(d, d, d, need - 8, 32, None) == -3
    assert h.lasr_manifold_extract(None, d, d, 8, 12, d, need, 32, None) == -1
    assert h.lasr_manifold_extract(d, None, d, 8, 12, d, need, 32, None) == -1
    assert h.lasr_manifold_extract(d, d, None, 8, 12, d, need, 32, None) == -1
    assert h.lasr_manifold_extract(d, d, d, -1, 12, d, need, 32, None) == -1
    assert h.lasr_manifold_extract(d, d, d, 8, 13, d, need, 32, None) == -1       # triangles come in pairs
    assert h.lasr_manifold_extract(d, d, d, 8, 12, d, need // 2, 32, None) == -3
    assert h.lasr_manifold_project(d, d, d, d, d, -1, 10, 10, None) == -1
    assert h.lasr_manifold_project(d, d, d, d, d, 5, 0, 10, None) == -1
    assert h.lasr_manifold_project(d, d, d, d, d, 5, 10, 0, None) == -1
    assert h.lasr_manifold_project(d, d, d, d, d, 0, 10, 10, None) == 0           # nothing to move
    for i in range(5):
        args = [d] * 5
        args[i] = None
        assert h.lasr_manifold_project(*args, 5, 10, 10, None) == -1, i
    assert h.lasr_manifold_guard(d, d, d, d, d, -1, 12, 1e-4, None) == -1
    assert h.lasr_manifold_guard(d, d, d, d, d, 8, -2, 1e-4, None) == -1
    assert h.lasr_manifold_guard(d, d, d, d, d, 8, 12, -1.0, None) == -1
    assert h.lasr_manifold_guard(d, d, d, d, d, 8, 12, float('nan'), None) == -1
    for i in range(5):
        args = [d] * 5
        args[i] = None
        assert h.lasr_manifold_guard(*args, 8, 12, 1e-4, None) == -1, i


def test_watertight_refuses_bad_input_before_the_device():
    import torch
    from lasr_amd.nnutils.manifold import watertight
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises((TypeError, ValueError)):
        watertight(v, f)                                     # CPU tensors: no fallback
    with pytest.raises(TypeError):
        watertight([[0, 0, 0]], f)
