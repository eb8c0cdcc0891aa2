"""bench.py --dump-outputs: what the last timed step computed goes to DIR/<name>.npy as float32, whole when it fits its budget and
otherwise as the same seeded choice of frames in every run, at most 64 MB in all.  The writer runs here on CPU tensors."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def fake_job(B, F, V, IS):
    g = torch.Generator().manual_seed(0)
    return types.SimpleNamespace(colors=torch.rand(B, 4, IS, IS, generator=g), gf=torch.randn(B, F, 9, generator=g),
                                 gt=torch.randn(B, F, 9, generator=g), mesh_grad=torch.randn(2, V, 3, generator=g))


def test_outputs_fit_the_budget_and_the_sample_is_fixed(tmp_path):
    B, F, V, IS = 48, 2420, 1212, 256                    # soft_colors 48 MB: over its budget; the face gradients fit
    job = fake_job(B, F, V, IS)
    info = bench.dump_outputs(job, str(tmp_path / 'a'))
    assert set(info) == {'soft_colors', 'grad_faces', 'grad_textures', 'mesh_grad'}
    files = {n: np.load(str(tmp_path / 'a' / (n + '.npy'))) for n in info}
    assert all(a.dtype == np.float32 for a in files.values())
    assert sum(os.path.getsize(str(tmp_path / 'a' / (n + '.npy'))) for n in info) <= 64e6
    rows = info['soft_colors']['frames']
    assert info['soft_colors']['shape'] == [B, 4, IS, IS] and rows == sorted(set(rows)) and 0 < len(rows) < B
    np.testing.assert_array_equal(files['soft_colors'], job.colors.numpy()[rows])
    for name, x in (('grad_faces', job.gf), ('grad_textures', job.gt), ('mesh_grad', job.mesh_grad)):
        assert info[name]['frames'] is None
        np.testing.assert_array_equal(files[name], x.numpy())
    # a second run with the same shapes writes the same frames
    again = bench.dump_outputs(job, str(tmp_path / 'b'))
    assert again == info
    np.testing.assert_array_equal(np.load(str(tmp_path / 'b' / 'soft_colors.npy')), files['soft_colors'])


def test_the_largest_launch_stays_under_64_MB(tmp_path):
    # 256 frames at 512x512: every array but the mesh gradient is sampled (one frame's storage, broadcast: 1 GB not allocated)
    B, F, V, IS = 256, 2420, 1212, 512
    job = types.SimpleNamespace(colors=torch.zeros(1, 4, IS, IS).expand(B, 4, IS, IS), gf=torch.zeros(1, F, 9).expand(B, F, 9),
                                gt=torch.zeros(1, F, 9).expand(B, F, 9), mesh_grad=torch.zeros(2, V, 3))
    info = bench.dump_outputs(job, str(tmp_path))
    assert all(info[n]['frames'] for n in ('soft_colors', 'grad_faces', 'grad_textures'))
    assert sum(os.path.getsize(str(tmp_path / (n + '.npy'))) for n in info) <= 64e6
