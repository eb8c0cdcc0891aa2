"""posed.sequence without a device (lasr_amd/nnutils/posed.py): what is refused before any shape is looked at, under each
caller's name, and that the callers and bake.py's re-exports go through the one module."""
import numpy as np
import pytest
import torch

WHO = ('bake_texture', 'track_points', 'reproj.evaluate')


@pytest.mark.parametrize('who', WHO)
def test_sequence_refuses_what_is_not_a_device_tensor(who):
    from lasr_amd import _lib
    from lasr_amd.nnutils import posed
    good = dict(verts=torch.zeros(1, 3, 3), faces=torch.tensor([[0, 1, 2]]), K=torch.ones(1, 4))
    for name in ('verts', 'faces', 'K'):
        for bad in (good[name].numpy(), good[name].tolist(), None):
            with pytest.raises(TypeError, match='^%s: %s must be a tensor$' % (who, name)):
                posed.sequence(who, **dict(good, **{name: bad}), H=4, W=4, max_size=8)
    with pytest.raises(TypeError) as e:                                # tensors, but on the host: there is no CPU fallback
        posed.sequence(who, good['verts'], good['faces'], good['K'], 4, 4, 8)
    assert str(e.value) == _lib._NEED_CUDA
    with pytest.raises(TypeError) as e:                                # before any shape is looked at
        posed.sequence(who, torch.zeros(3), good['faces'], good['K'], 0, 0, 8)
    assert str(e.value) == _lib._NEED_CUDA


def test_one_home_for_the_raster_helpers_and_the_chunk_size():
    from lasr_amd import vis
    from lasr_amd.nnutils import bake, posed, reproj, tracks
    assert bake.ndc_vertices is posed.ndc_vertices and bake.depth_range is posed.depth_range
    assert bake.face_index_raster is posed.face_index_raster
    assert bake.CHUNK_FRAMES == tracks.CHUNK_FRAMES == reproj.CHUNK_FRAMES == posed.CHUNK_FRAMES == vis.CHUNK_FRAMES
    assert not hasattr(tracks, 'bake') and not hasattr(reproj, 'bake')          # neither imports the texture baker to rasterise
    # the helpers' arithmetic needs no device: NDC of the pixel (u, v) = (IS/2, IS/4) is (0, 0.5), row 0 at the top
    v = torch.tensor([[[0., 0., 2.], [1., -1., 4.]]])
    K = torch.tensor([[8., 8., 4., 2.]])
    ndc = posed.ndc_vertices(v, K, 8)
    assert np.allclose(ndc.numpy(), [[[0., 0.5, 2.], [0.5, 1., 4.]]])
    assert posed.depth_range(v) == (1., 8.)
    with pytest.raises(ValueError, match=r'^bake_texture: every vertex must lie in front of the camera \(depths span -1 \.\. 4\)'):
        posed.depth_range(torch.tensor([[[0., 0., -1.], [0., 0., 4.]]]))
