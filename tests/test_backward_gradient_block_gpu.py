"""The gradient block of the LASR-mode backward (sr_backward.h, vertex-attribute path of sr_backward_kernel<true, NCH>) after its
products were regrouped: sm g[k] formed once per channel, the depth normalisation as one multiply-add on launch-uniform factors, the
softmax exponent as one product that carries v_exp_f32's log2(e), 1 / (gamma (near - far)) as one factor of d/dz, k2 dx and k2 dy
formed once.  Same bar as before: 1e-3 of the largest gradient of the float64 oracle.

One 64 x 64 frame of a 20-face icosahedron (ten faces towards the camera, ten away from it, all drawn: LASR renders double-sided)
plus a reversed duplicate of one front face; three, six and nine channels; the gradients stored (LASR_SR_GRADS_OVERWRITE, into
buffers full of NaN) and accumulated (into zeroed buffers); the face records reused from the forward (LASR_SR_RECORDS_VALID) and
rebuilt by the backward's own set-up launch.  Also: near / far within 5e-5 relative of the mesh's nearest / farthest vertex depth, so
that the per-face `every vertex strictly inside (near, far)` shortcut must be off for the faces at those vertices and the
per-fragment depth test runs; and near / far read on the device.
"""
import itertools

import numpy as np
import pytest
import torch

import raster_harness as rh
from lasr_amd import _lib, synth
from lasr_amd.soft_renderer import functional as srf
from raster_harness import check_grad

pytestmark = pytest.mark.gpu

IS = 64
NEAR, FAR = 1.0, 5.0


def icosahedron():
    """[21, 3, 3] float32: the 20 faces, outward winding, turned a little so that no edge is axis-aligned, and face 0 once more with
    its winding reversed."""
    p = (1 + 5 ** 0.5) / 2
    v = np.array([s for a, b in itertools.product((-1, 1), (-p, p)) for s in ((0, a, b), (a, b, 0), (b, 0, a))], np.float64)
    tri = [t for t in itertools.combinations(range(12), 3)
           if all(abs(np.linalg.norm(v[i] - v[j]) - 2) < 1e-9 for i, j in itertools.combinations(t, 2))]
    assert len(tri) == 20
    ax, ay = 0.37, 0.23
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    v = v @ (Rx @ Ry).T / np.linalg.norm(v[0])               # unit sphere
    faces = []
    for t in tri:
        a, b, c = v[list(t)]
        if np.dot(np.cross(b - a, c - a), a + b + c) < 0:
            b, c = c, b
        faces.append([a, b, c])
    f = np.asarray(faces)
    f = f * np.array([0.7, 0.7, 0.8]) + np.array([0.03, -0.02, 3.0])
    e1, e2 = f[:, 1, :2] - f[:, 0, :2], f[:, 2, :2] - f[:, 0, :2]
    front = [i for i in range(20) if e1[i, 0] * e2[i, 1] - e1[i, 1] * e2[i, 0] > 0]
    assert len(front) == 10
    dup = f[front[0]][[0, 2, 1]]
    return np.concatenate([f, dup[None]]).astype(np.float32)


def inputs(nch):
    fv = icosahedron()[None]
    ft = np.random.default_rng(31).uniform(0.05, 0.95, (1, fv.shape[1], 3, nch)).astype(np.float32)
    g = np.random.default_rng(32).standard_normal((1, nch + 1, IS, IS)).astype(np.float32)
    return fv, ft, g


def reference(nch, near, far):
    """(grad_faces, grad_textures) of the float64 oracle; computed once per case."""
    from oracle import sr_oracle
    fv, ft, g = inputs(nch)
    return rh.cached(('gradient block', nch, near, far),
                     lambda: rh.oracle_reference(sr_oracle, fv, ft, IS, None, dict(synth.LASR_MODES, near=near, far=far), g=g, dtype=np.float64)[1:])


def forward(dev, nch, near, far):
    fv, ft, g = inputs(nch)
    tfv = torch.from_numpy(fv).to(dev).requires_grad_(True)
    tft = torch.from_numpy(ft).to(dev).requires_grad_(True)
    img = srf.soft_rasterize(tfv, tft, IS, **dict(synth.LASR_MODES, near=near, far=far, background_color=[1.] * nch))
    return tfv, tft, img, torch.from_numpy(g).to(dev)


@pytest.mark.parametrize('reuse', [True, False], ids=['records reused', 'records rebuilt'])
@pytest.mark.parametrize('overwrite', [True, False], ids=['stored', 'accumulated'])
@pytest.mark.parametrize('nch', [3, 6, 9])
def test_gradients_with_every_flag_combination(cuda, nch, overwrite, reuse):
    tfv, tft, img, g = forward(cuda, nch, NEAR, FAR)
    ctx = img.grad_fn
    fv, tx, soft_colors, aggrs_info = ctx.saved_tensors
    N, F, T, size = ctx.geom
    assert (N, F, T, size) == (1, 21, 3, IS)
    fill = float('nan') if overwrite else 0.
    grad_faces = torch.full((N, F, 9), fill, dtype=torch.float32, device=cuda)
    grad_textures = torch.full(tuple(tx.shape), fill, dtype=torch.float32, device=cuda)
    flags = (_lib.SR_GRADS_OVERWRITE if overwrite else 0) | (_lib.SR_RECORDS_VALID if reuse else 0)
    assert ctx.nf is None and ctx.C == nch
    rh.backward(cuda, rh.record(fv, tx, soft_colors, aggrs_info, rh.operator_workspace(cuda)), g, *ctx.near_far, IS, flags=flags,
                into=(grad_faces, grad_textures), scalars=ctx.tail)
    srf.invalidate_records(cuda)                 # (a direct call wrote into the operator's workspace)
    gf_ref, gt_ref = reference(nch, NEAR, FAR)
    check_grad('grad_faces', grad_faces.cpu().numpy().reshape(gf_ref.shape), gf_ref)
    check_grad('grad_textures', grad_textures.cpu().numpy().reshape(gt_ref.shape), gt_ref)


def _tight_planes():
    z = icosahedron()[:, :, 2].astype(np.float64)
    return float(np.float32(z.min() * (1 - 5e-5))), float(np.float32(z.max() * (1 + 5e-5)))


@pytest.mark.parametrize('nch', [3, 6, 9])
def test_vertex_depths_next_to_the_planes(cuda, nch):
    # the nearest vertex 5e-5 (relative) behind near, the farthest 5e-5 before far: no fragment is culled (a clipped, normalised
    # interpolation stays within the vertex depths up to 1e-7), but the faces at those vertices must not take the per-face shortcut
    near, far = _tight_planes()
    z = icosahedron()[:, :, 2]
    assert z.min() * (1 - 1e-4) <= near < z.min() and z.max() < far <= z.max() * (1 + 1e-4)
    tfv, tft, img, g = forward(cuda, nch, near, far)
    img.backward(g)
    gf_ref, gt_ref = reference(nch, near, far)
    check_grad('grad_faces', tfv.grad.cpu().numpy(), gf_ref)
    check_grad('grad_textures', tft.grad.cpu().numpy(), gt_ref)


@pytest.mark.parametrize('planes', ['wide', 'tight'])
@pytest.mark.parametrize('nch', [3, 6, 9])
def test_near_far_read_on_the_device(cuda, nch, planes):
    near, far = (NEAR, FAR) if planes == 'wide' else _tight_planes()
    nf = torch.tensor([near, far], dtype=torch.float32, device=cuda)
    tfv, tft, img, g = forward(cuda, nch, nf[0], nf[1])
    img.backward(g)
    gf_ref, gt_ref = reference(nch, near, far)
    check_grad('grad_faces', tfv.grad.cpu().numpy(), gf_ref)
    check_grad('grad_textures', tft.grad.cpu().numpy(), gt_ref)
