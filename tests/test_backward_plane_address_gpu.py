"""The backward raster reads the pixel planes of an image -- the upstream gradient's and the rendered image's C + 1 planes, the two
aggregate planes -- through one wave-uniform base pointer per (image, tensor) and a 32-bit per-lane byte offset that is stepped by the
plane stride (sr_backward.h: plane_base, ld_plane).
A swapped, shifted or mis-strided base reads another plane, another image or another pixel, so the check is the gradients themselves,
against the C oracle run in float64 at the bar of tests/test_raster_parity_gpu.py (1e-3 of the largest gradient).

Shapes: the 20-face mesh of tests/test_face_constants_gpu.py with a third, shifted frame; image sides 8 (a face's pixel
rect is a fraction of a wave), 24 (no power of two: 16 + 8 pixel tiles) and 64; N = 1 and N = 3 (the last image's bases are the
farthest from the tensor's start); 3, 6 and 9 channels in LASR's modes and three channels with aggr_func_alpha = 'sum', which takes the generic
instantiation.  The reference is computed once per (side, channels, modes) for three frames; one frame is its first (images do not
interact).  In every case
  * the three plane tensors the backward reads are carved out of ONE buffer at starts that are 4-byte aligned and no more
    (odd float offsets from a 256-byte aligned allocation), next to planes filled with a large constant that a shifted base would read;
  * all planes of a tensor differ from each other (asserted), so exchanging two bases moves the gradients;
  * the backward on the forward's records (LASR_SR_RECORDS_VALID) and the backward that rebuilds them agree bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

import raster_harness as rh
from lasr_amd import _lib, synth
from raster_harness import check_grad

NEAR, FAR = 1.0, 5.0
SIGMA = 1e-4
N_MAX = 3
POISON = 1e6            # what lies between the carved tensors
LASR = 'lasr'
GENERIC = 'alpha_sum'


@functools.lru_cache(maxsize=None)
def frames(IS):
    fv = rh.constants_mesh(IS)
    third = fv[:1].copy()
    third[..., 0] -= 0.021
    third[..., 1] += 0.017
    out = np.concatenate([fv, third])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def textures(C):
    ft = np.random.default_rng(130 + C).uniform(0.1, 0.9, (N_MAX, frames(8).shape[1], 3, C)).astype(np.float32)
    ft.setflags(write=False)
    return ft


@functools.lru_cache(maxsize=None)
def upstream(IS, C):
    g = (np.random.default_rng(140 + C).standard_normal((N_MAX, C + 1, IS, IS)) / (IS * IS)).astype(np.float32)
    g.setflags(write=False)
    return g


def modes(kind):
    kw = dict(synth.LASR_MODES, near=NEAR, far=FAR, sigma_val=SIGMA)
    if kind == GENERIC:
        kw['aggr_func_alpha'] = 'sum'
    return kw


def reference(oracle, IS, C, kind):
    """float64 (grad_faces [3, F, 3, 3], grad_textures [3, F, 3, C]); computed once per case and left unchanged."""
    return rh.cached(('plane address', IS, C, kind),
                     lambda: rh.oracle_reference(oracle, frames(IS), textures(C), IS, None, modes(kind), g=upstream(IS, C), dtype=np.float64)[1:])


def run(dev, IS, N, C, kind):
    fv, ft = frames(IS)[:N], textures(C)[:N]
    F = fv.shape[1]
    tail = rh.tail(SIGMA, 'sum' if kind == GENERIC else 'prod')
    rec = rh.forward(dev, fv, ft, NEAR, FAR, IS, background=[1.] * C, scalars=tail, fill=7.)
    # the three tensors the backward reads, re-housed at 4-byte aligned starts
    buf, (c_colors, c_aggrs, c_g) = rh.carve_odd(dev, [(N, C + 1, IS, IS), (N, 2, IS, IS), (N, C + 1, IS, IS)], POISON)
    c_colors.copy_(rec.colors)
    c_aggrs.copy_(rec.aggrs)
    c_g.copy_(torch.from_numpy(np.array(upstream(IS, C)[:N])).to(dev))
    for t in (c_colors, c_aggrs, c_g):                                # every plane of a tensor is its own
        planes = t.reshape(-1, IS * IS).cpu().numpy()
        assert all(not np.array_equal(planes[i], planes[j]) for i in range(len(planes)) for j in range(i))
    out = []
    for flags in (_lib.SR_RECORDS_VALID, 0):
        gf, gt = rh.backward(dev, rec, c_g, NEAR, FAR, IS, flags=flags, colors=c_colors, aggrs=c_aggrs, scalars=tail)
        out.append((gf.cpu().numpy().reshape(N, F, 3, 3), gt.cpu().numpy().reshape(N, F, 3, C)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('C,kind', [(3, LASR), (6, LASR), (9, LASR), (3, GENERIC)])
@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('IS', [8, 24, 64])
def test_backward_through_scalar_plane_bases_against_the_float64_oracle(oracle, cuda, IS, N, C, kind):
    gf_ref, gt_ref = reference(oracle, IS, C, kind)
    (gf, gt), (gf2, gt2) = run(cuda, IS, N, C, kind)
    assert np.array_equal(gf, gf2) and np.array_equal(gt, gt2), 'the backward on the forward\'s records differs from the backward that rebuilds them'
    for n in range(N):                                                # every image has gradients of its own to get wrong
        assert np.abs(gf_ref[n]).max() > 0 and np.abs(gt_ref[n]).max() > 0
    check_grad('grad_faces', gf, gf_ref[:N])
    check_grad('grad_textures', gt, gt_ref[:N])
