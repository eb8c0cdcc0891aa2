"""Per-face constants of the raster passes that are prepared once instead of in every wave: the set-up kernel writes the near-tie
margin into record word R_TIE (sr_device.h: build_record), the backward reads it from there, fills the LDS extension of its distance
code from a static lane table and splits its wave index with a host-prepared multiplier (sr_backward.h).  Forward and backward run
through the C ABI and are held against the C oracle at the bars of tests/test_raster_parity_gpu.py (image 1e-4, gradients 1e-3 of the
largest gradient).

Shapes: 2 frames of a 20-face mesh at 32 x 32 and 24 x 24 (no power of two: 16 + 8 pixel tiles), sigma 1e-4 and 1e-5, 3 / 6 / 9
channels.  The forward is forced through the pair walk (one team and two teams per tile: it stages the same record words, and derives
its far thresholds from sigma per staged entry) and also runs with the library's own kernel choice.  The mesh
(tests/test_face_constants_cases.py checks these properties on the CPU):
  face 0      isosceles, its axis 2e-4 NDC beside a pixel column: inside pixels within the near-tie margin of a bisector; it covers the
              image centre, so it reaches all four 16 x 16 tiles and its record is staged four times
  faces 1..3  one face per obtuse corner 0, 1, 2
  face 4      an edge-on sliver (height 0.008 NDC) without record flag 16: tie scale 0, far = -inf, hq = 0, the generic path
  face 5      outside the image: an empty pixel rect
  faces 6..19 small well-conditioned faces
Two comparisons are bit for bit: the backward on the forward's records (LASR_SR_RECORDS_VALID) against the backward that rebuilds
them, and one frame rendered at two values of sigma in succession through ONE workspace against each rendered in a fresh workspace
(nothing a record keeps may depend on an earlier launch's sigma).
"""
import functools

import numpy as np
import pytest

import raster_harness as rh
from lasr_amd import _lib, synth
from raster_harness import check_grad, constants_mesh as mesh               # (tests/test_face_constants_cases.py checks the same mesh)

IMG_TOL = 1e-4          # tests/test_raster_parity_gpu.py
NEAR, FAR = 1.0, 5.0
N_FRAMES, N_FACES = 2, 20
SIZES = (32, 24)
SIGMAS = (1e-4, 1e-5)


@functools.lru_cache(maxsize=None)
def textures(C):
    ft = np.random.default_rng(30 + C).uniform(0.1, 0.9, (N_FRAMES, N_FACES, 3, C)).astype(np.float32)
    ft.setflags(write=False)
    return ft


@functools.lru_cache(maxsize=None)
def upstream(IS, C):
    g = (np.random.default_rng(40 + C).standard_normal((N_FRAMES, C + 1, IS, IS)) / (IS * IS)).astype(np.float32)
    g.setflags(write=False)
    return g


def reference(oracle, IS, sigma, C):
    """(image [N, C + 1, IS, IS], grad_faces, grad_textures [N, F, 3, C]) of the oracle; computed once per case."""
    kw = dict(synth.LASR_MODES, near=NEAR, far=FAR, sigma_val=sigma)
    return rh.cached(('face constants', IS, sigma, C),
                     lambda: rh.oracle_reference(oracle, mesh(IS), textures(C), IS, None, kw, g=upstream(IS, C)))


PAIR_WALK = (-1, -1, -1, -1, 0)           # pair_min_tiles = 0: every launch through the pair-walk kernel


class Launch:
    """Device buffers of one case -- inputs, outputs and ONE workspace kept from call to call -- and the two C-ABI calls."""

    def __init__(self, dev, IS, sigma, C, frames=slice(None)):
        self.fv, self.ft = mesh(IS)[frames], textures(C)[frames]
        self.g = np.ascontiguousarray(upstream(IS, C)[frames])
        self.dev, self.IS, self.C, self.sigma = dev, IS, C, sigma
        self.rec = None

    def fresh_workspace(self):
        self.rec = None

    def forward(self, options=None, flags=0, sigma=None):
        out = {}
        if self.rec is not None:
            out = dict(colors=self.rec.colors.fill_(7.), aggrs=self.rec.aggrs, ws=self.rec.ws)
        self.rec = rh.forward(self.dev, self.fv, self.ft, NEAR, FAR, self.IS, options=options, flags=flags, background=[1.] * self.C, out=out,
                              scalars=rh.tail(self.sigma if sigma is None else sigma), fill=7.)
        return self.rec.colors.cpu().numpy()

    def backward(self, flags):
        N, F = self.fv.shape[:2]
        gf, gt = rh.backward(self.dev, self.rec, self.g, NEAR, FAR, self.IS, flags=flags, scalars=rh.tail(self.sigma))
        return gf.cpu().numpy().reshape(N, F, 3, 3), gt.cpu().numpy().reshape(N, F, 3, self.C)


@pytest.mark.gpu
@pytest.mark.parametrize('C', [3, 6, 9])
@pytest.mark.parametrize('sigma', SIGMAS)
@pytest.mark.parametrize('IS', SIZES)
def test_forward_and_backward_against_the_oracle(oracle, cuda, IS, sigma, C):
    img_ref, gf_ref, gt_ref = reference(oracle, IS, sigma, C)
    L = Launch(cuda, IS, sigma, C)
    for name, options, flags in (('library default', None, 0), ('pair walk, two teams', PAIR_WALK, _lib.SR_PAIR_TWO_TEAMS),
                                 ('pair walk, one team', PAIR_WALK, _lib.SR_PAIR_ONE_TEAM)):
        img = L.forward(options, flags)
        err = float(np.abs(img - img_ref).max())
        print('%s: image max abs %.3e' % (name, err))
        assert np.isfinite(img).all() and err <= IMG_TOL, '%s: image max abs %.3e' % (name, err)
    # the backward on the pair walk's image and records, then rebuilding them: the same bits, and the oracle's gradients
    gf, gt = L.backward(_lib.SR_RECORDS_VALID)
    gf2, gt2 = L.backward(0)
    assert np.array_equal(gf, gf2) and np.array_equal(gt, gt2), 'the backward on the forward\'s records differs from the backward that rebuilds them'
    check_grad('grad_faces', gf, gf_ref)
    check_grad('grad_textures', gt, gt_ref)


@pytest.mark.gpu
@pytest.mark.parametrize('C', [3, 9])
@pytest.mark.parametrize('IS', SIZES)
def test_two_sigmas_through_one_workspace_equal_fresh_workspaces(cuda, IS, C):
    one = Launch(cuda, IS, SIGMAS[0], C, frames=slice(0, 1))
    for flags in (_lib.SR_PAIR_ONE_TEAM, _lib.SR_PAIR_TWO_TEAMS):
        one.fresh_workspace()
        shared = [one.forward(PAIR_WALK, flags, sigma=s).copy() for s in (SIGMAS[0], SIGMAS[1], SIGMAS[0])]
        fresh = []
        for s in SIGMAS:
            one.fresh_workspace()
            fresh.append(one.forward(PAIR_WALK, flags, sigma=s).copy())
        assert not np.array_equal(fresh[0], fresh[1])                                  # sigma shows in the image
        assert np.array_equal(shared[0], fresh[0]) and np.array_equal(shared[1], fresh[1]) and np.array_equal(shared[2], fresh[0])
