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
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from lasr_amd import _lib, synth

IMG_TOL = 1e-4          # tests/test_raster_parity_gpu.py
GRAD_REL = 1e-3
NEAR, FAR = 1.0, 5.0
N_FRAMES, N_FACES = 2, 20
SIZES = (32, 24)
SIGMAS = (1e-4, 1e-5)


def _tri(xy, z):
    return [[x, y, zz] for (x, y), zz in zip(xy, z)]


def _rot(t, k):                                  # the first vertex moves to index k
    return [t[(j - k) % 3] for j in range(3)]


@functools.lru_cache(maxsize=None)
def mesh(IS):
    """face_vertices [2, 20, 3, 3] (the second frame: the first moved a little), float32."""
    ax = 1. / IS + 2e-4                          # 2e-4 beside the pixel-centre column right of the image centre
    obt = [(0.02, 0.17), (-0.6, -0.15), (0.6, -0.1)]            # obtuse at its FIRST vertex
    faces = [_tri([(-0.5 + ax, -0.4), (0.5 + ax, -0.4), (ax, 0.55)], (2.5, 3.0, 3.5))]
    for k in range(3):
        t = _rot(_tri(obt, (2.2, 2.8, 3.1)), k)
        faces.append([[x + 0.1 * (k - 1), y + 0.25 * (k - 1), z + 0.1 * k] for x, y, z in t])
    # the sliver, around a pixel centre: its apex 0.008 NDC over the long edge -- below the 0.01 of flag 16 -- at an aspect of 7
    p = (2 * round(0.8 * IS) + 1 - IS) / IS
    faces.append(_tri([(p - 0.03, p - 0.004), (p + 0.03, p - 0.003), (p + 0.004, p + 0.0045)], (3.2, 3.3, 3.4)))
    faces.append(_tri([(2.0, -0.2), (2.4, -0.1), (2.1, 0.3)], (3.0, 3.0, 3.0)))                # outside the image
    rng = np.random.default_rng(20)
    while len(faces) < N_FACES:
        c = rng.uniform(-0.75, 0.75, 2)
        a0 = rng.uniform(0, 2 * math.pi)
        r = rng.uniform(0.12, 0.25, 3)
        ang = a0 + np.array([0., 2.1, 4.2]) + rng.uniform(-0.3, 0.3, 3)
        if rng.uniform() < 0.5:
            ang = ang[::-1]                                                                        # both windings
        faces.append(_tri([(c[0] + r[j] * math.cos(ang[j]), c[1] + r[j] * math.sin(ang[j])) for j in range(3)], rng.uniform(2., 4., 3)))
    f = np.asarray(faces, np.float32)
    fv = np.stack([f, f])
    fv[1, :, :, 0] += 0.013
    fv[1, :, :, 1] -= 0.007
    fv.setflags(write=False)
    return fv


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


def modes(sigma):
    return dict(synth.LASR_MODES, near=NEAR, far=FAR, sigma_val=sigma)


_refs = {}


def reference(oracle, IS, sigma, C, dtype=np.float32):
    """(image [N, C + 1, IS, IS], grad_faces, grad_textures [N, F, 3, C]) of the oracle, triple by triple (the alpha gradient counted
    once: tests/test_raster_parity_gpu.py::test_nine_channel_pass_vs_oracle_at_lasr_size); computed once per case."""
    key = (IS, sigma, C, np.dtype(dtype).name)
    if key not in _refs:
        fv, ft, g = mesh(IS).astype(dtype), textures(C).astype(dtype), upstream(IS, C).astype(dtype)
        kw = modes(sigma)
        img, gf, gts = [], 0, []
        for k in range(C // 3):
            ref = oracle.forward(fv, np.ascontiguousarray(ft[..., 3 * k:3 * k + 3]), IS, dtype=dtype, **kw)
            img.append(ref['soft_colors'])
            ga = g[:, C:C + 1] if k == 0 else np.zeros_like(g[:, C:C + 1])
            gf_k, gt_k = oracle.backward(ref, np.ascontiguousarray(np.concatenate([g[:, 3 * k:3 * k + 3], ga], 1)), IS, dtype=dtype, **kw)
            gf = gf + gf_k
            gts.append(gt_k)
        _refs[key] = (np.concatenate([p[:, :3] for p in img] + [img[0][:, 3:4]], 1), gf, np.concatenate(gts, -1))
    return _refs[key]


PAIR_WALK = _lib.SrOptions(-1, -1, -1, -1, 0)          # pair_min_tiles = 0: every launch through the pair-walk kernel


class Launch:
    """Device buffers of one case and the two C-ABI calls."""

    def __init__(self, dev, IS, sigma, C, frames=slice(None)):
        self.h = _lib.lib()
        fv, ft = mesh(IS)[frames], textures(C)[frames]
        self.N, self.F, self.IS, self.C = fv.shape[0], fv.shape[1], IS, C
        self.fv = torch.from_numpy(np.ascontiguousarray(fv)).to(dev).reshape(self.N, self.F, 9).contiguous()
        self.ft = torch.from_numpy(np.ascontiguousarray(ft)).to(dev).reshape(self.N, self.F, 3 * C).contiguous()
        self.g = torch.from_numpy(np.ascontiguousarray(upstream(IS, C)[frames])).to(dev)
        self.colors = torch.empty(self.N, C + 1, IS, IS, device=dev)
        self.aggrs = torch.empty(self.N, 2, IS, IS, device=dev)
        self.dev = dev
        self.fresh_workspace()
        m = synth.LASR_MODES
        self.tail = lambda s: (float(m['eps']), float(s), 2, float(math.log(1. / m['dist_eps'] - 1.)), float(m['gamma_val']), 1, 2, 1, 1)
        self.sigma = sigma
        self.bg = (ctypes.c_float * C)(*([1.] * C))
        self.st = torch.cuda.current_stream(dev).cuda_stream

    def fresh_workspace(self):
        self.ws = torch.zeros(self.h.lasr_sr_workspace_bytes(self.N, self.F, 3, self.IS), dtype=torch.uint8, device=self.dev)

    def forward(self, options=None, flags=0, sigma=None):
        self.colors.fill_(7.)
        _lib.check(self.h.lasr_sr_forward_opt(self.fv.data_ptr(), self.ft.data_ptr(), None, self.aggrs.data_ptr(), self.colors.data_ptr(),
                                              self.ws.data_ptr(), self.ws.numel(), self.N, self.F, 3, self.C, self.IS, NEAR, FAR, None,
                                              *self.tail(self.sigma if sigma is None else sigma), self.bg, flags,
                                              ctypes.byref(options) if options is not None else None, self.st), 'lasr_sr_forward_opt')
        return self.colors.cpu().numpy()

    def backward(self, flags):
        gf = torch.zeros(self.N, self.F, 9, device=self.dev)
        gt = torch.zeros(self.N, self.F, 3 * self.C, device=self.dev)
        _lib.check(self.h.lasr_sr_backward_ex(self.fv.data_ptr(), self.ft.data_ptr(), self.colors.data_ptr(), self.aggrs.data_ptr(),
                                              gf.data_ptr(), gt.data_ptr(), self.g.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                              self.N, self.F, 3, self.C, self.IS, NEAR, FAR, None, *self.tail(self.sigma), flags, self.st),
                   'lasr_sr_backward_ex')
        return gf.cpu().numpy().reshape(self.N, self.F, 3, 3), gt.cpu().numpy().reshape(self.N, self.F, 3, self.C)


def check_grad(what, a, b):
    scale = float(np.abs(b).max())
    d = float(np.abs(a - b).max())
    print('%s: max diff %.3e, largest gradient %.3e (%.2e of it)' % (what, d, scale, d / scale))
    assert np.isfinite(a).all() and scale > 0 and d <= GRAD_REL * scale, '%s: max diff %.3e vs largest gradient %.3e' % (what, d, scale)


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
