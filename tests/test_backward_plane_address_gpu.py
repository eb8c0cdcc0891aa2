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
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from lasr_amd import _lib, synth
from test_face_constants_gpu import mesh

GRAD_REL = 1e-3         # tests/test_raster_parity_gpu.py
NEAR, FAR = 1.0, 5.0
SIGMA = 1e-4
N_MAX = 3
POISON = 1e6            # what lies between the carved tensors
LASR = 'lasr'
GENERIC = 'alpha_sum'


@functools.lru_cache(maxsize=None)
def frames(IS):
    fv = mesh(IS)
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


_refs = {}


def reference(oracle, IS, C, kind):
    """float64 (grad_faces [3, F, 3, 3], grad_textures [3, F, 3, C]), triple by triple with the alpha gradient counted once
    (tests/test_raster_parity_gpu.py::test_nine_channel_pass_vs_oracle_at_lasr_size); computed once per case and left unchanged."""
    key = (IS, C, kind)
    if key not in _refs:
        dt = np.float64
        fv, ft, g = frames(IS).astype(dt), textures(C).astype(dt), upstream(IS, C).astype(dt)
        kw = modes(kind)
        gf, gts = 0, []
        for k in range(C // 3):
            ref = oracle.forward(fv, np.ascontiguousarray(ft[..., 3 * k:3 * k + 3]), IS, dtype=dt, **kw)
            ga = g[:, C:C + 1] if k == 0 else np.zeros_like(g[:, C:C + 1])
            gf_k, gt_k = oracle.backward(ref, np.ascontiguousarray(np.concatenate([g[:, 3 * k:3 * k + 3], ga], 1)), IS, dtype=dt, **kw)
            gf = gf + gf_k
            gts.append(gt_k)
        gt = np.concatenate(gts, -1)
        gf.setflags(write=False)
        gt.setflags(write=False)
        _refs[key] = (gf, gt)
    return _refs[key]


def carve(dev, shapes):
    """Tensors of `shapes` inside one POISON-filled float buffer: the first starts one float behind the (256-byte aligned) allocation,
    the gaps are odd numbers of floats, so every start is 4-byte aligned and no more."""
    sizes = [int(np.prod(s)) for s in shapes]
    buf = torch.full((sum(sizes) + 8 * len(sizes) + 8,), POISON, device=dev)
    assert buf.data_ptr() % 256 == 0
    out, at = [], 1
    for s, n in zip(shapes, sizes):
        t = buf[at:at + n].view(*s)
        assert t.data_ptr() % 8 == 4 and t.is_contiguous()
        out.append(t)
        at += n + (4 if n % 2 == 0 else 3)                          # the next start stays odd
    return buf, out


def run(dev, IS, N, C, kind):
    h = _lib.lib()
    fv, ft = frames(IS)[:N], textures(C)[:N]
    F = fv.shape[1]
    m = synth.LASR_MODES
    alpha_id = 1 if kind == GENERIC else 2
    tail = (float(m['eps']), float(SIGMA), 2, float(math.log(1. / m['dist_eps'] - 1.)), float(m['gamma_val']), 1, alpha_id, 1, 1)
    tfv = torch.from_numpy(np.array(fv)).to(dev).reshape(N, F, 9).contiguous()
    tft = torch.from_numpy(np.array(ft)).to(dev).reshape(N, F, 3 * C).contiguous()
    colors = torch.full((N, C + 1, IS, IS), 7., device=dev)
    aggrs = torch.empty(N, 2, IS, IS, device=dev)
    ws = torch.zeros(h.lasr_sr_workspace_bytes(N, F, 3, IS), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    bg = (ctypes.c_float * C)(*([1.] * C))
    _lib.check(h.lasr_sr_forward_opt(tfv.data_ptr(), tft.data_ptr(), None, aggrs.data_ptr(), colors.data_ptr(), ws.data_ptr(), ws.numel(),
                                     N, F, 3, C, IS, NEAR, FAR, None, *tail, bg, 0, None, st), 'lasr_sr_forward_opt')
    # the three tensors the backward reads, re-housed at 4-byte aligned starts
    buf, (c_colors, c_aggrs, c_g) = carve(dev, [(N, C + 1, IS, IS), (N, 2, IS, IS), (N, C + 1, IS, IS)])
    c_colors.copy_(colors)
    c_aggrs.copy_(aggrs)
    c_g.copy_(torch.from_numpy(np.array(upstream(IS, C)[:N])).to(dev))
    for t in (c_colors, c_aggrs, c_g):                                # every plane of a tensor is its own
        planes = t.reshape(-1, IS * IS).cpu().numpy()
        assert all(not np.array_equal(planes[i], planes[j]) for i in range(len(planes)) for j in range(i))
    out = []
    for flags in (_lib.SR_RECORDS_VALID, 0):
        gf = torch.zeros(N, F, 9, device=dev)
        gt = torch.zeros(N, F, 3 * C, device=dev)
        _lib.check(h.lasr_sr_backward_ex(tfv.data_ptr(), tft.data_ptr(), c_colors.data_ptr(), c_aggrs.data_ptr(), gf.data_ptr(), gt.data_ptr(),
                                         c_g.data_ptr(), ws.data_ptr(), ws.numel(), N, F, 3, C, IS, NEAR, FAR, None, *tail, flags, st),
                   'lasr_sr_backward_ex')
        out.append((gf.cpu().numpy().reshape(N, F, 3, 3), gt.cpu().numpy().reshape(N, F, 3, C)))
    return out


def check_grad(what, a, b):
    scale = float(np.abs(b).max())
    d = float(np.abs(a - b).max())
    print('%s: max diff %.3e, largest gradient %.3e (%.2e of it)' % (what, d, scale, d / scale))
    assert np.isfinite(a).all() and scale > 0 and d <= GRAD_REL * scale, '%s: max diff %.3e vs largest gradient %.3e' % (what, d, scale)


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
