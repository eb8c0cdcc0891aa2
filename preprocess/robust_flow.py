"""The variational optical flow with a gradient-constancy term, for footage whose lighting changes (--vf_gamma of auto_gen.py,
propagate_mask.py and auto_mask.py).

lasr_amd/nnutils/varflow.py keeps the brightness along the flow and nothing else, so an exposure step, a vignette or a cast shadow
is read as motion.  Here the data term also keeps the image gradient (Brox et al. 2004), which an additive change of the lighting
leaves untouched, and each of the two terms has its own robust penalty (Bruhn & Weickert 2005):
    E = beta psi(|I2(p + w) - I1(p)|^2) + gamma psi(|grad I2(p + w) - grad I1(p)|^2) + alpha psi(|grad u|^2 + |grad v|^2).
Three kernels are new (include/lasr_ops.h, lasr_amd/csrc/robustflow.hip): a level's derivative record, written once per level and
frame (lasr_rflow_derivs), the two motion tensors of a warp (lasr_rflow_tensor) and the lagged weights with the combined tensor the
solver sees (lasr_rflow_weights).  Pyramid, expansion, solver and consistency map are varflow's, unchanged.  The definition is
tests/robustflow_restated.py.  gamma = 5, beta = 1 are derived on closed-form fixtures, not on footage.

Everything takes device tensors and stays on the device; flow() launches and never synchronises.  Layouts are varflow's.
"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from lasr_amd import _lib                      # noqa: E402
from lasr_amd.nnutils import varflow           # noqa: E402

GAMMA, BETA = 5., 1.


def check_terms(gamma, beta):
    """-> (gamma, beta) as floats: both finite and >= 0, not both 0."""
    g, b = float(gamma), float(beta)
    if not (math.isfinite(g) and math.isfinite(b) and g >= 0 and b >= 0 and (g > 0 or b > 0)):
        raise ValueError('robust_flow: gamma and beta must be finite, not negative and not both 0, got %s and %s' % (gamma, beta))
    return g, b


def derivs(level):
    """A level fp32 [H,W,3] -> its derivative record [H,W,3,6]: per channel (I, Ix, Iy, Ixx, Ixy, Iyy)."""
    if not torch.is_tensor(level):
        raise TypeError('robust_flow: level must be a tensor')
    _lib.need_cuda(level)
    if level.ndimension() != 3 or level.shape[2] != 3 or level.dtype != torch.float32:
        raise ValueError('robust_flow: level must be float32 [H, W, 3], got %s %s' % (level.dtype, tuple(level.shape)))
    H, W = int(level.shape[0]), int(level.shape[1])
    varflow._sides(H, W, 'level')
    rec = torch.empty(H, W, 3, _lib.RFLOW_RECORD // 3, dtype=torch.float32, device=level.device)
    _lib.call('lasr_rflow_derivs', level.detach().contiguous(), rec, H, W)
    return rec


def tensor(R1, R2, uv):
    """The records of I1 and I2 [H,W,3,6], uv [2,H,W] -> (Jb, Jg), each [6,H,W], zero where p + uv(p) leaves the frame."""
    uv = varflow._planar(uv, 'uv')
    H, W = int(uv.shape[1]), int(uv.shape[2])
    shape = (H, W, 3, _lib.RFLOW_RECORD // 3)
    R1, R2 = varflow._f32(R1, shape, 'R1'), varflow._f32(R2, shape, 'R2')
    Jb = torch.empty(6, H, W, dtype=torch.float32, device=uv.device)
    Jg = torch.empty(6, H, W, dtype=torch.float32, device=uv.device)
    _lib.call('lasr_rflow_tensor', R1, R2, uv, Jb, Jg, H, W)
    return Jb, Jg


def weights(Jb, Jg, uv, d, eps=1e-3, beta=BETA, gamma=GAMMA):
    """-> (J [6,H,W] = (beta psi_b) Jb + (gamma psi_g) Jg, psi [2,H,W] = (1, psi_s)) of the increment d around uv: what varflow.sor takes."""
    gamma, beta = check_terms(gamma, beta)
    if not float(eps) > 0:
        raise ValueError('robust_flow: eps must be positive, got %s' % eps)
    uv = varflow._planar(uv, 'uv')
    H, W = int(uv.shape[1]), int(uv.shape[2])
    Jb, Jg, d = varflow._f32(Jb, (6, H, W), 'Jb'), varflow._f32(Jg, (6, H, W), 'Jg'), varflow._f32(d, (2, H, W), 'd')
    J = torch.empty(6, H, W, dtype=torch.float32, device=uv.device)
    psi = torch.empty(2, H, W, dtype=torch.float32, device=uv.device)
    _lib.call('lasr_rflow_weights', Jb, Jg, uv, d, J, psi, H, W, float(eps), beta, gamma)
    return J, psi


def flow_planar(imgA, imgB, gamma=GAMMA, beta=BETA, init=None, **over):
    """uint8 [H,W,3] x 2 -> uv [2,H,W]: the whole estimate A -> B.  Launches only: no host synchronisation.  init(level, uv) -> uv
    is varflow.flow_planar's."""
    p = varflow.params(**over)
    gamma, beta = check_terms(gamma, beta)
    if not (torch.is_tensor(imgA) and torch.is_tensor(imgB)):
        raise TypeError('robust_flow: imgA and imgB must be tensors')
    _lib.need_cuda(imgA, imgB)
    if tuple(imgA.shape) != tuple(imgB.shape):
        raise ValueError('robust_flow: the two frames differ in size: %s and %s' % (tuple(imgA.shape), tuple(imgB.shape)))
    A, B = varflow.pyramid(imgA), varflow.pyramid(imgB)
    uv = None
    for lev in range(len(A) - 1, -1, -1):
        R1, R2 = derivs(A[lev]), derivs(B[lev])                           # once per level: the warps below share them
        h, w = int(R1.shape[0]), int(R1.shape[1])
        uv = torch.zeros(2, h, w, dtype=torch.float32, device=R1.device) if uv is None else varflow.expand(uv, h, w)
        if init is not None:
            uv = init(lev, uv)
        d, scratch = torch.empty_like(uv), torch.empty_like(uv)
        for _ in range(int(p['NW'])):
            Jb, Jg = tensor(R1, R2, uv)
            d.zero_()
            for _ in range(int(p['NO'])):
                J, psi = weights(Jb, Jg, uv, d, p['eps'], beta, gamma)
                varflow.sor(J, psi, uv, d, p['alpha'], p['omega'], p['NI'], scratch)
            uv = uv + d
    return uv


def flow(imgA, imgB, gamma=GAMMA, beta=BETA, init=None, **over):
    """uint8 [H,W,3] x 2 on the device -> flow A -> B, fp32 [H,W,2] in pixels."""
    return flow_planar(imgA, imgB, gamma, beta, init, **over).permute(1, 2, 0).contiguous()


def flow_pair(imgA, imgB, gamma=GAMMA, beta=BETA, **over):
    """-> (f_ab, occ_ab, f_ba, occ_ba): both directions and their consistency maps (varflow.occlusion)."""
    f_ab, f_ba = flow(imgA, imgB, gamma, beta, **over), flow(imgB, imgA, gamma, beta, **over)
    return f_ab, varflow.occlusion(f_ab, f_ba), f_ba, varflow.occlusion(f_ba, f_ab)


def make_flow_fn(device='cuda', gamma=GAMMA, beta=BETA, **tuning):
    """-> flow_fn(imgA, imgB) of varflow.make_flow_fn (numpy in, numpy out, the reverse call of a pair served from a cache,
    flow_fn.stats), on this module's flow_pair."""
    gamma, beta = check_terms(gamma, beta)
    return varflow.make_flow_fn(device, pair=lambda a, b, **t: flow_pair(a, b, gamma, beta, **t), **tuning)
