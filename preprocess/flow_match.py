"""Large-displacement matching for the variational optical flow: small fast parts (--vf_match of auto_gen.py, propagate_mask.py and
auto_mask.py).

The flow of lasr_amd/nnutils/varflow.py is coarse to fine on a factor-2 pyramid, so a structure that is smaller than its own motion
(a leg, a head, a tail) vanishes at the levels coarse enough to see the motion and is not recovered below: there the flow follows
the background.  Here, at one pyramid level, an integer block-matching stage (SAD over 8-bit pixels, radius R = --vf_match) finds a
displacement per pixel in both directions; the matches that are forward-backward consistent, explain the images clearly better
than the upsampled flow (256 c1 < K ccur) and differ from it by more than a pixel replace it there, spread to their neighbours
under the same cost test, and the level's unchanged warps refine them (the "extended coarse-to-fine" idea of Xu, Jia & Matsushita
2012, reduced to a greedy per-pixel choice).  Four kernels (include/lasr_ops.h, lasr_amd/csrc/flowmatch.hip): lasr_flowmatch_quantise,
lasr_flowmatch_search (the hot path), lasr_flowmatch_select and lasr_flowmatch_propagate.  The definition is
tests/flowmatch_restated.py; all of it is integer arithmetic.  r = 2, kappa = 0.9, N = 16 are derived on closed-form fixtures, not
on footage.

Everything takes device tensors and stays on the device; every function launches and never synchronises.  A quantised frame is
[H,W] int32 holding r | g << 8 | b << 16; a displacement field is [H,W,2] int32 = (dx, dy); flow fields are varflow's.
"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from lasr_amd import _lib                      # noqa: E402
from lasr_amd.nnutils import varflow           # noqa: E402

DEFAULTS = dict(patch=2, level=-1, kappa=0.9, prop=16)
MAX_PROP, LEVEL_SIDE = 64, 512


def check(match, patch=2, level=-1, kappa=0.9, prop=16):
    """-> (R, r, L, K, N) as integers, K = rint(256 kappa); refused: R outside 1..32, r outside 1..3, N outside 0..64, L < -1, kappa
    outside (0, 1]."""
    for name, v in (('match', match), ('patch', patch), ('level', level), ('prop', prop)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError('flow_match: %s must be an integer, got %r' % (name, v))
    R, r, L, N = int(match), int(patch), int(level), int(prop)
    if not 1 <= R <= _lib.FLOWMATCH_MAX_R:
        raise ValueError('flow_match: the search radius must be 1..%d, got %d' % (_lib.FLOWMATCH_MAX_R, R))
    if not 1 <= r <= _lib.FLOWMATCH_MAX_PATCH:
        raise ValueError('flow_match: the patch radius must be 1..%d, got %d' % (_lib.FLOWMATCH_MAX_PATCH, r))
    if not 0 <= N <= MAX_PROP:
        raise ValueError('flow_match: the propagation takes 0..%d iterations, got %d' % (MAX_PROP, N))
    if L < -1:
        raise ValueError('flow_match: the level is -1 (chosen by size) or a pyramid level >= 0, got %d' % L)
    k = float(kappa)
    if not (math.isfinite(k) and 0 < k <= 1):
        raise ValueError('flow_match: kappa must be inside (0, 1], got %s' % kappa)
    return R, r, L, int(round(256. * k)), N


def check_terms(gamma, beta):
    """gamma = 0: varflow's flow, beta unused; gamma > 0: robust_flow's, which checks the pair itself.  Refused: a negative or
    non-finite weight."""
    g, b = float(gamma), float(beta)
    if not (math.isfinite(g) and math.isfinite(b) and g >= 0 and b >= 0):
        raise ValueError('flow_match: gamma and beta must be finite and not negative, got %s and %s' % (gamma, beta))
    return g, b


def pick_level(shapes, level=-1):
    """The level the stage runs on: `level` itself, or for -1 the finest of `shapes` (varflow.level_shapes, finest first) whose
    longer side is <= 512, the coarsest when none is."""
    if level >= 0:
        if level >= len(shapes):
            raise ValueError('flow_match: level %d of a pyramid of %d levels' % (level, len(shapes)))
        return int(level)
    for i, (h, w) in enumerate(shapes):
        if max(h, w) <= LEVEL_SIDE:
            return i
    return len(shapes) - 1


def _field(t, shape, dtype, name):
    if not torch.is_tensor(t):
        raise TypeError('flow_match: %s must be a tensor' % name)
    _lib.need_cuda(t)
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype:
        raise ValueError('flow_match: %s must be %s %s, got %s %s' % (name, dtype, tuple(shape), t.dtype, tuple(t.shape)))
    return t.detach().contiguous()


def _frames(qA, qB):
    if not torch.is_tensor(qA):
        raise TypeError('flow_match: qA must be a tensor')
    _lib.need_cuda(qA)
    if qA.ndimension() != 2:
        raise ValueError('flow_match: a quantised frame is [H, W], got %s' % (tuple(qA.shape),))
    H, W = int(qA.shape[0]), int(qA.shape[1])
    varflow._sides(H, W, 'qA')
    return _field(qA, (H, W), torch.int32, 'qA'), _field(qB, (H, W), torch.int32, 'qB'), H, W


def quantise(level):
    """uint8 [H,W,3] (the frame itself) or fp32 [H,W,3] (a pyramid level: clip(rint(255 I), 0, 255)) -> [H,W] int32 words."""
    if not torch.is_tensor(level):
        raise TypeError('flow_match: level must be a tensor')
    _lib.need_cuda(level)
    if level.ndimension() != 3 or level.shape[2] != 3 or level.dtype not in (torch.uint8, torch.float32):
        raise ValueError('flow_match: level must be uint8 or float32 [H, W, 3], got %s %s' % (level.dtype, tuple(level.shape)))
    H, W = int(level.shape[0]), int(level.shape[1])
    varflow._sides(H, W, 'level')
    level = level.detach().contiguous()
    out = torch.empty(H, W, dtype=torch.int32, device=level.device)
    if level.dtype == torch.uint8:
        _lib.call('lasr_flowmatch_quantise', level, None, out, H, W)
    else:
        _lib.call('lasr_flowmatch_quantise', None, level, out, H, W)
    return out


def search(qA, qB, match, patch=2):
    """-> (d [H,W,2] int32, c1 [H,W] int32): per pixel the displacement of least cost within the radius, and that cost."""
    R, r, _, _, _ = check(match, patch)
    qA, qB, H, W = _frames(qA, qB)
    d = torch.empty(H, W, 2, dtype=torch.int32, device=qA.device)
    c1 = torch.empty(H, W, dtype=torch.int32, device=qA.device)
    _lib.call('lasr_flowmatch_search', qA, qB, d, c1, H, W, R, r)
    return d, c1


def select(qA, qB, d_ab, c1, d_ba, uv, match, patch=2, kappa=0.9):
    """uv [2,H,W], the flow handed to the level -> (seeded [H,W] uint8, cand [H,W,2] int32, ccur [H,W] int32)."""
    R, r, _, K, _ = check(match, patch, -1, kappa)
    qA, qB, H, W = _frames(qA, qB)
    d_ab, d_ba = _field(d_ab, (H, W, 2), torch.int32, 'd_ab'), _field(d_ba, (H, W, 2), torch.int32, 'd_ba')
    c1 = _field(c1, (H, W), torch.int32, 'c1')
    uv = varflow._f32(uv, (2, H, W), 'uv')
    seeded = torch.empty(H, W, dtype=torch.uint8, device=qA.device)
    cand = torch.empty(H, W, 2, dtype=torch.int32, device=qA.device)
    ccur = torch.empty(H, W, dtype=torch.int32, device=qA.device)
    _lib.call('lasr_flowmatch_select', qA, qB, d_ab, c1, d_ba, uv, seeded, cand, ccur, H, W, R, r, K)
    return seeded, cand, ccur


def propagate(qA, qB, seeded, cand, ccur, patch=2, kappa=0.9, iters=1):
    """`iters` Jacobi iterations, each from one pair of buffers to another -> (seeded, cand); the inputs are left as they are."""
    _, r, _, K, N = check(1, patch, -1, kappa, iters)
    qA, qB, H, W = _frames(qA, qB)
    seeded, cand = _field(seeded, (H, W), torch.uint8, 'seeded'), _field(cand, (H, W, 2), torch.int32, 'cand')
    ccur = _field(ccur, (H, W), torch.int32, 'ccur')
    bufs = []                                                                      # (the caller's buffers are never written)
    for k in range(N):
        if len(bufs) < 2:
            bufs.append((torch.empty_like(seeded), torch.empty_like(cand)))
        s_out, c_out = bufs[k % 2]
        _lib.call('lasr_flowmatch_propagate', qA, qB, seeded, cand, ccur, s_out, c_out, H, W, r, K)
        seeded, cand = s_out, c_out
    return seeded, cand


def fuse(qA, qB, d_ab, c1, d_ba, uv, match, patch=2, kappa=0.9, prop=16):
    """Select, propagate and apply on the flow uv [2,H,W] handed to the level -> uv: the matched displacement on seeded pixels,
    every other value as it came."""
    seeded, cand, ccur = select(qA, qB, d_ab, c1, d_ba, uv, match, patch, kappa)
    seeded, cand = propagate(qA, qB, seeded, cand, ccur, patch, kappa, prop)
    return torch.where(seeded.bool()[None], cand.permute(2, 0, 1).float().contiguous(), uv).contiguous()


def matches(imgA, imgB, match, patch=2, level=-1):
    """uint8 [H,W,3] x 2 -> (L, qA, qB, (d_ab, c_ab), (d_ba, c_ba)): the level of the stage, its quantised frames and the two
    searches of the frame pair."""
    R, r, L, _, _ = check(match, patch, level)
    if not (torch.is_tensor(imgA) and torch.is_tensor(imgB)):
        raise TypeError('flow_match: imgA and imgB must be tensors')
    _lib.need_cuda(imgA, imgB)
    if tuple(imgA.shape) != tuple(imgB.shape) or imgA.ndimension() != 3 or imgA.dtype != torch.uint8 or imgB.dtype != torch.uint8:
        raise ValueError('flow_match: two uint8 [H, W, 3] frames of one size, got %s %s and %s %s'
                         % (imgA.dtype, tuple(imgA.shape), imgB.dtype, tuple(imgB.shape)))
    varflow._sides(int(imgA.shape[0]), int(imgA.shape[1]), 'img')
    L = pick_level(varflow.level_shapes(int(imgA.shape[0]), int(imgA.shape[1])), L)
    if L == 0:
        qA, qB = quantise(imgA), quantise(imgB)
    else:
        qA, qB = quantise(varflow.pyramid(imgA)[L]), quantise(varflow.pyramid(imgB)[L])
    return L, qA, qB, search(qA, qB, R, r), search(qB, qA, R, r)


def _split(tuning):
    mine = dict(DEFAULTS)
    mine.update({k: tuning[k] for k in DEFAULTS if k in tuning})
    return mine, {k: v for k, v in tuning.items() if k not in DEFAULTS}


def flow_pair(imgA, imgB, match, gamma=0., beta=1., **tuning):
    """-> (f_ab, occ_ab, f_ba, occ_ba) as varflow.flow_pair: both directions share the two searches.  gamma > 0: the flow is
    robust_flow's (brightness and gradient constancy).  tuning: patch, level, kappa, prop and varflow's parameters."""
    mine, over = _split(tuning)
    check(match, **mine)
    gamma, beta = check_terms(gamma, beta)
    varflow.params(**over)
    L, qA, qB, (d_ab, c_ab), (d_ba, c_ba) = matches(imgA, imgB, match, mine['patch'], mine['level'])

    def hook(q1, q2, d12, c12, d21):
        return lambda lev, uv: fuse(q1, q2, d12, c12, d21, uv, match, mine['patch'], mine['kappa'], mine['prop']) if lev == L else uv
    if float(gamma) > 0:
        import robust_flow                                                         # (beside this file)
        f_ab = robust_flow.flow(imgA, imgB, gamma, beta, hook(qA, qB, d_ab, c_ab, d_ba), **over)
        f_ba = robust_flow.flow(imgB, imgA, gamma, beta, hook(qB, qA, d_ba, c_ba, d_ab), **over)
    else:
        f_ab = varflow.flow(imgA, imgB, hook(qA, qB, d_ab, c_ab, d_ba), **over)
        f_ba = varflow.flow(imgB, imgA, hook(qB, qA, d_ba, c_ba, d_ab), **over)
    return f_ab, varflow.occlusion(f_ab, f_ba), f_ba, varflow.occlusion(f_ba, f_ab)


def make_flow_fn(device='cuda', match=24, gamma=0., beta=1., **tuning):
    """-> flow_fn(imgA, imgB) of varflow.make_flow_fn (numpy in, numpy out, the reverse call of a pair served from a cache,
    flow_fn.stats), on this module's flow_pair."""
    mine, over = _split(tuning)
    check(match, **mine)
    check_terms(gamma, beta)
    return varflow.make_flow_fn(device, pair=lambda a, b, **t: flow_pair(a, b, match, gamma, beta, **dict(mine, **t)), **over)
