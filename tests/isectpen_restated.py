"""Restatement of the intersection penalty of the optimiser (optimize.py --isect_wt; include/lasr_ops.h)
in torch on the CPU, for float64 and float32, and what tests/test_isectpen_cpu.py and tests/test_isectpen_gpu.py share.  Nothing here
imports the package: the kernels of lasr_amd/csrc/isectpen.hip and scripts/isect_penalty.py are compared against this file, not the
other way round.  The pairs are those of tests/meshcheck_restated.py, the value of a directed test is that of
tests/foldpen_restated.py; nothing is new except the set of pairs and the accumulation.

This file is the definition.  x [N,V,3] are the posed meshes of a step, faces [F,3] one topology.

Pairs: faces i < j that share no vertex index and whose closed float32 boxes overlap are candidates (meshcheck_restated.candidates).
A candidate is put to the six directed edge-against-triangle tests in this order: the edges (0,1), (1,2), (2,0) of i against j in
stored order, then those of j against i; orient and PIERCES strict and without contraction.  The pair INTERSECTS, and is counted in
n_pairs, when any test holds.  A face with an index outside [0, V) or with a repeated index takes part in nothing.

Value: for a test that holds, with edge (p, q), triangle (a, b, c) and n = (b - a) x (c - a), foldpen_restated._directed:
delta = min(|orient(a,b,c,p)|, |orient(a,b,c,q)|) / |n|; its gradient goes to the shallower end r (p on a tie), sign(orient(a,b,c,r))
n / |n|, and to a, b, c: minus that times the barycentric weights of r's foot, l_a = (1 - l_b) - l_c.  The value of a pair is the
sum over its tests that hold.  It is linear in the depth, so that a descent step carries the end across the plane.

Accumulation, in fixed point with Q = 2^40: every contribution c of a test (its depth, and each of the twelve coordinates of its
four vertex contributions), a number of the working precision, is added as llrint(double(c) Q) to an int64 accumulator: acc_loss
[N], acc_grad [N,V,3].  A test whose |n|^2 is 0 or not finite, or that has any contribution that is not finite or of magnitude
>= 2^20, is dropped as a whole and counted in n_dropped.  Integer sums commute: the result does not depend on the order of the
pairs.  loss = float32(double(acc_loss) 2^-40), gunit = float32(double(acc_grad) 2^-40): the gradient of loss[n] by x[n].  Each
rounding is at most 2^-41; an accumulator wraps beyond a sum of 2^23, which is not checked.
"""
import numpy as np
import torch

import foldpen_restated as fr
import meshcheck_restated as mr

Q = 2. ** 40
LIMIT = 2. ** 20
DT = fr.DT
# (edge end p, edge end q) of the edge's own face, by test; tests 0-2: face i against j, 3-5: j against i
TESTS = tuple((side, e0, e1) for side in (0, 1) for e0, e1 in mr.EDGES)


def _directed_variant(p, q, T):
    """foldpen_restated._directed in another order of operations of the same definition: the unit normal by a reciprocal, the foot's
    weights over |n| twice instead of |n|^2 once, l_a = 1 - (l_b + l_c)."""
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    dp, dq = fr._orient(a, b, c, p), fr._orient(a, b, c, q)
    s0, s1, s2 = fr._orient(p, q, a, b), fr._orient(p, q, b, c), fr._orient(p, q, c, a)
    holds = (((dp > 0) & (dq < 0)) | ((dp < 0) & (dq > 0))) & (((s0 > 0) & (s1 > 0) & (s2 > 0)) | ((s0 < 0) & (s1 < 0) & (s2 < 0)))
    n = fr._cross(b - a, c - a)
    n2 = torch.where(holds, fr._dot(n, n), torch.ones_like(dp))
    rt = torch.sqrt(n2)
    inv = 1 / rt
    at_q = dq.abs() < dp.abs()
    dr, r = torch.where(at_q, dq, dp), torch.where(at_q[:, None], q, p)
    delta = torch.where(holds, dr.abs() * inv, torch.zeros_like(dr))
    unit = torch.sign(dr)[:, None] * (n * inv[:, None])
    lb, lc = fr._dot(fr._cross(r - a, c - a), n) / rt / rt, fr._dot(fr._cross(b - a, r - a), n) / rt / rt
    return holds, delta, at_q, unit, torch.stack([1 - (lb + lc), lb, lc], -1), torch.stack([dp, dq, s0, s1, s2], -1)


def candidates(v, faces):
    """meshcheck_restated.candidates over the faces that take part: every index inside [0, V) and no index repeated."""
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < len(v))).all(1) & (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    at = np.nonzero(ok)[0]
    i, j = mr.candidates(v, faces[at])
    return at[i], at[j]


def pair_tests(x, faces, i, j, variant=False):
    """One mesh x [V,3] (a tensor of the working precision), candidate pairs (i [n], j [n]) -> dict of tensors: holds bool [n,6],
    delta [n,6], at_q bool [n,6], vert int64 [n,6,4] (the shallower end, then a, b, c of the triangle), contrib [n,6,4,3] (the
    gradient of delta by those four), n2 [n,6] (|n|^2 of the triangle, as computed), dets [n,6,5]."""
    faces = torch.as_tensor(np.asarray(faces).astype(np.int64)).reshape(-1, 3)
    i, j = torch.as_tensor(np.asarray(i, np.int64)), torch.as_tensor(np.asarray(j, np.int64))
    fi, fj = faces[i], faces[j]
    A, B = x[fi], x[fj]
    fn = _directed_variant if variant else fr._directed
    out = {k: [] for k in ('holds', 'delta', 'at_q', 'vert', 'contrib', 'n2', 'dets')}
    for side, e0, e1 in TESTS:
        X, Y, fX, fY = (A, B, fi, fj) if side == 0 else (B, A, fj, fi)
        holds, delta, at_q, unit, lam, dets = fn(X[:, e0], X[:, e1], Y)
        n = fr._cross(Y[:, 1] - Y[:, 0], Y[:, 2] - Y[:, 0])
        out['n2'].append(fr._dot(n, n))
        out['holds'].append(holds)
        out['delta'].append(delta)
        out['at_q'].append(at_q)
        out['dets'].append(dets)
        out['vert'].append(torch.cat([torch.where(at_q, fX[:, e1], fX[:, e0])[:, None], fY], 1))
        out['contrib'].append(torch.cat([unit[:, None], -lam[:, :, None] * unit[:, None]], 1))
    return {k: torch.stack(v, 1) for k, v in out.items()}


def quantise(c):
    """llrint(double(c) 2^40) as int64 (round half to even); c finite and below 2^20 in magnitude."""
    return np.rint(np.asarray(c).astype(np.float64) * Q).astype(np.int64)


def unquantise(acc):
    return (np.asarray(acc, np.int64).astype(np.float64) * (1. / Q)).astype(np.float32)


def dropped(holds, delta, contrib, n2):
    """numpy: the tests that hold and are dropped as a whole."""
    with np.errstate(invalid='ignore'):
        every = np.concatenate([delta[..., None], contrib.reshape(contrib.shape[:-2] + (12,))], -1).astype(np.float64)
        bad = ~np.isfinite(every) | (np.abs(every) >= LIMIT)
        n2 = n2.astype(np.float64)
        return holds & (bad.any(-1) | (n2 == 0) | ~np.isfinite(n2))


def penalty(verts, faces, dt=np.float64, variant=False):
    """verts [N,V,3] float32 -> dict: loss float32 [N], gunit float32 [N,V,3], n_pairs int64 [N], n_dropped int64 [N], acc_loss int64
    [N], acc_grad int64 [N,V,3]; value float64 [N] and grad float64 [N,V,3]: the same sums without the fixed point (contributions
    of dt added in float64), what the closed form is held against autograd by; frames: per mesh a dict with pairs [n,2] (the
    candidates), hit bool [n], holds, at_q, delta, dets, charged (holds and not dropped)."""
    faces = np.asarray(faces)
    verts = mr._frames(verts)
    N, V = verts.shape[:2]
    acc_loss, acc_grad = np.zeros(N, np.int64), np.zeros((N, V, 3), np.int64)
    value, grad = np.zeros(N), np.zeros((N, V, 3))
    n_pairs, n_dropped, frames = np.zeros(N, np.int64), np.zeros(N, np.int64), []
    for t, v in enumerate(verts):
        i, j = candidates(v, faces)
        x = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(DT[dt])
        r = {k: a.numpy() for k, a in pair_tests(x, faces, i, j, variant).items()}
        holds = r['holds']
        drop = dropped(holds, r['delta'], r['contrib'], r['n2'])
        charged = holds & ~drop
        n_pairs[t], n_dropped[t] = holds.any(1).sum(), drop.sum()
        acc_loss[t] = quantise(r['delta'][charged]).sum()
        np.add.at(acc_grad[t], r['vert'][charged].reshape(-1), quantise(r['contrib'][charged]).reshape(-1, 3))
        value[t] = r['delta'][charged].astype(np.float64).sum()
        np.add.at(grad[t], r['vert'][charged].reshape(-1), r['contrib'][charged].astype(np.float64).reshape(-1, 3))
        frames.append(dict(pairs=np.stack([i, j], -1).astype(np.int64).reshape(-1, 2), hit=holds.any(1), holds=holds, at_q=r['at_q'],
                           delta=r['delta'], dets=r['dets'], charged=charged))
    return dict(loss=unquantise(acc_loss), gunit=unquantise(acc_grad), n_pairs=n_pairs, n_dropped=n_dropped, acc_loss=acc_loss,
                acc_grad=acc_grad, value=value, grad=grad, frames=frames)


def autograd(verts, faces):
    """float64 autograd of the definition without the fixed point: -> (value [N], grad [N,V,3])."""
    faces = np.asarray(faces)
    verts = mr._frames(verts)
    value, grad = np.zeros(len(verts)), np.zeros(verts.shape)
    for t, v in enumerate(verts):
        i, j = candidates(v, faces)
        x = torch.from_numpy(np.ascontiguousarray(v, np.float32)).double().requires_grad_(True)
        total = pair_tests(x, faces, i, j)['delta'].sum()
        value[t] = float(total.detach())
        if len(i) and total.requires_grad:
            grad[t] = torch.autograd.grad(total, x, allow_unused=True)[0].numpy()
    return value, grad


def counts(verts, faces):
    """n_pairs [N] as scripts/eval_shape.py counts them."""
    return np.array([r['n_pairs'] for r in mr.self_intersections(verts, faces)], np.int64)


def descend(verts, faces, rate, steps, dt=np.float64):
    """Plain gradient descent on the penalty from verts [N,V,3], the gradient (gunit) in dt and the vertices kept in float32 (what
    the device holds): -> (the first step after which n_pairs of every mesh is 0, or None; the vertices; n_pairs after every step)."""
    faces = np.asarray(faces)
    x = np.array(mr._frames(verts), np.float32)
    history = []
    for step in range(1, steps + 1):
        g = penalty(x, faces, dt)['gunit']
        x = (x.astype(np.float64) - rate * g.astype(np.float64)).astype(np.float32)
        history.append(counts(x, faces))
        if not history[-1].any():
            return step, x, history
    return None, x, history


def conditions(verts, faces):
    """What the GPU comparisons rest on, per mesh: -> list of dicts: same = the float32 and float64 restatements agree on which
    tests hold and, where one holds, on which end is the shallower; two = every intersecting pair has exactly two tests that hold;
    diff = |float32 loss sum - float64 loss sum| without the fixed point."""
    a, b = penalty(verts, faces, np.float64), penalty(verts, faces, np.float32)
    out = []
    for t, (fa, fb) in enumerate(zip(a['frames'], b['frames'])):
        same = bool((fa['holds'] == fb['holds']).all() and (fa['at_q'][fa['holds']] == fb['at_q'][fa['holds']]).all())
        out.append(dict(same=same, two=bool((fa['holds'].sum(1)[fa['hit']] == 2).all()), diff=abs(float(a['value'][t] - b['value'][t])),
                        n_pairs=int(a['n_pairs'][t])))
    return out
