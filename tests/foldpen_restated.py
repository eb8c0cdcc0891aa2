"""Restatement of the fold penalty of the optimiser (optimize.py --fold_wt / --pierce_wt; include/lasr_ops.h, DESIGN.md section
4.21) in torch on the CPU, for float64 and float32, and what tests/test_foldpen_cpu.py and tests/test_foldpen_gpu.py share.  Nothing
here imports the package: the kernels of lasr_amd/csrc/foldpen.hip and scripts/fold_penalty.py are compared against this file, not
the other way round.  The topology, its keys and the fixtures are those of tests/meshnbr_restated.py.

This file is the definition.  x [N,V,3] are the posed meshes of a step, faces [F,3] one topology, the list the sorted keys of the
neighbour pass, phi the penalty's angle in radians (0 < phi <= pi / 2; float32(radians(fold_deg)) in every precision).

Crease term, per EDGE pair (i, j): nA = (A1 - A0) x (A2 - A0), nB likewise, d = (nAx nBx + nAy nBy) + nAz nBz, negated when `same`
is set, qa = |nA|^2, qb = |nB|^2, q = qa qb, s = |nA x nB|, theta = atan2(s, -d) in [0, pi] (0: a complete fold, pi: flat).  The value
is max(0, phi - theta)^2; a pair with q = 0 or q not finite has value 0 and gradient 0.  The gradient is the closed-form hinge
gradient: with x0 = A[(ca+1)%3], x1 = A[(ca+2)%3] (the shared edge), x2 = A[ca], x3 = B[cb] (the apexes), e = x1 - x0,
GA = -sign(orient(A0, A1, A2, x3)) |e| nA / qa, GB = -sign(orient(B0, B1, B2, x2)) |e| nB / qb, tA = ((x2 - x0) . e) / |e|^2,
tB = ((x3 - x0) . e) / |e|^2:  d theta / d x2 = GA, / d x3 = GB, / d x0 = -(1 - tA) GA - (1 - tB) GB, / d x1 = -tA GA - tB GB.
Both signs are 0 at the exact complete fold: the kink of the unsigned angle gets gradient 0.

Pierce term, per VERTEX pair: both directed tests of the neighbour pass (the edge opposite the shared corner of A against B, and of B
against A; orient and PIERCES strict and without contraction).  For a test that holds, with edge (p, q) and triangle (a, b, c),
n = (b - a) x (c - a): delta = min(|orient(a,b,c,p)|, |orient(a,b,c,q)|) / |n|, the depth itself.  Its gradient goes to the shallower
end point r (p on a tie): sign(orient(a,b,c,r)) n / |n|, and to a, b, c: minus that times the barycentric coordinates of r's foot in
the plane, l_b = ((r - a) x (c - a)) . n / |n|^2, l_c = ((b - a) x (r - a)) . n / |n|^2, l_a = 1 - l_b - l_c.  The value of the pair
is the sum over the tests that hold.

loss [N,2] = (crease sum, pierce sum) per mesh: the per-entry values in the working precision, added in float64 and rounded once.

The roles of the five slots of an entry's contribution row:
  vertex pair: 0 the shared vertex, 1 2 = A[(ca+1)%3] A[(ca+2)%3], 3 4 = B[(cb+1)%3] B[(cb+2)%3]
  edge pair:   0 = A[ca], 1 2 = A[(ca+1)%3] A[(ca+2)%3], 3 = B[cb], 4 unused
"""
import math

import numpy as np
import torch

import meshnbr_restated as nr

FOLD_DEG = 30.
DT = {np.float64: torch.float64, np.float32: torch.float32, torch.float64: torch.float64, torch.float32: torch.float32}


def phi_of(fold_deg=FOLD_DEG):
    """radians(fold_deg) in double, rounded once to float32."""
    return float(np.float32(math.radians(float(fold_deg))))


def _cross(u, w):
    return torch.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                        u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _orient(a, b, c, d):
    return _dot(_cross(b - a, c - a), d - a)


def _pick(T, k):
    """corner k[n] of triangles T [n,3,3]."""
    return T[torch.arange(T.shape[0]), k]


def _fields(top, kind):
    m = np.nonzero(np.asarray(top['kind']) == kind)[0]
    return (m,) + tuple(torch.from_numpy(np.asarray(top[k])[m].astype(np.int64)) for k in ('i', 'j', 'ca', 'cb', 'same'))


def slots(faces, top):
    """-> int64 [n_list,5]: the vertex index behind every slot of every entry, -1 for the unused slot 4 of an edge pair."""
    f = np.asarray(faces).astype(np.int64)
    i, j, ca, cb, kind = (np.asarray(top[k]) for k in ('i', 'j', 'ca', 'cb', 'kind'))
    n = np.arange(len(i))
    fa, fb = f[i], f[j]
    out = np.stack([fa[n, ca], fa[n, (ca + 1) % 3], fa[n, (ca + 2) % 3], fb[n, (cb + 1) % 3], fb[n, (cb + 2) % 3]], -1)
    edge = kind == nr.EDGE
    out[edge, 3] = fb[n, cb][edge]
    out[edge, 4] = -1
    return out


def crease(x, faces, top, phi, closed=False, wide=False):
    """One mesh x [V,3] (a tensor of the working precision) -> (value [n_edge], theta [n_edge], active bool [n_edge]) and, with
    closed, the rows [n_edge,5,3] of d value / d slot.  wide: the arc tangent alone in float64, rounded once (another order of
    operations of the same definition)."""
    _, i, j, ca, cb, same = _fields(top, nr.EDGE)
    faces = torch.as_tensor(np.asarray(faces).astype(np.int64))
    A, B = x[faces[i]], x[faces[j]]
    nA, nB = _cross(A[:, 1] - A[:, 0], A[:, 2] - A[:, 0]), _cross(B[:, 1] - B[:, 0], B[:, 2] - B[:, 0])
    d = _dot(nA, nB)
    d = torch.where(same == 1, -d, d)
    qa, qb = _dot(nA, nA), _dot(nB, nB)
    q = qa * qb
    good = (q > 0) & torch.isfinite(q)
    c = _cross(nA, nB)
    s2 = _dot(c, c)
    pos = good & (s2 > 0)
    s = torch.where(pos, torch.sqrt(torch.where(pos, s2, torch.ones_like(s2))), torch.zeros_like(s2))      # no gradient through s = 0
    theta = torch.atan2(s.double() if wide else s, torch.where(good, -d, torch.ones_like(d)).to(torch.float64 if wide else d.dtype)).to(d.dtype)
    active = good & (theta < phi)
    gap = torch.where(active, phi - theta, torch.zeros_like(theta))
    value = gap * gap
    if not closed:
        return value, theta, active
    one = torch.ones_like(q)
    x0, x1, x2, x3 = _pick(A, (ca + 1) % 3), _pick(A, (ca + 2) % 3), _pick(A, ca), _pick(B, cb)
    e = x1 - x0
    le2 = torch.where(active, _dot(e, e), one)
    le = torch.sqrt(le2)
    sa, sb = torch.sign(_orient(A[:, 0], A[:, 1], A[:, 2], x3)), torch.sign(_orient(B[:, 0], B[:, 1], B[:, 2], x2))
    GA = (-sa * le / torch.where(active, qa, one))[:, None] * nA
    GB = (-sb * le / torch.where(active, qb, one))[:, None] * nB
    tA, tB = (_dot(x2 - x0, e) / le2)[:, None], (_dot(x3 - x0, e) / le2)[:, None]
    g0, g1 = -(1 - tA) * GA - (1 - tB) * GB, -tA * GA - tB * GB
    rows = torch.stack([GA, g0, g1, GB, torch.zeros_like(GA)], 1) * (-2 * gap)[:, None, None]
    return value, theta, active, torch.where(active[:, None, None], rows, torch.zeros_like(rows))


def _directed(p, q, T):
    """Edge (p, q) [n,3] against triangles T [n,3,3] -> (holds bool, delta, q is the shallower end bool, its gradient direction
    [n,3], the three barycentric weights [n,3], the five determinants [n,5])."""
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    dp, dq = _orient(a, b, c, p), _orient(a, b, c, q)
    s0, s1, s2 = _orient(p, q, a, b), _orient(p, q, b, c), _orient(p, q, c, a)
    holds = (((dp > 0) & (dq < 0)) | ((dp < 0) & (dq > 0))) & (((s0 > 0) & (s1 > 0) & (s2 > 0)) | ((s0 < 0) & (s1 < 0) & (s2 < 0)))
    n = _cross(b - a, c - a)
    n2 = torch.where(holds, _dot(n, n), torch.ones_like(dp))
    at_q = dq.abs() < dp.abs()                                                     # a tie: p
    dr, r = torch.where(at_q, dq, dp), torch.where(at_q[:, None], q, p)
    delta = torch.where(holds, dr.abs() / torch.sqrt(n2), torch.zeros_like(dr))
    unit = torch.sign(dr)[:, None] * n / torch.sqrt(n2)[:, None]
    lb, lc = _dot(_cross(r - a, c - a), n) / n2, _dot(_cross(b - a, r - a), n) / n2
    return holds, delta, at_q, unit, torch.stack([1 - lb - lc, lb, lc], -1), torch.stack([dp, dq, s0, s1, s2], -1)


def pierce(x, faces, top, closed=False):
    """One mesh x [V,3] -> (value [n_vertex], holds bool [n_vertex,2], dets [n_vertex,2,5], |dp| - |dq| [n_vertex,2]) and, with
    closed, the rows [n_vertex,5,3]."""
    _, i, j, ca, cb, _ = _fields(top, nr.VERTEX)
    faces = torch.as_tensor(np.asarray(faces).astype(np.int64))
    A, B = x[faces[i]], x[faces[j]]
    n = torch.arange(len(i))
    t1 = _directed(_pick(A, (ca + 1) % 3), _pick(A, (ca + 2) % 3), B)
    t2 = _directed(_pick(B, (cb + 1) % 3), _pick(B, (cb + 2) % 3), A)
    value = t1[1] + t2[1]
    holds, dets = torch.stack([t1[0], t2[0]], -1), torch.stack([t1[5], t2[5]], 1)
    ties = torch.stack([t1[5][:, 0].abs() - t1[5][:, 1].abs(), t2[5][:, 0].abs() - t2[5][:, 1].abs()], -1)
    if not closed:
        return value, holds, dets, ties
    rows = torch.zeros(len(i), 5, 3, dtype=x.dtype)
    for (hold, _, at_q, unit, lam, _), own, corner in ((t1, 1, cb), (t2, 3, ca)):  # own: the first slot of the edge's own face
        unit = torch.where(hold[:, None], unit, torch.zeros_like(unit))
        rows[n, own + at_q.long()] += unit
        other = 4 - own                                                            # the first slot of the triangle's opposite edge
        for k in range(3):                                                         # stored corner k of the triangle
            slot = torch.where(corner == k, torch.zeros_like(corner), torch.where((corner + 1) % 3 == k, torch.full_like(corner, other),
                                                                                   torch.full_like(corner, other + 1)))
            rows[n, slot] += -lam[:, k, None] * unit
    return value, holds, dets, ties, rows


def penalty(verts, faces, fold_deg=FOLD_DEG, dt=np.float64, top=None, closed=True, variant=False):
    """verts [N,V,3] float32 -> dict of numpy arrays in dt: values [N,n_list] (list order), active bool [N,n_list], theta [N,n_edge],
    loss [N,2], and with closed the rows [N,n_list,5,3], slots [n_list,5] and grad [2,N,V,3]: the closed-form gradients of the
    crease sum and of the pierce sum, the rows added per vertex in float64.  variant: the same definition in another order of
    operations (the arc tangent in float64 and rounded once, the rows added per vertex in dt and in descending order): what two
    float32 evaluations may differ by."""
    faces = np.asarray(faces)
    top = top or nr.topology(faces)
    phi, tdt = phi_of(fold_deg), DT[dt]
    verts = nr._frames(verts)
    em, vm = np.nonzero(top['kind'] == nr.EDGE)[0], np.nonzero(top['kind'] == nr.VERTEX)[0]
    N, V, n = verts.shape[0], verts.shape[1], top['n_list']
    out = dict(values=torch.zeros(N, n, dtype=tdt), active=torch.zeros(N, n, dtype=torch.bool), theta=torch.zeros(N, len(em), dtype=tdt),
               rows=torch.zeros(N, n, 5, 3, dtype=tdt), dets=torch.zeros(N, len(vm), 2, 5, dtype=tdt), ties=torch.zeros(N, len(vm), 2, dtype=tdt),
               holds=torch.zeros(N, len(vm), 2, dtype=torch.bool))
    for t in range(N):
        x = torch.from_numpy(np.ascontiguousarray(verts[t], np.float32)).to(tdt)
        c, p = crease(x, faces, top, phi, closed, variant), pierce(x, faces, top, closed)
        out['values'][t, em], out['theta'][t], out['active'][t, em] = c[0], c[1], c[2]
        out['values'][t, vm], out['active'][t, vm] = p[0], p[1].any(1)
        out['holds'][t], out['dets'][t], out['ties'][t] = p[1], p[2], p[3]
        if closed:
            out['rows'][t, em], out['rows'][t, vm] = c[3], p[4]
    loss = torch.stack([out['values'][:, em].double().sum(1), out['values'][:, vm].double().sum(1)], 1).to(tdt)
    res = {k: v.numpy() for k, v in out.items()}
    res['loss'] = loss.numpy()
    if closed:
        sl = slots(faces, top)
        grad = np.zeros((2, N, V, 3), dt if variant else np.float64)
        for plane, m in ((0, em), (1, vm)):
            for s in (range(4, -1, -1) if variant else range(5)):
                ok = np.nonzero(sl[m, s] >= 0)[0][::-1 if variant else 1]
                for t in range(N):
                    np.add.at(grad[plane, t], sl[m, s][ok], res['rows'][t, m, s][ok].astype(grad.dtype))
        res.update(slots=sl, grad=grad.astype(np.float64))
    else:
        del res['rows']
    return res


def autograd(verts, faces, fold_deg=FOLD_DEG, top=None):
    """float64 autograd of the definition: -> (loss [N,2], grad [2,N,V,3]: of the crease sum and of the pierce sum)."""
    faces = np.asarray(faces)
    top = top or nr.topology(faces)
    phi = phi_of(fold_deg)
    verts = nr._frames(verts)
    loss, grad = np.zeros((len(verts), 2)), np.zeros((2,) + verts.shape)
    for t, v in enumerate(verts):
        for plane in (0, 1):
            x = torch.from_numpy(np.ascontiguousarray(v, np.float32)).double().requires_grad_(True)
            total = (crease(x, faces, top, phi)[0] if plane == 0 else pierce(x, faces, top)[0]).sum()
            loss[t, plane] = float(total.detach())
            if total.requires_grad:
                grad[plane, t] = torch.autograd.grad(total, x, allow_unused=True)[0].numpy()
    return loss, grad


def counts(verts, faces, fold_deg=nr.FOLD_DEG):
    """(n_creased [N], n_pierced [N]) as scripts/eval_shape.py --neighbours counts them."""
    res = nr.evaluate(verts, faces, fold_deg)
    return res['n_creased'], res['n_pierced']


def descend(verts, faces, rate, steps, fold_deg=FOLD_DEG, dt=np.float64, weights=(1., 1.), count_deg=nr.FOLD_DEG):
    """Plain gradient descent on weights . (crease, pierce) from verts [N,V,3], the closed-form gradient in dt and the vertices kept
    in float32 (what the device holds): -> (the first step after which both counts of every mesh are 0, or None; the vertices;
    the counts after every step)."""
    faces = np.asarray(faces)
    top = nr.topology(faces)
    x = np.array(nr._frames(verts), np.float32)
    history = []
    for step in range(1, steps + 1):
        g = penalty(x, faces, fold_deg, dt, top)['grad']
        x = (x.astype(np.float64) - rate * (weights[0] * g[0] + weights[1] * g[1])).astype(np.float32)
        history.append(counts(x, faces, count_deg))
        if not history[-1][0].any() and not history[-1][1].any():
            return step, x, history
    return None, x, history


def conditions(verts, faces, fold_deg=FOLD_DEG):
    """What the GPU comparisons rest on, per mesh: -> list of dicts: angle = the least distance in degrees of any theta from phi or
    from 0; det = the worst |det64| / |det32 - det64| over the ten determinants of the vertex pairs; tie = the same for |dp| - |dq|
    over the directed tests that hold (inf where the two precisions agree)."""
    faces = np.asarray(faces)
    top = nr.topology(faces)
    a, b = penalty(verts, faces, fold_deg, np.float64, top, False), penalty(verts, faces, fold_deg, np.float32, top, False)
    out = []

    def ratio(x64, x32):
        diff = np.abs(x64 - x32.astype(np.float64))
        if x64.size and (x64 == 0).any():
            return 0.
        return float((np.abs(x64)[diff > 0] / diff[diff > 0]).min()) if (diff > 0).any() else np.inf
    for t in range(a['values'].shape[0]):
        th = np.degrees(a['theta'][t])
        angle = float(min(np.abs(th - np.degrees(phi_of(fold_deg))).min(), np.abs(th).min())) if th.size else np.inf
        hold = a['holds'][t]
        out.append(dict(angle=angle, det=ratio(a['dets'][t], b['dets'][t]), tie=ratio(a['ties'][t][hold], b['ties'][t][hold]),
                        same=bool((a['active'][t] == b['active'][t]).all())))
    return out
