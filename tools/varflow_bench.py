#!/usr/bin/env python3
"""What does the variational optical flow cost?  (lasr_amd/nnutils/varflow.py, csrc/varflow.hip)

    python tools/varflow_bench.py [--sizes 1080x1920,480x854] [--iters 20] [--runs 3] [--gamma 5 [--beta 1]] [--json out.json]

On a seeded synthetic pair (a band-limited texture translated by (0.011 W, 0.004 H), default parameters: 5 warps x 3 weight
updates x 10 SOR iterations per level) these are timed, warm-up excluded, each as the median over --iters calls with device
events, and the whole measurement --runs times, the variants alternating inside a run:
  flow        one varflow.flow(): pyramids of both frames and every level's warps (launches only, no host synchronisation)
  sor_x10     lasr_varflow_sor with iters = 10 on the finest level (one launch per red-black iteration); a tenth of it is one iteration
  torch_x10   the same ten iterations composed from torch operators on the same GPU (replicate padding, slices, torch.where on a
              checkerboard); its edge weights are computed once per ten iterations, not per iteration as the kernel does, which
              favours it
  tensor, weights   the two other per-warp kernels on the finest level
With --gamma > 0 the flow with the gradient-constancy term (preprocess/robust_flow.py, csrc/robustflow.hip) is timed beside it in
the same alternation, on the same pair:
  rflow       one robust_flow.flow(gamma, beta): as flow, plus a derivative record per level and frame
  rf_derivs, rf_tensor, rf_weights   its three kernels on the finest level (derivs once per level and frame, tensor per warp,
              weights per weight update); rflow_over_flow is the ratio of the two medians
The torch composition's result is compared with the kernel's before anything is timed.  Per SOR iteration the script also reports
the bytes one sweep must move at the least (13 floats per pixel: du, dv, u, v, psi_s, five J planes and psi_d read, du and dv
written) over the measured time, to set against the HBM rate.  No test asserts a time.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'preprocess'))
from lasr_amd.nnutils import varflow   # noqa: E402
import robust_flow                     # noqa: E402


def make_pair(H, W, dev, seed=0):
    """Two uint8 frames: a smooth random texture and the same texture moved by a whole number of pixels (0.011 W, 0.004 H)."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    tex = 128 + sum(F.interpolate(torch.randn(1, 3, max(H // s, 2), max(W // s, 2), generator=g), size=(H, W), mode='bicubic',
                                  align_corners=False)[0].permute(1, 2, 0) * a for s, a in ((48, 40.), (16, 20.), (6, 8.)))
    d = (max(round(0.011 * W), 1), max(round(0.004 * H), 1))
    a = tex.round().clamp(0, 255).to(torch.uint8)
    b = torch.roll(tex, shifts=(d[1], d[0]), dims=(0, 1)).round().clamp(0, 255).to(torch.uint8)
    return a.to(dev), b.to(dev), d


def _pad(a):
    return F.pad(a[None, None], (1, 1, 1, 1), mode='replicate')[0, 0]


def torch_sor(J, psi, uv, d, alpha, omega, iters):
    """lasr_varflow_sor from torch operators.  -> the new d [2,H,W]."""
    psid, psis = psi
    u, v = uv
    du, dv = d[0].clone(), d[1].clone()
    H, W = u.shape
    ah = alpha * 0.5
    P = _pad(psis)
    wl, wr, wu, wd = ah * (psis + P[1:-1, :-2]), ah * (psis + P[1:-1, 2:]), ah * (psis + P[:-2, 1:-1]), ah * (psis + P[2:, 1:-1])
    wl[:, 0] = 0
    wr[:, -1] = 0
    wu[0] = 0
    wd[-1] = 0
    ws = ((wl + wr) + wu) + wd
    ys, xs = torch.meshgrid(torch.arange(H, device=u.device), torch.arange(W, device=u.device), indexing='ij')
    red = ((xs + ys) & 1) == 0

    def smooth(f):
        p = _pad(f)
        return ((wl * p[1:-1, :-2] + wr * p[1:-1, 2:]) + wu * p[:-2, 1:-1]) + wd * p[2:, 1:-1]
    for _ in range(iters):
        for m in (red, ~red):
            new = (1 - omega) * du + omega * (((smooth(u + du) - ws * u) - psid * (J[3] + J[1] * dv)) / (psid * J[0] + ws))
            du = torch.where(m, new, du)
            new = (1 - omega) * dv + omega * (((smooth(v + dv) - ws * v) - psid * (J[4] + J[1] * du)) / (psid * J[2] + ws))
            dv = torch.where(m, new, dv)
    return torch.stack([du, dv])


def timed(fn, iters):
    """Median / min / max milliseconds of fn over iters calls, each between two device events."""
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms)}


def bench_size(H, W, iters, runs, dev, gamma=0., beta=1.):
    p = varflow.params()
    A, B, shift = make_pair(H, W, dev)
    I1, I2 = varflow.pyramid(A)[0], varflow.pyramid(B)[0]
    uv = varflow.flow_planar(A, B)                                         # the finest level's state near the solution
    J = varflow.tensor(I1, I2, uv)
    d0 = torch.zeros_like(uv)
    psi = varflow.weights(J, uv, d0, p['eps'])
    scratch = torch.empty_like(uv)
    d = torch.empty_like(uv)

    def sor_x10():
        d.zero_()
        return varflow.sor(J, psi, uv, d, p['alpha'], p['omega'], 10, scratch)

    def torch_x10():
        return torch_sor(J, psi, uv, d0, p['alpha'], p['omega'], 10)

    variants = {'flow': lambda: varflow.flow(A, B), 'sor_x10': sor_x10, 'torch_x10': torch_x10,
                'tensor': lambda: varflow.tensor(I1, I2, uv), 'weights': lambda: varflow.weights(J, uv, d0, p['eps'])}
    if gamma > 0:
        R1, R2 = robust_flow.derivs(I1), robust_flow.derivs(I2)
        Jb, Jg = robust_flow.tensor(R1, R2, uv)
        variants.update({'rflow': lambda: robust_flow.flow(A, B, gamma, beta), 'rf_derivs': lambda: robust_flow.derivs(I1),
                         'rf_tensor': lambda: robust_flow.tensor(R1, R2, uv),
                         'rf_weights': lambda: robust_flow.weights(Jb, Jg, uv, d0, p['eps'], beta, gamma)})
    native, composed = sor_x10().clone(), torch_x10()
    f = uv.permute(1, 2, 0)
    inner = f[H // 8:-H // 8, W // 8:-W // 8]
    torch.cuda.synchronize()
    res = {'H': H, 'W': W, 'levels': len(varflow.level_shapes(H, W)), 'shift': shift,
           'flow_error_inner_px': float((inner - torch.tensor([float(shift[0]), float(shift[1])], device=dev)).norm(dim=-1).mean()),
           'max_abs_diff_torch_vs_kernel': float((native - composed).abs().max()), 'runs': []}
    for fn in variants.values():                                           # warm-up: every shape of the timed window
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(runs):
        run = {name: timed(fn, max(iters // 4, 3) if name == 'torch_x10' else iters) for name, fn in variants.items()}
        res['runs'].append(run)
        print(json.dumps(dict(run, H=H, W=W)), flush=True)
    for name in variants:
        med = [r[name]['median_ms'] for r in res['runs']]
        res[name] = {'median_ms': statistics.median(med), 'min_of_medians_ms': min(med), 'max_of_medians_ms': max(med)}
    it_ms = res['sor_x10']['median_ms'] / 10
    res['sor_iteration_ms'] = it_ms
    res['torch_iteration_ms'] = res['torch_x10']['median_ms'] / 10
    res['sor_floor_bytes'] = 13 * 4 * H * W
    res['sor_floor_gb_per_s'] = res['sor_floor_bytes'] / (it_ms * 1e-3) / 1e9
    if gamma > 0:
        res.update(gamma=gamma, beta=beta, rflow_over_flow=res['rflow']['median_ms'] / res['flow']['median_ms'])
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1080x1920,480x854')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--gamma', type=float, default=0., help='> 0: time the flow with the gradient-constancy term beside the plain one')
    ap.add_argument('--beta', type=float, default=1.)
    ap.add_argument('--json', default='')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit('varflow_bench.py: no HIP device: times are measured on the GPU or not at all')
    dev = torch.device('cuda:0')
    out = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'sizes': []}
    for s in args.sizes.split(','):
        H, W = (int(v) for v in s.split('x'))
        out['sizes'].append(bench_size(H, W, args.iters, args.runs, dev, args.gamma, args.beta))
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
