#!/usr/bin/env python3
"""What does the SSIM texture term cost?  (lasr_amd/csrc/ssim.hip, fused_ops.ssim_distance)

    python tools/ssim_bench.py kernels [--iters 20] [--repeats 3] [--json out.json]
    python tools/ssim_bench.py step    [--steps 200] [--repeats 3] [--json out.json]

kernels: at the shapes of spot3 stage 0 (a [4,3,256,256], b [32,3,256,256], repeat 8) and at its two pooled scales, the forward
(lasr_ssim_forward: tiles + fold) without and with the three saved derivative planes, the backward (lasr_ssim_backward) in its
two forms (moments recomputed | planes read back), the three-scale StructuralDistance forward + backward as a whole, and the same
with the torch composition (ssim_distance_torch), the only comparator there is.  The variants alternate inside one process; each
figure is the median over --iters calls between two device events, repeated --repeats times (median of the medians, their minimum
and maximum).  Bytes: what the kernels must move at least (a once per image, b, grad_b; + the planes) against the time.
step: optimize.py iterations per second at spot3 stage 0 under graph replay with --ptex_method alexnet (the default), ssim, and
--noperceptual: the three trainers live in one process and are timed in turns, --repeats rounds of --steps steps each.
No test asserts a time.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lasr_amd import _lib   # noqa: E402
from lasr_amd.nnutils import fused_ops, mesh_net   # noqa: E402


def interleaved(fns, iters, repeats):
    """{name: fn} timed in turns between two device events -> {name: median of the per-repeat medians, their min and max (ms)}."""
    meds = {k: [] for k in fns}
    for _ in range(repeats):
        ms = {k: [] for k in fns}
        for _ in range(iters):
            for k, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
        for k in fns:
            meds[k].append(statistics.median(ms[k]))
    return {k: {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v)} for k, v in meds.items()}


def textures(M, rep, S, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.nn.functional.interpolate(torch.rand(M, 3, S // 8, S // 8, generator=g), size=(S, S), mode='bilinear')
    a = (a * 255).round() / 255
    b = (a.repeat_interleave(rep, 0) + 0.05 * torch.randn(M * rep, 3, S, S, generator=g)).clamp(0, 1)
    return a.to(dev), b.to(dev)


def kernels(args, dev):
    M, rep = 4, 8
    N = M * rep
    out = {'shapes': 'a [%d,3,S,S], b [%d,3,S,S], repeat %d' % (M, N, rep), 'scales': []}
    for S in (256, 128, 64):
        a, b = textures(M, rep, S, dev)
        So = S - 10
        d = torch.empty(N, device=dev)
        gd = torch.rand(N, device=dev)
        gb = torch.empty_like(b)
        planes = torch.empty(N, 3, 3, So, So, device=dev)
        scratch = torch.empty(_lib.lib().lasr_ssim_scratch_floats(M, rep, S, S), device=dev)
        _lib.call('lasr_ssim_forward', a, b, d, planes, scratch, M, rep, S, S, 1.0)
        fns = {
            'forward': lambda: _lib.call('lasr_ssim_forward', a, b, d, None, scratch, M, rep, S, S, 1.0),
            'forward_saving_planes': lambda: _lib.call('lasr_ssim_forward', a, b, d, planes, scratch, M, rep, S, S, 1.0),
            'backward_recompute': lambda: _lib.call('lasr_ssim_backward', a, b, None, gd, gb, M, rep, S, S, 1.0),
            'backward_saved_planes': lambda: _lib.call('lasr_ssim_backward', a, b, planes, gd, gb, M, rep, S, S, 1.0),
        }
        bt = b.clone().requires_grad_(True)

        def torch_fb():
            bt.grad = None
            fused_ops.ssim_distance_torch(a, bt, rep, 1.0).backward(gd)

        def torch_f():
            with torch.no_grad():
                fused_ops.ssim_distance_torch(a, bt, rep, 1.0)
        fns['torch_forward'], fns['torch_forward_backward'] = torch_f, torch_fb
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        res = interleaved(fns, args.iters, args.repeats)
        img, pl = 4 * 3 * S * S, 4 * 9 * So * So
        floor = {'forward': (M + N) * img, 'forward_saving_planes': (M + N) * img + N * pl,
                 'backward_recompute': (M + 2 * N) * img, 'backward_saved_planes': (M + 2 * N) * img + N * pl}
        for k, nbytes in floor.items():
            res[k]['floor_bytes'] = nbytes
            res[k]['floor_gb_per_s'] = nbytes / (res[k]['median_ms'] * 1e-3) / 1e9
        out['scales'].append({'S': S, **res})
    a, b = textures(M, rep, 256, dev)
    gd = torch.rand(N, device=dev)
    bt = b.clone().requires_grad_(True)

    def module_fb(use_kernel, save):
        net = mesh_net.StructuralDistance(3, use_kernel)

        def fn():
            bt.grad = None
            old, fused_ops.SSIM_SAVE_PLANES = fused_ops.SSIM_SAVE_PLANES, save
            try:
                net.forward_pair(a, bt, repeat=rep, unit_range=True).backward(gd)
            finally:
                fused_ops.SSIM_SAVE_PLANES = old
        return fn
    fns = {'kernel_recompute': module_fb(True, False), 'kernel_saved_planes': module_fb(True, True), 'torch': module_fb(False, False)}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out['structural_distance_3_scales_forward_backward'] = interleaved(fns, args.iters, args.repeats)
    return out


def step(args, dev):
    import optimize
    from lasr_amd.nnutils import train_utils
    settings = {'alexnet': [], 'ssim': ['--ptex_method', 'ssim'], 'noperceptual': ['--noperceptual']}
    need = 6 + args.steps * args.repeats
    trainers = {}
    for name, extra in settings.items():
        opts = optimize.parse_flags(['--name', 'bench', '--checkpoint_dir', '', '--only_mean_sym', '--nouse_gtpose', '--subdivide', '3',
                                     '--n_bones', '21', '--n_hypo', '8', '--num_epochs', '5', '--batch_size', '1', '--opt_tex', 'yes',
                                     '--iters_per_epoch', str(need), '--use_graph'] + extra)
        opts.local_rank = dev.index
        torch.manual_seed(0)
        tr = train_utils.LASRTrainer(opts).init_training()
        tr.model.train()
        tr.reinit_bones()
        for i in range(6):                           # iteration 0 renders the part image; 1.. capture + replay the graph
            tr.module.iters = i
            tr.train_step(tr.set_input(tr.dataloader[i]))
        trainers[name] = tr
    torch.cuda.synchronize()
    rates = {k: [] for k in trainers}
    at = 6
    for _ in range(args.repeats):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                tr.module.iters = at + i
                tr.train_step(tr.set_input(tr.dataloader[at + i]))
            torch.cuda.synchronize()
            rates[name].append(args.steps / (time.perf_counter() - t0))
        at += args.steps
    return {'config': 'spot3 stage 0 (batch 1 pair, n_hypo 8, n_bones 21, 256x256), --use_graph, %d steps per turn' % args.steps,
            'iters_per_s': {k: {'median': statistics.median(v), 'min': min(v), 'max': max(v)} for k, v in rates.items()}}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['kernels', 'step'])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--json', default='')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit('ssim_bench.py: no HIP device: times are measured on the GPU or not at all')
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'repeats': args.repeats}
    res[args.what] = kernels(args, dev) if args.what == 'kernels' else step(args, dev)
    print(json.dumps(res))
    if args.json:
        if os.path.dirname(args.json):
            os.makedirs(os.path.dirname(args.json), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
