#!/usr/bin/env python3
"""What does watching a run cost?  The spot3 stage-0 optimisation step (the configuration of bench.py's optimize leg:
scripts/spot3.sh:24, batch 1 pair, 8 hypotheses, 21 bones, 256 x 256, --use_graph) timed without and with --monitor.

    python tools/monitor_bench.py [--iters 400] [--runs 3] [--monitor] [--json out.json]

Without --monitor the loop is train_step alone (on the parent commit this file measures the same thing, so its runs give the
run-to-run spread to compare with).  With --monitor every step also pushes its scalars into the ring, and once per 200 steps the
contact sheet is composed, copied and saved and the ring is flushed to scalars.csv, as LASRTrainer.train does per epoch.  For the
kernels' own times run it under `rocprofv3 --kernel-trace --stats -- python tools/monitor_bench.py --monitor --runs 1`:
scalar_ring_push_kernel, sheet_stats_kernel and sheet_compose_kernel appear in the kernel statistics."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(iters, monitor_on, out_dir):
    import optimize
    from lasr_amd.nnutils import train_utils
    flags = ['--name', 'bench', '--checkpoint_dir', '', '--only_mean_sym', '--nouse_gtpose', '--subdivide', '3', '--n_bones', '21',
             '--n_hypo', '8', '--num_epochs', '5', '--batch_size', '1', '--opt_tex', 'yes', '--iters_per_epoch', str(iters + 6), '--use_graph']
    if monitor_on:
        flags += ['--monitor', '--monitor_dir', out_dir]
    opts = optimize.parse_flags(flags)
    torch.manual_seed(0)
    tr = train_utils.LASRTrainer(opts).init_training()
    tr.model.train()
    tr.reinit_bones()
    mon = tr._monitor() if monitor_on else None
    m = tr.module
    m.epoch, m.optim_idx = 0, 0
    for i in range(6):                                   # iteration 0 renders the part image; 1.. capture + replay the graph
        m.iters = i
        _, aux = tr.train_step(tr.set_input(tr.dataloader[i]))
        if i == 0:
            first_aux = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in aux.items()}
        if mon is not None:
            mon.push(aux, tr, i + 1)
    if mon is not None:
        mon.images(0, m, first_aux, 0)
        mon.flush()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        m.iters = 6 + i
        _, aux = tr.train_step(tr.set_input(tr.dataloader[6 + i]))
        if mon is not None:
            mon.push(aux, tr, 7 + i)
            if (i + 1) % 200 == 0:                       # an epoch of the reference: one sheet, one flush
                sheet_aux = dict(aux, part_render=first_aux.get('part_render'))
                mon.images(1 + i // 200, m, sheet_aux, 0)
                mon.flush()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if mon is not None:
        mon.flush()
    torch.cuda.set_stream(torch.cuda.default_stream())
    return {'iters_per_s': iters / dt, 'ms_per_iter': dt / iters * 1e3, 'iters': iters, 'monitor': bool(monitor_on)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=400)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--monitor', action='store_true')
    ap.add_argument('--json', default='')
    args = ap.parse_args(argv)
    out_dir = tempfile.mkdtemp(prefix='lasr_monitor_')
    runs = []
    for r in range(args.runs):
        runs.append(run(args.iters, args.monitor, out_dir))
        print(json.dumps(runs[-1]), flush=True)
        torch.cuda.empty_cache()
    res = {'config': 'spot3 stage 0, --use_graph, %d iterations per run' % args.iters, 'monitor': args.monitor, 'runs': runs,
           'iters_per_s_min': min(r['iters_per_s'] for r in runs), 'iters_per_s_max': max(r['iters_per_s'] for r in runs)}
    print(json.dumps(res))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
