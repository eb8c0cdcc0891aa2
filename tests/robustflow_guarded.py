"""The guarded case of the three natives preprocess/robust_flow.py launches (tests/guarded.py): the same treatment the rows of
tests/guarded_cases.py give the natives launched from lasr_amd/, from a file of its own because that table names only the latter.
tests/test_robustflow_cpu.py holds the module's launch sites against NATIVES; tests/test_robustflow_gpu.py runs the case."""
import os
import sys

import torch

import guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVES = ('lasr_rflow_derivs', 'lasr_rflow_tensor', 'lasr_rflow_weights')


def robust_flow():
    folder = os.path.join(ROOT, 'preprocess')
    if folder not in sys.path:
        sys.path.insert(0, folder)
    import robust_flow as rf
    return rf


def _run(dev):
    rf = robust_flow()
    g = torch.Generator(device='cpu').manual_seed(71)
    out = []
    for H, W in ((47, 65), (2, 2)):
        A, B = torch.rand(H, W, 3, generator=g).to(dev), torch.rand(H, W, 3, generator=g).to(dev)
        uv = (3 * torch.randn(2, H, W, generator=g)).to(dev)                      # part of the warp leaves the frame
        d = (0.1 * torch.randn(2, H, W, generator=g)).to(dev)
        R1, R2 = rf.derivs(A), rf.derivs(B)
        Jb, Jg = rf.tensor(R1, R2, uv)
        out += [R1, R2, Jb, Jg] + list(rf.weights(Jb, Jg, uv, d, 1e-3, 1., 5.))
    return tuple(out)


CASE = guarded.Case('robustflow', _run, NATIVES)
