"""The guarded case of the four natives preprocess/flow_match.py launches (tests/guarded.py): the same treatment the rows of
tests/guarded_cases.py give the natives launched from lasr_amd/, from a file of its own because that table names only the latter.
tests/test_flowmatch_cpu.py holds the module's launch sites against NATIVES; tests/test_flowmatch_gpu.py runs the case."""
import os
import sys

import torch

import guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVES = ('lasr_flowmatch_quantise', 'lasr_flowmatch_search', 'lasr_flowmatch_select', 'lasr_flowmatch_propagate')


def flow_match():
    folder = os.path.join(ROOT, 'preprocess')
    if folder not in sys.path:
        sys.path.insert(0, folder)
    import flow_match as fm
    return fm


def _run(dev):
    """The 37 x 53 pair: a random texture and itself moved by (6, -4) with a block of it moved by (-9, 5), so that matches are
    seeded against a zero flow and spread; both sources of the quantisation; a 2 x 2 frame."""
    fm = flow_match()
    g = torch.Generator(device='cpu').manual_seed(83)
    H, W = 37, 53
    base = torch.randint(0, 256, (H + 32, W + 32, 3), generator=g, dtype=torch.uint8)
    A = base[16:16 + H, 16:16 + W].clone()
    B = base[20:20 + H, 10:10 + W].clone()
    B[8:20, 30:44] = base[16 - 5 + 8:16 - 5 + 20, 16 + 9 + 30:16 + 9 + 44]
    A, B = A.to(dev), B.to(dev)
    qA, qB = fm.quantise(A), fm.quantise(B)
    level = (torch.rand(H, W, 3, generator=g) * 1.2 - 0.1).to(dev)               # some values outside 0..1: the clip
    out = [qA, qB, fm.quantise(level)]
    # (clones are ordinary allocations: inputs that a relocated run moves into tight, poisoned copies)
    (d_ab, c_ab), (d_ba, c_ba) = fm.search(qA.clone(), qB.clone(), 12, 2), fm.search(qB, qA, 12, 2)
    uv = (2 * torch.randn(2, H, W, generator=g)).to(dev)
    seeded, cand, ccur = fm.select(qA, qB, d_ab, c_ab, d_ba, uv, 12, 2, 0.9)
    s3, c3 = fm.propagate(qA.clone(), qB.clone(), seeded.clone(), cand.clone(), ccur.clone(), 2, 0.9, 3)
    out += [d_ab, c_ab, d_ba, c_ba, seeded, cand, ccur, s3, c3, fm.fuse(qA, qB, d_ab, c_ab, d_ba, uv, 12, 2, 0.9, 3)]
    tiny = torch.randint(0, 256, (2, 2, 3), generator=g, dtype=torch.uint8).to(dev)
    q = fm.quantise(tiny)
    out += list(fm.search(q, q.flip(0), 32, 3))
    return tuple(out)


CASE = guarded.Case('flowmatch', _run, NATIVES)
