"""The guarded case of the native scripts/isect_penalty.py reaches (tests/guarded.py): the same treatment the rows of
tests/guarded_cases.py give the natives launched from lasr_amd/, from a file of its own because that table names only the latter.
The module launches lasr_isectpen_forward itself and nothing else.  tests/test_isectpen_cpu.py holds the module's launch site
against NATIVES; tests/test_isectpen_gpu.py runs the case."""
import os
import sys

import torch

import guarded
import meshcheck_restated as mr
import meshnbr_restated as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVES = ('lasr_isectpen_forward',)


def isect_penalty():
    folder = os.path.join(ROOT, 'scripts')
    if folder not in sys.path:
        sys.path.insert(0, folder)
    import isect_penalty as ip
    return ip


def both(pen, verts, upstream=None):
    """-> (loss [N], gradient [N,V,3] of upstream . loss (default: ones), n_pairs [N], n_dropped [N])."""
    x = verts.clone().requires_grad_(True)
    loss = pen(x)
    w = torch.ones_like(loss) if upstream is None else torch.as_tensor(upstream, dtype=torch.float32, device=verts.device)
    grad, = torch.autograd.grad((loss * w).sum(), x)
    return (loss.detach(), grad) + tuple(pen.counts(verts))


def bad_faces(faces, V, outside_at=3, repeated_at=8):
    """The face list with an index V in row outside_at, -1 in the next row and a repeated index in row repeated_at."""
    faces = faces.clone()
    faces[outside_at, 1] = V
    faces[outside_at + 1, 2] = -1
    faces[repeated_at, 2] = faces[repeated_at, 0]
    return faces


def _run(dev):
    """pinch2 (320 faces: a full tile and one of 64), the three frames of two2 (640 faces, six tile pairs), the 257-face mesh (a
    one-face tile), batch3 under an upstream gradient, pinch2 with faces that name no vertex or one twice, and two faces alone."""
    ip = isect_penalty()
    out = []
    for name in ('pinch2', 'two2', 'tile257'):
        v, f = (torch.from_numpy(a).to(dev) for a in mr.fixture(name))
        out += list(both(ip.IsectPenalty(f), v))
    v, f = (torch.from_numpy(a).to(dev) for a in nr.fixture('batch3'))
    out += list(both(ip.IsectPenalty(f, n_verts=v.shape[1]), v, (1., 0.5, -2.)))
    v, f = (torch.from_numpy(a).to(dev) for a in mr.fixture('pinch2'))
    out += list(both(ip.IsectPenalty(bad_faces(f, v.shape[1])), v))
    pts = torch.tensor([[(0, 0, 0), (4, 0, 0), (0, 4, 0), (1, 1, -0.5), (1, 1, 2), (5, 5, 1)]], dtype=torch.float32).to(dev)
    out += list(both(ip.IsectPenalty(torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32).to(dev)), pts))
    return tuple(out)


CASE = guarded.Case('isectpen', _run, NATIVES)
