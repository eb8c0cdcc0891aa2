"""The guarded case of the natives scripts/fold_penalty.py reaches (tests/guarded.py): the same treatment the rows of
tests/guarded_cases.py give the natives launched from lasr_amd/, from a file of its own because that table names only the latter.
The module launches lasr_foldpen_forward and lasr_foldpen_backward itself and reaches lasr_meshnbr_list through
scripts/shape_neighbours.py, whose sorted keys it walks.  tests/test_foldpen_cpu.py holds the module's launch sites against NATIVES;
tests/test_foldpen_gpu.py runs the case."""
import os
import sys

import torch

import guarded
import meshnbr_restated as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHED = ('lasr_foldpen_forward', 'lasr_foldpen_backward')                       # by the module's own call sites
NATIVES = LAUNCHED + ('lasr_meshnbr_list',)


def fold_penalty():
    folder = os.path.join(ROOT, 'scripts')
    if folder not in sys.path:
        sys.path.insert(0, folder)
    import fold_penalty as fp
    return fp


def bad_keys(keys, F, face_at=7, corner_at=11):
    """The list with a key that names face F in place of its entry face_at, and one with the corner code 3 in place of entry
    corner_at."""
    keys = keys.clone()
    keys[face_at] = (keys[face_at] & 0xffffffff) | (F << 32)
    keys[corner_at] = keys[corner_at] | 3
    return keys


def both(pen, verts, upstream=(1., 1.)):
    """-> (loss [N,2], values [N,n], gradient [N,V,3] of upstream . loss summed over the meshes)."""
    x = verts.clone().requires_grad_(True)
    loss = pen(x)
    w = torch.tensor(upstream, dtype=torch.float32, device=verts.device)
    grad, = torch.autograd.grad((loss * w).sum(), x)
    return loss.detach(), pen.entries(verts)[1], grad


def _run(dev):
    """The three frames on the topology of 320 faces (1890 entries: no multiple of 64 or 256), its folded frame alone, the 257-face
    mesh, a mesh with a reversed face, a list with a key that names no face, and one face alone: values and gradients."""
    fp = fold_penalty()
    out = []
    verts, faces = (torch.from_numpy(a).to(dev) for a in nr.fixture('batch3'))
    pen = fp.FoldPenalty(faces, 30.)
    out += list(both(pen, verts, (1., 0.5)))
    out += list(both(pen, verts[2:].clone()))
    for name in ('tile257', 'flip1'):
        v, f = (torch.from_numpy(a).to(dev) for a in nr.fixture(name))
        out += list(both(fp.FoldPenalty(f, 90.), v))
    out += list(both(fp.FoldPenalty(faces, 30., keys=bad_keys(pen.keys, faces.shape[0])), verts))
    one = fp.FoldPenalty(torch.tensor([[0, 1, 2]], dtype=torch.int32).to(dev), 30., n_verts=3)
    out += list(both(one, verts[:1, :3].clone()))
    return tuple(out)


CASE = guarded.Case('foldpen', _run, NATIVES)
