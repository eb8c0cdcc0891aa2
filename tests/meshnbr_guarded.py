"""The guarded case of the natives scripts/shape_neighbours.py reaches (tests/guarded.py): the same treatment the rows of
tests/guarded_cases.py give the natives launched from lasr_amd/, from a file of its own because that table names only the latter.
The module launches lasr_meshnbr_list and lasr_meshnbr_test itself and reaches lasr_meshcheck_faces through
lasr_amd/nnutils/meshcheck.py, whose records the test pass reads.  tests/test_meshnbr_cpu.py holds the module's launch sites against
NATIVES; tests/test_meshnbr_gpu.py runs the case."""
import os
import sys

import torch

import guarded
import meshnbr_restated as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHED = ('lasr_meshnbr_list', 'lasr_meshnbr_test')                              # by the module's own call sites
NATIVES = LAUNCHED + ('lasr_meshcheck_faces',)


def shape_neighbours():
    folder = os.path.join(ROOT, 'scripts')
    if folder not in sys.path:
        sys.path.insert(0, folder)
    import shape_neighbours as sn
    return sn


def _sorted_hits(res, max_pairs):
    """The hit lists as sorted keys, zero past each frame's end: the order the lanes arrive in is not defined."""
    h = res['hits'].long()
    n = (res['n_pierced'] + res['n_creased']).clamp(max=max_pairs)
    key = (h[..., 0] << 32) | (h[..., 1] << 8) | h[..., 2]
    key = torch.where(torch.arange(h.shape[1], device=h.device)[None] < n[:, None], key, torch.full_like(key, 1 << 62))
    key = torch.sort(key, 1)[0]
    return torch.where(key == 1 << 62, torch.zeros_like(key), key)


def _run(dev):
    """The three frames on the topology of 320 faces (clean, two creased pairs, two pierced and three creased), the list of it made
    with room and made again after an overflow, a hit list too short for its frame, the 257-face mesh (a one-face tile), a mesh with a
    reversed face, and one face alone."""
    sn = shape_neighbours()
    out = []
    verts, faces = (torch.from_numpy(a).to(dev) for a in nr.fixture('batch3'))
    keys, counts = sn.neighbour_list(faces)
    short, _ = sn.neighbour_list(faces.clone(), capacity=8)
    out += [keys, short] + [counts[k].reshape(1) for k in sorted(counts)]
    for v, f, mp in ((verts, faces, 16), (verts[2:].clone(), faces.clone(), 3)) + tuple(
            tuple(torch.from_numpy(a).to(dev) for a in nr.fixture(name)) + (5,) for name in ('tile257', 'flip1')):
        res = sn.neighbour_tests(v, f, 20., mp)
        out += [res['n_pierced'], res['n_creased'], res['nbr_count'], res['min_cos']]
        if mp != 3:                                                                # (which three of five hits a short list keeps is not defined)
            out.append(_sorted_hits(res, mp))
    one = sn.neighbour_tests(verts[:1, :3].clone(), torch.tensor([[0, 1, 2]], dtype=torch.int32).to(dev))
    out += [one['n_pierced'], one['nbr_count']]
    return tuple(out)


CASE = guarded.Case('meshnbr', _run, NATIVES)
