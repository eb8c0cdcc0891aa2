"""lasr_sr_workspace_bytes comes from the one workspace layout of the raster launcher (lasr_amd/csrc/sr_raster.hip: sr_layout), which
also places the records, rects, choice word and tile-order table of every call.  tests/golden/sr_workspace_bytes.npz holds the
sizes the library returned before that layout existed, for 917 (N, F, T, IS) -- F % 64 in {0, 1, 63}, IS % 8 in {0, 1, 7}, IS = 0 (the
backward's records-only size), N = 0, F = 0 and negative sizes (which return 0): callers size their buffers with it, so it must
not move by a byte."""
import os

import numpy as np

from lasr_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sr_workspace_bytes.npz')


def test_workspace_bytes_are_what_they_were_for_every_recorded_size():
    d = np.load(GOLDEN)
    args, want = d['args'], d['bytes']
    assert len(args) >= 200 and args.shape == (len(want), 4)
    N, F, IS = args[:, 0], args[:, 1], args[:, 3]
    for r in (0, 1, 63):
        assert ((F % 64 == r) & (F > 0)).any()
    for r in (0, 1, 7):
        assert ((IS % 8 == r) & (IS > 0)).any()
    assert (IS == 0).any() and (N == 0).any() and (F == 0).any() and (N < 0).any() and (F < 0).any()
    h = _lib.lib()
    got = np.array([h.lasr_sr_workspace_bytes(*map(int, a)) for a in args], dtype=np.int64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(args[i].tolist(), int(want[i]), int(got[i])) for i in bad[:5]]
    assert (want[(N < 0) | (F < 0)] == 0).all()
