"""The chunk arithmetic of the pair-walk forward kernel (lasr_amd/csrc/sr_forward_pairs.h: chunk_count, chunk_size, chunk_pos),
restated in Python and checked for every list length a round can have, and the scenes of tests/test_pair_walk_chunk_deal_gpu.py
looked at on the CPU: a scene whose tile holds another number of entries than its name claims, or that renders background only,
would prove nothing about the deal."""
import math

import numpy as np
import pytest

from lasr_amd import synth
from test_pair_walk_chunk_deal_gpu import CASES, background, oracle_image

CAP = 64            # PW_CAP: list entries per chunk
LIST = 1024         # PW_LIST: list entries per round
TILE = 16           # PW_TILE


def chunk_count(count):
    return (count + CAP - 1) // CAP


def chunk_size(count, nch, c):
    return count // nch + (1 if c < count % nch else 0) if c < nch else 0


def chunk_pos(nch, c, l):
    return c + l * nch


def test_the_chunks_partition_the_list_for_every_count_a_round_can_have():
    for count in range(LIST + 1):
        _check_count(count)


def _check_count(count):
    nch = chunk_count(count)
    sizes = [chunk_size(count, nch, c) for c in range(nch)]
    chunks = [[chunk_pos(nch, c, l) for l in range(n)] for c, n in enumerate(sizes)]
    assert sorted(p for ch in chunks for p in ch) == list(range(count))                    # every position exactly once
    assert all(ch == sorted(ch) and len(set(ch)) == len(ch) for ch in chunks)              # ascending: face order within a chunk
    assert all(0 < n <= CAP for n in sizes) and (not sizes or max(sizes) - min(sizes) <= 1)
    assert nch == (0 if count == 0 else math.ceil(count / CAP))                            # no more chunks than consecutive ones
    for split in (1, 2):
        # team t takes the chunks t, t + split, ...; every team makes the same number of trips (they meet at the same barriers),
        # a trip past the last chunk has no entries, and together the teams' trips cover every chunk once
        trips = [[cb + t for cb in range(0, nch, split)] for t in range(split)]
        assert len({len(tr) for tr in trips}) == 1 and len(trips[0]) == -(-nch // split)
        assert sorted(c for tr in trips for c in tr if c < nch) == list(range(nch))
        assert all(chunk_size(count, nch, c) == 0 for tr in trips for c in tr if c >= nch)


def tile_entries(fv, IS):
    """Per frame and 16x16 tile, bounds on the number of list entries: [N, ty, tx] counts of the faces with a pixel centre of the tile
    inside them or within the distance threshold (the list is conservative: these are in it), and of the faces whose bounding box,
    widened by the threshold radius and a pixel, meets the tile's pixel centres (no other face can be)."""
    m = synth.LASR_MODES
    thr = math.log(1. / m['dist_eps'] - 1.) * m['sigma_val']
    r = math.sqrt(thr)
    c = (2 * np.arange(IS) + 1 - IS) / IS
    X, Y = np.meshgrid(c, c[::-1])
    nt = (IS + TILE - 1) // TILE
    lo = np.zeros((fv.shape[0], nt, nt), np.int64)
    hi = np.zeros_like(lo)
    for n in range(fv.shape[0]):
        for t in fv[n].astype(np.float64):
            x, y = t[:, 0], t[:, 1]
            if not (np.isfinite(t).all() and np.abs(t[:, :2]).max() < 1e3):
                box = np.ones((IS, IS), bool)           # (huge coordinates: anywhere, for the upper bound only)
                hit = np.zeros((IS, IS), bool)
            else:
                pad = r + 2. / IS
                box = (X >= x.min() - pad) & (X <= x.max() + pad) & (Y >= y.min() - pad) & (Y <= y.max() + pad)
                a, b, d = t[0, :2], t[1, :2], t[2, :2]
                best = np.full((IS, IS), np.inf)
                sign = []
                for p, q in ((a, b), (b, d), (d, a)):
                    e = q - p
                    s = np.clip(((X - p[0]) * e[0] + (Y - p[1]) * e[1]) / max(e @ e, 1e-300), 0, 1)
                    best = np.minimum(best, (p[0] + s * e[0] - X) ** 2 + (p[1] + s * e[1] - Y) ** 2)
                    sign.append(e[0] * (Y - p[1]) - e[1] * (X - p[0]))
                inside = ((sign[0] > 0) & (sign[1] > 0) & (sign[2] > 0)) | ((sign[0] < 0) & (sign[1] < 0) & (sign[2] < 0))
                hit = inside | (best < 0.9 * thr)
            for ty in range(nt):
                for tx in range(nt):
                    sl = (slice(ty * TILE, (ty + 1) * TILE), slice(tx * TILE, (tx + 1) * TILE))
                    lo[n, ty, tx] += hit[sl].any()
                    hi[n, ty, tx] += box[sl].any()
    return lo, hi


# what each scene is there for: (chunk sizes of its fullest tile, exactly) or a lower bound on that tile's entries
EXACT = {'stack of 65': [33, 32], 'stack of 128': [64, 64], 'stack of 129': [43, 43, 43], 'stack of 130': [44, 43, 43]}
AT_LEAST = {'crowded 16': 65, 'ragged 20': 65, 'ragged 33': 65, 'tame and not tame': 65, 'six channels': 65, 'nine channels': 65,
            'three frames': 65, 'eight frames': 65, 'long list': LIST - 256 + 1}


def test_every_scene_states_what_it_is_for():
    assert set(EXACT) | set(AT_LEAST) == set(CASES) and not set(EXACT) & set(AT_LEAST)


@pytest.mark.parametrize('name', list(CASES))
def test_the_scene_fills_its_tile_as_claimed_and_is_not_background_only(oracle, name):
    build, IS, _ = CASES[name]
    fv, ft, near, far = build()
    C = ft.shape[-1]
    lo, hi = tile_entries(fv, IS)
    if name in EXACT:
        assert lo.shape == (1, 1, 1) and lo[0, 0, 0] == hi[0, 0, 0] == fv.shape[1] == sum(EXACT[name])
        count = int(lo[0, 0, 0])
        nch = chunk_count(count)
        assert [chunk_size(count, nch, c) for c in range(nch)] == EXACT[name]
    else:
        # more than one chunk in some tile (for the long list: more entries than the kernel gathers before it walks a round),
        # and no multiple of 64 can be told from the bounds alone -- ragged chunk sizes are the common case, not the claim
        assert lo.max() >= AT_LEAST[name], (name, int(lo.max()))
    img = oracle_image(oracle, name)
    assert img.shape == (fv.shape[0], C + 1, IS, IS) and np.isfinite(img).all()
    bg = np.asarray(background(C), np.float32)[None, :, None, None]
    assert img[:, C].max() > 1e-2 and img[:, C].min() < 0.5                     # alpha: something drawn, something left free
    assert (np.abs(img[:, :C] - bg).max(1) > 1e-3).sum() >= 4
