"""Two pieces of integer bookkeeping in the backward raster's prologue (lasr_amd/csrc/sr_backward.h), checked on the CPU alone.

The (image, face) split of a wave: bn = gw / F runs as a multiplication by a host-prepared multiplier and a shift (sr_common.h:
face_div).  lasr_selftest_face_div evaluates exactly that function with the multiplier make_args puts into the kernel's arguments; it
must equal Python's // wherever a quotient can change: gw = q F - 1, q F, q F + 1 for EVERY q up to the largest wave index the
entry points accept, (2^31 - 1) / 64 (check_common), for each F below.  For F = 1, 2, 3 that is every gw.

The LDS extension of the distance code (sr_device.h: euclid_one_ext): which record word lane L copies comes from the static table
k_bwd_ext_tbl instead of per-lane index arithmetic.  The table is read out of the header, decoded as bwd_ext_word_tbl decodes it, and
held against the layout restated below, for all 64 lanes and the three obtuse corners.
"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF_MAX = 0x7fffffff // 64                       # check_common: N * F <= (2^31 - 1) / 64
F_CASES = [1, 2, 3, 64, 1280, 2420, 2560, 65535]


def face_div(F, gw):
    from lasr_amd import _lib
    h = _lib.lib()
    gw = np.ascontiguousarray(gw, np.int32)
    out = np.full(gw.shape, -7, np.int32)
    assert h.lasr_selftest_face_div(int(F), gw.ctypes.data_as(ctypes.c_void_p), int(gw.size), out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out


def boundaries(F):
    """Every gw in [0, NF_MAX] within one of a multiple of F, ascending."""
    if F <= 3:
        return np.arange(NF_MAX + 1, dtype=np.int64)
    q = np.arange(NF_MAX // F + 2, dtype=np.int64) * F
    g = np.unique(np.concatenate([q - 1, q, q + 1, [NF_MAX]]))
    return g[(g >= 0) & (g <= NF_MAX)]


@pytest.mark.parametrize('F', F_CASES)
def test_magic_multiplier_division_equals_floor_division_on_every_boundary(F):
    g = boundaries(F)
    assert g[0] == 0 and g[-1] == NF_MAX and (F > 3 or g.size == NF_MAX + 1)
    for i in range(0, g.size, 1 << 22):
        part = g[i:i + (1 << 22)]
        got = face_div(F, part)
        want = part // F
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, 'F = %d: gw = %d gives %d, // gives %d' % (F, part[bad[0]], got[bad[0]], want[bad[0]])


def test_face_div_rejects_what_the_entry_points_reject():
    from lasr_amd import _lib
    h = _lib.lib()
    g, o = np.array([NF_MAX + 1], np.int32), np.zeros(1, np.int32)
    assert h.lasr_selftest_face_div(3, g.ctypes.data_as(ctypes.c_void_p), 1, o.ctypes.data_as(ctypes.c_void_p)) == -1
    g[0] = 5
    assert h.lasr_selftest_face_div(0, g.ctypes.data_as(ctypes.c_void_p), 1, o.ctypes.data_as(ctypes.c_void_p)) == -1


# ---- the lane table

def header():
    return open(os.path.join(ROOT, 'lasr_amd', 'csrc', 'sr_device.h')).read()


def constant(name):
    m = re.search(r'\b%s\s*=\s*(0x[0-9a-fA-F]+|\d+)' % name, header())
    assert m, name
    return int(m.group(1), 0)


def table():
    m = re.search(r'k_bwd_ext_tbl\[BX\]\s*=\s*\{(.*?)\};', header(), re.S)
    assert m
    return [int(v, 0) for v in re.findall(r'0x[0-9a-fA-F]+|\d+', m.group(1))]


def formula(L, c):
    """The extension's layout (sr_device.h: euclid_one_ext, bwd_ext_formula) for lane L of a face whose obtuse corner is c: (record word a, record word b or None when the value
    is a alone and a - b otherwise, constant or None)."""
    R_E, R_IDEN, R_FACE, BX_OBT = constant('R_E'), constant('R_IDEN'), constant('R_FACE'), constant('BX_OBT')
    k, i = L >> 4, L & 15
    o = 2 if c == 0 else c - 1
    obt = BX_OBT <= L < BX_OBT + 4
    ia = R_E + 3 * k + i if i < 3 else ((R_E + 6 if k == 2 else R_E + 4 * k + 1) if i == 3 else R_IDEN + k)
    if obt:
        ia = R_FACE + 3 * (o if L & 2 else c) + (L & 1)
    ib = R_FACE + 3 * c + (L & 1)
    kb = 0 if k == 2 else k + 1
    cst = None
    if 5 <= i < 8:
        cst = 1. if i - 5 == k else 0.
    if 8 <= i < 11:
        cst = 1. if i - 8 == kb else 0.
    return ia, (ib if obt and (L & 2) else None), cst


def decode(t, L, c):
    """bwd_ext_word_tbl (sr_device.h) for table entry t."""
    ONE, ZERO, C, O, R_FACE = constant('BXT_ONE'), constant('BXT_ZERO'), constant('BXT_C'), constant('BXT_O'), constant('R_FACE')
    o = 2 if c == 0 else c - 1
    cb, ob = R_FACE + 3 * c, R_FACE + 3 * o
    ia = (t & 63) + (ob if t & O else cb if t & C else 0)
    cst = 0. if t & ZERO else 1. if t & ONE else None
    return ia, (cb + (L & 1) if t & O else None), cst


def test_the_table_holds_one_entry_per_lane_and_only_known_bits():
    T = table()
    assert len(T) == constant('BX') == 64
    known = 63 | constant('BXT_ONE') | constant('BXT_ZERO') | constant('BXT_C') | constant('BXT_O')
    assert all(0 <= t <= known and (t & ~known) == 0 for t in T)
    assert {constant('BXT_ONE'), constant('BXT_ZERO'), constant('BXT_C'), constant('BXT_O')} == {0x40, 0x80, 0x100, 0x200}


@pytest.mark.parametrize('c', [0, 1, 2])
def test_the_lane_table_selects_the_words_of_the_index_formula(c):
    T = table()
    REC = constant('REC')
    for L in range(64):
        ia, ib, cst = formula(L, c)
        ja, jb, jcst = decode(T[L], L, c)
        assert 0 <= ja < REC and (jb is None or 0 <= jb < REC), (L, c)          # every load stays inside the record
        assert cst == jcst, 'lane %d, corner %d: constant %r, table %r' % (L, c, cst, jcst)
        if cst is None:
            assert (ia, ib) == (ja, jb), 'lane %d, corner %d: words %r, table %r' % (L, c, (ia, ib), (ja, jb))


def test_the_formula_restated_here_names_the_layout_the_kernel_reads():
    # euclid_one_ext's layout: block k at 16 k holds e[k][0..2], e[k][(k+1)%3], 1 / den[k], the 0 / 1 factors of t[k] = ta and of
    # t[(k+1)%3] = tb; words 12..15 hold x_c, y_c, x_o - x_c, y_o - y_c
    R_E, R_IDEN, R_FACE = constant('R_E'), constant('R_IDEN'), constant('R_FACE')
    for k in range(3):
        b = (k + 1) % 3
        assert [formula(16 * k + i, 1)[0] for i in range(5)] == [R_E + 3 * k, R_E + 3 * k + 1, R_E + 3 * k + 2, R_E + 3 * k + b, R_IDEN + k]
        assert [formula(16 * k + 5 + j, 1)[2] for j in range(3)] == [1. if j == k else 0. for j in range(3)]
        assert [formula(16 * k + 8 + j, 1)[2] for j in range(3)] == [1. if j == b else 0. for j in range(3)]
    for c in range(3):
        o = (c + 2) % 3
        assert [formula(12 + j, c)[:2] for j in range(4)] == [(R_FACE + 3 * c, None), (R_FACE + 3 * c + 1, None),
                                                              (R_FACE + 3 * o, R_FACE + 3 * c), (R_FACE + 3 * o + 1, R_FACE + 3 * c + 1)]


# ---- the mesh of tests/test_face_constants_gpu.py holds the cases its docstring names (float64 on the fp32 vertices)

from test_face_constants_gpu import N_FACES, SIGMAS, SIZES, mesh       # noqa: E402

NEAR_TIE, NEAR_TIE_ABS = 0.985, 2.4e-6          # sr_device.h


def face_facts(t):
    x, y = t[:, 0].astype(np.float64), t[:, 1].astype(np.float64)
    det = x[2] * (y[0] - y[1]) + x[0] * (y[1] - y[2]) + x[1] * (y[2] - y[0])
    obtuse = -1
    hk2, well = [], True
    for k in range(3):
        b, c = (k + 1) % 3, (k + 2) % 3
        if obtuse < 0 and (x[b] - x[k]) * (x[c] - x[k]) + (y[b] - y[k]) * (y[c] - y[k]) < 0:
            obtuse = k
        l2 = (x[c] - x[b]) ** 2 + (y[c] - y[b]) ** 2
        hk2.append(det * det / l2)
        well = well and 1e-4 < hk2[-1] < 1e4 and l2 < 16.
    return det, obtuse, hk2, well


def barycentrics(t, IS):
    x, y = t[:, 0].astype(np.float64), t[:, 1].astype(np.float64)
    det = face_facts(t)[0]
    c = (2 * np.arange(IS) + 1 - IS) / IS
    X, Y = np.meshgrid(c, c[::-1])
    adj = np.array([[y[1] - y[2], x[2] - x[1], x[1] * y[2] - x[2] * y[1]],
                    [y[2] - y[0], x[0] - x[2], x[2] * y[0] - x[0] * y[2]],
                    [y[0] - y[1], x[1] - x[0], x[0] * y[1] - x[1] * y[0]]]) / det
    return [adj[k, 0] * X + adj[k, 1] * Y + adj[k, 2] for k in range(3)], X, Y


@pytest.mark.parametrize('IS', SIZES)
def test_the_mesh_holds_every_case(IS):
    fv = mesh(IS)
    assert fv.shape == (2, N_FACES, 3, 3)
    thr = max(SIGMAS) * np.log(1. / 1e-4 - 1.)
    ties = []
    for frame in fv:
        facts = [face_facts(t) for t in frame]
        assert [f[1] for f in facts[1:4]] == [0, 1, 2] and all(f[3] for f in facts[1:4])                  # one face per obtuse corner
        assert not facts[4][3] and all(f[3] for i, f in enumerate(facts) if i != 4)                       # the sliver alone lacks flag 16
        assert frame[5, :, 0].min() - np.sqrt(thr) > 1.                                                  # beyond the last pixel centre: empty rect
        # face 0: an inside pixel within the near-tie margin of a bisector, but not ON it (2e-4 NDC is far outside fp32 rounding)
        w, X, Y = barycentrics(frame[0], IS)
        hk2 = facts[0][2]
        inside = (np.minimum(np.minimum(w[0], w[1]), w[2]) > 0) & (np.maximum(np.maximum(w[0], w[1]), w[2]) < 1)
        q = np.sort(np.stack([w[2] ** 2 * hk2[2], w[0] ** 2 * hk2[0], w[1] ** 2 * hk2[1]]), 0)
        tie = inside & (~(q[0] < NEAR_TIE * q[1]) | ~((q[1] - q[0]) ** 2 > 4. * NEAR_TIE_ABS ** 2 / min(hk2) * q[1]))
        ties.append(int(tie.sum()))
        assert not tie.any() or (q[1] - q[0])[tie].min() > 1e-6 * q[1][tie].max()
        # ... and it reaches all four 16 x 16 tiles (inside pixels in each)
        rows, cols = np.nonzero(inside)
        assert {(r // 16, c // 16) for r, c in zip(rows, cols)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert all(np.all((t[:, 2] > 1.5) & (t[:, 2] < 4.5)) for t in frame)
    assert ties[0] >= 3                 # (the second frame is the first moved by a fifth of a pixel: its axis lies between columns)
