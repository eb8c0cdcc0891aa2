"""The shapes of tests/test_dispatch_variants_gpu.py, looked at on the CPU alone.

  1. The meshes and point sets built there have the properties their tests rely on: the valences of the gather mesh, the chunk every
     duplicate face falls in, the sub-range every duplicate target falls in, dummy bones whose logit is below the underflow point.
  2. The thresholds the shapes were chosen for are where they were: every entry of PINS is a piece of source text that must be
     present in the named file.  Whoever moves a threshold sees this test fail and moves the shapes with it.
  3. Every float64 reference against its own float32 run at the new shapes.  The gaps are printed, and the bar each GPU test applies
     is held against the rule in the docstring of tests/test_dispatch_variants_gpu.py: never below the operator's existing bar, and
     above it only where the gap exceeds a quarter of it, then 16 x gap (a stricter bar than the rule gives is always allowed; the
     gap may come out up to a quarter larger on another CPU before this complains).
"""
import os

import numpy as np
import pytest
import torch

import test_dispatch_variants_gpu as dv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join('lasr_amd', 'csrc')


# ---- 1. the shapes have the properties claimed ----------------------------------------------------------------------------------
def test_dummy_bones_lie_below_the_underflow_point():
    # float32 expf(x) is 0 below x = -104; the issue asks for logits below -1e4.  The logits of the real bones stay above -1e3,
    # so logit - max is below -1e4 + 1e3 for every dummy bone at every vertex.
    ts, rs, lc, verts, _ = dv.skin_inputs(24)
    fts, frs, flc = dv.skin_far_bones(17)
    from oracle import path_oracle as po
    H = dv.SKIN_H

    def logits(t, r, l):
        d = t.double().view(H, -1, 1, 3) - verts.double()[:, None]
        d = d.matmul(po.quaternion_to_rotation_matrix(r.double()).view(H, -1, 3, 3))
        return -10 * (l.double().exp().view(H, -1, 1, 3) * d.pow(2)).sum(3)
    real, far = logits(ts, rs, lc), logits(fts, frs, flc)
    print('real logits: max over bones in [%.1f, %.1f]; dummy logits <= %.3g' % (real.max(1)[0].min(), real.max(1)[0].max(), far.max()))
    assert float(far.max()) < -1e7 and float(real.max(1)[0].min()) > -1e3
    w = torch.cat([real, far], 1).float().softmax(1)
    assert float(w[:, 24:].abs().max()) == 0.0


def test_gather_mesh_has_the_valences_on_the_cap_and_on_the_block_boundaries():
    f = dv.gather_mesh()
    assert f.min() >= 0 and f.max() < dv.GATHER_V
    val = np.bincount(f.reshape(-1), minlength=dv.GATHER_V)
    assert {v: int(val[v]) for v in dv.GATHER_HUBS} == {0: 30, 63: 31, 64: 37, 255: 30, 256: 31}
    assert val[dv.GATHER_ISOLATED] == 0
    others = np.delete(val, list(dv.GATHER_HUBS))
    assert others.max() <= 5                                           # nothing else comes near the cap
    # block boundaries of both variants: 63 | 64 (64 vertices per block), 255 | 256 (256 per block; also a boundary of the 64s)
    assert 63 // 64 != 64 // 64 and 255 // 256 != 256 // 256 and 255 // 64 != 256 // 64
    # a hub's corners are scattered over the corner list (the kernels sort them): not ascending as filed
    corners = np.nonzero(f.reshape(-1) == 64)[0]
    assert len(corners) == 37 and corners.max() - corners.min() > len(f)
    # closed part: every edge of the tetrahedron is shared by two of its faces
    tet = f[np.isin(f, [1, 2, 3, 4]).all(1)]
    edges = np.sort(np.concatenate([tet[:, [0, 1]], tet[:, [1, 2]], tet[:, [2, 0]]]), 1)
    assert len(tet) == 4 and (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()
    # the launch-size threshold
    blocks = (dv.GATHER_V + 63) // 64
    assert blocks == 5 and dv.gather_big_n() == dv.GATHER_BIG_N == 410 and 409 * blocks < 2048 <= 410 * blocks


@pytest.mark.parametrize('Q', dv.NEAREST_TIE_Q)
def test_nearest_point_tie_sets_put_duplicates_into_different_sub_ranges(Q):
    a, b = dv.nearest_tie_sets(Q)
    per = (Q + 15) // 16
    sub = np.arange(Q) // per
    for k in range(per):
        for s in (1, 3, 7, 15):
            if k + per * s < Q:
                assert sub[k + per * s] == s != sub[k] and np.array_equal(b[:, k + per * s], b[:, k])
    d = ((a[:, :, None].astype(np.int64) - b[:, None].astype(np.int64)) ** 2).sum(-1)
    assert d.max() < 2 ** 24 and np.array_equal(a, np.round(a)) and np.array_equal(b, np.round(b))   # exact in float32
    mins = d == d.min(2, keepdims=True)
    across = np.array([[len(set(sub[m])) for m in row] for row in mins])
    inside = np.array([[np.bincount(sub[m]).max() for m in row] for row in mins])
    print('Q = %d: queries whose minimum lies in several sub-ranges: %d of %d; several times in one: %d'
          % (Q, (across > 1).sum(), across.size, (inside > 1).sum()))
    assert (across > 1).mean() > 0.5 and (inside > 1).sum() > 0
    # the winner is not always in the first sub-range, and the highest index among the equals is another one
    first, last = d.argmin(2), Q - 1 - d[:, :, ::-1].argmin(2)
    assert (sub[first] > 0).any() and (first != last).mean() > 0.5


def test_nearest_point_sizes_leave_sub_ranges_empty():
    for P, Q in dv.NEAREST_SIZES:
        per = (Q + 15) // 16
        live = sum(1 for s in range(16) if s * per < Q)
        assert (live < 16) == (Q not in (16, 31)), (Q, live)
    assert [(Q + 15) // 16 for _, Q in dv.NEAREST_SIZES] == [1, 1, 1, 2, 2]


def test_point_mesh_shapes_straddle_the_chunk_size_step():
    assert [dv.pmf_tile(F) for F in dv.PMF_F] == [32, 64, 64]
    chunks = [-(-F // dv.pmf_tile(F)) for F in dv.PMF_F]
    assert chunks == [64, 33, 33]
    assert [F - (c - 1) * dv.pmf_tile(F) for F, c in zip(dv.PMF_F, chunks)] == [32, 1, 32]           # faces in the last chunk: ragged twice
    assert [(P + 255) // 256 for P in dv.PMF_P] == [1, 2]                                           # one block of points, two blocks
    for F in dv.PMF_F:
        verts, faces, pts = dv.pmf_mesh(F, 257)
        assert faces.shape == (F, 3) and int(faces.max()) < verts.shape[1] and pts.shape == (2, 257, 3)
        tri = verts[0][faces].double()
        area = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=1)
        assert float(area.min()) > 1e-5                                                             # no degenerate triangle


def test_point_mesh_tie_case_has_its_duplicates_in_the_first_and_the_last_chunk():
    verts, faces, pts, near_face, near_point = dv.pmf_tie_case()
    F, T, P0 = dv.PMF_TIE_F, dv.PMF_TIE_T, dv.PMF_TIE_P0
    FT = dv.pmf_tile(F)
    assert faces.shape == (F, 3) and pts.shape == (1, 2 * P0, 3) and FT == 64
    assert np.array_equal(faces[:T], faces[F - T:])
    chunk = np.arange(F) // FT
    assert (chunk[:T] == 0).all() and (chunk[F - T:] == chunk[-1]).all() and chunk[-1] == 32 and F - 32 * FT == 32
    assert np.array_equal(pts[0, :P0], pts[0, P0:])
    block = np.arange(2 * P0) // 256
    assert (block[:T] == 0).all() and (block[P0:P0 + T] == 1).all()      # a base triangle's nearest point and its copy: two blocks
    # float64 distances (plane distance inside the prism, nearest edge outside): the nearest face of every point is its base
    # triangle, in both copies and in nothing else by a margin; the restatement's loss is the sum of these minima
    from oracle import path_oracle as po
    v, p = torch.from_numpy(verts).double(), torch.from_numpy(pts).double()
    tri = v[0][torch.from_numpy(faces)]
    d = torch.stack([_point_triangle_d2(p[0], tri[f]) for f in range(F)], 1).numpy()                 # [2 P0, F]
    assert np.array_equal(d.argmin(1), near_face)
    assert np.array_equal(d[:, :T], d[:, F - T:])
    srt = np.sort(d, 1)
    assert (srt[:, 0] == srt[:, 1]).all() and (srt[:, 2] > srt[:, 0] + 1.0).all()                   # exactly the two copies, nothing near
    assert np.array_equal(d[:, :T].argmin(0), near_point[:T])
    col = np.sort(d[:, :T], 0)
    assert (col[0] == col[1]).all() and (col[2] > col[0] * 1.2).all()
    assert abs(float(po.point_mesh_face_distance(v, torch.from_numpy(faces), p))
               - (d.min(1).mean() + d.min(0).mean())) < 1e-9 * d.min(0).mean()


def _point_triangle_d2(p, tri):
    """Squared distance of points p [n,3] to one triangle [3,3] (float64): inside the prism the plane distance, else the nearest edge."""
    a, b, c = tri
    n = torch.linalg.cross(b - a, c - a)
    n = n / n.norm()
    q = p - ((p - a) @ n)[:, None] * n
    inside = torch.ones(len(p), dtype=torch.bool)
    for u, w in ((a, b), (b, c), (c, a)):
        inside &= (torch.linalg.cross((w - u).expand_as(q), q - u) @ n) >= 0
    best = torch.full((len(p),), float('inf'), dtype=p.dtype)
    for u, w in ((a, b), (b, c), (c, a)):
        t = (((p - u) @ (w - u)) / ((w - u) @ (w - u))).clamp(0, 1)
        best = torch.minimum(best, (p - (u + t[:, None] * (w - u))).pow(2).sum(1))
    return torch.where(inside, ((p - a) @ n).pow(2), best)


def test_lbs_shapes_sit_on_the_kernel_choice_and_the_padding():
    ks = sorted({K for K, _ in dv.LBS_CASES})
    assert ks == [17, 18, 64, 65, 66]
    assert [(K - 1 + 15) & ~15 for K in ks] == [16, 32, 64, 64, 80]      # bones padded to 16s: 16 | 17 and 63, 64 in one tile row
    assert [K <= 65 for K in ks] == [True, True, True, True, False]
    assert sorted({-(-V // 64) for K, V in dv.LBS_CASES if K <= 65}) == [1, 2]
    assert sorted({-(-V // 256) for K, V in dv.LBS_CASES if K > 65}) == [1, 2]


def test_render_table_and_loss_table_shapes_sit_on_the_chunk_boundaries():
    assert dv.rt_chunks(48 * 48) == (2, 1152) and dv.rt_chunks(47 * 47) == (2, 1105) and (47 * 47) % 4 == 1
    assert [dv.rt_chunks(S * S)[0] for S in dv.LOSS_S] == [1, 2, 2]       # the loss tables split like the render tables (pinned below)
    assert [S * S for S in dv.LOSS_S] == [2025, 2116, 4096] and dv.rt_chunks(4096) == (2, 2048)


# ---- 2. the thresholds are where the shapes expect them -------------------------------------------------------------------------
PINS = [
    ('fused.hip', 'constexpr int SKIN_MAX_BONES = 64;'),
    ('fused.hip', '    if (H < 0 || J < 0 || V < 0 || J > SKIN_MAX_BONES) return LASR_E_BADARG;'),
    ('fused.hip', '    if (J <= 24)      LASR_LAUNCH(K_SKIN_FORWARD, skin_forward_kernel<24>, grid, dim3(64), 0,'),
    ('fused.hip', '    else if (J <= 40) LASR_LAUNCH(K_SKIN_FORWARD, skin_forward_kernel<40>, grid, dim3(64), 0,'),
    ('fused.hip', '    else              LASR_LAUNCH(K_SKIN_FORWARD, skin_forward_kernel<0>, grid, dim3(64), 0,'),
    ('fused.hip', 'constexpr int COS_TP = 32;'),
    ('fused.hip', 'constexpr int COS_CG = 8;'),
    ('fused.hip', '    switch (C % COS_CG == 0 ? C / COS_CG : 0) {         // AlexNet: 64, 192, 384, 256, 256 channels\n'
                  '        case 8:  LASR_COS_BWD(8); break;\n'
                  '        case 24: LASR_COS_BWD(24); break;\n'
                  '        case 32: LASR_COS_BWD(32); break;\n'
                  '        case 48: LASR_COS_BWD(48); break;\n'
                  '        default: LASR_COS_BWD(0);\n'),
    ('fused.hip', 'constexpr int GATHER_CAP = 30;'),
    ('fused.hip', '        if (m <= GATHER_CAP) {'),
    ('fused.hip', '    if ((long long)N * ((V + 63) / 64) >= 2048) {'),
    ('fused.hip', 'face_gather_backward_kernel<256>, dim3((V + 255) / 256, N), dim3(256)'),
    ('fused.hip', '(face_gather_backward_kernel<64, 1024>), dim3((V + 63) / 64, N), dim3(1024)'),
    ('fused.hip', '    const int per = (Q + 15) >> 4, q0 = sub * per, q1 = min(Q, q0 + per);'),
    ('fused.hip', '        if (ob < best || (ob == best && oa < arg)) { best = ob; arg = oa; }'),
    ('fused.hip', 'nearest_point_kernel, dim3((P + 15) / 16, N), dim3(256)'),
    ('fused.hip', '__host__ __device__ inline int pmf_tile(int n) { int t = 32; while ((n + t - 1) / t > 64) t *= 2; return t; }'),
    ('fused.hip', '    FT = pmf_tile(F); PT = 256;'),
    ('fused.hip', '            if (d[u] < best) { best = d[u]; barg = a[u]; }'),
    ('ops.hip', 'constexpr int LBS_CHUNK = 256;'),
    ('ops.hip', 'constexpr int LBSB_VERTS = 64;'),
    ('ops.hip', 'constexpr int LBSB_MAX_K = 65;'),
    ('ops.hip', '    if (K <= LBSB_MAX_K) {'),
    ('ops.hip', '        const int nbp = (K - 1 + 15) & ~15;'),
    ('ops.hip', 'constexpr int LOSS_PX_PER_BLOCK = 2048;'),
    ('ops.hip', '__host__ __device__ inline int loss_nch(int P) { int n = (P + LOSS_PX_PER_BLOCK - 1) / LOSS_PX_PER_BLOCK; '
                'return n < 1 ? 1 : (n > 64 ? 64 : n); }'),
    ('post_raster.hip', 'constexpr int PR_PX_PER_BLOCK = 2048;'),
    ('post_raster.hip', '__host__ __device__ inline int pr_nch(int P) { int n = (P + PR_PX_PER_BLOCK - 1) / PR_PX_PER_BLOCK; '
                        'return n < 1 ? 1 : (n > 64 ? 64 : n); }'),
    ('post_raster.hip', '    const int per = (P + A.nch - 1) / A.nch;'),
    ('post_raster.hip', '    const bool v4 = (P % 4) == 0 && (per % 4) == 0 && (flow_obs_image_stride % 4) == 0 && (bits & 15) == 0;'),
    ('glue.hip', '    const long long chunks = (P + 4095) / 4096;'),
    ('glue.hip', '    if (base + 4096 <= P && (((size_t)(d + base)) & 15) == 0) {'),
]


@pytest.mark.parametrize('name,text', PINS, ids=['%s:%d' % (n, i) for i, (n, _) in enumerate(PINS)])
def test_the_threshold_is_where_the_shapes_expect_it(name, text):
    src = open(os.path.join(ROOT, CSRC, name)).read()
    assert src.count(text) >= 1, ('%s no longer holds %r: a dispatch threshold moved -- move the shapes of '
                                  'tests/test_dispatch_variants_gpu.py to both sides of the new one' % (name, text))


# ---- 3. float32 against float64, restatement against itself ---------------------------------------------------------------------
def gap(name, a32, a64, relative, existing, bar=None):
    """existing: the operator's bar; bar: what the GPU test applies at this case (default: the existing one)."""
    g = dv.worst(a32, a64, relative)
    return rule(name, g, existing, existing if bar is None else bar)


def rule(name, g, existing, bar):
    print('%-46s gap %.3e  bar %.1e  (gap = %.1f %% of the existing bar %.1e)' % (name, g, bar, 100 * g / existing, existing))
    assert bar >= existing, '%s: a bar below the operator\'s' % name
    assert bar <= dv.bar_for(existing, 1.25 * g), ('%s: bar %.1e, but with a gap of %.3e the rule gives %.1e'
                                                  % (name, bar, g, dv.bar_for(existing, g)))
    return g


@pytest.mark.parametrize('J', dv.SKIN_J)
def test_gap_skin_weights(J):
    args = dv.skin_inputs(J)
    (w32, g32), (w64, g64) = dv.skin_reference(*args, dtype=torch.float32), dv.skin_reference(*args)
    gap('skin J=%d weights' % J, w32, w64, False, dv.SKIN_BAR_W)
    for n, a, b in zip(('ctl_ts', 'ctl_rs', 'log_ctl'), g32, g64):
        gap('skin J=%d grad %s' % (J, n), a, b, True, dv.SKIN_BAR_G)


@pytest.mark.parametrize('C', dv.COS_C)
def test_gap_cosine_distance(C):
    for rep, h in dv.COS_REP_H:
        fa, fb, gout = dv.cos_inputs(C, rep, h)
        (d32, g32), (d64, g64) = dv.cos_reference(fa, fb, gout, rep, torch.float32), dv.cos_reference(fa, fb, gout, rep)
        gap('cosine C=%d rep=%d h=%d distance' % (C, rep, h), d32, d64, False, dv.COS_BAR_D)
        dead = torch.isnan(g64)
        assert torch.equal(torch.isnan(g32), dead) and int(dead.sum()) * dv.COS_DEAD_PER <= dead.numel()     # the reference alone
        assert dead[0, :, 0, 0].all() and int(dead.sum()) == C
        gap('cosine C=%d rep=%d h=%d gradient' % (C, rep, h), g32[~dead], g64[~dead], True, dv.COS_BAR_G)


def test_gap_face_gather():
    f = torch.from_numpy(dv.gather_mesh())[None]
    for C in (1, 3):
        gout = torch.randn(1, f.shape[1], 3, C, generator=torch.Generator().manual_seed(C))
        gap('gather C=%d' % C, dv.gather_reference(f, gout, dv.GATHER_V, torch.float32), dv.gather_reference(f, gout, dv.GATHER_V),
            True, dv.GATHER_BAR)


def test_gap_nearest_point():
    for P, Q in dv.NEAREST_SIZES:
        g = torch.Generator().manual_seed(P * 100 + Q)
        a, b = torch.randn(2, P, 3, generator=g), torch.randn(2, Q, 3, generator=g)
        d32 = (a[:, :, None] - b[:, None]).pow(2).sum(-1)
        rd, ri = dv.nearest_reference(a.numpy(), b.numpy())
        assert np.array_equal(d32.argmin(2).numpy(), ri)               # no near-tie that float32 would decide the other way
        g = gap('nearest P=%d Q=%d' % (P, Q), d32.min(2)[0], torch.from_numpy(rd), False, dv.NEAREST_BAR, dv.NEAREST_BARS[P, Q][1])
        assert abs(g - dv.NEAREST_BARS[P, Q][0]) <= 0.25 * g                # the gap written next to the bar is the gap


@pytest.mark.parametrize('F,P', [(F, P) for F in dv.PMF_F for P in dv.PMF_P])
def test_gap_point_mesh_distance(F, P):
    verts, faces, pts = dv.pmf_mesh(F, P)
    a, b = dv.pmf_reference(verts, faces, pts, torch.float32), dv.pmf_reference(verts, faces, pts)
    g = abs(float(a[0]) - float(b[0])) / abs(float(b[0]))
    rule('point-mesh F=%d P=%d loss' % (F, P), g, dv.PMF_BAR_LOSS, dv.PMF_BAR_LOSS)
    for k, name in ((0, 'verts'), (1, 'points')):
        wrote, bar = dv.PMF_BARS_G[F, P][k]
        g = gap('point-mesh F=%d P=%d grad %s' % (F, P, name), a[1 + k], b[1 + k], True, dv.PMF_BAR_G, bar)
        assert abs(g - wrote) <= 0.25 * g


@pytest.mark.parametrize('K,V', dv.LBS_CASES)
def test_gap_lbs(K, V):
    leaves, up, _ = dv.lbs_inputs(K, V)
    for tocam in (0, 1):
        (o32, g32), (o64, g64) = dv.lbs_reference(leaves, K, tocam, up, dtype=torch.float32), dv.lbs_reference(leaves, K, tocam, up)
        gap('lbs K=%d V=%d tocam=%d out' % (K, V, tocam), o32, o64, True, dv.LBS_BAR_OUT)
        for n, a, b in zip(('verts', 'Rmat', 'Tmat', 'skin'), g32, g64):
            gap('lbs K=%d V=%d tocam=%d grad %s' % (K, V, tocam, n), a, b, True, dv.LBS_BAR_G)


@pytest.mark.parametrize('IS,seed', [(48, 21), (47, 22)])
def test_gap_render_tables(IS, seed):
    from test_render_tables_gpu import make_case
    case = make_case(2, 2, IS, seed=seed)
    (t32, g32), (t64, g64) = dv.rt_reference(case, 2, torch.float32), dv.rt_reference(case, 2)
    for n, a, b in zip(('mask', 'flow', 'tex'), t32, t64):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=3e-5 / 4, atol=1e-7 / 4, err_msg=n)
    for n, a, b in zip(('px', 'pp', 'fl'), g32, g64):
        gap('render tables IS=%d grad %s' % (IS, n), a, b, True, dv.RT_BAR_G)


@pytest.mark.parametrize('S', dv.LOSS_S)
def test_gap_loss_tables(S):
    d = dv.loss_inputs(S)
    a, b = dv.loss_tables(d, dtype=torch.float32), dv.loss_tables(d, dtype=torch.float64)
    for k in b:
        gap('loss tables S=%d %s' % (S, k), a[k], b[k], True, dv.LOSS_BAR)
