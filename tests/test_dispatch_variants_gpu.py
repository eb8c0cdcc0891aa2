"""Every size-dispatched operator variant of ops.hip / fused.hip / glue.hip / post_raster.hip at the smallest shapes on both sides of
its dispatch decision, against the float64 restatement of the operation on the CPU.

Several operators choose a kernel, a template instantiation or a code branch by size.  The operator tests (tests/test_ops_gpu.py,
tests/test_step_fusions_gpu.py, tests/test_render_tables_gpu.py) probe them at the sizes LASR runs; here the same restatements and
the same bars are applied where the choice changes:

  skin weights            J = 24 | 25, 40 | 41, 64 | 65   skin_forward_kernel<24> | <40> | <0> | refused
  cosine distance         C / 8 = 8, 24, 32, 48 | other   cosdist_backward_kernel<CPT> | the two-pass form (C = 512, 72, 63)
  face gather backward    N ceil(V / 64) = 2047 | 2048    face_gather_backward_kernel<64, 1024> | <256>; lists of 30 | 31 entries
  nearest point           Q < 16, sub-range boundaries    16 ascending sub-ranges, merge "lowest index wins"
  point-mesh distance     F = 2048 | 2049                 pmf_tile 32 | 64; ragged last chunk; ties across chunks and point blocks
  LBS backward            K = 65 | 66                     MFMA | VALU kernel; K - 1 = 16 | 17 (bone padding); V = 63 | 64 | 65
  render tables backward  aligned | off by one float      16-byte form | scalar form on the same data
  loss tables             P = 2025 | 2116, 4096           one chunk | two chunks, two whole chunks
  fill planes             P = 4095 | 4096 | 4097          16-byte path | scalar tail, aligned and unaligned destination

The builders of the shapes are module-level functions: tests/test_dispatch_variants_cases.py proves on the CPU that they have the
properties claimed here (valences, chunks, sub-ranges, underflow), pins the thresholds in the source text, and measures the gap
between each restatement in float32 and in float64, which the bars below were checked against before anything ran on a GPU.

Bars.  Each is the operator's existing bar.  Rule for the larger shapes: with gap = |restatement in float32 - restatement in
float64| at the new shape (CPU alone), a gap above a quarter of the existing bar would raise the bar to 16 x gap (the convention of
tests/test_icp_gpu.py).  The gaps measured are written next to each bar.  Two bars moved: the absolute bar of the nearest-point
distance at three sizes (few targets: the nearest one is far away and float32 rounds a distance of 20 to 2e-6), and the gradient
bar of the point-mesh distance at F = 2080, P = 257.  Every other gap is below a quarter of its bar and the bar is the operator's.
"""
import numpy as np
import pytest
import torch

from lasr_amd import _lib
from lasr_amd.nnutils import fused_ops, geom_utils, image_losses, mesh_net
from lasr_amd.soft_renderer import functional as srf
from oracle import path_oracle as po

pytestmark = pytest.mark.gpu


def bar_for(existing, gap):
    """The rule of the module docstring."""
    return existing if gap <= existing / 4 else max(existing, 16 * gap)


def worst(got, ref, relative):
    """max |got - ref|, over max |ref| when the bar is relative to the largest entry."""
    got = got.detach().double().cpu()
    ref = ref.detach().double()
    e = float((got - ref).abs().max())
    return e / max(float(ref.abs().max()), 1e-20) if relative else e


def check(name, got, ref, bar, relative):
    e = worst(got, ref, relative)
    print('%-44s err %.3e  bar %.1e' % (name, e, bar))
    assert e <= bar, '%s: %.3e above %.1e' % (name, e, bar)


# =================================================================================================================================
# skin weights: lasr_skin_weights_forward picks <24> for J <= 24, <40> for J <= 40, <0> above, refuses J > 64
# =================================================================================================================================
SKIN_H, SKIN_V = 2, 70                                   # one full wave of vertices and a ragged one
SKIN_J = (24, 25, 40, 41, 64)
# bars of test_skin_weights_match_restatement; largest gaps float32 / float64 restatement over J: weights 5.0e-7 (J = 24),
# gradients 2.8e-6 of the largest entry
SKIN_BAR_W, SKIN_BAR_SUM, SKIN_BAR_G = 2e-6, 1e-5, 2e-4


def skin_inputs(J, seed=0):
    """(ctl_ts [H,J,3], ctl_rs [H,J,4], log_ctl [H,J,3], verts [H,V,3], upstream [H,J,V]): bones at vertices, as the operator test."""
    g = torch.Generator().manual_seed(1000 * J + seed)
    H, V = SKIN_H, SKIN_V
    verts = torch.randn(H, V, 3, generator=g) * 0.4
    ts = verts[:, torch.randperm(V, generator=g)[:J]] + 0.01 * torch.randn(H, J, 3, generator=g)
    rs = torch.randn(H, J, 4, generator=g) * 0.2 + torch.tensor([0., 0., 0., 1.])
    lc = torch.randn(H, J, 3, generator=g) * 0.3 + 1.0
    return ts, rs, lc, verts, torch.randn(H, J, V, generator=g)


def skin_far_bones(n):
    """n bones per hypothesis so far from every vertex that their logit is below -1e4 (tests/..._cases.py: below -1e7): the
    softmax numerator expf(logit - max) is exactly 0 in float32."""
    k = torch.arange(n, dtype=torch.float32)
    ts = torch.stack([1000. + k, 1000. - k, 1000. + 2 * k], 1)[None].repeat(SKIN_H, 1, 1)
    rs = torch.tensor([0., 0., 0., 1.]).repeat(SKIN_H, n, 1)
    return ts, rs, torch.zeros(SKIN_H, n, 3)


def skin_reference(ts, rs, lc, verts, gout, dtype=torch.float64):
    leaves = [t.reshape(-1, t.shape[-1]).detach().clone().to(dtype).requires_grad_(True) for t in (ts, rs, lc)]
    w = po.skin_weights(*leaves, verts.to(dtype))
    (w * gout.to(dtype)).sum().backward()
    return w.detach(), [t.grad for t in leaves]


def skin_on_gpu(cuda, ts, rs, lc, verts, gout=None):
    leaves = [t.reshape(-1, t.shape[-1]).clone().to(cuda).requires_grad_(True) for t in (ts, rs, lc)]
    w = fused_ops.skin_weights(*leaves, verts.to(cuda))
    if gout is not None:
        (w * gout.to(cuda)).sum().backward()
    return w.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize('J', SKIN_J)
def test_skin_weights_on_both_sides_of_every_instantiation(cuda, J):
    ts, rs, lc, verts, gout = skin_inputs(J)
    ref, gref = skin_reference(ts, rs, lc, verts, gout)
    out, grads = skin_on_gpu(cuda, ts, rs, lc, verts, gout)
    assert out.shape == (SKIN_H, J, SKIN_V)
    check('skin J=%d weights' % J, out, ref, SKIN_BAR_W, False)
    assert float((out.sum(1) - 1).abs().max()) <= SKIN_BAR_SUM
    for name, a, b in zip(('ctl_ts', 'ctl_rs', 'log_ctl'), grads, gref):
        check('skin J=%d grad %s' % (J, name), a, b, SKIN_BAR_G, True)


def test_skin_weights_of_65_bones_are_refused(cuda):
    # SKIN_MAX_BONES = 64: the host entry returns LASR_E_BADARG before any launch and the binding raises; no torch fallback
    ts, rs, lc, verts, _ = skin_inputs(64)
    more = [torch.cat([t, t[:, :1]], 1) for t in (ts, rs, lc)]
    with pytest.raises(_lib.LasrNativeError):
        skin_on_gpu(cuda, *more, verts)


@pytest.mark.parametrize('J_big', [40, 41])
def test_skin_weight_instantiations_give_the_same_bits(cuda, J_big):
    # fused.hip: "Same expressions in the same order as the three-pass form: bit-identical weights".  24 real bones through <24>;
    # the same 24 followed by bones whose weight underflows to an exact 0 through <40> (J = 40) and <0> (J = 41): the maximum is
    # the same and every partial sum gains an exact zero, so the first 24 rows must be the same bits.
    ts, rs, lc, verts, _ = skin_inputs(24)
    small, _ = skin_on_gpu(cuda, ts, rs, lc, verts)
    fts, frs, flc = skin_far_bones(J_big - 24)
    big, _ = skin_on_gpu(cuda, torch.cat([ts, fts], 1), torch.cat([rs, frs], 1), torch.cat([lc, flc], 1), verts)
    assert big.shape == (SKIN_H, J_big, SKIN_V)
    assert float(big[:, 24:].abs().max()) == 0.0, 'the appended bones must weigh exactly 0'
    assert torch.equal(big[:, :24], small)


# =================================================================================================================================
# cosine distance, single-layer operator: lasr_cosdist_backward switches on C / 8 (8, 24, 32, 48: registers; other: two passes)
# =================================================================================================================================
COS_N = 4
COS_C = (64, 192, 256, 384, 512, 72, 63)
COS_REP_H = [(1, 5), (1, 8), (2, 5), (2, 8)]              # h = 5: P = 25 < one 32-pixel tile; h = 8: P = 64 = two whole tiles
# bars of test_perceptual_cosine_reduction_matches_reference_formula; largest gaps over all cases: distance 6.8e-8, gradient 2.0e-7
COS_BAR_D, COS_BAR_G = 2e-6, 1e-5
COS_DEAD_PER = 100                                         # the gradient comparison may mask one entry in 100 (the dead pixel): 1 %


def cos_inputs(C, rep, h):
    g = torch.Generator().manual_seed(C * 100 + rep * 10 + h)
    fa = torch.relu(torch.randn(COS_N // rep, C, h, h, generator=g))
    fb = torch.relu(torch.randn(COS_N, C, h, h, generator=g))
    fb[0, :, 0, 0] = 0                                     # a dead pixel: all channels zero
    return fa, fb, torch.randn(COS_N, generator=g)


def cos_reference(fa, fb, gout, rep, dtype=torch.float64):
    b = fb.detach().clone().to(dtype).requires_grad_(True)
    d = 1. - mesh_net.cos_sim(fa.to(dtype).repeat_interleave(rep, 0), b)
    (d * gout.to(dtype)).sum().backward()
    return d.detach(), b.grad


def cos_on_gpu(cuda, fa, fb, gout, rep):
    b = fb.clone().to(cuda).requires_grad_(True)
    d = fused_ops.cosine_distance(fa.to(cuda), b, rep)
    (d * gout.to(cuda)).sum().backward()
    return d.detach(), b.grad


@pytest.mark.parametrize('rep,h', COS_REP_H)
@pytest.mark.parametrize('C', COS_C)
def test_cosine_distance_at_every_channel_instantiation(cuda, C, rep, h):
    fa, fb, gout = cos_inputs(C, rep, h)
    ref, gref = cos_reference(fa, fb, gout, rep)
    out, grad = cos_on_gpu(cuda, fa, fb, gout, rep)
    check('cosine C=%d distance' % C, out, ref, COS_BAR_D, False)
    dead = torch.isnan(gref)                               # autograd: sqrt'(0) at the dead pixel; the kernel drops the term
    assert dead[0, :, 0, 0].all() and int(dead.sum()) * COS_DEAD_PER <= dead.numel() and torch.isfinite(grad).all()
    gd = grad.cpu().double()
    e = float((gd - gref)[~dead].abs().max()) / float(gref[~dead].abs().max())
    print('cosine C=%d rep=%d h=%d gradient err %.3e  bar %.1e' % (C, rep, h, e, COS_BAR_G))
    assert e <= COS_BAR_G


@pytest.mark.parametrize('rep,h', COS_REP_H)
def test_cosine_register_and_two_pass_forms_give_the_same_bits(cuda, rep, h):
    # C = 64 runs cosdist_backward_kernel<8>; with 8 all-zero channels appended to both sides C = 72 runs the two-pass form.  Channel
    # c belongs to group c % 8, so every group's sum gains one exact zero at its end: same distance, same gradient bits.
    fa, fb, gout = cos_inputs(64, rep, h)
    d64, g64 = cos_on_gpu(cuda, fa, fb, gout, rep)
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[0], 8, h, h)], 1)          # noqa: E731
    d72, g72 = cos_on_gpu(cuda, pad(fa), pad(fb), gout, rep)
    assert torch.equal(d72, d64)
    assert torch.equal(g72[:, :64], g64)
    assert float(g72[:, 64:].abs().max()) == 0.0


# =================================================================================================================================
# face gather backward: <256> when N * ceil(V / 64) >= 2048, else <64, 1024>; per-vertex lists of GATHER_CAP = 30, rescan above
# =================================================================================================================================
GATHER_V = 300
GATHER_HUBS = {0: 30, 63: 31, 64: 37, 255: 30, 256: 31}    # vertex -> valence: on the cap, one above it, on the block boundaries
GATHER_ISOLATED = 299
GATHER_BIG_N = 410                                         # the smallest N with N * ceil(300 / 64) >= 2048 (asserted below)
GATHER_BAR = 1e-5                                          # of the largest entry (test_face_gather_matches_index_select); gap 1.4e-7


def gather_mesh():
    """[F,3] int64: a tetrahedron (closed), a strip over the ordinary vertices, and one open fan per hub of GATHER_HUBS with
    exactly that many triangles; vertex GATHER_ISOLATED is in no face.  The faces are shuffled, so the corners of a hub come
    scattered over the corner list."""
    special = set(GATHER_HUBS) | {GATHER_ISOLATED}
    pool = [v for v in range(GATHER_V) if v not in special]
    faces = [[pool[0], pool[1], pool[2]], [pool[0], pool[2], pool[3]], [pool[0], pool[3], pool[1]], [pool[1], pool[3], pool[2]]]
    rest = pool[4:]
    faces += [[rest[i], rest[i + 1], rest[i + 2]] for i in range(0, len(rest) - 2, 3)]
    for k, (hub, n) in enumerate(sorted(GATHER_HUBS.items())):
        rim = [rest[(50 * k + i) % len(rest)] for i in range(n + 1)]
        faces += [[hub, rim[i], rim[i + 1]] if i % 2 == 0 else [rim[i], hub, rim[i + 1]] for i in range(n)]
    faces = np.asarray(faces, np.int64)
    return faces[np.random.default_rng(5).permutation(len(faces))]


def gather_big_n(V=GATHER_V):
    return -(-2048 // ((V + 63) // 64))


def gather_reference(faces, gout, V, dtype=torch.float64):
    """Gradient of the index_select restatement (the CPU branch of srf.face_vertices)."""
    a = torch.zeros(gout.shape[0], V, gout.shape[-1], dtype=dtype, requires_grad=True)
    (srf.face_vertices(a, faces) * gout.to(dtype)).sum().backward()
    return a.grad


def gather_backward_on_gpu(cuda, faces, gout, V):
    N, F, _, C = gout.shape
    out = torch.full((N, V, C), float('nan'), device=cuda)
    _lib.call('lasr_face_gather_backward', gout.to(cuda), faces.to(cuda).contiguous(), out, N, V, F, C)
    return out


@pytest.mark.parametrize('C', [1, 3])
def test_face_gather_backward_small_and_big_launch_on_one_mesh(cuda, C):
    f = torch.from_numpy(gather_mesh())
    F, V = f.shape[0], GATHER_V
    blocks = (V + 63) // 64
    big = gather_big_n()
    assert big == GATHER_BIG_N and big * blocks >= 2048 > (big - 1) * blocks and 1 * blocks < 2048
    g = torch.Generator().manual_seed(C)
    gout = torch.randn(1, F, 3, C, generator=g)
    ref = gather_reference(f[None], gout, V)
    one = gather_backward_on_gpu(cuda, f[None], gout, V)                               # <64, 1024>
    check('gather C=%d N=1' % C, one, ref, GATHER_BAR, True)
    assert float(one[0, GATHER_ISOLATED].abs().max()) == 0.0
    many = gather_backward_on_gpu(cuda, f[None].repeat(big, 1, 1), gout.repeat(big, 1, 1, 1), V)   # <256>
    # ascending corner index in both variants by construction: every replica of the big launch has the small launch's bits
    assert torch.equal(many, one.expand(big, V, C))
    # one mesh of a small launch with its faces in reverse order (its sums run in another order: held to the restatement only)
    faces3 = f[None].repeat(3, 1, 1)
    faces3[1] = faces3[1].flip(0)
    gout3 = torch.randn(3, F, 3, C, generator=g)
    check('gather C=%d reversed' % C, gather_backward_on_gpu(cuda, faces3, gout3, V), gather_reference(faces3, gout3, V),
          GATHER_BAR, True)


# =================================================================================================================================
# nearest point: 16 ascending sub-ranges of ceil(Q / 16) targets, merged with "lowest index wins"
# =================================================================================================================================
NEAREST_SIZES = [(15, 1), (16, 15), (17, 16), (33, 17), (5, 31)]
NEAREST_TIE_Q = (17, 48, 100)
NEAREST_BAR = 1e-6                                         # absolute, test_nearest_point_and_chamfer (hundreds of targets: small distances)
# (P, Q): (gap of the float32 restatement, bar): the existing bar where the gap is at most a quarter of it, else 16 x gap
NEAREST_BARS = {(15, 1): (2.06e-6, 3.3e-5), (16, 15): (3.56e-7, 5.7e-6), (17, 16): (1.85e-7, 1e-6), (33, 17): (4.18e-7, 6.7e-6),
                (5, 31): (3.1e-8, 1e-6)}


def nearest_tie_sets(Q, P=33):
    """(a [2,P,3], b [2,Q,3]) with small integer coordinates (every squared distance exact in float32).  The targets are drawn
    from six distinct points, so duplicates lie inside sub-ranges and across them, and b[k + per * s] = b[k] for s = 1, 3, 7,
    15 puts an exact copy of the first sub-range's points into other sub-ranges."""
    rng = np.random.default_rng(Q)
    per = (Q + 15) // 16
    pool = np.array([[0, 0, 0], [3, 1, 0], [-2, 2, 1], [1, -3, 2], [4, 4, -1], [-1, 0, 5]], np.float32)
    b = pool[rng.integers(0, 6, (2, Q))]
    for k in range(per):
        for s in (1, 3, 7, 15):
            if k + per * s < Q:
                b[:, k + per * s] = b[:, k]
    a = rng.integers(-4, 6, (2, P, 3)).astype(np.float32)
    return a, b


def nearest_reference(a, b):
    """float64 distances, numpy's first-minimum argmin."""
    d = ((np.asarray(a, np.float64)[:, :, None] - np.asarray(b, np.float64)[:, None]) ** 2).sum(-1)
    return d.min(2), d.argmin(2)


@pytest.mark.parametrize('P,Q', NEAREST_SIZES)
def test_nearest_point_with_fewer_targets_than_sub_ranges(cuda, P, Q):
    g = torch.Generator().manual_seed(P * 100 + Q)
    a, b = torch.randn(2, P, 3, generator=g), torch.randn(2, Q, 3, generator=g)
    d2, idx = fused_ops.nearest_point(a.to(cuda), b.to(cuda))
    rd, ri = nearest_reference(a.numpy(), b.numpy())
    assert np.array_equal(idx.cpu().numpy(), ri)
    check('nearest P=%d Q=%d' % (P, Q), d2, torch.from_numpy(rd), NEAREST_BARS[P, Q][1], False)


@pytest.mark.parametrize('Q', NEAREST_TIE_Q)
def test_nearest_point_gives_a_tie_to_the_lowest_index(cuda, Q):
    a, b = nearest_tie_sets(Q)
    d2, idx = fused_ops.nearest_point(torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda))
    rd, ri = nearest_reference(a, b)
    assert np.array_equal(idx.cpu().numpy(), ri)
    assert np.array_equal(d2.cpu().numpy().astype(np.float64), rd)                     # integers: exact


def test_nearest_point_of_a_nan_query_is_index_zero(cuda):
    # no candidate passes `d < best`: the "nothing found" marker unpacks to index 0 (chamfer.hip relies on the same value)
    g = torch.Generator().manual_seed(9)
    a, b = torch.randn(1, 17, 3, generator=g), torch.randn(1, 40, 3, generator=g)
    a[0, 3, 1] = float('nan')
    _, idx = fused_ops.nearest_point(a.to(cuda), b.to(cuda))
    _, ri = nearest_reference(a.numpy(), b.numpy())
    assert int(idx[0, 3]) == 0
    keep = np.arange(17) != 3
    assert np.array_equal(idx.cpu().numpy()[0, keep], ri[0, keep])


# =================================================================================================================================
# point-mesh distance: pmf_tile(F) = 32 faces per chunk up to F = 2048, doubling above; blocks of 256 points
# =================================================================================================================================
PMF_F = (2048, 2049, 2080)
PMF_P = (255, 257)
# bars of test_point_mesh_distance_matches_restatement; the loss gap is at most 5.4e-8.  The closest-point formula loses digits for
# points a few triangle sizes away, and the triangles here are small: the gradient gaps are a good part of the bar.
PMF_BAR_LOSS, PMF_BAR_G = 1e-5, 2e-4
# (F, P): ((gap of grad verts, its bar), (gap of grad points, its bar)): the existing bar up to a gap of a quarter of it, else 16 x gap
PMF_BARS_G = {(2048, 255): ((4.97e-5, 2e-4), (4.60e-5, 2e-4)), (2048, 257): ((3.84e-5, 2e-4), (1.49e-5, 2e-4)),
              (2049, 255): ((4.4e-6, 2e-4), (5.2e-6, 2e-4)), (2049, 257): ((1.00e-5, 2e-4), (9.4e-6, 2e-4)),
              (2080, 255): ((1.33e-5, 2e-4), (1.77e-5, 2e-4)), (2080, 257): ((5.22e-5, 8.4e-4), (5.97e-5, 9.6e-4))}


def pmf_tile(F):
    """fused.hip: pmf_tile."""
    t = 32
    while (F + t - 1) // t > 64:
        t *= 2
    return t


def pmf_mesh(F, P, seed=0):
    """(verts [2,V,3], faces [F,3], points [2,P,3]): the first F triangles of a bumpy 32 x 33 grid of quads (not closed; vertices of
    the dropped triangles stay unused), points scattered over it."""
    g = torch.Generator().manual_seed(F * 10 + P + seed)
    nx, ny = 32, 33
    ix, iy = torch.meshgrid(torch.arange(nx + 1), torch.arange(ny + 1), indexing='ij')
    base = torch.stack([ix.reshape(-1) / nx - 0.5, iy.reshape(-1) / ny - 0.5, torch.zeros((nx + 1) * (ny + 1))], 1).float()
    vid = lambda i, j: i * (ny + 1) + j                                                # noqa: E731
    faces = []
    for i in range(nx):
        for j in range(ny):
            faces += [[vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)], [vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)]]
    faces = torch.tensor(faces[:F], dtype=torch.int64)
    verts = base[None].repeat(2, 1, 1) + torch.tensor([0.004, 0.004, 0.05]) * torch.randn(2, base.shape[0], 3, generator=g)
    pts = (torch.rand(2, P, 3, generator=g) - 0.5) * torch.tensor([1.1, 1.1, 0.3])
    return verts, faces, pts


def pmf_reference(verts, faces, pts, dtype=torch.float64):
    v, p = verts.detach().clone().to(dtype).requires_grad_(True), pts.detach().clone().to(dtype).requires_grad_(True)
    loss = po.point_mesh_face_distance(v, faces, p)
    (loss * 1.7).backward()
    return loss.detach(), v.grad, p.grad


@pytest.mark.parametrize('P', PMF_P)
@pytest.mark.parametrize('F', PMF_F)
def test_point_mesh_distance_around_the_chunk_size_step(cuda, F, P):
    verts, faces, pts = pmf_mesh(F, P)
    assert faces.shape[0] == F
    ref, gv, gp = pmf_reference(verts, faces, pts)
    v, p = verts.clone().to(cuda).requires_grad_(True), pts.clone().to(cuda).requires_grad_(True)
    out = fused_ops.point_mesh_face_distance(v, faces.to(cuda), p)
    (out * 1.7).backward()
    e = abs(float(out.detach()) - float(ref)) / abs(float(ref))
    print('point-mesh F=%d P=%d loss err %.3e  bar %.1e' % (F, P, e, PMF_BAR_LOSS))
    assert e <= PMF_BAR_LOSS
    check('point-mesh F=%d P=%d grad verts' % (F, P), v.grad, gv, PMF_BARS_G[F, P][0][1], True)
    check('point-mesh F=%d P=%d grad points' % (F, P), p.grad, gp, PMF_BARS_G[F, P][1][1], True)


PMF_TIE_F, PMF_TIE_T, PMF_TIE_P0 = 2080, 16, 257


def pmf_tie_case():
    """Every base triangle twice -- faces 0..15 (first chunk) and 2064..2079 (last, ragged chunk) are bitwise the same 16 triangles
    -- and every point twice (p and p + 257: another block of 256 points).  The base triangles lie 4 apart in z = 0; point j hangs
    over the interior of base triangle j % 16 at height 0.05 + 0.01 (j // 16), so its nearest triangle is that one (both copies:
    a tie) and the nearest point of base triangle t is point t (and its copy: a tie).  The 2048 faces in between are small
    triangles 1000 away.  -> (verts [1,V,3], faces [F,3], points [1,2 P0,3], expected nearest face of every point [2 P0],
    expected nearest point of the 32 base faces [32])."""
    T, F, P0 = PMF_TIE_T, PMF_TIE_F, PMF_TIE_P0
    rng = np.random.default_rng(11)
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    base = np.concatenate([tri + np.array([4 * t, 0, 0], np.float32) for t in range(T)])            # 3 T vertices
    nfill = F - 2 * T
    fill = (rng.uniform(0, 1, (nfill, 3, 3)) + np.array([1000, 0, 0]) + 3 * np.arange(nfill)[:, None, None] * np.array([0, 1, 0])
            ).astype(np.float32).reshape(-1, 3)
    verts = np.concatenate([base, fill])
    f_base = np.arange(3 * T).reshape(T, 3)
    f_fill = 3 * T + np.arange(3 * nfill).reshape(nfill, 3)
    faces = np.concatenate([f_base, f_fill, f_base]).astype(np.int64)
    j = np.arange(P0)
    p = np.stack([4 * (j % T) + 0.25 + 0.01 * (j % 7), 0.25 + 0.01 * (j % 5), 0.05 + 0.01 * (j // T)], 1).astype(np.float32)
    pts = np.concatenate([p, p])
    near_face = np.concatenate([j % T, j % T])
    near_point = np.concatenate([np.arange(T), np.arange(T)])
    return verts[None], faces, pts[None], near_face, near_point


def test_point_mesh_ties_across_chunks_go_to_the_lower_index(cuda):
    verts, faces, pts, near_face, near_point = pmf_tie_case()
    N, V, F, P = 1, verts.shape[1], faces.shape[0], pts.shape[1]
    dv = lambda a: torch.from_numpy(a).to(cuda)                                        # noqa: E731
    dp, df = torch.empty(N, P, device=cuda), torch.empty(N, F, device=cuda)
    ap = torch.full((N, P), -1, dtype=torch.int32, device=cuda)
    af = torch.full((N, F), -1, dtype=torch.int32, device=cuda)
    scratch = torch.empty(_lib.lib().lasr_point_mesh_scratch_floats(N, F, P), dtype=torch.float32, device=cuda)
    _lib.call('lasr_point_mesh_forward', dv(verts), dv(faces), dv(pts), dp, ap, df, af, scratch, N, V, F, P)
    ap, af = ap.cpu().numpy()[0], af.cpu().numpy()[0]
    T = PMF_TIE_T
    assert np.array_equal(ap, near_face)                                               # never T..F-1: not the copy in the last chunk
    assert np.array_equal(af[:T], near_point[:T]) and np.array_equal(af[F - T:], near_point[T:])
    assert af.min() >= 0 and af.max() < PMF_TIE_P0                                     # every face: the first copy of its point
    h = pts[0, :, 2].astype(np.float64) ** 2                                           # over the interior: the squared height
    assert np.abs(dp.cpu().numpy()[0] - h).max() <= 1e-6 * h.max()
    assert np.abs(df.cpu().numpy()[0, :T] - h[:T]).max() <= 1e-6 * h.max()


# =================================================================================================================================
# LBS: lbs_backward runs the MFMA kernel for K <= 65 (bones padded to 16s, 64 vertices per block), the VALU kernel above
# =================================================================================================================================
LBS_CASES = [(K, V) for K in (17, 18, 64, 65, 66) for V in (63, 64, 65)] + [(66, 256), (66, 257)]
# bars of test_obj_to_cam_vs_oracle_at_lasr_sizes (output) and of the LBS tests of test_step_fusions_gpu.py (gradients), both of
# the largest entry; largest gaps over all cases: output 2.0e-7, gradients 4.5e-7
LBS_BAR_OUT, LBS_BAR_G = 2e-6, 2e-5


def lbs_inputs(K, V, N=2):
    g = torch.Generator().manual_seed(K * 1000 + V)
    leaves = [torch.randn(N, V, 3, generator=g), torch.randn(N * K, 3, 3, generator=g), torch.randn(N * K, 1, 3, generator=g),
              torch.softmax(torch.randn(N, max(K - 1, 1), V, 1, generator=g), 1)]
    return leaves, torch.randn(N, V, 3, generator=g), torch.randn(N, V, 3, generator=g)


def lbs_reference(leaves, K, tocam, up, up_blend=None, dtype=torch.float64):
    from test_step_fusions_gpu import _lbs_reference
    a = [t.clone().to(dtype).requires_grad_(True) for t in leaves]
    out = _lbs_reference(*a, K, tocam)
    tot = (out * up.to(dtype)).sum()
    if up_blend is not None:
        blend = _lbs_reference(*a, K, 0)
        tot = tot + (blend * up_blend.to(dtype)).sum()
        out = (out, blend)
    tot.backward()
    return out, [t.grad for t in a]


@pytest.mark.parametrize('tocam', [0, 1])
@pytest.mark.parametrize('K,V', LBS_CASES)
def test_lbs_on_both_sides_of_the_kernel_choice(cuda, K, V, tocam):
    leaves, up, _ = lbs_inputs(K, V)
    ref, gref = lbs_reference(leaves, K, tocam, up)
    b = [t.clone().to(cuda).requires_grad_(True) for t in leaves]
    out = geom_utils.obj_to_cam(b[0], b[1], b[2], K, 1, b[3], tocam=bool(tocam))
    check('lbs K=%d V=%d tocam=%d out' % (K, V, tocam), out, ref, LBS_BAR_OUT, True)
    (out * up.to(cuda)).sum().backward()
    for name, x, y in zip(('verts', 'Rmat', 'Tmat', 'skin'), b, gref):
        check('lbs K=%d V=%d tocam=%d grad %s' % (K, V, tocam, name), x.grad, y, LBS_BAR_G, True)


def test_lbs_both_outputs_at_the_last_matrix_core_size(cuda):
    K, V = 65, 65
    leaves, up0, up1 = lbs_inputs(K, V)
    (rcam, rblend), gref = lbs_reference(leaves, K, 1, up0, up1)
    b = [t.clone().to(cuda).requires_grad_(True) for t in leaves]
    cam, blend = geom_utils.obj_to_cam_both(b[0], b[1], b[2], K, 1, b[3])
    check('lbs both cam', cam, rcam, LBS_BAR_OUT, True)
    check('lbs both blend', blend, rblend, LBS_BAR_OUT, True)
    ((cam * up0.to(cuda)).sum() + (blend * up1.to(cuda)).sum()).backward()
    for name, x, y in zip(('verts', 'Rmat', 'Tmat', 'skin'), b, gref):
        check('lbs both grad %s' % name, x.grad, y, LBS_BAR_G, True)


# =================================================================================================================================
# render tables backward: the 16-byte form needs P % 4 == 0, whole quads per chunk and 16-byte aligned planes; else the scalar form
# =================================================================================================================================
RT_BAR_G = 2e-4                                            # of the largest entry (test_render_tables_gpu.py); gaps <= 3.1e-7
RT_WT = 0.7


def rt_chunks(P):
    """(chunks, pixels per chunk) of post_raster.hip: pr_nch / pr_range."""
    nch = min(64, max(1, (P + 2047) // 2048))
    return nch, (P + nch - 1) // nch


def rt_reference(case, H, dtype=torch.float64):
    """Tables, pair and the gradients of one fixed scalar of them, from the reference lines (test_render_tables_gpu.reference)."""
    from test_render_tables_gpu import reference
    px, masks, occ, flow_obs, imgs, pp, fl = case
    I, IS = masks.shape[0], px.shape[-1]
    leaves = [t.clone().to(dtype).requires_grad_(True) for t in (px, pp, fl)]
    ref = reference(leaves[0], masks.to(dtype), occ.to(dtype), flow_obs.to(dtype), imgs.to(dtype), leaves[1], leaves[2], H, RT_WT, True)
    cot, cot_pair = rt_cotangents(I, H, IS)
    total = sum((c.to(dtype) * t).sum() for c, t in zip(cot, ref[:3])) + (cot_pair.to(dtype) * ref[6]).sum()
    return [t.detach() for t in ref[:3]], torch.autograd.grad(total, leaves)


def rt_cotangents(I, H, IS):
    g = torch.Generator().manual_seed(5)
    return [torch.randn(I, H, generator=g) for _ in range(3)], torch.randn(2 * I * H, 3, IS, IS, generator=g) * 1e-3


def rt_on_gpu(cuda, case, H, misalign):
    px, masks, occ, flow_obs, imgs, pp, fl = [t.to(cuda) for t in case]
    I, IS = masks.shape[0], px.shape[-1]
    if misalign:                                           # px one float into a larger allocation: 4 bytes off a 16-byte boundary
        buf = torch.empty(px.numel() + 1, device=cuda)
        buf[1:].copy_(px.reshape(-1))
        px = buf[1:].view(px.shape)
        assert px.data_ptr() % 16 == 4 and px.is_contiguous()
    else:
        assert px.data_ptr() % 16 == 0
    px, pp, fl = px.requires_grad_(True), pp.requires_grad_(True), fl.requires_grad_(True)
    out = fused_ops.render_tables(px, masks, occ, flow_obs, fused_ops.obs_pair(imgs, masks), pp, fl, RT_WT, True)
    cot, cot_pair = rt_cotangents(I, H, IS)
    tot = sum((c.to(cuda) * t).sum() for c, t in zip(cot, out[:3])) + (cot_pair.to(cuda) * out[7]).sum()
    return [t.detach() for t in out[:3]], torch.autograd.grad(tot, [px, pp, fl])


def rt_check_tables(tabs, ref):
    for k, name in enumerate(('mask', 'flow', 'tex')):
        np.testing.assert_allclose(tabs[k].cpu().numpy(), ref[k].numpy(), rtol=3e-5, atol=1e-7, err_msg=name)


def test_render_tables_backward_both_forms_on_the_same_data(cuda):
    from test_render_tables_gpu import make_case
    I, H, IS = 2, 2, 48
    P = IS * IS
    nch, per = rt_chunks(P)
    assert P % 4 == 0 and per % 4 == 0 and nch == 2        # two chunks of whole quads: the 16-byte form, unless a plane is unaligned
    case = make_case(I, H, IS, seed=21)
    ref, gref = rt_reference(case, H)
    t4, g4 = rt_on_gpu(cuda, case, H, misalign=False)      # render_tables_backward_kernel<true>
    t1, g1 = rt_on_gpu(cuda, case, H, misalign=True)       # render_tables_backward_kernel<false>
    rt_check_tables(t4, ref)
    rt_check_tables(t1, ref)
    for name, a, b, r in zip(('px', 'pp', 'fl'), g4, g1, gref):
        check('render tables 16-byte form grad ' + name, a, r, RT_BAR_G, True)
        check('render tables scalar form grad ' + name, b, r, RT_BAR_G, True)
        # to each other at the same bar: the per-pixel arithmetic is shared, the intrinsics' sums associate differently
        check('render tables forms against each other ' + name, a, b.double().cpu(), RT_BAR_G, True)


def test_render_tables_backward_with_a_pixel_count_that_is_no_multiple_of_four(cuda):
    from test_render_tables_gpu import make_case
    I, H, IS = 2, 2, 47
    assert (IS * IS) % 4 != 0 and rt_chunks(IS * IS)[0] == 2
    case = make_case(I, H, IS, seed=22)
    ref, gref = rt_reference(case, H)
    tabs, grads = rt_on_gpu(cuda, case, H, misalign=False)
    rt_check_tables(tabs, ref)
    for name, a, r in zip(('px', 'pp', 'fl'), grads, gref):
        check('render tables P=%d grad %s' % (IS * IS, name), a, r, RT_BAR_G, True)


# =================================================================================================================================
# separate loss tables (ops.hip): chunks of 2048 pixels
# =================================================================================================================================
LOSS_S = (45, 46, 64)                                      # P = 2025: one chunk; 2116: just above one; 4096: exactly two
LOSS_I, LOSS_H = 2, 3
LOSS_BAR = 1e-5                                            # of the largest entry (test_ops_gpu.py: close(..., 1e-5)); gaps <= 2.0e-7


def loss_inputs(S):
    rng = np.random.default_rng(S)
    I, H = LOSS_I, LOSS_H
    t = lambda a: torch.from_numpy(a.astype(np.float32))                               # noqa: E731
    occ = rng.standard_normal((I, S, S))
    occ[rng.uniform(0, 1, occ.shape) < 0.2] = 0.0
    bg = rng.uniform(0, 1, (I, H, S, S)) < 0.5
    bg[0, 0] = True                                        # one (image, hypothesis) with nothing selected
    return dict(pred=t(rng.uniform(0, 1, (I, H, S, S))), masks=t(rng.uniform(0, 1, (I, S, S)) > 0.4), occ=t(occ),
                flow_rd=t(rng.standard_normal((I, H, S, S, 2))), flow_obs=t(rng.standard_normal((I, 3, S, S))), bg=torch.from_numpy(bg),
                obs=t(rng.uniform(0, 1, (I, 3, S, S))), white=t(rng.uniform(0, 1, (I, 3, S, S))), rnd=t(rng.uniform(0, 1, (I, H, 3, S, S))),
                fg=t(rng.uniform(0, 1, (I, H, S, S))), w=t(rng.uniform(0.5, 1.5, (I, H))))


def loss_tables(d, dtype=None, device=None):
    """{name: tensor} of the three tables, the flow map and the gradients of sum(w * table), through path_oracle (dtype given, CPU)
    or through the HIP operators (device given)."""
    on_gpu = device is not None
    cv = (lambda t: t.to(device)) if on_gpu else (lambda t: t if t.dtype == torch.bool else t.to(dtype))
    mod = image_losses if on_gpu else po
    x = {k: cv(v) for k, v in d.items()}
    leaves = {k: x[k].clone().requires_grad_(True) for k in ('pred', 'flow_rd', 'rnd', 'fg')}
    res = {}
    res['mask'] = mod.mask_loss_table(leaves['pred'], x['masks'], x['occ'])
    res['flow'], res['flow map'] = mod.flow_loss_table(leaves['flow_rd'], x['flow_obs'], x['bg'], x['occ'], x['masks'])
    res['tex'] = mod.tex_loss_table(x['obs'], x['white'], leaves['rnd'], leaves['fg'], x['occ'], 0.7)
    (sum((res[k] * x['w']).sum() for k in ('mask', 'flow', 'tex'))).backward()
    res = {k: v.detach() for k, v in res.items()}
    res.update({'grad ' + k: v.grad for k, v in leaves.items()})
    return res


@pytest.mark.parametrize('S', LOSS_S)
def test_loss_tables_just_above_one_chunk_and_at_two_whole_chunks(cuda, S):
    d = loss_inputs(S)
    ref = loss_tables(d, dtype=torch.float64)
    out = loss_tables(d, device=cuda)
    for k in ref:
        check('loss tables S=%d %s' % (S, k), out[k].reshape(ref[k].shape), ref[k], LOSS_BAR, True)


# =================================================================================================================================
# fill planes: 16-byte stores where a whole 4096-float piece of a plane is 16-byte aligned, scalar stores elsewhere
# =================================================================================================================================
@pytest.mark.parametrize('offset', [32, 33])               # floats into the enclosing buffer: 16-byte aligned / 4 bytes off
@pytest.mark.parametrize('C', [1, 4, 16])
@pytest.mark.parametrize('P', [4095, 4096, 4097, 8197])
def test_fill_planes_fills_its_planes_and_nothing_else(cuda, P, C, offset):
    N, guard = 3, 12345.0
    n = N * C * P
    buf = torch.full((n + 64,), guard, device=cuda)
    dst = buf[offset:offset + n].view(N, C, P)
    assert dst.data_ptr() % 16 == (0 if offset == 32 else 4)
    vals = [0.25 * (c + 1) for c in range(C)]
    fused_ops.fill_planes(dst, vals)
    want = torch.tensor(vals).view(1, C, 1).expand(N, C, P)
    assert torch.equal(dst.cpu(), want)
    assert bool((buf[:offset] == guard).all()) and bool((buf[offset + n:] == guard).all())
