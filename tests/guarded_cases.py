"""The table of tests/test_guarded_ops_gpu.py: one Case (tests/guarded.py) per operator and ragged shape.

Shapes are the smallest at which an index can go wrong, never workload sizes: every case has a dimension that is one more than
a multiple of the unit its kernel works in, and every family has the degenerate size 1.
  pixels   : image sides 17 and 47 (289 = 9 * 32 + 1 pixels; 2209 = one 2048-pixel chunk + 161), I and H in {1, 3}
  meshes   : V in {1, 17, 65} (one over the 16-vertex LBS wave, one over the 64-vertex gather block), K in {1, 2, 21}, N in {1, 3};
             the geodesic sphere of level 1 (+ 5 vertices no face uses) and a fan whose hub has 40 faces
  cosdist  : (C, h) in {(5, 7), (64, 7), (384, 3)} (49 pixels = 32 + 17; 384 channels = the register limit), rep in {1, 3}
  points   : P and F in {1, 257} (one over a 256-point block)
  raster   : sides 8, 24, 33; F in {1, 65, 257}; N = 3, and N = 8 at side 64 (the smallest launch that builds its own tile order)
Every callable rebuilds its inputs from a fixed seed on the CPU, so the three runs of run_case see the same bits.

exact=False appears only where a FLOAT atomic feeds the result (the other atomics of the kernels are integer counters and slot
cursors, which leave the values exact):
  sr_backward.h: sr_backward_kernel credits surface texels with atomicAdd -> grad_textures of texture_type='surface'
  sr_fp64.hip: backward_kernel accumulates both gradients with atomicAdd (double)"""
import importlib

import numpy as np
import torch

from guarded import Case
from lasr_amd import synth

CASES = []
NOT_COVERED = {}
# natives whose device inputs do not reach them as tensor arguments, so guarded.run_relocated cannot move them (their outputs and
# scratch are guarded all the same); the conditions are those of tests/test_guarded_alloc_cpu.py
NOT_RELOCATED = {
    'lasr_monitor_sheet': 'its ten planes, control points and palette are addresses inside the SheetInputs structure',
    'lasr_icp_init': 'it has no input: rotations, translations, errors, status and workspace are all allocated by its wrapper',
    'lasr_manifold_extract': 'it has no input: the voxels come from lasr_voxelize and the workspace from lasr_manifold_count, both '
                             'in allocations of the wrapper',
}


def case(name, natives, **kw):
    def deco(fn):
        CASES.append(Case(name, fn, natives, **kw))
        return fn
    return deco


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _leaf(t, dev):
    return t.clone().to(dev).requires_grad_(True)


def _back(outs, leaves, dev, seed=99):
    """Gradients of sum_o <o, fixed random cotangent> with respect to the leaves (those that get one)."""
    g = _gen(seed)
    outs = [o for o in outs if o is not None and o.requires_grad]
    cots = [torch.randn(tuple(o.shape), generator=g).to(dev) for o in outs]
    grads = torch.autograd.grad(outs, leaves, cots, allow_unused=True)
    return tuple(x for x in grads if x is not None)


def _tensors(*xs):
    return tuple(x for x in xs if x is not None)


# ---- meshes ---------------------------------------------------------------------------------------------------------------------
def _mesh(name):
    """(vertices float32 [V,3], faces int64 [F,3])."""
    if name == 'sphere17':                                  # geodesic sphere of level 1 + 5 vertices no face refers to
        v, f = synth.geodesic_sphere(1)
        extra = np.array([[2, 2, 2], [-2, 2, 1], [2, -2, 1], [1, 2, -2], [-1, -2, 2]], np.float32) * 0.4
        return np.concatenate([v, extra]).astype(np.float32), np.asarray(f, np.int64)
    if name == 'fan65':                                     # hub of 40 faces (more than the per-vertex list), 24 unused rim vertices
        ang = np.linspace(0, 2 * np.pi, 64, endpoint=False)
        rim = np.stack([np.cos(ang), np.sin(ang), 0.1 * np.sin(3 * ang)], 1)
        v = np.concatenate([[[0, 0, 0.3]], rim]).astype(np.float32) * 0.6
        return v, np.array([[0, 1 + i, 2 + i] for i in range(40)], np.int64)
    if name == 'one':                                       # one vertex, one (degenerate) face
        return np.array([[0.1, -0.2, 0.3]], np.float32), np.zeros((1, 3), np.int64)
    raise KeyError(name)


def _random_faces(g, V, F):
    return torch.stack([torch.randperm(V, generator=g)[:3] for _ in range(F)]).long()


# ---- pixel operators --------------------------------------------------------------------------------------------------------------
def _pixel_shapes():
    return [(3, 3, 17), (1, 1, 47), (1, 3, 17), (3, 1, 47)]


def _loss_inputs(I, H, S, seed):
    g = _gen(seed)
    masks = (torch.rand(I, S, S, generator=g) > 0.4).float()
    occ = torch.randn(I, S, S, generator=g)
    occ[occ.abs() < 0.3] = 0.0
    occ[:, 0, 0] = 1.0                                       # (at least one observed pixel per image)
    masks[:, 0, 0] = 1.0
    return g, masks, occ


def _add_pixel_cases(I, H, S):
    tag = 'I%d-H%d-S%d' % (I, H, S)

    @case('mask_loss_table/' + tag, ['lasr_mask_loss_forward', 'lasr_mask_loss_backward'])
    def _(dev):
        from lasr_amd.nnutils import image_losses
        g, masks, occ = _loss_inputs(I, H, S, 1)
        pred = _leaf(torch.rand(I, H, S, S, generator=g), dev)
        out = image_losses.mask_loss_table(pred, masks.to(dev), occ.to(dev))
        return (out,) + _back([out], [pred], dev)

    @case('flow_loss_table/' + tag, ['lasr_flow_loss_forward_vis', 'lasr_flow_loss_backward'])
    def _(dev):
        from lasr_amd.nnutils import image_losses
        g, masks, occ = _loss_inputs(I, H, S, 2)
        flow_rd = _leaf(torch.randn(I, H, S, S, 2, generator=g) * 0.1, dev)
        flow_obs = (torch.randn(I, 3, S, S, generator=g) * 0.1).to(dev)
        bg = torch.rand(I, H, S, S, generator=g) < 0.3
        bg[:, :, 0, 0] = False
        loss, fmap, vis = image_losses.flow_loss_table(flow_rd, flow_obs, bg.to(dev), occ.to(dev), masks.to(dev), with_vis=True)
        return (loss, fmap, vis) + _back([loss], [flow_rd], dev)

    @case('tex_loss_table/' + tag, ['lasr_tex_loss_forward', 'lasr_tex_loss_backward'])
    def _(dev):
        from lasr_amd.nnutils import image_losses
        g, masks, occ = _loss_inputs(I, H, S, 3)
        obs, white = torch.rand(I, 3, S, S, generator=g).to(dev), torch.rand(I, 3, S, S, generator=g).to(dev)
        rnd, fg = _leaf(torch.rand(I, H, 3, S, S, generator=g), dev), _leaf(torch.rand(I, H, S, S, generator=g), dev)
        out = image_losses.tex_loss_table(obs, white, rnd, fg, occ.to(dev), 0.7)
        return (out,) + _back([out], [rnd, fg], dev)

    @case('flow_reproject/' + tag, ['lasr_flow_reproject_forward', 'lasr_flow_reproject_backward'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        from test_render_tables_gpu import make_case
        px10, _, _, _, _, pp, fl = make_case(I, H, S, seed=4)
        N = I * H
        px = _leaf(px10[:, 3:].contiguous(), dev)
        pp0, fl0 = pp.to(dev), fl.to(dev)
        pp1, fl1 = _leaf(pp.roll(1, 0) * 0.5, dev), _leaf(fl.roll(1, 0) + 0.25, dev)
        flow, bg = fused_ops.flow_reproject(px, pp0, pp1, fl0, fl1)
        assert N == flow.shape[0]
        return (flow, bg) + _back([flow], [px, pp1, fl1], dev)

    @case('flow_reproject_planes/' + tag, ['lasr_flow_reproject_planes_forward', 'lasr_flow_reproject_planes_backward'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        from test_render_tables_gpu import make_case
        px10, _, _, _, _, pp, fl = make_case(I, H, S, seed=5)
        px10 = _leaf(px10, dev)
        pp1, fl1 = _leaf(pp.roll(1, 0) * 0.5, dev), _leaf(fl.roll(1, 0) + 0.25, dev)
        flow, bg = fused_ops.flow_reproject_planes(px10[:, 3:9], pp.to(dev), pp1, fl.to(dev), fl1)
        return (flow, bg) + _back([flow], [px10, pp1, fl1], dev)

    @case('obs_pair/' + tag, ['lasr_obs_pair'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        g, masks, _ = _loss_inputs(I, H, S, 6)
        return (fused_ops.obs_pair(torch.rand(I, 3, S, S, generator=g).to(dev), masks.to(dev)),)

    @case('fill_planes/' + tag, ['lasr_fill_planes'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        dst = fused_ops.torch.empty(I, H + 1, S, S, dtype=torch.float32, device=dev)     # (the module's allocator: guarded)
        values = [0.25 * (c + 1) for c in range(H + 1)]
        held = torch.arange((I + 2) * (H + 1) * S * S, dtype=torch.float32).reshape(I + 2, H + 1, S, S).to(dev)
        fused_ops.fill_planes(held[1:I + 1], values)        # a caller's buffer, filled in place: images 0 and I + 1 are neighbours
        return (fused_ops.fill_planes(dst, values), held)

    for want_pair in (False, True):
        for from_imgs in (False, True):
            # the batch is [frame t block ; frame t' block]: I * H must be even (pr_args refuses an odd one), so I = 2 and 6 here
            _add_render_tables(2 * I, H, S, want_pair, from_imgs, 'I%d-H%d-S%d' % (2 * I, H, S))


def _add_render_tables(I, H, S, want_pair, from_imgs, tag):
    name = '%s/%s-pair%d' % ('render_tables_imgs' if from_imgs else 'render_tables', tag, want_pair)
    natives = ['lasr_render_tables_forward_imgs' if from_imgs else 'lasr_render_tables_forward', 'lasr_render_tables_backward']
    if not from_imgs:
        natives.append('lasr_obs_pair')

    @case(name, natives)
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        from test_render_tables_gpu import make_case
        px, masks, occ, flow_obs, imgs, pp, fl = make_case(I, H, S, seed=7)
        masks[:, 0, 0], occ[:, 0, 0] = 1.0, 1.0
        px, pp, fl = _leaf(px, dev), _leaf(pp, dev), _leaf(fl, dev)
        masks, occ, flow_obs, imgs = masks.to(dev), occ.to(dev), flow_obs.to(dev), imgs.to(dev)
        if from_imgs:
            out = fused_ops.render_tables_imgs(px, masks, occ, flow_obs, imgs, pp, fl, 0.7, want_pair)
        else:
            out = fused_ops.render_tables(px, masks, occ, flow_obs, fused_ops.obs_pair(imgs, masks), pp, fl, 0.7, want_pair)
        for t in out[3:7]:                                      # flow, bg, fmap, vis: data, whichever path
            assert t.requires_grad is False
        if from_imgs:
            assert out[-1].requires_grad is False               # the observed pair the pass formed itself
        diff = list(out[:3]) + ([out[7]] if want_pair else [])
        return tuple(out) + _back(diff, [px, pp, fl], dev)


for _shape in _pixel_shapes():
    _add_pixel_cases(*_shape)


def _add_ssim(M, rep, S, save):
    @case('ssim/M%d-rep%d-S%d-save%d' % (M, rep, S, save), ['lasr_ssim_forward', 'lasr_ssim_backward'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        g = _gen(8)
        obs = torch.rand(M, 3, S, S + 2, generator=g).to(dev)
        rnd = _leaf(torch.rand(M * rep, 3, S, S + 2, generator=g), dev)
        d = fused_ops.ssim_distance(obs, rnd, rep, 1.0, save_planes=save)
        return (d,) + _back([d], [rnd], dev)


for _a in [(1, 1, 11, True), (1, 3, 17, True), (3, 1, 47, True), (1, 3, 17, False)]:
    _add_ssim(*_a)


# ---- cosine distances ----------------------------------------------------------------------------------------------------------------
def _add_cosdist(C, h, rep, N):
    @case('cosdist/C%d-h%d-rep%d-N%d' % (C, h, rep, N), ['lasr_cosdist_forward', 'lasr_cosdist_backward'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        g = _gen(9)
        fa = torch.randn(N // rep, C, h, h, generator=g).to(dev)
        fb = _leaf(torch.randn(N, C, h, h, generator=g), dev)
        d = fused_ops.cosine_distance(fa, fb, rep)
        return (d,) + _back([d], [fb], dev)


for _a in [(5, 7, 1, 1), (64, 7, 3, 3), (384, 3, 1, 3), (5, 7, 3, 6), (2, 1, 1, 1)]:
    _add_cosdist(*_a)


def _add_cosdist_multi(rep, N, layers):
    @case('cosdist_multi/rep%d-N%d-L%d' % (rep, N, len(layers)), ['lasr_cosdist_multi_forward', 'lasr_cosdist_multi_backward'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        g = _gen(10)
        fa = [torch.randn(N // rep, C, h, h, generator=g).to(dev) for C, h in layers]
        fb = [_leaf(torch.randn(N, C, h, h, generator=g), dev) for C, h in layers]
        d = fused_ops.cosine_distance_layers(fa, fb, rep)
        return (d,) + _back([d], fb, dev)


_add_cosdist_multi(1, 1, [(5, 7), (64, 7), (384, 3)])
_add_cosdist_multi(3, 3, [(384, 3), (5, 7), (64, 7)])
_add_cosdist_multi(1, 3, [(2, 1)])


# ---- mesh operators ---------------------------------------------------------------------------------------------------------------
def _lbs_inputs(N, V, K, dev, seed):
    g = _gen(seed)
    verts = _leaf(torch.randn(N, V, 3, generator=g) * 0.3, dev)
    R = _leaf(torch.linalg.qr(torch.randn(N * K, 3, 3, generator=g))[0], dev)
    T = _leaf(torch.randn(N * K, 1, 3, generator=g) * 0.2, dev)
    skin = _leaf(torch.softmax(torch.randn(N, max(K - 1, 1), V, 1, generator=g), 1), dev) if K > 1 else None
    return verts, R, T, skin


def _add_lbs(N, V, K):
    tag = 'N%d-V%d-K%d' % (N, V, K)
    for tocam in (True, False):
        @case('obj_to_cam/%s-tocam%d' % (tag, tocam), ['lasr_lbs_forward', 'lasr_lbs_backward'])
        def _(dev, tocam=tocam):
            from lasr_amd.nnutils import geom_utils
            verts, R, T, skin = _lbs_inputs(N, V, K, dev, 11)
            out = geom_utils.obj_to_cam(verts, R, T, K, 1, skin, tocam=tocam)
            return (out,) + _back([out], _tensors(verts, R, T, skin), dev)

    @case('obj_to_cam/%s-points-only' % tag, ['lasr_lbs_forward', 'lasr_lbs_backward'])
    def _(dev):
        from lasr_amd.nnutils import geom_utils
        verts, R, T, skin = _lbs_inputs(N, V, K, dev, 12)
        out = geom_utils.obj_to_cam(verts, R.detach(), T.detach(), K, 1, None if skin is None else skin.detach())
        return (out,) + _back([out], [verts], dev)

    @case('obj_to_cam_both/' + tag, ['lasr_lbs_forward_both', 'lasr_lbs_backward_both'])
    def _(dev):
        from lasr_amd.nnutils import geom_utils
        verts, R, T, skin = _lbs_inputs(N, V, K, dev, 13)
        cam, blend = geom_utils.obj_to_cam_both(verts, R, T, K, 1, skin)
        return (cam, blend) + _back([cam, blend], _tensors(verts, R, T, skin), dev)


for _a in [(3, 17, 21), (1, 65, 2), (1, 1, 1), (3, 65, 1)]:
    _add_lbs(*_a)


def _add_pinhole(n2, H, V):
    @case('pinhole_cam/n%d-H%d-V%d' % (n2, H, V), ['lasr_pinhole_forward', 'lasr_pinhole_backward'])
    def _(dev):
        from lasr_amd.nnutils import geom_utils
        g = _gen(14)
        v = torch.randn(n2 * H, V, 4, generator=g) * 0.3
        v[:, :, 2] += 8
        v, pp, fl = _leaf(v, dev), _leaf(0.1 * torch.randn(n2, 2, generator=g), dev), _leaf(torch.rand(n2 * H, generator=g) + 8, dev)
        out = geom_utils.pinhole_cam(v, pp, fl)
        return (out,) + _back([out], [v, pp, fl], dev)


for _a in [(1, 1, 1), (1, 3, 17), (3, 1, 65)]:
    _add_pinhole(*_a)


def _add_project_points(n2, H, K):
    @case('project_points/n%d-H%d-K%d' % (n2, H, K), ['lasr_project_points_forward', 'lasr_project_points_backward'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        g = _gen(15)
        M, nb = n2 * H, K - 1
        rest, ctl = _leaf(0.3 * torch.randn(H * nb, 3, generator=g), dev), _leaf(0.3 * torch.randn(H * nb, 3, generator=g), dev)
        R = torch.randn(M * K, 3, 3, generator=g).to(dev)
        T = torch.randn(M * K, 3, generator=g)
        T.view(M, K, 3)[:, 0, 2] += 8
        ppoint, scale = (0.1 * torch.randn(n2, 2, generator=g)).to(dev), (torch.rand(n2, H, generator=g) + 8).to(dev)
        out = fused_ops.project_points(rest, ctl, R, T.to(dev), ppoint, scale, H, K)
        return (out,) + _back([out], [rest, ctl], dev)


for _a in [(1, 1, 2), (2, 3, 21), (1, 3, 2)]:
    _add_project_points(*_a)


def _pose_inputs(B, H, K, dev, seed):
    g = _gen(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                                     # noqa: E731
    n2, M = 2 * B, 2 * B * H
    cams = torch.cat([1 + 0.3 * torch.rand(n2, 1, generator=g), torch.randn(n2, 6, generator=g)], 1).to(dev)
    pp = (20 * r(n2, 2)).to(dev)
    quat = torch.nn.functional.normalize(r(M * K, 4) + torch.tensor([0, 0, 0, 3.]), dim=1)
    v = dict(scale=1 + 0.1 * r(n2, H).abs(), depth=8 + r(n2, K).abs(), ppoint=0.1 * r(n2, 2), quat=quat, trans=0.1 * r(n2 * K, 2),
             rest=0.2 * r(H, max(K - 1, 0) * 3), ctl=0.2 * r(H, max(K - 1, 0) * 3))
    return cams, pp, {k: _leaf(t, dev) for k, t in v.items()}


def _add_pose(B, H, K):
    tag = 'B%d-H%d-K%d' % (B, H, K)

    @case('pose_chain/' + tag, ['lasr_pose_chain_forward', 'lasr_pose_chain_backward'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        cams, pp, v = _pose_inputs(B, H, K, dev, 16)
        out = fused_ops.pose_chain(cams, pp, v['scale'], v['depth'], v['ppoint'], v['quat'], v['trans'], v['rest'], v['ctl'], H, K, 256)
        out = _tensors(*out)
        leaves = [v[k] for k in ('scale', 'depth', 'ppoint', 'quat', 'trans')] + ([v['rest'], v['ctl']] if K > 1 else [])
        return out + _back(out, leaves, dev)

    @case('intrinsics/' + tag, ['lasr_intrinsics_forward', 'lasr_intrinsics_backward'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        cams, pp, v = _pose_inputs(B, H, K, dev, 17)
        out = fused_ops.intrinsics(cams, pp, v['scale'], v['depth'], v['ppoint'], 256)
        return tuple(out) + _back(out, [v['scale'], v['depth'], v['ppoint']], dev)

    for pair in (False, True):
        @case('bone_fixup/%s-pair%d' % (tag, pair), ['lasr_bone_fixup_pair_forward', 'lasr_bone_fixup_pair_backward'] if pair else
              ['lasr_bone_fixup_forward', 'lasr_bone_fixup_backward'])
        def _(dev, pair=pair):
            from lasr_amd.nnutils import fused_ops
            g = _gen(18)
            MK = 2 * B * H * K
            q = torch.linalg.qr(torch.randn(MK, 3, 3, generator=g))[0]
            leaves = [_leaf(q.reshape(MK, 9), dev), _leaf(torch.randn(MK, 2, generator=g), dev),
                      _leaf(torch.randn(MK, 1, generator=g) + 8, dev)]
            rest = _leaf(0.3 * torch.randn(H, (K - 1) * 3, generator=g), dev) if K > 1 else None
            out = fused_ops.bone_fixup(leaves[0], leaves[1], leaves[2], rest, H, K, pair_angle=pair)
            return tuple(out) + _back(out, leaves + ([rest] if K > 1 else []), dev)


for _a in [(1, 1, 1), (1, 3, 21), (2, 1, 2)]:
    _add_pose(*_a)


def _add_small(n):
    @case('geodesic_distance/n%d' % n, ['lasr_geodesic_forward', 'lasr_geodesic_backward'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        g = _gen(19)
        m1 = _leaf(torch.linalg.qr(torch.randn(n, 3, 3, generator=g))[0], dev)
        m2 = _leaf(torch.linalg.qr(torch.randn(n, 3, 3, generator=g))[0] + 0.01 * torch.randn(n, 3, 3, generator=g), dev)
        out = fused_ops.geodesic_distance(m1, m2)
        return (out,) + _back([out], [m1, m2], dev)

    @case('quat_to_rotmat/n%d' % n, ['lasr_quat_to_rotmat_forward', 'lasr_quat_to_rotmat_backward'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        q = _leaf(torch.randn(n, 4, generator=_gen(20)), dev)
        out = fused_ops.quat_to_rotmat(q)
        return (out,) + _back([out], [q], dev)


for _n in (1, 17, 65):
    _add_small(_n)


def _add_skin(H, J, V):
    @case('skin_weights/H%d-J%d-V%d' % (H, J, V), ['lasr_skin_weights_forward', 'lasr_skin_weights_backward'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        g = _gen(21)
        ts, lc = _leaf(0.3 * torch.randn(H * J, 3, generator=g), dev), _leaf(0.2 * torch.randn(H * J, 3, generator=g) - 1, dev)
        rs = _leaf(torch.nn.functional.normalize(torch.randn(H * J, 4, generator=g), dim=1), dev)
        verts = (0.3 * torch.randn(H, V, 3, generator=g)).to(dev)
        out = fused_ops.skin_weights(ts, rs, lc, verts)
        return (out,) + _back([out], [ts, rs, lc], dev)


for _a in [(1, 2, 1), (3, 20, 17), (1, 2, 65), (3, 21, 65)]:
    _add_skin(*_a)


@case('weighted_mean_sum', ['lasr_weighted_means_forward', 'lasr_weighted_means_backward'])
def _(dev):
    from lasr_amd.nnutils import fused_ops
    g = _gen(22)
    xs = [_leaf(torch.randn(*s, generator=g), dev) for s in [(1,), (17,), (3, 3), (17, 17), (2209,)]]
    total, sums = fused_ops.weighted_mean_sum([(x, 0.5 + i, i % 3) for i, x in enumerate(xs)])
    return (total, sums) + _back([total], xs, dev)


def _add_mean_shape(H, Vp, S, R):
    @case('mean_shape/H%d-Vp%d-S%d-R%d' % (H, Vp, S, R), ['lasr_mean_shape_forward', 'lasr_mean_shape_backward'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        g = _gen(23)
        mean_v, tex = _leaf(torch.randn(H, Vp, 3, generator=g), dev), _leaf(torch.randn(H, Vp, 3, generator=g), dev)
        flip = torch.tensor([[-1., 1., 1.]]).to(dev) if S else None
        mask = (torch.rand(Vp + S, 3, generator=g) > 0.2).float().to(dev) if S else None
        out = fused_ops.mean_shape(mean_v, tex, flip, mask, R, S)
        return tuple(out) + _back(out, [mean_v, tex], dev)


for _a in [(1, 1, 0, 1), (3, 10, 7, 2), (1, 40, 25, 3)]:
    _add_mean_shape(*_a)


def _add_chamfer(N, P, Q):
    @case('chamfer/N%d-P%d-Q%d' % (N, P, Q), ['lasr_chamfer_forward', 'lasr_chamfer_backward'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        g = _gen(24)
        a, b = _leaf(torch.randn(N, P, 3, generator=g), dev), _leaf(torch.randn(N, Q, 3, generator=g), dev)
        out = fused_ops.chamfer(a, b)
        return (out,) + _back([out], [a, b], dev)

    P2 = max(P, 2)                                          # (no gradient here: one query point alone would be one value)

    @case('nearest_point/N%d-P%d-Q%d' % (N, P2, Q), ['lasr_nearest_point'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        g = _gen(25)
        d2, idx = fused_ops.nearest_point(torch.randn(N, P2, 3, generator=g).to(dev), torch.randn(N, Q, 3, generator=g).to(dev))
        return (d2, idx)

    @case('chamfer_3DDist/N%d-P%d-Q%d' % (N, P, Q), ['lasr_chamfer3d_forward', 'lasr_chamfer3d_backward'])
    def _(dev):
        from lasr_amd.chamfer3D.dist_chamfer_3D import chamfer_3DDist
        g = _gen(26)
        a, b = _leaf(torch.randn(N, P, 3, generator=g), dev), _leaf(torch.randn(N, Q, 3, generator=g), dev)
        d1, d2, i1, i2 = chamfer_3DDist()(a, b)
        return (d1, d2, i1, i2) + _back([d1, d2], [a, b], dev)

    @case('nn_tiled/N%d-P%d-Q%d' % (N, P2, Q), ['lasr_nn_tiled'])
    def _(dev):
        from lasr_amd.chamfer3D import dist_chamfer_3D
        g = _gen(27)
        a, b = torch.randn(N, P2, 3, generator=g).to(dev), torch.randn(N, Q, 3, generator=g).to(dev)
        R = torch.linalg.qr(torch.randn(N, 3, 3, generator=g))[0].to(dev)
        d2, idx = dist_chamfer_3D.nn_tiled(a, b, R, (0.1 * torch.randn(N, 3, generator=g)).to(dev))
        return (d2, idx)


for _a in [(1, 1, 1), (3, 17, 65), (1, 257, 1), (3, 1, 257), (1, 257, 257)]:
    _add_chamfer(*_a)


def _add_point_mesh(N, V, F, P):
    @case('point_mesh_face_distance/N%d-V%d-F%d-P%d' % (N, V, F, P),
          ['lasr_point_mesh_forward', 'lasr_point_mesh_backward', 'lasr_face_gather_backward', 'lasr_face_gather_backward_csr'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        from lasr_amd.soft_renderer.functional import geometry
        geometry.invalidate_incidence()
        g = _gen(28)
        faces = _random_faces(g, V, F).to(dev)
        res = []
        for _ in range(2):                                # the second sight of a face tensor takes the incidence lists
            verts, pts = _leaf(torch.randn(N, V, 3, generator=g), dev), _leaf(torch.randn(N, P, 3, generator=g), dev)
            d = fused_ops.point_mesh_face_distance(verts, faces, pts)
            res += [d.detach().reshape(1)] + list(_back([d], [verts, pts], dev))
        return tuple(res)


for _a in [(1, 3, 1, 1), (3, 65, 257, 1), (1, 17, 1, 257), (3, 65, 257, 257)]:
    _add_point_mesh(*_a)


def _criteria(mesh, dev):
    from lasr_amd.nnutils import loss_utils
    v, f = _mesh(mesh)
    vt, ft = torch.from_numpy(v), torch.from_numpy(f)
    return (vt, loss_utils.LaplacianLoss(vt, ft).to(dev), loss_utils.ARAPLoss(vt, ft).to(dev), loss_utils.FlattenLoss(ft).to(dev))


def _add_mesh_losses(mesh, N, NA):
    tag = '%s-N%d-NA%d' % (mesh, N, NA)

    def inputs(dev, seed):
        vt, lap, arap, flat = _criteria(mesh, dev)
        g = _gen(seed)
        x = _leaf(vt[None] + 0.05 * torch.randn(N, vt.shape[0], 3, generator=g), dev)
        d0 = _leaf(vt[None] + 0.05 * torch.randn(NA, vt.shape[0], 3, generator=g), dev)
        d1 = _leaf(vt[None] + 0.05 * torch.randn(NA, vt.shape[0], 3, generator=g), dev)
        return g, x, d0, d1, lap, arap, flat

    @case('laplacian/' + tag, ['lasr_laplacian_forward', 'lasr_laplacian_backward'])
    def _(dev):
        g, x, d0, d1, lap, arap, flat = inputs(dev, 29)
        out = lap(x)
        return (out,) + _back([out], [x], dev)

    @case('arap/' + tag, ['lasr_arap_forward', 'lasr_arap_backward'])
    def _(dev):
        g, x, d0, d1, lap, arap, flat = inputs(dev, 30)
        out = arap(d0, d1)
        return (out,) + _back([out], [d0, d1], dev)

    @case('flatten/' + tag, ['lasr_flatten_forward', 'lasr_flatten_backward'])
    def _(dev):
        g, x, d0, d1, lap, arap, flat = inputs(dev, 31)
        out = flat(x)
        return (out,) + _back([out], [x], dev)

    for NC, P in ((0, 0), (3, 17)):
        @case('mesh_regularisers/%s-NC%d' % (tag, NC), ['lasr_step_regularisers_forward', 'lasr_step_regularisers_backward'])
        def _(dev, NC=NC, P=P):
            from lasr_amd.nnutils import fused_ops
            g, x, d0, d1, lap, arap, flat = inputs(dev, 32)
            leaves, pair = [x, d0, d1], None
            if NC:
                ctl = _leaf(0.3 * torch.randn(NC, P, 3, generator=g), dev)
                leaves, pair = leaves + [ctl], (ctl, ctl * torch.tensor([-1., 1., 1.], device=dev))
            out = fused_ops.mesh_regularisers(x, d0, d1, lap, flat, arap, pair)
            return tuple(out) + _back(out, leaves, dev)


_add_mesh_losses('sphere17', 3, 1)
_add_mesh_losses('fan65', 1, 1)
_add_mesh_losses('fan65', 3, 3)


def _raster_geometry(mesh, N, dev, seed):
    v, f = _mesh(mesh)
    g = _gen(seed)
    V = v.shape[0]
    cam = torch.from_numpy(v)[None] * 0.5 + 0.05 * torch.randn(N, V, 3, generator=g)
    cam[:, :, 2] += 8
    tex, pp, fl = torch.rand(N, V, 3, generator=g), 0.1 * torch.randn(N, 2, generator=g), torch.rand(N, generator=g) + 8
    return g, [_leaf(t, dev) for t in (cam, tex, pp, fl)], torch.from_numpy(f), V


def _add_raster_glue(mesh, N):
    tag = '%s-N%d' % (mesh, N)
    eye = [0.0, 0.0, -2.732]

    N2 = 2 * N          # raster_inputs / raster_faces pair image n with (n + N/2) % N and refuse an odd batch: 2 and 6 images there

    @case('raster_inputs/%s-N%d' % (mesh, N2), ['lasr_raster_inputs_forward', 'lasr_raster_inputs_backward'])
    def _(dev):
        from lasr_amd.nnutils import fused_ops
        g, leaves, f, V = _raster_geometry(mesh, N2, dev, 33)
        pre, attrs, nf = fused_ops.raster_inputs(*leaves, eye)
        return (pre, attrs, nf) + _back([pre, attrs], leaves, dev)

    for shared in (True, False):
        @case('raster_faces/%s-N%d-shared%d' % (mesh, N2, shared), ['lasr_raster_faces_forward', 'lasr_raster_faces_backward'])
        def _(dev, shared=shared):
            from lasr_amd.nnutils import fused_ops
            g, leaves, f, V = _raster_geometry(mesh, N2, dev, 34)
            faces = f[None].to(dev) if shared else torch.stack([f.roll(n, 0) for n in range(N2)]).to(dev)
            fv, fa, nf = fused_ops.raster_faces(*leaves, eye, faces.contiguous(), fused_ops.face_incidence(faces, V))
            return (fv, fa, nf) + _back([fv, fa], leaves, dev)

    for C in ((3, 9) if mesh == 'one' else (1, 3, 9)):       # (one vertex with one channel: every output would be one value)
        @case('face_vertices/%s-C%d' % (tag, C), ['lasr_face_gather_forward', 'lasr_face_gather_backward', 'lasr_face_gather_backward_csr'])
        def _(dev, C=C):
            from lasr_amd.soft_renderer.functional import geometry
            geometry.invalidate_incidence()
            g, _, f, V = _raster_geometry(mesh, N, dev, 35)
            faces = f[None].repeat(N, 1, 1).to(dev)
            res = []
            for _ in range(2):                            # the second sight of a face tensor takes the incidence lists
                attr = _leaf(torch.randn(N, V, C, generator=g), dev)
                out = geometry.face_vertices(attr, faces)
                res += [out] + list(_back([out], [attr], dev))
            return tuple(res)


_add_raster_glue('sphere17', 3)
_add_raster_glue('fan65', 1)
_add_raster_glue('one', 1)
_add_raster_glue('fan65', 3)


# ---- the rasteriser through the operator -------------------------------------------------------------------------------------------
HARD = dict(dist_func='hard', aggr_func_rgb='hard', aggr_func_alpha='hard')
SURFACE_ATOMIC = dict(exact=False, atomic='sr_backward.h: sr_backward_kernel (surface texels)', tol=1e-3,
                      tol_from='tests/test_raster_parity_gpu.py::test_surface_textures (GRAD_REL)')
FP64_ATOMIC = dict(exact=False, atomic='sr_fp64.hip: backward_kernel', tol=1e-9,
                   tol_from='tests/test_raster_fp64_gpu.py::test_every_mode_combination_against_the_double_oracle')


from raster_harness import raster_batch as _raster_batch             # noqa: E402 (the raster tests render the same batch)


def _add_raster(N, F, IS, C=3, modes=None, surface=0, dtype=torch.float32, **kw):
    modes = modes or {}
    name = 'soft_rasterize/N%d-F%d-IS%d-C%d%s%s%s' % (N, F, IS, C, '-hard' if modes else '', '-surface%d' % surface if surface else '',
                                                       '-fp64' if dtype == torch.float64 else '')
    natives = ['lasr_sr_forward_f64', 'lasr_sr_backward_f64'] if dtype == torch.float64 else ['lasr_sr_forward_opt', 'lasr_sr_backward_ex']

    @case(name, natives, **kw)
    def _(dev):
        from lasr_amd.soft_renderer import functional as srf
        op = importlib.import_module('lasr_amd.soft_renderer.functional.soft_rasterize')    # (the package re-exports the function)
        op._workspaces.clear()                             # (a workspace of this run's own, not a larger earlier call's)
        fv, near, far = _raster_batch(N, F)
        g = _gen(37)
        tfv = _leaf(torch.from_numpy(fv).to(dtype), dev)
        tft = _leaf(torch.rand(N, F, surface * surface if surface else 3, C, generator=g).to(dtype), dev)
        opts = dict(synth.LASR_MODES, near=near, far=far, **modes)
        if surface:
            opts['texture_type'] = 'surface'
        img = srf.soft_rasterize(tfv, tft, IS, **opts)
        up = (torch.randn(N, C + 1, IS, IS, generator=g) / (IS * IS)).to(dtype).to(dev)
        if dtype == torch.float64:                          # (that path allocates with zeros / ones: the gradient it reads is guarded)
            up = op.torch.empty(up.shape, dtype=dtype, device=dev).copy_(up)
        grads = torch.autograd.grad([img], [tfv, tft], [up], allow_unused=True)
        op._workspaces.clear()
        return (img,) + tuple(x for x in grads if x is not None)


for _N, _F, _IS in [(3, 1, 8), (3, 65, 24), (3, 257, 33), (8, 65, 64)]:
    for _C in (3, 6, 9):
        _add_raster(_N, _F, _IS, _C)
    _add_raster(_N, _F, _IS, 3, HARD)
    _add_raster(_N, _F, _IS, 3, surface=2, inexact=[2], **SURFACE_ATOMIC)
for _N, _F, _IS in [(3, 1, 8), (3, 65, 24), (3, 257, 33)]:
    _add_raster(_N, _F, _IS, 3, dtype=torch.float64, inexact=[1, 2], **FP64_ATOMIC)
    _add_raster(_N, _F, _IS, 3, HARD, dtype=torch.float64, inexact=[1, 2], **FP64_ATOMIC)
_add_raster(3, 65, 24, 3, surface=2, dtype=torch.float64, inexact=[1, 2], **FP64_ATOMIC)


# ---- everything else that launches: the smallest case of the operator's own GPU test, made ragged ---------------------------------------
def _guarded_copy(module, t):
    """t re-housed in a tensor from `module`'s own allocator (guarded under the harness): for wrappers that allocate nothing with
    torch.empty themselves (zero-filled outputs), so that at least the tensors they write next to are banded."""
    return module.torch.empty(tuple(t.shape), dtype=t.dtype, device=t.device).copy_(t)


def _sequence(dev, T=3):
    """(verts [T,162,3], faces int64 [320,3], K [T,4]) of tests/tracks_cases.sphere_case on the device; frames of 47 x 61 pixels."""
    import tracks_cases as tc
    v, f, K = tc.sphere_case(T)
    return torch.from_numpy(v).to(dev), torch.from_numpy(np.asarray(f, np.int64)).to(dev), torch.from_numpy(K).to(dev)


SEQ_H, SEQ_W = 47, 61


@case('load_textures', ['lasr_load_textures'])
def _(dev):
    mod = importlib.import_module('lasr_amd.soft_renderer.functional.load_textures')
    g = _gen(40)
    image = _guarded_copy(mod, torch.rand(17, 33, 3, generator=g).to(dev))
    uv = torch.rand(65, 3, 2, generator=g).to(dev)
    upd = (torch.rand(65, generator=g) > 0.2).int().to(dev)
    return (mod.load_textures(image, uv, 3, upd), mod.load_textures(image, uv[:1], 1))


for _dt in (torch.float32, torch.float64):
    @case('create_texture_image/%s' % str(_dt).split('.')[1], ['lasr_create_texture_image_f64' if _dt == torch.float64 else
                                                              'lasr_create_texture_image'])
    def _(dev, dt=_dt):
        obj_io = importlib.import_module('lasr_amd.soft_renderer.functional.obj_io')
        tex = torch.rand(17, 9, 3, generator=_gen(41)).to(dt).to(dev)                # 17 faces: a 5 x 4 grid of tiles, three unused
        image, vt = obj_io.create_texture_image(tex, 5)
        one, _ = obj_io.create_texture_image(tex[:1], 2)
        return (torch.from_numpy(image.copy()), torch.from_numpy(vt), torch.from_numpy(one.copy()))

    @case('voxelization/%s' % str(_dt).split('.')[1], ['lasr_voxelize_f64' if _dt == torch.float64 else 'lasr_voxelize'])
    def _(dev, dt=_dt):
        vox = importlib.import_module('lasr_amd.soft_renderer.functional.voxelization')
        v, f = synth.geodesic_sphere(1)
        faces = torch.from_numpy((v * 0.35 + 0.5)[f]).to(dt)
        faces = torch.stack([faces, faces * 0.8 + 0.1, faces * 0.5 + 0.3]).to(dev)   # [3,20,3,3] in the unit cube
        return (vox.voxelization(faces, 17), vox.voxelization(faces[:1, :1], 1), vox.voxelization(faces[:1], 65))


@case('kp_transfer', ['lasr_kp_transfer'])
def _(dev):
    from lasr_amd.nnutils import keypoints
    g = _gen(42)
    colors = torch.randn(3, 4, 33, 33, generator=g)
    colors[:, 2] = (torch.rand(3, 33, 33, generator=g) > 0.4).float() * 5            # depth plane: 0 = background
    kp = torch.rand(3, 5, 2, generator=g) * torch.tensor([17., 33.])
    idx, pred = keypoints.kp_transfer(colors.to(dev), kp.to(dev), 17, 33)
    idx1, pred1 = keypoints.kp_transfer(None, kp[:1, :1].to(dev), 2, 2)
    return (idx, pred, idx1, pred1)


@case('rig', ['lasr_rig_pack', 'lasr_rig_quats', 'lasr_rig_skin', 'lasr_rig_stats'])
def _(dev):
    from lasr_amd.nnutils import rig
    g = _gen(43)
    J, V, T = 9, 65, 3
    skin = torch.softmax(3 * torch.randn(J, V, generator=g), 0).to(dev)
    R = torch.linalg.qr(torch.randn(T, J + 1, 3, 3, generator=g))[0]
    R = R * torch.linalg.det(R).sign()[..., None, None]
    rest, trans = torch.randn(V, 3, generator=g).to(dev), torch.randn(T, J + 1, 3, generator=g).to(dev)
    out = []
    for k in (4, 8):
        joints, weights, dropped = rig.pack_influences(skin, k)
        quat = rig.rotation_keys(R.to(dev))
        posed = rig.skin_packed(rest, joints, weights, quat, trans)
        out += [joints, weights, dropped, quat, posed, rig.deviation(posed, posed.flip(0))]
    body = rig.skin_packed(rest[:1], None, None, quat[:, :1].contiguous(), trans[:, :1].contiguous())      # one vertex, the body alone
    return tuple(out) + (body,)


@case('phong_render', ['lasr_sr_forward_bg', 'lasr_phong_shade'])
def _(dev):
    from lasr_amd import phong
    v, f = synth.geodesic_sphere(1)
    g = _gen(44)
    verts = (torch.from_numpy(v)[None] * 0.6 + 0.03 * torch.randn(3, 12, 3, generator=g)).to(dev)
    return (phong.render(verts, torch.from_numpy(f).to(dev), torch.rand(12, 3, generator=g).to(dev), 17),
            phong.render(verts[:1], torch.from_numpy(f[:1]).to(dev), torch.rand(12, 3, generator=g).to(dev), 1))


@case('vis_shade', ['lasr_sr_forward_bg', 'lasr_vis_shade'])
def _(dev):
    from lasr_amd import vis
    v, f = synth.geodesic_sphere(1)
    g = _gen(45)
    verts = torch.from_numpy(v)[None] * 0.6 + 0.03 * torch.randn(3, 12, 3, generator=g)
    verts[:, :, 2] += 8
    K = torch.tensor([[150., 140., 16.3, 9.1]]).repeat(3, 1)
    frames = torch.randint(0, 256, (3, 17, 33, 3), generator=g, dtype=torch.uint8).to(dev)
    a = vis.shade(verts.to(dev), torch.from_numpy(f).to(dev), torch.rand(12, 3, generator=g).to(dev), K.to(dev), 33, 17, 33, n_opaque=13)
    b = vis.shade(verts.to(dev), torch.from_numpy(f).to(dev), torch.rand(12, 3, generator=g).to(dev), K.to(dev), 33, 17, 33, frames=frames)
    return (a, b)


@case('flow_to_image', ['lasr_flow_to_image'])
def _(dev):
    from lasr_amd.ext_utils import flowlib
    g = _gen(46)
    flow = (4 * torch.randn(3, 17, 47, 2, generator=g)).to(dev)
    mask = (torch.rand(3, 17, 47, generator=g) > 0.4).float().to(dev)
    return (flowlib.flow_to_image(flow), flowlib.flow_to_image(flow, mask), flowlib.flow_to_image(flow[:1, :1, :1]))


@case('monitor_sheet', ['lasr_monitor_sheet'])
def _(dev):
    import flowvis_cases as fc
    from lasr_amd.nnutils import monitor
    out = []
    for IS, n_bones in ((17, 4), (17, 1)):
        c = fc.sheet_case(IS, n_bones)
        B, H, cam = c['batch_size'], c['n_hypo'], c['optim_cam']
        t = {k: torch.from_numpy(v).to(dev) for k, v in c.items() if isinstance(v, np.ndarray) and k != 'part_render'}
        px = t['px']
        part = torch.from_numpy(c['part_render'].base).to(dev)[:, :3] if n_bones > 1 else None
        planes = dict(flow_obs=(t['flow'][0, :2], 0), flow_rd=(t['flow_rd'].view(2 * B, H, IS, IS, 2)[0, cam], -1),
                      vis_mask=(t['vis_mask'][0, cam], None), flow_err=(t['flow_rd_map'][0, cam], None), mask_pred=(px[:, 9][cam], None),
                      mask_gt=(t['masks'][0], None), part=(part[0] if part is not None else None, 0), img1=(t['imgs'][0], 0),
                      img2=(t['imgs'][B], 0), texture=(px[:, :3][cam], 0))
        ctl = t['ctl_proj'][cam] if n_bones > 1 else None
        pal = torch.from_numpy(synth.label_palette(max(n_bones - 1, 1))).to(dev)
        scratch = torch.zeros(16, dtype=torch.int32, device=dev)
        out += [monitor.sheet(planes, ctl, pal, IS, scratch), scratch]
    return tuple(out)


@case('scalar_ring', ['lasr_scalar_ring_push'])
def _(dev):
    import flowvis_cases as fc
    from lasr_amd.nnutils import monitor
    ring = monitor.ScalarRing(len(fc.RING_COUNTS), 4, dev)
    sets = [[monitor.torch.empty(n, dtype=torch.float32, device=dev) for n in fc.RING_COUNTS] for _ in range(2)]
    for n, vals in enumerate(fc.ring_pushes(5)):
        for d, v in zip(sets[n % 2], vals):
            d.copy_(torch.from_numpy(v))
        ring.push(sets[n % 2])
    return (ring.ring, ring.head)


@case('bake', ['lasr_sr_forward_bg', 'lasr_bake_accumulate', 'lasr_bake_resolve', 'lasr_bake_mirror', 'lasr_bake_blend'])
def _(dev):
    from lasr_amd.nnutils import bake
    tv, tf, tK = _sequence(dev)
    g = _gen(47)
    frames = torch.randint(0, 256, (3, SEQ_H, SEQ_W, 3), generator=g, dtype=torch.uint8).to(dev)
    masks = (torch.rand(3, SEQ_H, SEQ_W, generator=g) > 0.2).float().to(dev)
    tex, w = bake.bake_texture(tv, tf, tK, frames, masks, texture_res=3, fallback=torch.rand(162, 3, generator=g).to(dev))
    tex1, w1 = bake.bake_texture(tv[:1], tf[:1], tK[:1], frames[:1], texture_res=1)
    rest = tv[0] - tv[0].mean(0)
    m, src, info = bake.complete_texture(tf, tex, w, fill='mirror', rest_verts=rest, iters=3)
    b, src_b, _ = bake.complete_texture(tf, tex, w, fill='blend', iters=2)
    return (tex, w, tex1, w1, m, src, info['texels'], info['src'], info['d2'], b, src_b)


@case('tracks', ['lasr_sr_forward_bg', 'lasr_track_anchor', 'lasr_track_project', 'lasr_track_splat_keys', 'lasr_track_splat_resolve'])
def _(dev):
    from lasr_amd.nnutils import tracks
    tv, tf, tK = _sequence(dev)
    g = _gen(48)
    Q = 257
    q = torch.stack([torch.randint(0, 3, (Q,), generator=g).float(), torch.rand(Q, generator=g) * SEQ_H, torch.rand(Q, generator=g) * SEQ_W], 1)
    tr, state, anc = tracks.track_points(tv, tf, tK, q.to(dev), SEQ_H, SEQ_W, snap_radius=2, window=1)
    tr1, state1, _ = tracks.track_points(tv[:1], tf, tK[:1], q[:1].to(dev) * torch.tensor([0., 1., 1.], device=dev), SEQ_H, SEQ_W)
    frames = torch.randint(0, 256, (3, SEQ_H, SEQ_W, 3), generator=g, dtype=torch.uint8).to(dev)
    colors = torch.randint(0, 256, (Q, 3), generator=g, dtype=torch.uint8).to(dev)
    seen = torch.where(torch.isfinite(tr).all(2), state, torch.zeros_like(state))
    out = tracks.splat(frames, torch.nan_to_num(tr), seen, colors, radius=2)
    return (tr, state, anc['face'], anc['bary'], anc['facing'], anc['snapped'], tr1, state1, out)


@case('reproj', ['lasr_sr_forward_bg', 'lasr_reproj_pixels', 'lasr_reproj_boundary'])
def _(dev):
    from lasr_amd.nnutils import reproj
    tv, tf, tK = _sequence(dev)
    g = _gen(49)
    masks = (torch.rand(3, SEQ_H, SEQ_W, generator=g) > 0.5).float().to(dev)
    masks[:, 10:30, 15:45] = 1.
    flows = torch.cat([2 * torch.randn(2, SEQ_H, SEQ_W, 2, generator=g), (torch.rand(2, SEQ_H, SEQ_W, 1, generator=g) > 0.2).float()], 3).to(dev)
    occs = (torch.rand(2, SEQ_H, SEQ_W, generator=g) * 12).to(dev)
    frames = torch.randint(0, 256, (3, SEQ_H, SEQ_W, 3), generator=g, dtype=torch.uint8).to(dev)
    colors = torch.randint(0, 256, (3, 162, 3), generator=g, dtype=torch.uint8).to(dev)
    a = reproj.evaluate(tv, tf, tK, masks, flows=flows, occs=occs, frames=frames, colors=colors, bound_th=2)
    b = reproj.evaluate(tv[:1], tf, tK[:1], masks[:1])
    return (a['counts'], a['sums'], a['bits'], a['boundary_bits'], b['counts'], b['bits'], b['boundary_bits'])


@case('meshcheck', ['lasr_meshcheck_faces', 'lasr_meshcheck_pairs'])
def _(dev):
    from lasr_amd.nnutils import meshcheck
    g = _gen(50)
    v, f = _mesh('sphere17')
    verts = torch.from_numpy(v)[None] + 0.4 * torch.randn(3, 17, 3, generator=g)          # crumpled: faces cross
    faces = torch.from_numpy(f).to(dev)
    n, count, _, _ = meshcheck.self_intersections(verts.to(dev), faces, max_pairs=65)
    vol, area = meshcheck.volume_area(verts.to(dev), faces)
    n1, count1, _, _ = meshcheck.self_intersections(verts[:1].to(dev), faces[:1], max_pairs=1)
    big = torch.randn(1, 65, 3, generator=g).to(dev)
    n2, count2, _, _ = meshcheck.self_intersections(big, _random_faces(g, 65, 257).to(dev), max_pairs=17)
    return (n, count, vol, area, n1, count1, n2, count2)


@case('manifold_remesh', ['lasr_voxelize', 'lasr_manifold_repair', 'lasr_manifold_count', 'lasr_manifold_extract',
                          'lasr_point_mesh_forward', 'lasr_manifold_project', 'lasr_manifold_guard'])
def _(dev):
    from lasr_amd.nnutils import manifold
    v, f = synth.geodesic_sphere(1)
    g = _gen(51)
    verts = (torch.from_numpy(v) * torch.tensor([0.7, 0.45, 0.5]) + 0.02 * torch.randn(12, 3, generator=g)).to(dev)
    r = manifold.remesh(verts, torch.from_numpy(f).to(dev), 1)
    return (r['verts'], r['faces'], r['lattice'], r['moved'], r['voxels'])


@case('icp', ['lasr_icp_init', 'lasr_icp_iterate'])
def _(dev):
    from lasr_amd.nnutils.icp import iterative_closest_point
    g = _gen(52)
    Y = torch.randn(3, 65, 3, generator=g) * torch.tensor([1.0, 0.6, 0.4])
    X = torch.randn(3, 257, 3, generator=g) * torch.tensor([1.0, 0.6, 0.4]) + 0.1
    sol = iterative_closest_point(X.to(dev), Y.to(dev), max_iterations=5, relative_rmse_thr=-1., chunk=2)
    one = iterative_closest_point(X[:1, :1].to(dev), Y[:1, :1].to(dev), max_iterations=2, relative_rmse_thr=-1.)
    return (sol.rmse, sol.Xt, sol.RTs.R, sol.RTs.T, one.rmse, one.Xt, one.RTs.T)


@case('vcn', ['lasr_vcn_corr_proj', 'lasr_vcn_flow_reg'])
def _(dev):
    from lasr_amd.ext_nnutils import vcn
    g = _gen(53)
    b, C, h, w, Fo, md = 3, 5, 7, 9, 12, 2                       # (the projection has 12 or 16 outputs)
    c1, c2 = torch.randn(b, C, h, w, generator=g).to(dev), torch.randn(b, C, h, w, generator=g).to(dev)
    fl = torch.randn(b, 2, h, w, generator=g).to(dev)
    W, sc, sh = torch.randn(Fo, C, generator=g).to(dev), (torch.rand(Fo, generator=g) + 0.5).to(dev), torch.randn(Fo, generator=g).to(dev)
    cost = vcn.corr_proj(c1, c2, fl, W, sc, sh, md, md)
    cost0 = vcn.corr_proj(c1[:1, :, :1, :1].contiguous(), c2[:1, :, :1, :1].contiguous(), None, W, sc, sh, md, md)
    flow, ent = vcn.flow_reg(cost, fl, md, md)
    flow0, ent0 = vcn.flow_reg(cost0, None, md, md)
    return (cost, cost0, flow, ent, flow0, ent0)


@case('varflow', ['lasr_varflow_reduce', 'lasr_varflow_expand', 'lasr_varflow_tensor', 'lasr_varflow_weights', 'lasr_varflow_sor',
                  'lasr_varflow_occ'])
def _(dev):
    from lasr_amd.nnutils import varflow
    g = _gen(54)
    base = torch.rand(47 + 4, 65 + 4, 3, generator=g)
    base = torch.nn.functional.avg_pool2d(base.permute(2, 0, 1)[None], 5, 1, 2)[0].permute(1, 2, 0)     # smooth: a flow exists
    A = (base[2:49, 2:67] * 255).to(torch.uint8).to(dev)
    B = (base[3:50, 1:66] * 255).to(torch.uint8).to(dev)
    return tuple(varflow.flow_pair(A, B, NW=2, NO=2, NI=3)) + tuple(varflow.flow_pair(A[:2, :2].contiguous(), B[:2, :2].contiguous(), NW=1, NO=1, NI=1))


@case('motionseg', ['lasr_motionseg_conf', 'lasr_motionseg_moments', 'lasr_motionseg_solve', 'lasr_motionseg_evidence'])
def _(dev):
    from lasr_amd.nnutils import motionseg
    g = _gen(55)
    H, W = 17, 47
    y, x = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing='ij')
    f = torch.stack([1.5 + 0.01 * x, -0.5 + 0.02 * y], 2) + 0.05 * torch.randn(H, W, 2, generator=g)
    f[5:10, 20:30] += 3.                                       # a region that moves against the dominant motion
    fb = -f + 0.1 * torch.randn(H, W, 2, generator=g)
    f, fb = f.to(dev), fb.to(dev)
    conf = motionseg.confidence(f, fb)
    state = motionseg.fit(f, conf, iters=3)
    e = motionseg.evidence(f, conf, state)
    one = motionseg.evidence(f[:1, :1].contiguous(), conf[:1, :1].contiguous(), state)
    return (conf, state, e, one)


@case('maskprop', ['lasr_maskprop_hist', 'lasr_maskprop_unary', 'lasr_maskprop_meanfield'])
def _(dev):
    from lasr_amd.nnutils import maskprop
    from lasr_amd import _lib
    g = _gen(56)
    H, W = 17, 47
    img_s = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    img_t = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    P = torch.zeros(H, W)
    P[4:12, 10:30] = 1.
    fts, fst = torch.randn(H, W, 2, generator=g).to(dev), torch.randn(H, W, 2, generator=g).to(dev)
    hist = torch.zeros(2, _lib.MASKPROP_BINS, dtype=torch.int32, device=dev)
    return (maskprop.step(img_s, img_t, P.to(dev), fts, fst, hist, maskprop.params()),
            maskprop.step(img_s[:1, :1].contiguous(), img_t[:1, :1].contiguous(), P[4:5, 10:11].to(dev), fts[:1, :1].contiguous(),
                          fst[:1, :1].contiguous(), hist, maskprop.params(K=1, R=1)))


@case('gather_rows', ['lasr_gather_rows'])
def _(dev):
    packed = importlib.import_module('lasr_amd.dataloader.packed')
    g = _gen(57)
    rows = [dict(a=torch.randn(2, 3, 5, generator=g), b=torch.randn(2, 1, generator=g), c=torch.randn(2, 17, generator=g)) for _ in range(5)]
    table = packed.PackedTable(rows, dev)
    ids = _guarded_copy(packed, torch.tensor([4, 0, 2], device=dev))
    out = table.gather(ids, clone=True)
    one = table.gather(ids[:1], clone=True)
    return tuple(out.values()) + tuple(one.values())


@case('tail_step', ['lasr_tail_step', 'lasr_mean_shape_forward', 'lasr_face_gather_forward', 'lasr_sr_forward_opt'])   # (+ the trainer's set-up)
def _(dev):
    import tempfile
    from test_step_tail_gpu import make, set_grads
    with tempfile.TemporaryDirectory() as tmp:
        import pathlib
        tr = make(pathlib.Path(tmp), dev, True)
        set_grads(tr, 1, 5.0)
        tr.step_tail()                                          # step 1 (torch): creates the optimizer state
        for seed, scale in ((2, 5.0), (3, 1e-3)):
            set_grads(tr, seed, scale)
            tr.step_tail()
        return tuple(p.detach().clone() for p in tr.module.parameters()) + (tr.grad_meanv_norm.reshape(1), tr.grad_cam_norm.reshape(1))


def by_name():
    out = {c.name: c for c in CASES}
    assert len(out) == len(CASES), 'two cases of one name'
    return out
