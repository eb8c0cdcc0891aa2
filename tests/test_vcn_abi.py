"""lasr_vcn_* check every size and pointer on the host and return LASR_E_* before any launch (no GPU needed)."""
import ctypes

from lasr_amd import _lib

BADARG, WORKSPACE = -1, -3
P = ctypes.c_void_p(16)                                       # never dereferenced: every call below fails its host checks


def _cp(ws_bytes=1 << 30, B=1, C=64, F=16, H=8, W=8, md=4, mdv=4, c1=P, out=P, pw=P, ws=P):
    return _lib.lib().lasr_vcn_corr_proj(c1, P, None, pw, P, P, out, ws, ws_bytes, B, C, F, H, W, md, mdv, None)


def _fr(B=1, F=16, H=8, W=8, md=4, mdv=4, cost=P, flow=P, ent=P):
    return _lib.lib().lasr_vcn_flow_reg(cost, None, flow, ent, B, F, H, W, md, mdv, None)


def test_workspace_size():
    h = _lib.lib()
    assert h.lasr_vcn_corr_proj_workspace_bytes(2, 10, 12) == 2 * 2 * 10 * 12 * 4
    assert h.lasr_vcn_corr_proj_workspace_bytes(0, 10, 12) == 0 and h.lasr_vcn_corr_proj_workspace_bytes(1, -1, 12) == 0


def test_corr_proj_rejects_bad_sizes_and_pointers():
    for kw in (dict(B=0), dict(C=0), dict(C=1025), dict(F=8), dict(F=32), dict(H=0), dict(W=-3), dict(md=0), dict(md=8),
               dict(mdv=-1), dict(mdv=5), dict(B=30000, mdv=1), dict(H=70000, W=1), dict(c1=None), dict(out=None), dict(pw=None)):
        assert _cp(**kw) == BADARG, kw
    assert _cp(ws=None) == WORKSPACE
    assert _cp(ws_bytes=2 * 8 * 8 * 4 - 1) == WORKSPACE


def test_flow_reg_rejects_bad_sizes_and_pointers():
    for kw in (dict(B=0), dict(F=0), dict(F=1025), dict(H=0), dict(W=0), dict(md=0), dict(md=8), dict(mdv=-1), dict(mdv=5),
               dict(B=5000, F=16), dict(H=65536, W=65536), dict(cost=None), dict(flow=None), dict(ent=None)):
        assert _fr(**kw) == BADARG, kw
