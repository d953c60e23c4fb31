"""The node-major trunk entry points' refusals (lg_gcn_fwd_nm*, lg_gcn_bwd_nm*), host side: every
combination here returns before any HIP call, so no GPU is needed.  The codes and their order
(LG_EINVAL -1 before LG_EUNSUPPORTED -2 where both apply, as the checks run) are the library's
contract with models/library.py, which relies on a refusal instead of a silent replacement.
Every pointer that has to be non-NULL is a host buffer; none is dereferenced on these paths."""
from __future__ import annotations

import ctypes

import pytest

OK, EINVAL, EUNSUP = 0, -1, -2
B, N, D, S = 16, 661, 64, 29


@pytest.fixture(scope="module")
def env():
    from models import _native as nat
    bufs = [ctypes.create_string_buffer(64) for _ in range(13)]
    return nat, nat.load_library(), [ctypes.addressof(b) for b in bufs], bufs


def _fwd(env, fn="lg_gcn_fwd_nm_bits", flags=0, p=0.0, ymask=True, D=D, B=B, N=N, null=None, alias=False):
    """lg_gcn_fwd_nm_bits / _skip / lg_gcn_fwd_nm; null: index of an operand passed as NULL."""
    nat, lib, P, _ = env
    ops = [P[0], P[1], P[2], P[3], P[4], P[5]]  # nodetab, pairs, x, W, bias, y
    if alias:
        ops[5] = ops[2]
    if null is not None:
        ops[null] = None
    tail = () if fn == "lg_gcn_fwd_nm" else (P[6] if ymask else None,)
    return getattr(lib, fn)(*ops, B, N, D, 2193, flags, p, 0, 0, None, *tail)


def _fwd_x0(env, flags=0, p=0.0, D=D, B=B, S=S, null=None):
    nat, lib, P, _ = env
    ops = [P[0], P[1], P[2], P[3], P[4], P[5], P[6], P[7]]  # nodetab_s, pairs_s, xs0, x0bits, node_bias, W, bias, y
    if null is not None:
        ops[null] = None
    return lib.lg_gcn_fwd_nm_x0(*ops, B, N, S, D, flags, p, 0, 0, None)


def _bwd(env, fn="lg_gcn_bwd_nm_bits", flags=0, y=True, ymask=True, slot=False, dnb=False, D=D, B=B, null=None,
         alias=False):
    """lg_gcn_bwd_nm_bits / _skip / lg_gcn_bwd_nm with a workspace size of 0: nothing here gets as
    far as the workspace check."""
    nat, lib, P, _ = env
    ops = [P[0], P[1], P[2], P[3] if y else None, P[4], P[5], P[6], P[7], P[8]]  # tab_t, pairs_t, dy, y, x, W, dx, dW, db
    if alias:
        ops[6] = ops[2]
    if null is not None:
        ops[null] = None
    tail = () if fn == "lg_gcn_bwd_nm" else (P[12] if ymask else None,)
    return getattr(lib, fn)(*ops, P[9] if slot else None, P[10] if dnb else None, B, N, D, flags, 1.0, 1.0, P[11], 0,
                            None, *tail)


def _bwd_x0(env, flags=0, p=0.0, D=D, B=B, S=S, null=None):
    nat, lib, P, _ = env
    # tab_t, pairs_t, pos_slot_t, dy, xs0, x0bits, node_bias, W, dx, dW, db, node_slot, dnode_bias
    ops = [P[i] for i in range(13)]
    if null is not None:
        ops[null] = None
    return lib.lg_gcn_bwd_nm_x0(*ops, B, N, S, D, flags, p, 1.0, P[11], 0, None)


def test_forward_refusals(env):
    nat = env[0]
    for fn in ("lg_gcn_fwd_nm_bits", "lg_gcn_fwd_nm"):
        for i in (0, 1, 2, 3, 5):  # bias (4) is optional without LG_F_BIAS
            assert _fwd(env, fn, null=i) == EINVAL, (fn, i)
        assert _fwd(env, fn, alias=True) == EINVAL          # x == y
        assert _fwd(env, fn, flags=nat.LG_F_BIAS, null=4) == EINVAL
        assert _fwd(env, fn, flags=nat.LG_F_DROPOUT, p=1.0) == EINVAL
        assert _fwd(env, fn, flags=nat.LG_F_DROPOUT, p=-0.1) == EINVAL
        assert _fwd(env, fn, B=-1) == EINVAL and _fwd(env, fn, N=0) == EINVAL
        for xf in (0, nat.LG_F_BF16X3, nat.LG_F_NM3, nat.LG_F_F32_MFMA, nat.LG_F_BF16, nat.LG_F_BF16 | nat.LG_F_PC):
            assert _fwd(env, fn, flags=xf, D=48) == EUNSUP, (fn, hex(xf))
            assert _fwd(env, fn, flags=xf, B=0) == OK         # nothing to do: no launch
            assert _fwd(env, fn, flags=xf, B=20000) == EUNSUP  # N B D 4 bytes past the buffer addressing
        # the argument checks come first
        assert _fwd(env, fn, D=48, null=2) == EINVAL
        assert _fwd(env, fn, D=48, flags=nat.LG_F_DROPOUT, p=1.0) == EINVAL
    assert _fwd(env, "lg_gcn_fwd_nm_bits", ymask=False, B=0) == OK  # the mask is optional here


def test_skip_forward_refusals(env):
    nat = env[0]
    fn = "lg_gcn_fwd_nm_skip"
    assert _fwd(env, fn, ymask=False) == EINVAL
    for bad in (nat.LG_F_BF16, nat.LG_F_NM3, nat.LG_F_F32_MFMA, nat.LG_F_BF16 | nat.LG_F_PC):
        assert _fwd(env, fn, flags=bad) == EUNSUP, hex(bad)
        assert _fwd(env, fn, flags=bad, ymask=False) == EINVAL  # the missing mask is reported first
        assert _fwd(env, fn, flags=bad, null=2) == EUNSUP       # and the transform before the operands
    for ok in (0, nat.LG_F_BF16X3):
        assert _fwd(env, fn, flags=ok, null=3) == EINVAL
        assert _fwd(env, fn, flags=ok, alias=True) == EINVAL
        assert _fwd(env, fn, flags=ok, D=48) == EUNSUP
        assert _fwd(env, fn, flags=ok, B=0) == OK


def test_x0_forward_refusals(env):
    nat = env[0]
    for i in (2, 3, 4):  # xs0, x0bits, node_bias
        assert _fwd_x0(env, null=i) == EINVAL, i
    assert _fwd_x0(env, S=-1) == EINVAL and _fwd_x0(env, S=0x10000) == EINVAL
    assert _fwd_x0(env, S=0xFFFF, B=4096) == EUNSUP  # S B D 4 bytes past the buffer addressing
    for bad in (nat.LG_F_NM3, nat.LG_F_F32_MFMA, nat.LG_F_NM3 | nat.LG_F_BF16):
        assert _fwd_x0(env, flags=bad) == EUNSUP, hex(bad)
        assert _fwd_x0(env, flags=bad, null=3) == EINVAL
    for ok in (0, nat.LG_F_BF16X3, nat.LG_F_BF16, nat.LG_F_BF16 | nat.LG_F_PC):
        assert _fwd_x0(env, flags=ok, null=0) == EINVAL
        assert _fwd_x0(env, flags=ok, null=7) == EINVAL
        assert _fwd_x0(env, flags=ok | nat.LG_F_BIAS, null=6) == EINVAL
        assert _fwd_x0(env, flags=ok | nat.LG_F_DROPOUT, p=1.0) == EINVAL
        assert _fwd_x0(env, flags=ok, D=48) == EUNSUP
        assert _fwd_x0(env, flags=ok, B=0) == OK


def test_backward_refusals(env):
    nat = env[0]
    MI = nat.LG_F_MASK_IN
    for fn in ("lg_gcn_bwd_nm_bits", "lg_gcn_bwd_nm"):
        for i in (0, 1, 2, 4, 5, 6, 7):  # y (3) and db (8) are optional
            assert _bwd(env, fn, null=i) == EINVAL, (fn, i)
        assert _bwd(env, fn, slot=True) == EINVAL and _bwd(env, fn, dnb=True) == EINVAL  # one without the other
        assert _bwd(env, fn, B=-1) == EINVAL
        for xf in (0, nat.LG_F_BF16X3, nat.LG_F_BF16):
            assert _bwd(env, fn, flags=xf, D=48) == EUNSUP, (fn, hex(xf))
            assert _bwd(env, fn, flags=xf | MI, D=48, slot=True, dnb=True) == EUNSUP
            assert _bwd(env, fn, flags=xf, B=20000) == EUNSUP
            assert _bwd(env, fn, flags=xf | MI, y=False, ymask=False) == EINVAL  # MASK_IN needs y or its bits
        assert _bwd(env, fn, D=48, null=2) == EINVAL  # the argument checks come first
    assert _bwd(env, "lg_gcn_bwd_nm", flags=MI, y=False) == EINVAL
    assert _bwd(env, "lg_gcn_bwd_nm_bits", flags=MI, y=False, D=48) == EUNSUP  # the bits stand in for y


def test_skip_backward_refusals(env):
    nat = env[0]
    fn, MI, MO = "lg_gcn_bwd_nm_skip", nat.LG_F_MASK_IN, nat.LG_F_MASK_OUT
    assert _bwd(env, fn, flags=MO) == EINVAL                # MASK_IN is required
    assert _bwd(env, fn, flags=MI, ymask=False) == EINVAL   # as bits, whether y is there or not
    assert _bwd(env, fn, flags=MI, alias=True) == EINVAL    # dy is read after dx is written
    assert _bwd(env, fn, flags=MI | nat.LG_F_BF16) == EUNSUP
    assert _bwd(env, fn, flags=nat.LG_F_BF16) == EINVAL     # the missing MASK_IN is reported first
    assert _bwd(env, fn, flags=MI | nat.LG_F_BF16, null=4) == EUNSUP
    for ok in (0, nat.LG_F_BF16X3):
        assert _bwd(env, fn, flags=MI | ok, null=4) == EINVAL
        assert _bwd(env, fn, flags=MI | ok, slot=True) == EINVAL
        assert _bwd(env, fn, flags=MI | ok, D=48) == EUNSUP
        assert _bwd(env, fn, flags=MI | MO | ok, D=48, slot=True, dnb=True) == EUNSUP


def test_x0_backward_refusals(env):
    nat = env[0]
    for i in (2, 4, 5, 6):  # pos_slot_t, xs0, x0bits, node_bias
        assert _bwd_x0(env, null=i) == EINVAL, i
    assert _bwd_x0(env, S=-1) == EINVAL and _bwd_x0(env, S=0x10000) == EINVAL
    assert _bwd_x0(env, S=0xFFFF, B=4096) == EUNSUP
    assert _bwd_x0(env, flags=nat.LG_F_DROPOUT, p=1.0) == EINVAL
    for xf in (0, nat.LG_F_BF16X3, nat.LG_F_BF16):
        # layer 0 has no MASK_IN form; its entry point passes neither y nor bits, so the refusal
        # is the missing mask's (LG_EINVAL), ahead of the unsupported combination's
        assert _bwd_x0(env, flags=xf | nat.LG_F_MASK_IN) == EINVAL
        assert _bwd_x0(env, flags=xf, null=3) == EINVAL
        assert _bwd_x0(env, flags=xf, null=11) == EINVAL  # node_slot without dnode_bias
        assert _bwd_x0(env, flags=xf, D=48) == EUNSUP
        assert _bwd_x0(env, flags=xf, B=20000, S=1) == EUNSUP
