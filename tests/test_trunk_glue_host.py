"""The trunk ops' host-side glue (models/library.py), no GPU: named saved state, the backward's
return tuple by parameter name, the count of arguments autograd saw, mask_words and the three
output layouts against the layouts the ops document."""
from __future__ import annotations

import pytest
import torch

from models import library


class _Ctx:
    """The two things of an autograd context that _save_named / _saved_named use."""

    def save_for_backward(self, *ts):
        self.saved_tensors = ts


@pytest.mark.parametrize("n", [0, 1, 3])
def test_saved_state_round_trip(n):
    a, b = torch.zeros(2), torch.ones(3)
    lst = [torch.full((1,), float(i)) for i in range(n)]
    ctx = _Ctx()
    library._save_named(ctx, a=a, lst=lst, none=None, b=b, shared=a, tup=tuple(lst))
    assert len(ctx.saved_tensors) == 3 + 2 * n and all(torch.is_tensor(t) for t in ctx.saved_tensors)
    got = library._saved_named(ctx)
    assert list(got) == ["a", "lst", "none", "b", "shared", "tup"]
    assert got["a"] is a and got["b"] is b and got["shared"] is a and got["none"] is None
    assert isinstance(got["lst"], list) and len(got["lst"]) == n and all(x is y for x, y in zip(got["lst"], lst))
    assert isinstance(got["tup"], list) and all(x is y for x, y in zip(got["tup"], lst))
    ctx.saved_tensors = ctx.saved_tensors[:-1]
    with pytest.raises(ValueError):  # tensors that do not match what was recorded: an error, not a shifted read
        library._saved_named(ctx)


OPS = [(library.gnn_trunk, 26, {"edge_w": 1}), (library.gnn_trunk_norm, 21, {"edge_w": 1}),
       (library.encoder_trunk, 26, {"edge_w": 3, "rowptr": 2, "col": 1})]


@pytest.mark.parametrize("op,n_all,trailing", OPS, ids=[o[0]._qualname for o in OPS])
def test_named_grads_and_args_seen(op, n_all, trailing):
    names, defaults = library._positional(op)
    assert len(names) == n_all and "bf16" not in names and "skip" not in names  # keyword-only: not autograd's
    assert [n for n, d in zip(names, defaults) if d is None] == list(trailing)
    full = [object()] * n_all  # every argument given (none equals its default)
    assert library._args_seen(op, full) == n_all
    t = torch.zeros(1)
    for name, k in trailing.items():  # `name` and everything after it left at the default
        assert library._args_seen(op, full[:n_all - k] + [None] * k) == n_all - k
        # a default in front of a given argument is not trailing: it is seen
        if k > 1:
            assert library._args_seen(op, full[:n_all - k] + [None] * (k - 1) + [t]) == n_all
    gw, gb, ge = [torch.ones(1)], torch.zeros(1), torch.ones(2)
    out = library._named_grads(op, n_all, weights=gw, node_bias=gb, edge_w=ge)
    assert len(out) == n_all
    assert out[names.index("weights")] is gw and out[names.index("node_bias")] is gb and out[names.index("edge_w")] is ge
    assert sum(o is not None for o in out) == 3
    cut = library._named_grads(op, n_all - len(trailing), weights=gw, edge_w=ge)  # edge_w never reached autograd
    assert len(cut) == n_all - len(trailing) and sum(o is not None for o in cut) == 1
    assert library._named_grads(op, 5) == (None,) * 5
    with pytest.raises(KeyError):
        library._named_grads(op, n_all, wieghts=gw)


@pytest.mark.parametrize("B", [0, 1, 15, 16, 17])
def test_mask_words(B):
    for N in (1, 661):
        assert library.mask_words(N, B) == N * ((B + 15) // 16) * 64


@pytest.mark.parametrize("L", [0, 1, 3])
def test_layouts_match_the_documented_output_lists(L):
    B, N, S, D, i16, f32 = 20, 661, 29, 64, torch.int16, torch.float32
    nmask = library.mask_words(N, B)
    # gnn_trunk: [x_0, ..., x_L, ymask, x0bits]
    for nm, skip, x0c in ((True, False, False), (True, False, True), (True, True, False), (False, False, False)):
        ent, pos = library._gnn_trunk_layout(L, B, N, S, D, nm, skip, x0c)
        act = (N, B, D) if nm else (B, N, D)
        assert len(ent) == L + 3
        assert ent[0] == ((S, B, D) if x0c else act, f32) and ent[1:L + 1] == [(act, f32)] * L
        assert ent[L + 1] == (((nmask if nm and L else 0) * (L if skip else 1),), i16)
        assert ent[L + 2] == ((nmask if x0c and L else 0,), i16)
        assert pos == dict(xs=list(range(L + 1)), xns=None, ymask=L + 1, x0bits=L + 2, h=L)
    # gnn_trunk_norm: [xn_L, x_0 .. x_L, xn_0 .. xn_{L-1}, stats, ymask]
    ent, pos = library._gnn_trunk_norm_layout(L, B, N, D)
    assert len(ent) == 2 * L + 4 and ent[:2 * L + 2] == [((N, B, D), f32)] * (2 * L + 2)
    assert ent[-2:] == [((L + 1, N * B, 2), f32), ((nmask * L,), i16)]
    assert pos["h"] == 0 and pos["xs"] == list(range(1, L + 2)) and pos["xns"] == list(range(L + 2, 2 * L + 2)) + [0]
    assert pos["stats"] == 2 * L + 2 and pos["ymask"] == 2 * L + 3 and pos["x0bits"] is None
    # encoder_trunk: [x_1, ..., x_L, ymask, xs0, x0bits, h_seq, gates]
    for save in (False, True):
        ent, pos = library._encoder_trunk_layout(L, B, N, S, D, 36, 64, save)
        rows = 16 * ((B * S + 15) // 16)
        assert len(ent) == L + 5 and ent[:L] == [((N, B, D), f32)] * L
        assert ent[L:L + 3] == [((nmask,), i16), ((S, B, D), f32), ((nmask,), i16)]
        assert ent[L + 3:] == ([((36, rows, 64), f32), ((36, rows, 4, 64), f32)] if save else [((0,), f32)] * 2)
        assert pos == dict(xs=[L + 1] + list(range(L)), xns=None, ymask=L, x0bits=L + 2, h=L - 1, h_seq=L + 3,
                           gates=L + 4)


@pytest.mark.parametrize("L", [0, 1, 3])
def test_trunk_fields_names_the_flat_lists(L):
    out = list(range(L + 3))
    f = library.trunk_fields("gnn_trunk", out)
    assert (f.xs, f.xns, f.ymask, f.x0bits, f.h) == (out[:L + 1], None, out[-2], out[-1], out[L])
    out = list(range(2 * L + 4))
    f = library.trunk_fields("gnn_trunk_norm", out)
    assert f.xs == out[1:L + 2] and f.xns == out[L + 2:2 * L + 2] + [out[0]] and f.h == out[0]
    assert (f.stats, f.ymask, f.x0bits) == (out[-2], out[-1], None)
    if L:  # the fused op needs layers
        out = list(range(L + 5))
        f = library.trunk_fields("encoder_trunk", out)
        assert f.xs == [out[L + 1]] + out[:L] and f.h == out[L - 1] and f.xns is None
        assert (f.ymask, f.x0bits, f.h_seq, f.gates) == (out[L], out[L + 2], out[L + 3], out[L + 4])
    with pytest.raises(KeyError):
        library.trunk_fields("gnn_trunk_backward", out)
