"""The fused GRU pair's saved steps in lane order (lg_gru_node_init_fwd / lg_gru_node_init_bwd,
include/leakgnn.h): h_seq [L][nb16][NU][64][4] and gates [L][nb16][4][NU][64][4], sequences in
blocks of 16 with B * S rounded up, element (t, seq, unit i) at block seq >> 4, u = i >> 4, lane
16 * ((i >> 2) & 3) + (seq & 15), reg i & 3.  Only where the values live changes: un-blocked by
that index map, the buffers are lg_gru_fwd's bit for bit (padded entries exactly 0), and the
backward on them gives lg_sensor_proj_bwd + lg_gru_bwd's gradients bit for bit.  The shapes put
a case on every block edge: one backward block with padded lanes, an exact fit, an odd number of
16-blocks (a backward half with no forward block) with and without padded lanes."""
from __future__ import annotations

import functools

import pytest
import torch

from helpers import LTA_INP, lta_ids

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
L, N = 5, 40
SHAPES = [(1, 29), (2, 16), (2, 20), (3, 11)]  # nb16 = 2 (3 padded), 2 (exact), 3 (8 padded), 3 (15 padded)


def _unblock_h(hb, nb16, H):
    """[L][nb16][NU][q][j][reg] -> rows [L][16 nb16][H], unit 16 u + 4 q + reg of sequence 16 blk + j"""
    return hb.view(L, nb16, H // 16, 4, 16, 4).permute(0, 1, 4, 2, 3, 5).reshape(L, nb16 * 16, H)


def _unblock_g(gb, nb16, H):
    """[L][nb16][plane][NU][q][j][reg] -> rows [L][16 nb16][4][H]"""
    return gb.view(L, nb16, 4, H // 16, 4, 16, 4).permute(0, 1, 5, 2, 3, 4, 6).reshape(L, nb16 * 16, 4, H)


@functools.lru_cache(maxsize=None)
def _case(B, S, H, I):
    """Both forwards and both backwards of one case, run once (the tests only compare)."""
    from models import _native as nat
    lib = nat.load_library()
    p, ck = nat.ptr, nat.check
    gen = torch.Generator().manual_seed(1000 * B + 10 * S + H + I)
    rnd = lambda *s, k=1.0: (torch.randn(*s, generator=gen) * k).to(DEV)
    r, tf = rnd(B, L, S), (rnd(B, L, 9) if I == 10 else None)
    w = [rnd(3 * H, I, k=0.25), rnd(3 * H, H, k=0.125), rnd(3 * H, k=0.25), rnd(3 * H, k=0.25)]
    Wp, bias = rnd(H, H + 1, k=0.125), rnd(H, k=0.5)
    sidx = torch.randperm(N, generator=gen)[:S].to(DEV)
    slot = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    slot[sidx] = torch.arange(S, dtype=torch.int32, device=DEV)
    st = nat.stream_of(r)
    nseq, nb16 = B * S, (B * S + 15) // 16
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    # row layout: lg_gru_fwd, then the node init's sensor rows from its h_last
    hs, gt, hl = nan(L, nseq, H), nan(L, nseq, 4, H), nan(B, S, H)
    ck(lib.lg_gru_fwd(p(r), p(tf), *(p(t) for t in w), p(hs), p(gt), p(hl), B, L, S, I, H, st), "lg_gru_fwd")
    xs0, bits = nan(S, B, H), torch.zeros(N * ((B + 15) // 16) * 64, device=DEV, dtype=torch.int16)
    ck(lib.lg_node_init_bits_fwd(p(slot), p(sidx), p(hl), p(Wp), p(bias), p(xs0), p(bits), B, N, S, H, H,
                                 nat.LG_F_DROPOUT, 0.1, 123, 0, st), "lg_node_init_bits_fwd")
    # the fused forward: blocked layout
    hb, gb, hl2 = nan(L, nb16 * 16, H), nan(L, nb16 * 16, 4, H), nan(B, S, H)
    xs0f, bitsf = nan(S, B, H), torch.zeros_like(bits)
    ck(lib.lg_gru_node_init_fwd(p(r), p(tf), *(p(t) for t in w), p(hb), p(gb), p(hl2), p(slot), p(sidx), p(Wp), p(bias),
                                p(xs0f), p(bitsf), B, L, S, I, H, N, nat.LG_F_DROPOUT, 0.1, 123, 0, st),
       "lg_gru_node_init_fwd")
    # backward: lg_sensor_proj_bwd + lg_gru_bwd (no dx) on the row layout
    dx0, live, dbin = rnd(N, B, H), (torch.rand(S, generator=gen) > 0.2).float().to(DEV), rnd(H)
    emp = lambda *s: torch.empty(*s, device=DEV)
    dh, dWp, dbp = emp(B, S, H), nan(H, H + 1), nan(H)
    wsp = torch.empty(int(lib.lg_sensor_proj_bwd_workspace_bytes(B, S, H, H)), device=DEV, dtype=torch.uint8)
    ck(lib.lg_sensor_proj_bwd(p(dx0), p(sidx), p(live), p(hl), p(Wp), p(dbin), p(dh), p(dWp), p(dbp), B, N, S, H, H,
                              nat.LG_F_NODE_MAJOR, p(wsp), wsp.numel(), st), "lg_sensor_proj_bwd")
    dws = [nan(*t.shape) for t in w]
    ws = torch.empty(int(lib.lg_gru_bwd_workspace_bytes(B, S, I, H)), device=DEV, dtype=torch.uint8)
    ck(lib.lg_gru_bwd(p(r), p(tf), p(w[0]), p(w[1]), p(hs), p(gt), p(dh), None, *(p(t) for t in dws), B, L, S, I, H,
                      p(ws), ws.numel(), st), "lg_gru_bwd")
    # the fused backward on the blocked buffers
    dwf, dWpf, dbpf = [nan(*t.shape) for t in w], nan(H, H + 1), nan(H)
    wsf = torch.empty(int(lib.lg_gru_node_init_bwd_workspace_bytes(B, S, I, H)), device=DEV, dtype=torch.uint8)
    ck(lib.lg_gru_node_init_bwd(p(r), p(tf), p(w[0]), p(w[1]), p(hb), p(gb), p(dx0), p(sidx), p(live), p(Wp), p(dbin),
                                *(p(t) for t in dwf), p(dWpf), p(dbpf), B, L, S, I, H, N, p(wsf), wsf.numel(), st),
       "lg_gru_node_init_bwd")
    torch.cuda.synchronize()
    return dict(nseq=nseq, nb16=nb16, hs=hs, gt=gt, hl=hl, xs0=xs0, hb=hb, gb=gb, hl2=hl2, xs0f=xs0f,
                ref=dws + [dWp, dbp], fused=dwf + [dWpf, dbpf])


CASES = [(B, S, H, I) for (B, S) in SHAPES for H in (32, 64) for I in (1, 10)]


@pytest.mark.parametrize("B,S,H,I", CASES)
def test_blocked_forward_equals_row_layout(B, S, H, I):
    c = _case(B, S, H, I)
    n = c["nseq"]
    h, g = _unblock_h(c["hb"], c["nb16"], H), _unblock_g(c["gb"], c["nb16"], H)
    assert torch.equal(h[:, :n], c["hs"]), "h_seq differs"
    assert torch.equal(g[:, :n], c["gt"]), "gates differ"
    assert (h[:, n:] == 0).all() and (g[:, n:] == 0).all(), "padded entries are not 0"
    assert torch.equal(c["hl2"], c["hl"]), "h_last differs"
    assert torch.equal(c["xs0f"], c["xs0"]), "xs0 differs"


@pytest.mark.parametrize("B,S,H,I", CASES)
def test_blocked_backward_equals_row_layout(B, S, H, I):
    c = _case(B, S, H, I)
    for name, a, b in zip(("dw_ih", "dw_hh", "db_ih", "db_hh", "dproj_w", "dproj_b"), c["fused"], c["ref"]):
        assert torch.equal(a, b), f"{name} differs: {(a - b).abs().max():.3e}"


@pytest.fixture(scope="module")
def detector():
    from models.detector import LeakDetector
    sensors, pipes = lta_ids()
    torch.manual_seed(0)
    m = LeakDetector(LTA_INP, sensors, pipes).to(DEV).train()
    with torch.no_grad():
        for c in m.convs:
            c.bias.normal_(0, 0.1)
    return m, len(pipes)


@pytest.mark.parametrize("B", [16, 17, 22, 32])  # B * 29 sequences: nb16 = 29, 31 (padded), 40 (padded), 58
def test_fused_encoder_equals_separate_ops_at_block_edges(detector, B):
    """LeakDetector in train mode, fuse_encoder True against False (the row-layout ops): logits and
    every parameter gradient bit for bit, at odd and even nb16 with and without padded lanes."""
    m, npipes = detector
    gen = torch.Generator().manual_seed(7 + B)
    r = torch.randn(B, 36, 29, generator=gen).to(DEV)
    tf = torch.randn(B, 36, 9, generator=gen).to(DEV)
    lab = torch.randint(0, npipes + 1, (B,), generator=gen).to(DEV)
    res = []
    for fused in (False, True):
        m.fuse_encoder = fused
        assert m._fused_encoder(r, tf, B, 661, 64, True) == fused
        m.zero_grad(set_to_none=True)
        torch.manual_seed(13)
        logits = m(r, tf)
        torch.nn.functional.cross_entropy(logits, lab).backward()
        res.append((logits.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
    assert torch.equal(res[1][0], res[0][0]), "logits differ"
    for k in res[0][1]:
        assert torch.equal(res[1][1][k], res[0][1][k]), f"grad {k} differs: {(res[1][1][k] - res[0][1][k]).abs().max():.3e}"
