"""Stacked sensor encoder (nn.GRU(num_layers > 1)) on the HIP kernels: leakgnn::gru_stack
(layer 0 on lg_gru_fwd, upper layers on lg_gru_seq_fwd / lg_gru_seq_bwd) against torch.nn.GRU
on the CPU in fp64 — eval parity over widths and shapes, train-mode dropout replayed mask for
mask from oracle/dropout_ref.py, determinism, a one-layer stack (layer 0's backward with the
last step's gradient alone), the dense-input entry points on their own, the
detector with a two-layer encoder, and the one-layer defaults unchanged."""
import numpy as np
import pytest
import torch

from conftest import LTA_INP
from helpers import assert_close, assert_grads_match_truth, lta_ids, load

pytestmark = pytest.mark.gpu
DEV = "cuda"

NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def _seq_input(r, tf, B, S, L):
    """x_t = [r[b, t, s], tfeat[b, t]] per sequence b*S + s, (B*S, L, I)."""
    x = r.permute(0, 2, 1).reshape(B * S, L, 1)
    if tf is not None:
        x = torch.cat([x, tf[:, None].expand(B, S, L, 9).reshape(B * S, L, 9)], dim=-1)
    return x


# ------------------------------------------------------------------ 1. eval parity
CASES = ([(64, 2, True, s) for s in [(3, 5, 36), (3, 11, 36), (2, 3, 1), (1, 1, 2)]]
         + [(32, 3, True, s) for s in [(3, 5, 36), (3, 11, 36), (2, 3, 1), (1, 1, 2)]]
         + [(64, 2, False, (3, 11, 36)), (48, 2, True, (3, 11, 36)), (48, 2, True, (1, 1, 2)),
            (17, 3, False, (3, 5, 36)), (17, 3, False, (2, 3, 1))])


@pytest.mark.parametrize("H,nl,use_time,shape", CASES)
def test_gru_stack_eval_matches_torch(H, nl, use_time, shape):
    """h_L of the top layer within 1e-5 of torch.nn.GRU (CPU fp64), every gradient (all layers'
    weights and biases, residual, tfeat) within 4x torch fp32's own error or 1e-5."""
    from models.detector import SharedSensorGRUEncoder
    B, S, L = shape
    torch.manual_seed(3)
    enc = SharedSensorGRUEncoder(hidden_size=H, num_layers=nl, use_time=use_time).eval()
    r = torch.randn(B, L, S)
    tf = torch.randn(B, L, 9) if use_time else None

    def run(dt, dev):
        m = SharedSensorGRUEncoder(hidden_size=H, num_layers=nl, use_time=use_time).eval()
        m.load_state_dict(enc.state_dict())
        m = m.to(dt).to(dev)
        ri = r.to(dt).to(dev).requires_grad_(True)
        ti = tf.to(dt).to(dev).requires_grad_(True) if use_time else None
        if dev == "cpu":
            _, hl = m.gru(_seq_input(ri, ti, B, S, L))
            out = hl[-1].view(B, S, H)
        else:
            out = m(ri, ti)
        g = torch.Generator().manual_seed(5)
        out.backward(torch.randn(out.shape, generator=g, dtype=torch.float64).to(dt).to(dev))
        grads = {n: p.grad for n, p in m.gru.named_parameters()}
        grads["residual"] = ri.grad
        if use_time:
            grads["tfeat"] = ti.grad
        return out.detach().cpu(), grads

    hg, gg = run(torch.float32, DEV)
    h64, g64 = run(torch.float64, "cpu")
    _, g32 = run(torch.float32, "cpu")
    assert len(g64) == 4 * nl + 1 + int(use_time)
    assert_close(hg, h64, what=f"GRU stack h_L (H={H}, layers={nl})")
    assert_grads_match_truth(gg, g32, g64)


# ------------------------------------------------------------------ 2. / 3. train-mode dropout
P_DROP, SEED = 0.25, 0x1234_5678_9ABC


def _weights(H, I, nl, gen):
    k = 1.0 / H ** 0.5
    ws = {n: [] for n in NAMES}
    for l in range(nl):
        for n, shp in zip(NAMES, [(3 * H, I if l == 0 else H), (3 * H, H), (3 * H,), (3 * H,)]):
            ws[n].append((torch.rand(shp, generator=gen) * 2 - 1) * k)
    return ws


def _masks(nl, L, nseq, H):
    from oracle.dropout_ref import keep_mask
    from models.ops import GRU_STACK_SALT
    idx = np.arange(L * nseq * H, dtype=np.uint64)
    return [torch.from_numpy(keep_mask(SEED, GRU_STACK_SALT + l, idx, P_DROP).reshape(L, nseq, H)) for l in range(nl - 1)]


def _chain(ws, r, tf, dt, masks, up):
    """Single-layer nn.GRUs chained with the given keep masks ([L][Nseq][H]) and 1 / (1 - p)."""
    B, L, S = r.shape
    nl, H = len(ws["weight_hh"]), ws["weight_hh"][0].shape[1]
    leaves = {f"{n}_l{l}": ws[n][l].to(dt).requires_grad_(True) for n in NAMES for l in range(nl)}
    ri, ti = r.to(dt).requires_grad_(True), tf.to(dt).requires_grad_(True)
    x = _seq_input(ri, ti, B, S, L).permute(1, 0, 2)  # (L, Nseq, I)
    for l in range(nl):
        g = torch.nn.GRU(x.shape[-1], H).to(dt)
        out, _ = torch.func.functional_call(g, {f"{n}_l0": leaves[f"{n}_l{l}"] for n in NAMES}, (x,))
        x = out * masks[l].to(dt) / (1.0 - P_DROP) if l < nl - 1 else out
    hL = x[-1].view(B, S, H)
    hL.backward(up.to(dt))
    grads = {n: t.grad for n, t in leaves.items()}
    grads.update(residual=ri.grad, tfeat=ti.grad)
    return hL.detach(), grads


def _op_train(ws, r, tf, up):
    nl = len(ws["weight_hh"])
    lw = {n: [t.to(DEV).requires_grad_(True) for t in ws[n]] for n in NAMES}
    ri, ti = r.to(DEV).requires_grad_(True), tf.to(DEV).requires_grad_(True)
    seed = torch.tensor([SEED], dtype=torch.long)
    out = torch.ops.leakgnn.gru_stack(ri, ti, lw["weight_ih"], lw["weight_hh"], lw["bias_ih"], lw["bias_hh"], P_DROP,
                                      seed, True)
    out[0].backward(up.float().to(DEV))
    grads = {f"{n}_l{l}": lw[n][l].grad for n in NAMES for l in range(nl)}
    grads.update(residual=ri.grad, tfeat=ti.grad)
    return out[0].detach(), grads


def _train_inputs(H, nl=3, shape=(3, 11, 36)):
    B, S, L = shape
    gen = torch.Generator().manual_seed(21)
    ws = _weights(H, 10, nl, gen)
    r, tf = torch.randn(B, L, S, generator=gen), torch.randn(B, L, 9, generator=gen)
    up = torch.randn(B, S, H, generator=gen, dtype=torch.float64)
    return ws, r, tf, up


@pytest.mark.parametrize("H", [64, 48])
def test_gru_stack_dropout_exact_masks(H):
    """Train mode, p = 0.25, three layers: both boundaries' masks rebuilt on the host from the
    seed; h_L and every gradient against the fp64 chain with those masks (the bars of the eval test)."""
    ws, r, tf, up = _train_inputs(H)
    masks = _masks(3, 36, 33, H)
    for m in masks:
        assert 0.6 < m.float().mean().item() < 0.9
    assert not torch.equal(masks[0], masks[1])
    hg, gg = _op_train(ws, r, tf, up)
    h64, g64 = _chain(ws, r, tf, torch.float64, masks, up)
    _, g32 = _chain(ws, r, tf, torch.float32, masks, up)
    assert_close(hg, h64, what=f"GRU stack h_L, dropout (H={H})")
    assert_grads_match_truth(gg, g32, g64)


@pytest.mark.parametrize("H", [64, 48])
def test_gru_stack_deterministic(H):
    ws, r, tf, up = _train_inputs(H)
    h1, g1 = _op_train(ws, r, tf, up)
    h2, g2 = _op_train(ws, r, tf, up)
    assert torch.equal(h1, h2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n


@pytest.mark.parametrize("H,input_grads", [(64, True), (64, False), (32, True), (32, False), (48, True)])
def test_gru_stack_one_layer_dh_last_only(H, input_grads):
    """A one-layer stack: layer 0 is the top layer, so lg_gru_seq_bwd runs in the encoder input
    form with dh_last alone (dh_seq NULL), with and without dx.  h_L is bit-equal to gru_encoder
    (the same lg_gru_fwd call); the gradients against a one-layer nn.GRU in fp64."""
    ws, r, tf, up = _train_inputs(H, nl=1)
    lw = {n: [ws[n][0].to(DEV).requires_grad_(True)] for n in NAMES}
    ri, ti = r.to(DEV).requires_grad_(input_grads), tf.to(DEV).requires_grad_(input_grads)
    out = torch.ops.leakgnn.gru_stack(ri, ti, lw["weight_ih"], lw["weight_hh"], lw["bias_ih"], lw["bias_hh"], 0.0,
                                      torch.zeros(1, dtype=torch.long), True)
    out[0].backward(up.float().to(DEV))
    with torch.no_grad():
        enc = torch.ops.leakgnn.gru_encoder(ri, ti, *(lw[n][0] for n in NAMES), False)[0]
    assert torch.equal(out[0], enc)
    gg = {f"{n}_l0": lw[n][0].grad for n in NAMES}
    _, g64 = _chain(ws, r, tf, torch.float64, [], up)
    _, g32 = _chain(ws, r, tf, torch.float32, [], up)
    if input_grads:
        gg.update(residual=ri.grad, tfeat=ti.grad)
    else:
        assert ri.grad is None and ti.grad is None
        g64, g32 = ({n: g[n] for n in gg} for g in (g64, g32))
    assert_grads_match_truth(gg, g32, g64)


# ------------------------------------------------------------------ 4. the dense entry points alone
def test_gru_seq_saved_layouts_feed_backward():
    """lg_gru_seq_fwd on a dense input (H = I = 64, |x| up to ~4: the staging scale comes from the
    data), its h_seq / gates into lg_gru_seq_bwd with dh_seq = 0 and a dh_last, against a one-layer
    nn.GRU in fp64."""
    from models import _native as nat
    lib = nat.load_library()
    H, L, nseq = 64, 36, 33
    gen = torch.Generator().manual_seed(8)
    ws = _weights(H, H, 1, gen)
    w = [ws[n][0] for n in NAMES]
    x = torch.randn(L, nseq, H, generator=gen)
    up = torch.randn(nseq, H, generator=gen, dtype=torch.float64)
    d = [t.to(DEV).contiguous() for t in w]
    xd = x.to(DEV)
    h_seq, gates = torch.empty(L, nseq, H, device=DEV), torch.empty(L, nseq, 4, H, device=DEV)
    st = nat.stream_of(xd)
    p = nat.ptr
    nat.check(lib.lg_gru_seq_fwd(p(xd), p(d[0]), p(d[1]), p(d[2]), p(d[3]), p(h_seq), p(gates), nseq, L, H, H, 0, 0.0,
                                 0, 0, st), "lg_gru_seq_fwd")
    dh_seq, dh_last = torch.zeros(L, nseq, H, device=DEV), up.float().to(DEV)
    dx = torch.empty(L, nseq, H, device=DEV)
    out = [torch.empty_like(d[0]), torch.empty_like(d[1]), torch.empty(3 * H, device=DEV), torch.empty(3 * H, device=DEV)]
    wsb = torch.empty(int(lib.lg_gru_seq_bwd_workspace_bytes(nseq, H, H)), device=DEV, dtype=torch.uint8)
    nat.check(lib.lg_gru_seq_bwd(p(xd), None, None, p(d[0]), p(d[1]), p(h_seq), p(gates), p(dh_seq), p(dh_last), p(dx),
                                 p(out[0]), p(out[1]), p(out[2]), p(out[3]), 0, 0, nseq, L, H, H, 0, 0.0, 0, 0,
                                 p(wsb), wsb.numel(), st), "lg_gru_seq_bwd")
    torch.cuda.synchronize()

    def truth(dt):
        g = torch.nn.GRU(H, H).to(dt)
        with torch.no_grad():
            for n, t in zip(NAMES, w):
                getattr(g, n + "_l0").copy_(t)
        xi = x.to(dt).requires_grad_(True)
        o, _ = g(xi)
        o[-1].backward(up.to(dt))
        gr = {n: getattr(g, n + "_l0").grad for n in NAMES}
        gr["x"] = xi.grad
        return o.detach(), gr
    o64, g64 = truth(torch.float64)
    _, g32 = truth(torch.float32)
    assert_close(h_seq, o64, what="lg_gru_seq_fwd h_seq")
    gg = dict(zip(NAMES, out))
    gg["x"] = dx
    assert_grads_match_truth(gg, g32, g64)


# ------------------------------------------------------------------ 5. detector level
def test_detector_two_layer_encoder_vs_oracle():
    """LeakDetector(sensor_layers=2), eval, B = 4, against the oracle with its encoder's GRU
    replaced by a two-layer nn.GRU holding the same weights (CPU, fp32 and fp64): the logits
    against the fp64 run, the gradients against it with the fp32 run as the yardstick;
    capture["h_s"] is filled on this route."""
    from models.detector import LeakDetector
    from oracle.detector_ref import LeakDetectorRef
    sensors, pipes = lta_ids()
    torch.manual_seed(11)
    m = LeakDetector(LTA_INP, sensors, pipes, sensor_layers=2).eval()
    with torch.no_grad():
        for c in m.convs:
            c.bias.normal_(0, 0.1)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    B = 4
    gen = torch.Generator().manual_seed(12)
    r, tf = torch.randn(B, 36, 29, generator=gen), torch.randn(B, 36, 9, generator=gen)
    lab = torch.randint(0, len(pipes) + 1, (B,), generator=gen)

    def ref(dt, up=None):
        mr = LeakDetectorRef(LTA_INP, sensors, pipes).eval()
        mr.sensor_encoder.gru = torch.nn.GRU(10, 64, num_layers=2, batch_first=True)
        mr.load_state_dict(sd)
        mr = mr.to(dt)
        out = mr(r.to(dt), tf.to(dt))
        if up is None:
            lo = out.detach().requires_grad_(True)
            torch.nn.functional.cross_entropy(lo, lab).backward()
            up = lo.grad.clone()
        out.backward(up.to(dt))
        return out.detach(), {n: p.grad.detach() for n, p in mr.named_parameters()}, up

    o64, g64, up = ref(torch.float64)
    _, g32, _ = ref(torch.float32, up)
    m = m.to(DEV)
    m.capture = {}
    lg = m(r.to(DEV), tf.to(DEV))
    lg.backward(up.float().to(DEV))
    assert tuple(m.capture["h_s"].shape) == (B, 29, 64)
    assert_close(lg, o64, what="logits, two-layer encoder (vs fp64)")
    assert "sensor_encoder.gru.weight_ih_l1" in g64
    assert_grads_match_truth({n: p.grad for n, p in m.named_parameters()}, g32, g64)


def test_detector_two_layer_encoder_train_step():
    """Train mode with sensor_dropout = 0.2: a finite step whose gradients reach every parameter."""
    from models.detector import LeakDetector
    sensors, pipes = lta_ids()
    m = LeakDetector(LTA_INP, sensors, pipes, sensor_layers=2, sensor_dropout=0.2).to(DEV).train()
    r, tf = torch.randn(8, 36, 29, device=DEV), torch.randn(8, 36, 9, device=DEV)
    lab = torch.randint(0, len(pipes) + 1, (8,), device=DEV)
    loss = torch.nn.functional.cross_entropy(m(r, tf), lab)
    loss.backward()
    assert torch.isfinite(loss)
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n


# ------------------------------------------------------------------ 6. defaults unchanged
def test_one_layer_defaults_unchanged():
    from models.detector import LeakDetector, SharedSensorGRUEncoder
    torch.manual_seed(4)
    enc = SharedSensorGRUEncoder().to(DEV).eval()
    r, tf = torch.randn(3, 36, 5, device=DEV), torch.randn(3, 36, 9, device=DEV)
    g = enc.gru
    with torch.no_grad():
        a = enc(r, tf)
        b = torch.ops.leakgnn.gru_encoder(r, tf, g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0, False)[0]
    assert torch.equal(a, b)
    sensors, pipes = lta_ids()
    keys = set(LeakDetector(LTA_INP, sensors, pipes).state_dict())
    gold = {k[len("param."):] for k in load("detector_b2.npz") if k.startswith("param.")}
    assert gold and keys == gold
