"""K-hop diffusion of the node init on the GPU: the two kernel forms of lg_diffuse_fwd / lg_diffuse_bwd
against each other bit for bit and against an fp64 restatement, the entry points' refusals, and the
detector with diffuse_hops against a test-local oracle (eval parity with plain, skip and pre-norm trunks,
fixed edge weights, train mode on the kernels' own keep decisions, the general-width path), the
default's guard, a captured training step and opcheck.

Kernel truth: the recurrence z_{k+1} = (1 - alpha) Ahat z_k + alpha x_0 in fp64 torch on the same fp32
inputs, Ahat dense from ops.GCNGraph's CSR; the backward by autograd.  The bound per output is
max(RTOL x scale, 2 x the fp32 torch composition's own error), scale = max |truth| (the form of
tests/test_gpu_norm.py)."""
from __future__ import annotations

import copy
import ctypes
import functools

import pytest
import torch

from helpers import LTA_INP, RTOL, assert_close, assert_grads_match_truth, check_relu_ties, hip_relu_masks, lta_ids
from test_gpu_edge_weight import conv_ref
from test_gpu_skip import _batch, _fixed_seed, _kernel_graph, _log_w

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 256  # NaN floats behind every output


# ----------------------------------------------------------------------------- 1. the kernels alone
def _lib():
    from models import _native as nat
    return nat.load_library(), nat


def _dense(g, transpose=False, dtype=torch.float64):
    """Ahat (N, N) from the graph's CSR: row n holds w[k] at col[k] for k in rowptr[n] .. rowptr[n + 1]."""
    N = g.num_nodes
    rp, col, w = g.rowptr.cpu().long(), g.col.cpu().long(), g.w.cpu()
    nnz = int(rp[-1])
    rows = torch.repeat_interleave(torch.arange(N), rp[1:] - rp[:-1])
    A = torch.zeros(N, N, dtype=torch.float64)
    A.index_put_((rows, col[:nnz]), w[:nnz].double(), accumulate=True)
    return (A.t() if transpose else A).contiguous().to(dtype)


def _recur(A, x, hops, alpha):
    z = x
    for _ in range(hops):
        z = (1.0 - alpha) * torch.einsum("nm,mbd->nbd", A, z) + alpha * x
    return z


def _call(g, src, hops, alpha, *, bwd=False, hopwise=False, x0=None, scale=1.0, flags=None):
    """One entry-point call on (N, B, D) src with NaN guard rows behind the output; returns (rc, out)."""
    lib, nat = _lib()
    N, B, D = src.shape
    fl = (nat.LG_F_DIFFUSE_HOPWISE if hopwise else 0) | (nat.LG_F_MASK_OUT if x0 is not None else 0)
    fl = fl if flags is None else flags
    buf = torch.full((src.numel() + GUARD,), float("nan"), device=DEV)
    nb = int(lib.lg_diffuse_workspace_bytes(B, N, D, hops, fl, int(bwd)))
    ws = torch.empty(max(nb, 0), device=DEV, dtype=torch.uint8)
    st = torch.cuda.current_stream().cuda_stream
    tab, pairs = (g.nodetab_t, g.pairs_t) if bwd else (g.nodetab, g.pairs)
    if bwd:
        rc = lib.lg_diffuse_bwd(tab.data_ptr(), pairs.data_ptr(), src.data_ptr(), None if x0 is None else x0.data_ptr(),
                                buf.data_ptr(), B, N, D, hops, alpha, fl, scale, ws.data_ptr() if nb > 0 else None,
                                max(nb, 0), st)
    else:
        rc = lib.lg_diffuse_fwd(tab.data_ptr(), pairs.data_ptr(), src.data_ptr(), buf.data_ptr(), B, N, D, hops, alpha,
                                fl, ws.data_ptr() if nb > 0 else None, max(nb, 0), st)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[src.numel():]).all()), "a store past the output"
    return rc, buf[:src.numel()].view(N, B, D)


def _inputs(N, B, D, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(N, B, D, generator=gen)).to(DEV)  # a node init: non-negative, with zeros
    gr = torch.randn(N, B, D, generator=gen).to(DEV)
    return x, gr


CASES = [(B, D, hops, alpha) for B in (1, 20) for D in (32, 64) for hops in (1, 2, 3, 12) for alpha in (0.1, 0.5)]


@pytest.mark.parametrize("B,D,hops,alpha", CASES)
def test_resident_and_hopwise_give_the_same_bits(B, D, hops, alpha):
    """The resident form against the forced hop-wise form, forward and backward, and two runs of each
    form: torch.equal.  hops odd and even (ping-pong parity); the hub row has overflow pairs."""
    g, N = _kernel_graph()
    lib, _ = _lib()
    assert lib.lg_diffuse_slice(N, D) == 32
    x, gr = _inputs(N, B, D)
    for src, bwd in ((x, False), (gr, True)):
        outs = []
        for hopwise in (False, True, False, True):
            rc, o = _call(g, src, hops, alpha, bwd=bwd, hopwise=hopwise)
            assert rc == 0
            assert bool(torch.isfinite(o).all())
            outs.append(o.clone())
        assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3]), f"bwd={bwd}: a form does not repeat"
        assert torch.equal(outs[0], outs[1]), f"bwd={bwd}: resident and hop-wise differ"


@pytest.mark.parametrize("B,D,hops,alpha", CASES)
def test_kernels_vs_fp64_and_adjoint(B, D, hops, alpha):
    """Forward and backward (autograd of the fp64 recurrence) within max(RTOL x scale, 2 x the fp32 torch
    composition's own error); then <diffuse(x), g> against <x, diffuse_bwd(g)>: both are sums of N B D
    products, so the bar's scale is the sum of |truth z . g| terms and its fp32 yardstick the same
    identity evaluated on the fp32 composition."""
    g, N = _kernel_graph()
    x, gr = _inputs(N, B, D, seed=1)
    A64 = _dense(g)
    x64 = x.double().cpu().requires_grad_(True)
    z64 = _recur(A64, x64, hops, alpha)
    z64.backward(gr.double().cpu())
    dx64 = x64.grad
    A32 = A64.float().to(DEV)
    x32 = x.clone().requires_grad_(True)
    z32 = _recur(A32, x32, hops, alpha)
    z32.backward(gr)
    _, z = _call(g, x, hops, alpha)
    _, dx = _call(g, gr, hops, alpha, bwd=True)
    for name, got, truth, ref in (("z", z, z64.detach(), z32.detach()), ("dx0", dx, dx64, x32.grad)):
        err = (got.double().cpu() - truth).abs().max().item()
        e32 = (ref.double().cpu() - truth).abs().max().item()
        scale = truth.abs().max().item()
        print(f"diffuse {name} B={B} D={D} K={hops} a={alpha}: err {err:.3e} (fp32 torch {e32:.3e}, scale {scale:.3e})")
        assert err <= max(RTOL * scale, 2 * e32), (name, err, e32, scale)
    ip = lambda a, b: (a.double().cpu() * b.double().cpu()).sum().item()  # noqa: E731
    lhs, rhs = ip(z, gr), ip(x, dx)
    scale = (z64.detach() * gr.double().cpu()).abs().sum().item()
    e32 = abs(ip(z32.detach(), gr) - ip(x, x32.grad))
    print(f"adjoint: <z, g> {lhs:.9e} <x, dx> {rhs:.9e} (fp32 torch gap {e32:.3e}, scale {scale:.3e})")
    assert abs(lhs - rhs) <= max(RTOL * scale, 2 * e32)


@pytest.mark.parametrize("hopwise", [False, True])
@pytest.mark.parametrize("D", [32, 64])
def test_alpha_one_is_exact_and_mask(D, hopwise):
    """alpha = 1: z == x_0 and dx0 == g exactly (the products with 1 - alpha = 0 vanish).  LG_F_MASK_OUT:
    the output equals (the unmasked dx0) * scale_out * [x0 > 0], torch.equal."""
    g, N = _kernel_graph()
    x, gr = _inputs(N, 20, D, seed=2)
    for hops in (1, 3):
        _, z = _call(g, x, hops, 1.0, hopwise=hopwise)
        _, dx = _call(g, gr, hops, 1.0, bwd=True, hopwise=hopwise)
        assert torch.equal(z, x) and torch.equal(dx, gr)
    scale = 1.0 / 0.9
    for hops in (1, 2, 12):
        _, plain = _call(g, gr, hops, 0.1, bwd=True, hopwise=hopwise)
        _, masked = _call(g, gr, hops, 0.1, bwd=True, hopwise=hopwise, x0=x, scale=scale)
        want = torch.where(x > 0, plain * torch.tensor(scale, device=DEV), torch.zeros_like(plain))
        assert torch.equal(masked, want)
        assert 0.2 < float((x > 0).float().mean()) < 0.8


def _path_graph(N):
    from models import ops
    a = torch.arange(N - 1)
    ei = torch.stack([torch.cat([a, a + 1]), torch.cat([a + 1, a])])
    return ops.GCNGraph.build(ei, N, DEV, add_self_loops=True, normalize=True)


def _path_truth(N, x, hops, alpha):
    """The recurrence on a path graph in fp64 without a dense matrix: Ahat = D^-1/2 (A + I) D^-1/2."""
    deg = torch.full((N,), 3.0, dtype=torch.float64)
    deg[0] = deg[-1] = 2.0
    dis = deg.rsqrt().view(N, 1, 1)
    z = x
    for _ in range(hops):
        y = dis * z
        s = y.clone()
        s[1:] += y[:-1]
        s[:-1] += y[1:]
        z = (1.0 - alpha) * dis * s + alpha * x
    return z


@pytest.mark.parametrize("N,slice_", [(769, 16), (1537, 8), (None, 0)])
def test_slices_and_fallback_to_hopwise(N, slice_):
    """Path graphs, B = 2, D = 32.  N = 769 and 1537: one row more than the 32- and the 16-float
    slices hold (the resident form's narrower slices; equal to the forced hop-wise form bit for bit).
    N = None: the smallest N for which lg_diffuse_slice says no slice fits: the entry point takes the
    hop-wise form by itself (its workspace size is then non-zero).  All against fp64 (the path's Ahat is
    symmetric, so the backward's truth is the forward recurrence on g)."""
    lib, _ = _lib()
    if N is None:
        N = 1
        while lib.lg_diffuse_slice(N, 32) > 0:
            N += 256
        while lib.lg_diffuse_slice(N - 1, 32) == 0:
            N -= 1
        assert lib.lg_diffuse_workspace_bytes(2, N, 32, 3, 0, 0) == N * 2 * 32 * 4
        assert lib.lg_diffuse_workspace_bytes(2, N - 1, 32, 3, 0, 0) == 0
    assert lib.lg_diffuse_slice(N, 32) == slice_ and lib.lg_diffuse_slice(N - 1, 32) == 2 * slice_ or slice_ == 0
    g = _path_graph(N)
    x, gr = _inputs(N, 2, 32, seed=3)
    for hops in (2, 3):
        for src, bwd in ((x, False), (gr, True)):
            rc, got = _call(g, src, hops, 0.1, bwd=bwd)
            rc2, hw = _call(g, src, hops, 0.1, bwd=bwd, hopwise=True)
            assert rc == 0 and rc2 == 0 and torch.equal(got, hw)
            truth = _path_truth(N, src.double().cpu(), hops, 0.1)
            err = (got.double().cpu() - truth).abs().max().item()
            ref = _path_truth(N, src.cpu(), hops, 0.1)  # the same composition in fp32 torch
            e32 = (ref.double() - truth).abs().max().item()
            assert err <= max(RTOL * truth.abs().max().item(), 2 * e32), (N, hops, bwd, err, e32)


def test_entry_point_refusals():
    """D outside {32, 64}: LG_EUNSUPPORTED; hops outside 1..64, alpha outside [0, 1] (NaN included), an
    output aliasing its input, a NULL pointer, the mask without x0, a missing workspace: LG_EINVAL;
    unknown flags: LG_EUNSUPPORTED; B == 0: LG_OK.  No refused call writes anything."""
    lib, nat = _lib()
    g, N = _kernel_graph()
    EINVAL, EUNSUP = -1, -2
    x, gr = _inputs(N, 4, 32)
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full_like(x, float("nan"))
    T, P = g.nodetab.data_ptr(), g.pairs.data_ptr()

    def fwd(x0=x.data_ptr(), z=out.data_ptr(), B=4, D=32, hops=2, alpha=0.1, flags=0, ws=None, nb=0, tab=T):
        return lib.lg_diffuse_fwd(tab, P, x0, z, B, N, D, hops, alpha, flags, ws, nb, st)

    def bwd(gp=gr.data_ptr(), x0=None, dx=out.data_ptr(), B=4, D=32, hops=2, alpha=0.1, flags=0, ws=None, nb=0):
        return lib.lg_diffuse_bwd(g.nodetab_t.data_ptr(), g.pairs_t.data_ptr(), gp, x0, dx, B, N, D, hops, alpha, flags,
                                  1.0, ws, nb, st)

    for D in (16, 48, 128):
        assert fwd(D=D) == EUNSUP and bwd(D=D) == EUNSUP
    for hops in (0, -1, 65):
        assert fwd(hops=hops) == EINVAL and bwd(hops=hops) == EINVAL
    for alpha in (-0.01, 1.01, float("nan")):
        assert fwd(alpha=alpha) == EINVAL and bwd(alpha=alpha) == EINVAL
    assert fwd(z=x.data_ptr()) == EINVAL and bwd(dx=gr.data_ptr()) == EINVAL
    assert fwd(x0=None) == EINVAL and fwd(z=None) == EINVAL and fwd(tab=None) == EINVAL and fwd(B=-1) == EINVAL
    assert bwd(flags=nat.LG_F_MASK_OUT) == EINVAL                       # the mask without x0
    assert bwd(flags=nat.LG_F_MASK_OUT, x0=out.data_ptr()) == EINVAL    # x0 aliasing the output
    assert fwd(flags=nat.LG_F_DIFFUSE_HOPWISE) == EINVAL and bwd(flags=nat.LG_F_DIFFUSE_HOPWISE) == EINVAL  # no workspace
    assert fwd(flags=nat.LG_F_RELU) == EUNSUP and fwd(flags=nat.LG_F_MASK_OUT) == EUNSUP and bwd(flags=nat.LG_F_BF16) == EUNSUP
    assert lib.lg_diffuse_slice(N, 48) == EUNSUP and lib.lg_diffuse_workspace_bytes(4, N, 48, 2, 0, 0) == EUNSUP
    assert fwd(B=0) == 0 and bwd(B=0) == 0
    assert fwd(hops=1, flags=nat.LG_F_DIFFUSE_HOPWISE) == 0  # one hop needs no workspace in either form
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    out.fill_(float("nan"))
    for rc in (fwd(hops=0), bwd(alpha=2.0), fwd(D=16)):
        assert rc != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_ops_diffuse_autograd_and_opcheck():
    """ops.diffuse(x, graph, hops, alpha): forward equals the entry point's, x.grad equals lg_diffuse_bwd's
    (torch.equal); hops = 0 and a window-major rank are refused; opcheck of leakgnn::diffuse."""
    from models import ops
    g, N = _kernel_graph()
    x, gr = _inputs(N, 20, 64, seed=4)
    xr = x.clone().requires_grad_(True)
    z = ops.diffuse(xr, g, 3, 0.1)
    z.backward(gr)
    assert torch.equal(z.detach(), _call(g, x, 3, 0.1)[1]) and torch.equal(xr.grad, _call(g, gr, 3, 0.1, bwd=True)[1])
    with pytest.raises(ValueError):
        ops.diffuse(x, g, 0, 0.1)
    with pytest.raises(ValueError):
        ops.diffuse(x, g, 2, 1.5)
    with pytest.raises(ValueError):
        ops.diffuse(x.view(N * 20, 64), g, 2, 0.1)
    with pytest.raises(NotImplementedError):
        ops.diffuse(x[:, :, :48].contiguous(), g, 2, 0.1)
    torch.library.opcheck(torch.ops.leakgnn.diffuse.default,
                          (x.clone().requires_grad_(True), g.nodetab, g.pairs, g.nodetab_t, g.pairs_t, 2, 0.5),
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor",
                                      "test_aot_dispatch_dynamic"))


# ----------------------------------------------------------------------------- 2. the detector's oracle
@functools.lru_cache(maxsize=None)
def _ref_cls():
    from oracle import gcn_ref, graph_ref
    from oracle.detector_ref import LeakDetectorRef

    class DiffuseRef(LeakDetectorRef):
        """LeakDetectorRef with the hop loop between the node init and layer 0, and the skip / pre-norm
        layer loops of tests/test_gpu_skip.py and tests/test_gpu_norm.py.  Ahat is gcn_norm restated
        densely in the run's own dtype (self loops of weight 1, symmetric normalisation by the target's
        weighted degree); link_w: per-link weights or None."""

        def __init__(self, *a, gnn_layers=2, node_hidden=64, skip=False, norm=False, hops=0, alpha=0.1, **kw):
            super().__init__(*a, gnn_layers=gnn_layers, node_hidden=node_hidden, **kw)
            self.skip, self.hops, self.alpha, self.link_w = skip, hops, alpha, None
            if norm:
                self.norms = torch.nn.ModuleList(torch.nn.LayerNorm(node_hidden) for _ in range(gnn_layers + 1))

        def ahat(self, dt, dev):
            N = len(self.node_names)
            ei = self.edge_index_single.to(dev)
            w = torch.ones(ei.shape[1], dtype=dt, device=dev) if self.link_w is None \
                else self.link_w.to(dt).to(dev).repeat_interleave(2)
            loop = torch.arange(N, device=dev)
            row, col, w = torch.cat([ei[0], loop]), torch.cat([ei[1], loop]), torch.cat([w, torch.ones(N, dtype=dt, device=dev)])
            deg = torch.zeros(N, dtype=dt, device=dev).index_add_(0, col, w)
            dis = deg.pow(-0.5)
            A = torch.zeros(N, N, dtype=dt, device=dev)
            return A.index_put_((col, row), dis[row] * w * dis[col], accumulate=True)

        def forward(self, residual, tfeat=None):
            B, L, S = residual.shape
            N = len(self.node_names)
            h_s = self.sensor_encoder(residual, tfeat)
            dev = residual.device
            h0 = torch.zeros(B, N, h_s.shape[-1], dtype=residual.dtype, device=dev)
            idx = self.sensor_node_idx.to(dev)
            h0[:, idx, :] = h_s
            mask = torch.zeros(N, 1, dtype=residual.dtype, device=dev)
            mask[idx, 0] = 1.0
            h = torch.cat([h0, mask.unsqueeze(0).expand(B, -1, -1)], dim=-1)
            h = self.dropout(self._relu("init", self.sensor_to_node(h)))
            self.trace["node_init"] = h
            if self.hops:
                A, z = self.ahat(residual.dtype, dev), h
                for _ in range(self.hops):
                    z = (1.0 - self.alpha) * torch.einsum("nm,bmd->bnd", A, z) + self.alpha * h
                h = z
                self.trace["z"] = z
            x = h.reshape(B * N, -1)
            ei = torch.from_numpy(graph_ref.batchify(self.edge_index_single.numpy(), N, B)).to(dev)
            norms = getattr(self, "norms", None)
            for i, conv in enumerate(self.convs):
                br = self.dropout(self._relu(f"conv{i}", conv(norms[i](x) if norms is not None else x, ei)))
                x = x + br if self.skip else br
                self.trace[f"conv{i}"] = x
            if norms is not None:
                x = norms[len(self.convs)](x)
            h_nodes = x.view(B, N, -1)
            u, v = self.pipe_ends[:, 0].to(dev), self.pipe_ends[:, 1].to(dev)
            h_u, h_v = h_nodes[:, u, :], h_nodes[:, v, :]
            feat = torch.cat([h_u, h_v, self._abs("absdiff", h_u - h_v)], dim=-1)
            mlp = self.edge_head.mlp
            pipe_logits = mlp[3](mlp[2](self._relu("edge", mlp[0](feat)))).squeeze(-1)
            batch = torch.arange(B, device=dev).repeat_interleave(N)
            pooled = gcn_ref.global_mean_pool(x, batch, size=B)
            nmlp = self.noleak_head.mlp
            noleak = nmlp[3](nmlp[2](self._relu("noleak", nmlp[0](pooled)))).squeeze(-1).unsqueeze(-1)
            return torch.cat([pipe_logits, noleak], dim=-1)

    return DiffuseRef


@functools.lru_cache(maxsize=None)
def _random_sd(layers: int, norm: bool = False, seed: int = 47, kw: tuple = ()):
    """A random state dict (conv biases off zero, the norms off 1 and 0); shared, read-only."""
    sensors, pipes = lta_ids()
    torch.manual_seed(seed)
    ref = _ref_cls()(LTA_INP, sensors, pipes, gnn_layers=layers, norm=norm, **dict(kw)).eval()
    with torch.no_grad():
        for c in ref.convs:
            c.bias.normal_(0, 0.1)
        for n in getattr(ref, "norms", []):
            n.weight.normal_(1.0, 0.2)
            n.bias.normal_(0, 0.1)
    return {k: v.clone() for k, v in ref.state_dict().items()}


def _oracle(sd, r, tf, dt, dev, cfg, up=None, lab=None, masks=None, log_w=None, kw=None):
    """The oracle in eval mode: (logits, parameter grads, pre-activations, upstream gradient).  cfg =
    (layers, hops, alpha, skip, norm); log_w: fixed link log-weights (the convs then run conv_ref)."""
    layers, hops, alpha, skip, norm = cfg
    sensors, pipes = lta_ids()
    mr = _ref_cls()(LTA_INP, sensors, pipes, gnn_layers=layers, skip=skip, norm=norm, hops=hops, alpha=alpha,
                    **(kw or {})).eval()
    mr.load_state_dict(sd)
    mr = mr.to(dt).to(dev)
    mr.sensor_encoder.gru.train()  # MIOpen's RNN backward needs training mode (1 layer: no dropout)
    mr.relu_masks = masks or {}
    if log_w is not None:
        mr.link_w = log_w.exp()
        ew = log_w.exp().to(dt).to(dev).repeat_interleave(2).repeat(r.shape[0])
        for c in mr.convs:
            c.forward = lambda x, ei, c=c: conv_ref(x, ei, ew, c.lin.weight, c.bias, x.shape[0])
    out = mr(r.to(dt).to(dev), tf.to(dt).to(dev))
    if up is None:
        lo = out.detach().requires_grad_(True)
        torch.nn.functional.cross_entropy(lo, lab).backward()
        up = lo.grad.clone()
    out.backward(up.to(dt).to(dev))
    pre = {k[len("pre_"):]: v.detach() for k, v in mr.trace.items() if k.startswith("pre_")}
    return out.detach().cpu(), {n: p.grad.detach().cpu() for n, p in mr.named_parameters()}, pre, up


def _detector(sd, cfg, **kw):
    from models.detector import LeakDetector
    layers, hops, alpha, skip, norm = cfg
    sensors, pipes = lta_ids()
    m = LeakDetector(LTA_INP, sensors, pipes, gnn_layers=layers, skip="residual" if skip else "none",
                     norm="layer" if norm else "none", diffuse_hops=hops, diffuse_alpha=alpha, **kw).to(DEV).eval()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) <= {"edge_weight"}
    return m


def _masks(m, B, scale=None):
    """The kink decisions of a captured forward in the oracle's shapes (plain: [x_l > 0]; skip / norm:
    capture["fmask"]; the heads' |h_u - h_v| on their own input).  scale (train mode): floats, keep x
    1 / (1 - p), so the eval-mode oracle's z * mask is dropout(relu(z)) on the kernels' keep decisions."""
    N, P = len(m.node_names), len(m.pipe_ids)
    cap = m.capture
    assert cap["node_major"] and tuple(cap["z"].shape) == tuple(cap["xs"][0].shape)
    src = dict(cap, xs=list(cap["xs"][:-1]) + [cap["xns"][-1]]) if m.norm == "layer" else cap
    if not len(m.convs):  # the heads read z_K, which is no ReLU site
        src = dict(cap, xs=[cap["xs"][0], cap["z"]])
    masks = hip_relu_masks(src, B, N, P, m.pipe_ends)
    if not len(m.convs):
        del masks["conv0"]
    if m.skip == "residual":
        for l, fm in enumerate(cap["fmask"]):
            masks[f"conv{l}"] = fm.permute(1, 0, 2).reshape(B, N, -1).cpu()
    if scale is not None:
        masks = {k: (v.to(torch.float64) * scale if v.dtype == torch.bool else v) for k, v in masks.items()}
    return masks


def _parity(layers, hops, B, skip=False, norm=False, log_w=None, train_p=None, alpha=0.1):
    cfg = (layers, hops, alpha, skip, norm)
    sd = _random_sd(layers, norm)
    r, tf, lab = _batch(B)
    _, _, pre64, up = _oracle(sd, r, tf, torch.float64, "cpu", cfg, lab=lab, log_w=log_w)
    kw = dict(edge_weight=log_w.exp()) if log_w is not None else {}
    if train_p is not None:
        kw["dropout"] = train_p
    m = _detector(sd, cfg, **kw)
    if train_p is not None:
        m.train()
    m.capture = {}
    assert not m._fused_encoder(r.to(DEV), tf.to(DEV), B, 661, 64, True)
    lg = m(r.to(DEV), tf.to(DEV))
    lg.backward(up.float().to(DEV))
    if train_p is None:
        masks = _masks(m, B)
        ties = check_relu_ties(pre64, masks)
    else:
        masks, ties = _masks(m, B, scale=1.0 / (1.0 - train_p)), -1
    o64, g64, _, _ = _oracle(sd, r, tf, torch.float64, "cpu", cfg, up=up, masks=masks, log_w=log_w)
    o32, g32, _, _ = _oracle(sd, r, tf, torch.float32, "cpu", cfg, up=up, masks=masks, log_w=log_w)
    _, g32d, _, _ = _oracle(sd, r, tf, torch.float32, DEV, cfg, up=up, masks=masks, log_w=log_w)
    got = {n: p.grad for n, p in m.named_parameters()}
    assert set(g64) <= set(got) and all(got[n] is not None for n in g64)
    scale = o64.abs().max().item()
    e_gpu = (lg.detach().double().cpu() - o64).abs().max().item()
    e_ref = (o32.double() - o64).abs().max().item()
    print(f"diffuse L={layers} K={hops} B={B} skip={skip} norm={norm} weighted={log_w is not None} train_p={train_p}: "
          f"logits err vs fp64 {e_gpu:.3e} (fp32 oracle's own {e_ref:.3e}, scale {scale:.3e}, RTOL x scale "
          f"{RTOL * scale:.3e}), ties {ties}")
    assert_close(lg, o32, what=f"L={layers} K={hops} B={B} logits")
    assert_grads_match_truth(got, g32, g64, ref32=g32d, rtol_tensor=5e-5)
    return m, lg


# ----------------------------------------------------------------------------- 3. eval parity
@pytest.mark.parametrize("layers,hops,B", [(2, 4, 4), (2, 12, 20), (0, 3, 4)])
def test_diffuse_detector_vs_oracle(layers, hops, B):
    """L-TOWN-A, eval, random weights: logits within RTOL of the fp32 oracle, every parameter gradient
    against the fp64 oracle on the HIP path's side of every kink (assert_grads_match_truth).  B = 4:
    node-major below 16 windows (a diffusion model takes that layout at every B); layers = 0: the
    heads read z_K."""
    m, _ = _parity(layers, hops, B)
    assert "z" in m.capture and m.capture["node_major"]


def test_diffuse_with_skip_vs_oracle():
    _parity(4, 4, 20, skip=True)


def test_diffuse_with_skip_and_norm_vs_oracle():
    _parity(2, 4, 20, skip=True, norm=True)


def test_diffuse_with_fixed_edge_weights_vs_oracle():
    """edge_weight = inv_length links (a buffer): the hops read the weighted tables with no further code."""
    m, _ = _parity(2, 4, 4, log_w=_log_w())
    assert "edge_weight" in m.state_dict()


def test_diffuse_train_mode_on_the_kernels_masks():
    """Train mode, p = 0.1, (2, 4, 20), one fixed seed: two forwards are bit-identical; logits and
    gradients match the oracle evaluated on the kernels' own keep decisions, kept units x 1 / (1 - p)."""
    from models import library
    orig = _fixed_seed(987654321)
    try:
        m, lg = _parity(2, 4, 20, train_p=0.1)
        with torch.no_grad():
            r, tf, _ = (t.to(DEV) for t in _batch(20))
            m.capture = None
            again = m(r, tf)
    finally:
        library.seed_tensor = orig
    assert torch.equal(again, lg.detach())


def test_diffuse_general_widths_vs_oracle():
    """(sensor_hidden, node_hidden) = (48, 40), 2 layers, 3 hops, B = 4: _forward_general composes the hops
    from leakgnn::spmm_cols (an independent route); logits within RTOL of the fp32 oracle, and far
    from the same model's without hops."""
    kw = dict(sensor_hidden=48, node_hidden=40)
    cfg = (2, 3, 0.1, False, False)
    sd = _random_sd(2, False, 11, tuple(kw.items()))
    r, tf, lab = _batch(4, seed=12)
    o32, g32, _, up = _oracle(sd, r, tf, torch.float32, "cpu", cfg, lab=lab, kw=kw)
    m = _detector(sd, cfg, **kw)
    assert not m._widths_tiled()
    lg = m(r.to(DEV), tf.to(DEV))
    lg.backward(up.to(DEV))
    with torch.no_grad():
        plain = _detector(sd, (2, 0, 0.1, False, False), **kw)(r.to(DEV), tf.to(DEV))
    assert_close(lg, o32, what="logits (48, 40)")
    assert (lg - plain).abs().max().item() > 100 * RTOL * o32.abs().max().item()
    assert float(m.sensor_to_node.weight.grad.abs().max()) > 0


# ----------------------------------------------------------------------------- 4. the default, reach
@pytest.mark.parametrize("skip,norm", [("none", "none"), ("residual", "none"), ("residual", "layer")])
def test_zero_hops_is_the_detector_without_the_keywords(skip, norm):
    """diffuse_hops = 0 (any alpha): logits and every gradient torch.equal to a detector built without
    the keywords, identical state-dict keys; B = 32 (the plain model: the fused encoder_trunk op)."""
    from models.detector import LeakDetector
    sensors, pipes = lta_ids()
    sd = _random_sd(2, norm == "layer")
    r, tf, lab = (t.to(DEV) for t in _batch(32))
    outs = []
    for kw in ({}, {"diffuse_hops": 0, "diffuse_alpha": 0.3}):
        m = LeakDetector(LTA_INP, sensors, pipes, skip=skip, norm=norm, **kw).to(DEV).eval()
        m.load_state_dict(sd)
        assert m._fused_encoder(r, tf, 32, 661, 64, True) == (skip == "none")
        lg = m(r, tf)
        torch.nn.functional.cross_entropy(lg, lab).backward()
        outs.append((lg.detach(), [p.grad.clone() for p in m.parameters()], list(m.state_dict())))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][2] == outs[1][2]
    assert all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))


def test_hops_reach_where_the_layers_do_not():
    """A non-sensor node 3 hops from the nearest sensor: with gnn_layers = 2 and no hops its features
    are the same in every window (no sensor within reach), with diffuse_hops = 4 they depend on the
    window; a node 7 or more hops away stays window-independent at reach 6."""
    sd = _random_sd(2)
    r, tf, _ = (t.to(DEV) for t in _batch(20))
    m0, m4 = _detector(sd, (2, 0, 0.1, False, False)), _detector(sd, (2, 4, 0.1, False, False))
    N = len(m0.node_names)
    ei = m0.edge_index_single
    dist = torch.full((N,), -1, dtype=torch.long)
    dist[m0.sensor_node_idx] = 0
    d = 0
    while True:
        near = dist[ei[0]] == d
        new = ei[1][near][dist[ei[1][near]] < 0]
        if new.numel() == 0:
            break
        d += 1
        dist[new] = d
    n3, far = int(torch.nonzero(dist == 3)[0]), torch.nonzero((dist > 6) | (dist < 0)).flatten()
    feats = []
    for m in (m0, m4):
        m.capture = {}
        m.compress_x0 = False
        with torch.no_grad():
            m(r, tf)
        assert m.capture["node_major"]
        feats.append(m.capture["xs"][-1])  # (N, B, D)
    same = lambda x: bool((x == x[:1]).all())  # noqa: E731
    assert same(feats[0][n3]) and not same(feats[1][n3])
    assert far.numel() > 0 and all(same(feats[1][int(n)]) for n in far[:8])


# ----------------------------------------------------------------------------- 5. captured step, opcheck
def test_captured_step_with_hops_matches_eager():
    """gnn_layers = 2, diffuse_hops = 4, B = 32, dropout 0: warm-up + 3 replays of a CapturedTrainStep
    equal warm-up + 3 eager steps (tests/test_graph_step.py's bars: loss 1e-6, parameters 1e-5)."""
    from models import library
    from models.detector import LeakDetector
    from models.graph_step import CapturedTrainStep
    sensors, pipes = lta_ids()
    torch.manual_seed(0)
    m1 = LeakDetector(LTA_INP, sensors, pipes, gnn_layers=2, dropout=0.0, diffuse_hops=4).to(DEV).train()
    m2 = copy.deepcopy(m1)
    r, tf, lab = (t.to(DEV) for t in _batch(32, seed=1))
    mk = lambda m: torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4, fused=True, capturable=True)  # noqa: E731
    o1, o2 = mk(m1), mk(m2)

    def eager():
        o1.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(m1(r, tf), lab)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m1.parameters(), 1.0)
        o1.step()
        return loss

    step = CapturedTrainStep(m2, torch.nn.functional.cross_entropy, o2, (r, tf), lab, clip=1.0, warmup=2)
    for _ in range(2):
        eager()
    for _ in range(3):
        l1, l2 = eager(), step()
    torch.cuda.synchronize()
    assert_close(l2, l1, rtol=1e-6, what="loss")
    for (n, a), b in zip(m2.named_parameters(), m1.parameters()):
        assert bool(torch.isfinite(a).all()), n
        assert_close(a, b, rtol=1e-5, what=n)
    word = ctypes.c_uint32(0)
    assert library.load_library().lg_spin_errors(ctypes.byref(word), 0) == 0 and word.value == 0


@pytest.mark.parametrize("skip", [False, True])
def test_opcheck_gnn_trunk_hops(skip):
    """gnn_trunk(hops=2), B = 3, two layers, with dropout; the list ends in z.  edge_w requiring grad
    with hops > 0 is refused; so is bf16."""
    m = _detector(_random_sd(2), (2, 2, 0.1, skip, False))
    g, inc, slot, sidx, live, nons = m._device_state(DEV)
    seed = torch.tensor([12345], dtype=torch.long)
    B = 3
    h_s = torch.randn(B, 29, 64, device=DEV, requires_grad=True)
    Wn = torch.randn(64, 65, device=DEV).div_(8).requires_grad_(True)
    nb = torch.randn(64, device=DEV, requires_grad=True)
    wts = [c.lin.weight.detach().clone().requires_grad_(True) for c in m.convs]
    bs = [c.bias.detach().clone().normal_(0, 0.1).requires_grad_(True) for c in m.convs]
    args = (h_s, Wn, nb, wts, bs, slot, sidx, nons, live, g.nodetab, g.pairs, g.rowptr, g.col, g.w, g.nodetab_t,
            g.pairs_t, g.rowptr_t, g.col_t, g.w_t, 0.1, True, seed, None, None, None, None)
    kw = {"bf16": False, "skip": skip, "hops": 2, "alpha": 0.1}
    torch.library.opcheck(torch.ops.leakgnn.gnn_trunk.default, args, kw,
                          test_utils=("test_schema", "test_autograd_registration", "test_faketensor",
                                      "test_aot_dispatch_dynamic"))
    out = torch.ops.leakgnn.gnn_trunk(*args, **kw)
    plain = torch.ops.leakgnn.gnn_trunk(*args, bf16=False, skip=skip)
    assert len(out) == len(plain) + 1 and tuple(out[-1].shape) == (661, B, 64)
    assert torch.equal(out[0], plain[0]) and not torch.equal(out[1], plain[1])  # the same node init, another layer 0
    edge_w = g.w.detach().clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        torch.ops.leakgnn.gnn_trunk(*args[:-1], edge_w, **kw)
    with pytest.raises(ValueError):
        torch.ops.leakgnn.gnn_trunk(*args, bf16=True, hops=2, alpha=0.1)
