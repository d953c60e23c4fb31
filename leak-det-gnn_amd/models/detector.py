"""LeakDetector on MI355X: drop-in for reference models/detector.py.

Same module tree, constructor / forward signatures and state-dict keys as the
reference (detector.py:28-218), so models/train_detector.py, eval/event_evaluator.py
and models/window_evaluator.py use it unchanged:

  sensor_encoder.gru.*              SharedSensorGRUEncoder   (detector.py:28-73)
  sensor_to_node.{weight,bias}      node init Linear(65, 64)  (detector.py:160, 184-190)
  convs.{i}.lin.weight, convs.{i}.bias   GCNConv               (detector.py:162-164)
  edge_head.mlp.{0,3}.*             EdgeHead                  (detector.py:76-88)
  noleak_head.mlp.{0,3}.*           NoLeakHead                (detector.py:91-102)

What runs where (forward + backward): everything on libleakgnn HIP kernels behind the
registered ops of models/library.py (leakgnn::encoder_trunk / gru_encoder / sensor_proj /
gnn_trunk / detector_heads) and models/loss.py (leakgnn::cross_entropy):
  * the GRU sensor encoder with the node init (sensor projection, mask column, ReLU,
    dropout) fused into its epilogue, and the projection's backward into the GRU backward;
    a stacked encoder (LeakDetector(sensor_layers > 1), nn.GRU's num_layers and inter-layer
    dropout) runs leakgnn::gru_stack instead — layer 0 on the same kernel, the upper layers
    on the dense-input kernels (lg_gru_seq_fwd / lg_gru_seq_bwd) — followed by gnn_trunk: the
    fused encoder_trunk op is one-layer only;
  * every GCNConv + ReLU + dropout on the node-major trunk kernels over ONE device-resident
    single-graph CSR (the (2, B*E) batchified edge_index of the reference,
    detector.py:195-196, is never built);
  * the fused EdgeHead (endpoint gather -> MLP -> logit, the (B, P, 3D) features never
    materialised), the per-window mean pool with the NoLeakHead MLP, and their backward
    with the node scatter streamed per tile;
  * the loss (CrossEntropyLoss) and, in the training scripts, clip_grad_norm_ + AdamW
    (models/optim.py).
There is no CPU path: forward raises on CPU tensors.

Edge weights (LeakDetector(..., edge_weight=, learn_edge_weight=); not in the reference, whose
GCNConv calls pass none): one positive weight per link of the .inp link table, shared by the
link's two directed edges, through PyG's weighted gcn_norm (lg_graph_build_w).  Fixed weights
are a buffer (`edge_weight`); learned ones a parameter `edge_log_weight` = log of the link
weight, whose gradient comes through the trunk ops' edge_w input (library._layer_dw,
lg_sddmm_nm).  With neither, nothing differs from the unweighted detector.

Residual trunk (LeakDetector(..., gnn_layers=N, skip="residual"); not in the reference): every
GCN layer is x = x + dropout(relu(conv(x))), the form deep GCNs are trained in (a non-sensor
node sees only sensors within gnn_layers hops: utils.sensor_reach).  The skip runs on the
fp32-tier node-major kernels (lg_gcn_fwd_nm_skip / lg_gcn_bwd_nm_skip) at every batch size,
through the unfused route: the encoder module, then leakgnn::gnn_trunk with x_0 materialised.
skip="none" (the default) is the detector as before, bit for bit.

Pre-norm trunk (LeakDetector(..., skip="residual", norm="layer"); not in the reference): a
LayerNorm in front of every branch and one in front of the heads (self.norms, gnn_layers + 1
stock nn.LayerNorm modules): xn_l = LN_l(x_l), x_{l+1} = x_l + dropout(relu(conv(xn_l))), the
heads read xn_L.  The branch is the plain layer's kernel; the skip's add and the next norm are
one launch (lg_add_layernorm_fwd, lg_layernorm_bwd: csrc/norm.hip) under leakgnn::gnn_trunk_norm.
norm="none" (the default) is the detector as before: no `norms` attribute, no state-dict key.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import library, ops
from .gcn import GCNConv, global_mean_pool  # noqa: F401  (re-exported PyG-compatible API)
from .utils import WDNGraph, build_wdn_graph_from_inp, link_edge_weights


class SharedSensorGRUEncoder(nn.Module):
    """One GRU shared by all sensors: (B, L, S) residuals (+ (B, L, 9) time features) -> (B, S, d)."""

    def __init__(self, time_dim: int = 9, hidden_size: int = 64, num_layers: int = 1, dropout: float = 0.0,
                 use_time: bool = True) -> None:
        super().__init__()
        self.use_time = bool(use_time)
        self.hidden_size = int(hidden_size)
        self.gru = nn.GRU(input_size=1 + (time_dim if self.use_time else 0), hidden_size=self.hidden_size,
                          num_layers=num_layers, batch_first=True, dropout=dropout if num_layers > 1 else 0.0)

    def forward(self, r: torch.Tensor, tfeat: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(B, L, S) residuals (+ (B, L, 9) time features) -> (B, S, hidden): h_L of the shared GRU
        over the B*S sensor sequences, on the fused HIP GRU (lg_gru_fwd / lg_gru_bwd; num_layers > 1:
        library.gru_stack, the top layer's h_L)."""
        if self.use_time and tfeat is None:
            raise ValueError("tfeat required when use_time=True")
        if not r.is_cuda:
            raise RuntimeError("SharedSensorGRUEncoder runs on a ROCm GPU only (libleakgnn has no CPU path)")
        g = self.gru
        if not 1 <= g.hidden_size <= 1024 or g.bidirectional or not g.bias:
            raise NotImplementedError("the HIP GRU kernels cover unidirectional GRUs with bias, hidden 1..1024 "
                                      "(32 / 64 tiled, others generic), any number of layers")
        f = ops._f32
        # contiguous once here: a strided tfeat (a slice of a longer segment) would otherwise be
        # saved as is and copied again in the backward
        tf = f(tfeat).contiguous() if self.use_time else None
        r = f(r)
        if g.num_layers == 1:
            ws = [f(t) for t in (g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)]
            save = torch.is_grad_enabled() and any(t.requires_grad
                                                   for t in [r, *ws] + ([tf] if tf is not None else []))
            return torch.ops.leakgnn.gru_encoder(r, tf, *ws, save)[0]
        # stacked: layer 0 as above, the upper layers on the dense-input kernels (library.gru_stack),
        # dropout between layers in train mode from the library's counter RNG
        ws = [[f(getattr(g, f"{n}_l{l}")) for l in range(g.num_layers)]
              for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        save = torch.is_grad_enabled() and any(t.requires_grad for t in [r, *sum(ws, [])] + ([tf] if tf is not None else []))
        p = float(g.dropout) if self.training else 0.0
        seed = library.seed_tensor(r.device) if p > 0.0 else _NO_SEED
        return torch.ops.leakgnn.gru_stack(r, tf, *ws, p, seed, save)[0]


class EdgeHead(nn.Module):
    def __init__(self, node_dim: int, hidden_dim: int = 128, dropout: float = 0.1) -> None:
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(node_dim * 3, hidden_dim), nn.ReLU(), nn.Dropout(dropout),
                                 nn.Linear(hidden_dim, 1))

    def forward(self, h_u: torch.Tensor, h_v: torch.Tensor) -> torch.Tensor:
        return self.forward_feat(torch.cat([h_u, h_v, (h_u - h_v).abs()], dim=-1))

    def forward_feat(self, feat: torch.Tensor) -> torch.Tensor:
        """feat = cat[h_u, h_v, |h_u - h_v|] already built (by lg_pipe_gather_fwd)."""
        return self.mlp(feat).squeeze(-1)


class NoLeakHead(nn.Module):
    def __init__(self, node_dim: int, hidden_dim: int = 128, dropout: float = 0.1) -> None:
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(node_dim, hidden_dim), nn.ReLU(), nn.Dropout(dropout),
                                 nn.Linear(hidden_dim, 1))

    def forward(self, pooled: torch.Tensor) -> torch.Tensor:
        return self.mlp(pooled).squeeze(-1)


def _batchify_edge_index(edge_index_single: torch.Tensor, num_nodes: int, batch_size: int) -> torch.Tensor:
    """(2, E) -> (2, E*B) disjoint union, column b*E + e = edge e offset by b*N (detector.py:105-114).
    Runs on the device (lg_batchify_edge_index); bit-exact."""
    return ops.batchify_edge_index(edge_index_single, num_nodes, batch_size)


class _EdgeWeightAnchor(torch.autograd.Function):
    """The graph's normalised coefficients w as a function of the learned link log-weights,
    WITHOUT device work in the forward: the values were computed when the graph was last
    reweighted (GCNGraph.reweight, under no_grad), and every forward that wants the gradient
    hangs a fresh autograd edge on them, so two backward passes between two optimizer steps
    need no second reweight.  backward: dL/dw -> per directed edge (leakgnn::gcn_edge_norm_backward,
    lg_gcn_norm_bwd) -> per link (the sum of a link's two edges: repeat_interleave(2)'s
    backward) -> times the link weight (exp's backward)."""

    @staticmethod
    def forward(ctx, log_w: torch.Tensor, g) -> torch.Tensor:
        ctx.norm = (g.normalize, g.fill)
        # the tensors of THIS reweight: a later one replaces g's attributes, not these
        ctx.save_for_backward(g.edge_weight, g.dis, g.rowptr, g.col, g.eid, g.rowptr_t, g.col_t, g.eid_t)
        return g.w.detach()

    @staticmethod
    def backward(ctx, dw: torch.Tensor):
        per_edge = ctx.saved_tensors[0]
        dv = torch.ops.leakgnn.gcn_edge_norm_backward(dw.contiguous(), *ctx.saved_tensors, *ctx.norm)
        return dv.view(-1, 2).sum(dim=1) * per_edge.view(-1, 2)[:, 0], None


def check_link_weight(edge_weight: torch.Tensor, n_links: int) -> torch.Tensor:
    """A positive floating tensor of shape (n_links,), checked on the host (ops.check_edge_weight's
    rules, plus positivity: a link weight is a length or a conductance, and its log is learned)."""
    try:
        ops.check_edge_weight(edge_weight, n_links)
    except ValueError as e:
        raise ValueError(str(e) + " (one weight per link of the .inp link table)") from None
    if n_links and not bool((edge_weight.detach() > 0).all()):
        raise ValueError(f"edge_weight must be positive (shape ({n_links},), one weight per link)")
    return edge_weight


class LeakDetector(nn.Module):
    """residual (B, L_det, S), tfeat (B, L_det, 9) -> logits (B, num_pipes + 1); class P = no leak."""

    def __init__(self, inp_path: str | Path, sensor_node_ids: Sequence[str], pipe_ids_in_order: Sequence[str],
                 sensor_hidden: int = 64, node_hidden: int = 64, gnn_layers: int = 2, dropout: float = 0.1,
                 use_time: bool = True, include_links: Sequence[str] = ("PIPES", "PUMPS", "VALVES"),
                 mlp_dtype: str = "fp32", sensor_layers: int = 1, sensor_dropout: float = 0.0,
                 edge_weight: Optional[torch.Tensor] = None, learn_edge_weight: bool = False,
                 skip: str = "none", norm: str = "none", diffuse_hops: int = 0, diffuse_alpha: float = 0.1) -> None:
        """edge_weight: None, or a positive floating (n_links,) tensor, one weight per link in the
        order of the link table build_wdn_graph_from_inp walks (utils.link_edge_weights builds one
        from the .inp file); link j is the directed edges 2j and 2j + 1 of edge_index_single.
        learn_edge_weight: the link weights are learned, exp(edge_log_weight), starting from
        edge_weight (or 1).
        skip: "none", or "residual": every GCN layer x = x + dropout(relu(conv(x))).  An attribute
        like mlp_dtype: no parameter, no state-dict entry.
        norm: "none", or "layer" (needs skip="residual"): pre-norm, a LayerNorm in front of every
        branch and of the heads; adds `norms` (gnn_layers + 1 nn.LayerNorm(node_hidden)).
        diffuse_hops, diffuse_alpha: K > 0 propagates the node init K hops before layer 0, z_{k+1} =
        (1 - alpha) Ahat z_k + alpha x_0 (APPNP; leakgnn::diffuse): reach gnn_layers + K with no
        parameter.  Attributes like skip: no state-dict entry; 0: the detector without them."""
        super().__init__()
        if not isinstance(diffuse_hops, int) or not 0 <= diffuse_hops <= 64:
            raise ValueError(f"diffuse_hops must be an integer in 0..64, got {diffuse_hops!r}")
        if not 0.0 <= float(diffuse_alpha) <= 1.0:
            raise ValueError(f"diffuse_alpha must be in [0, 1], got {diffuse_alpha!r}")
        if diffuse_hops > 0 and mlp_dtype == "bf16":
            raise NotImplementedError("diffuse_hops > 0 needs mlp_dtype='fp32': the hops run on the fp32-tier "
                                      "node-major trunk (lg_diffuse_fwd / lg_diffuse_bwd) only")
        if diffuse_hops > 0 and learn_edge_weight:
            raise NotImplementedError("diffuse_hops > 0 takes fixed edge weights only: the weight gradient through "
                                      "the hops would need every z_k saved and is not built")
        self.diffuse_hops, self.diffuse_alpha = int(diffuse_hops), float(diffuse_alpha)
        if skip not in ("none", "residual"):
            raise ValueError(f"skip must be 'none' or 'residual', got {skip!r}")
        if skip == "residual" and mlp_dtype == "bf16":
            raise NotImplementedError("skip='residual' needs mlp_dtype='fp32': the skip lives on the fp32-tier "
                                      "trunk kernels (lg_gcn_fwd_nm_skip / lg_gcn_bwd_nm_skip) only")
        self.skip = skip
        if norm not in ("none", "layer"):
            raise ValueError(f"norm must be 'none' or 'layer', got {norm!r}")
        if norm == "layer" and skip != "residual":
            raise ValueError("norm='layer' is the pre-norm residual block: it needs skip='residual'")
        if norm == "layer" and mlp_dtype == "bf16":
            raise NotImplementedError("norm='layer' needs mlp_dtype='fp32': the norm lives on the fp32-tier "
                                      "trunk kernels (lg_add_layernorm_fwd / lg_layernorm_bwd) only")
        self.norm = norm
        if mlp_dtype not in ("fp32", "bf16"):
            raise ValueError(f"mlp_dtype must be 'fp32' or 'bf16', got {mlp_dtype!r}")
        if learn_edge_weight and mlp_dtype == "bf16":
            raise NotImplementedError("learn_edge_weight=True needs mlp_dtype='fp32': the gradient of the edge "
                                      "weights through the trunk (lg_sddmm_nm) exists on the fp32 tier only")
        # "bf16": BASELINE configs[2]'s tier — the GCN transforms and the EdgeHead MLP as one
        # bf16 MFMA product with fp32 accumulate (LG_F_BF16); activations stay fp32.  Not an
        # fp32-parity mode (2e-2 relative on logits).  Not a state-dict entry.
        self.mlp_dtype = mlp_dtype
        self.graph: WDNGraph = build_wdn_graph_from_inp(inp_path=inp_path, sensor_node_ids=sensor_node_ids,
                                                        pipe_ids_in_order=pipe_ids_in_order,
                                                        include_links=include_links, add_self_loops=False,
                                                        make_undirected=True)
        self.node_names = self.graph.node_names
        self.node_to_idx = self.graph.node_to_idx
        self.pipe_ids = self.graph.pipe_ids
        self.pipe_to_idx = self.graph.pipe_to_idx
        self.pipe_ends = torch.tensor(self.graph.pipe_ends, dtype=torch.long)
        self.edge_index_single = self.graph.edge_index
        self.sensor_node_ids = list(sensor_node_ids)
        self.sensor_node_idx = torch.tensor([self.node_to_idx[n] for n in self.sensor_node_ids], dtype=torch.long)

        self.sensor_encoder = SharedSensorGRUEncoder(hidden_size=sensor_hidden, num_layers=sensor_layers,
                                                     dropout=sensor_dropout, use_time=use_time)
        self.sensor_to_node = nn.Linear(sensor_hidden + 1, node_hidden)
        self.convs = nn.ModuleList(
            [GCNConv(node_hidden, node_hidden, add_self_loops=True, normalize=True) for _ in range(gnn_layers)])
        if norm == "layer":
            self.norms = nn.ModuleList(nn.LayerNorm(node_hidden) for _ in range(gnn_layers + 1))
        self.dropout = nn.Dropout(dropout)
        self.edge_head = EdgeHead(node_hidden, hidden_dim=128, dropout=dropout)
        self.noleak_head = NoLeakHead(node_hidden, hidden_dim=128, dropout=dropout)
        self._dev_state: Dict[torch.device, tuple] = {}
        # Test hook: a dict here receives the step's ReLU outputs as the kernels produced them
        # ("xs": node init + every GCN layer, "edge_hidden", "noleak_hidden"), so parity tests
        # can evaluate the fp64 truth on the same side of every ReLU kink.  None: nothing kept.
        self.capture: Optional[dict] = None
        # graph_step.CapturedTrainStep at world > 1: forward keeps the trunk output (the heads'
        # input) as `boundary` while keep_boundary is set, so the backward can stop there and
        # the heads' gradient all-reduce overlaps the trunk backward (overlap_split)
        self.keep_boundary = False
        # node-major trunk: keep the node init compressed (sensor rows + [x0 > 0] bits,
        # lg_node_init_bits_fwd) instead of materialising x_0 (43 MB at B = 256)
        self.compress_x0 = True
        # EdgeHead backward node sums: True = streamed per tile through the pipe schedule (each
        # node's incidences summed in schedule order); False = the reference's order (items
        # ascending, as index_add over pipe ids), per-window scatter.  Read when the device
        # state is first built.
        self.incidence_schedule = True
        # node-major training: the GRU encoder, node init and GCN layers as one op
        # (library.encoder_trunk: the node init formed in the GRU's epilogue, the projection's
        # backward in the GRU backward's); False: the encoder module, then library.gnn_trunk
        self.fuse_encoder = True
        self.boundary: Optional[torch.Tensor] = None
        self._batched_edges: Dict[tuple, torch.Tensor] = {}  # (B, device) -> (2, B*E): the general path's edge_index
        # edge weights: a buffer `edge_weight` (fixed) or a parameter `edge_log_weight` (learned),
        # both (n_links,); neither: the unweighted graph, no state-dict entry
        self.learn_edge_weight = bool(learn_edge_weight)
        n_links = self.edge_index_single.size(1) // 2
        assert 2 * n_links == self.edge_index_single.size(1), "make_undirected=True gives two directed edges per link"
        if edge_weight is not None:
            edge_weight = check_link_weight(edge_weight, n_links).detach().to(torch.float32)
        if self.learn_edge_weight:
            self.edge_log_weight = nn.Parameter(edge_weight.log() if edge_weight is not None else torch.zeros(n_links))
        elif edge_weight is not None:
            self.register_buffer("edge_weight", edge_weight.clone(), persistent=True)
        self.weighted = self.learn_edge_weight or edge_weight is not None
        # device -> (tensor, _version) of the weights the device graph was last built from; None
        # after a reweight recorded into a HIP graph (its replays move the weights, not _version)
        self._ew_stamp: Dict[torch.device, Optional[tuple]] = {}
        self._reweights = 0  # GCNGraph.reweight calls so far (tests: an unchanged version launches none)
        self._batched_weights: Dict[tuple, tuple] = {}  # (B, device) -> (stamp, (B*E,)): the general path's fixed weights

    def overlap_split(self):
        """Parameters whose gradients are final once the backward reaches `boundary` (the
        heads: EdgeHead + NoLeakHead, detector.py:206-218 of the reference)."""
        return list(self.edge_head.parameters()) + list(self.noleak_head.parameters())

    # -- device-resident graph state (built once per device; not part of state_dict)
    def _device_state(self, device: torch.device):
        st = self._dev_state.get(device)
        if st is None:
            N = len(self.node_names)
            src = self._link_weight_source()
            graph = ops.GCNGraph.build(self.edge_index_single, N, device, add_self_loops=True, normalize=True,
                                       edge_weight=self._per_edge_weights(device) if self.weighted else None)
            if self.weighted:
                self._ew_stamp[device] = (src, src._version)
            inc = ops.Incidence.build(self.pipe_ends, N, device, schedule=self.incidence_schedule)
            slot = torch.full((N,), -1, dtype=torch.int32)
            for s, n in enumerate(self.sensor_node_idx.tolist()):
                slot[n] = s  # duplicate sensor ids: last write wins, as h0[:, idx] = h_s does
            live = torch.tensor([float(slot[n] == s) for s, n in enumerate(self.sensor_node_idx.tolist())])
            nonsensor = torch.nonzero(slot < 0).flatten()
            graph.x0marks = None  # built on the first node-major forward that compresses x_0 (_x0marks)
            st = (graph, inc, slot.to(device), self.sensor_node_idx.to(device),
                  None if bool(live.all()) else live.to(device), nonsensor.to(device))
            self._dev_state[device] = st
        return st

    def _link_weight_source(self) -> Optional[torch.Tensor]:
        """The state-dict tensor the link weights come from (None: unweighted)."""
        if self.learn_edge_weight:
            return self.edge_log_weight
        return self.edge_weight if self.weighted else None

    def _per_edge_weights(self, device: torch.device) -> torch.Tensor:
        """(E,) weights of edge_index_single's directed edges: link j's weight at 2j and 2j + 1.
        Carries the autograd edge to edge_log_weight when the weights learn (the general path)."""
        src = self._link_weight_source()
        w = src.exp() if self.learn_edge_weight else src
        return w.to(device=device, dtype=torch.float32).repeat_interleave(2)

    def _sync_edge_weights(self, graph, device: torch.device) -> None:
        """Bring the device graph up to the current link weights: when the source tensor's
        _version has moved since the graph was last built from it (an optimizer step, a
        load_state_dict), GCNGraph.reweight (device work only) and the sensor-marked tables
        refreshed in place.  An unchanged version does nothing, so an eval loop never reweights.
        While a HIP graph is being captured the launches of LEARNED weights are always recorded (every replay then
        reweights from the weights it finds) and the stamp is dropped, as a replayed optimizer
        step moves no _version: the next eager forward reweights again."""
        src = self._link_weight_source()
        # (fixed weights are a buffer no captured step writes: they follow the stamp alone)
        capturing = self.learn_edge_weight and torch.cuda.is_current_stream_capturing()
        stamp = self._ew_stamp.get(device)
        if not capturing and stamp is not None and stamp[0] is src and stamp[1] == src._version:
            return
        with torch.no_grad():
            graph.reweight(self._per_edge_weights(device))
        self._reweights += 1
        if graph.x0marks is not None:
            graph.x0marks.refresh(graph)
        self._ew_stamp[device] = None if capturing else (src, src._version)

    def invalidate_edge_weights(self) -> None:
        """Forget which weights the device graphs were built from: the next forward reweights.
        For whoever changes the weights without moving their _version, i.e. replays a HIP graph
        that holds an optimizer step (the training CLI, after each replay).  No device work."""
        self._ew_stamp.clear()

    def _x0marks(self, graph, slot: torch.Tensor):
        """The compressed layer-0 input's sensor-marked node tables (lg_nm_table_sensor_mark),
        built once per device on the first forward that uses them (window-major batches never
        do).  Its launches must run eagerly, not be recorded into a graph being captured."""
        if graph.x0marks is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("LeakDetector: run one eager node-major forward before capturing a graph "
                                   "(the compressed node init's tables are built on first use)")
            graph.x0marks = ops.SensorMarks.build(graph, slot)
        return graph.x0marks

    def _fused_encoder(self, residual: torch.Tensor, tfeat: Optional[torch.Tensor], B: int, N: int, D: int,
                       nm: bool) -> bool:
        """Whether this forward runs the encoder, node init and layers as ONE op
        (library.encoder_trunk): the node-major trunk with the compressed node init, the
        reference encoder (1 layer, bias) with node_hidden == sensor_hidden, and residual /
        tfeat as data (no gradient wanted for them: the fused backward forms no dx)."""
        g = self.sensor_encoder.gru
        if not (self.fuse_encoder and g.num_layers == 1 and g.bias and not g.bidirectional):
            return False
        if self.skip != "none":  # the skip is not folded into encoder_trunk and the X0 kernels
            return False
        if self.diffuse_hops:  # nor is the diffusion stage: it needs the dense node init
            return False
        if self.capture is not None:  # the capture reads h_s, which the fused op never forms
            return False
        if residual.requires_grad or (tfeat is not None and self.sensor_encoder.use_time and tfeat.requires_grad):
            return False
        return library.encoder_trunk_supported(B, N, g.hidden_size, D, len(self.convs), nm, self.compress_x0)

    def _widths_tiled(self) -> bool:
        """Whether the trunk and heads run the tiled kernels: sensor_hidden == node_hidden in
        {32, 64} (the reference's callers use 64 and 64, train_detector.py:250-254)."""
        return (self.sensor_encoder.hidden_size in ops.SUPPORTED_D
                and self.sensor_to_node.out_features == self.sensor_encoder.hidden_size)

    def _forward_general(self, residual: torch.Tensor, tfeat: Optional[torch.Tensor]) -> torch.Tensor:
        """Any sensor_hidden / node_hidden (detector.py:128-129): the reference's forward
        (:170-218) composed from the width-general pieces — the GRU encoder (lg_gru_fwd's generic
        kernel off 32 / 64), GCNConv's general path (lg_spmm_cols propagate, library GEMM
        transform) over the batchified edge_index, and library GEMMs / device indexing for the
        node init and the heads; dropout from torch's generator (the tiled path's counter RNG
        is a kernel feature).  A generality path: the bench's widths never take it."""
        B, L, S = residual.shape
        dev = residual.device
        graph, inc, slot, sensor_idx, slot_live, nonsensor = self._device_state(dev)
        N = len(self.node_names)
        h_s = self.sensor_encoder(residual, tfeat)                           # (B, S, Ds)
        # h0 rows: [h_s of the node's sensor, 1] for sensor nodes (last duplicate wins, as
        # h0[:, idx] = h_s), zeros for the rest (:178-187)
        has = (slot >= 0).to(h_s.dtype).view(1, N, 1)
        h0 = torch.cat([h_s.index_select(1, slot.clamp(min=0).long()) * has, has.expand(B, N, 1)], dim=-1)
        p = float(self.dropout.p)
        x = F.dropout(F.relu(self.sensor_to_node(h0)), p, self.training).reshape(B * N, -1)
        if self.diffuse_hops:  # the hops composed from the width-general propagate, window by window
            g, a = graph, self.diffuse_alpha
            x0 = x.view(B, N, -1).transpose(0, 1).reshape(N, -1)  # [N][B * D]: one propagate serves every window
            z = x0
            for _ in range(self.diffuse_hops):
                z = (1.0 - a) * torch.ops.leakgnn.spmm_cols(z, None, g.rowptr, g.col, g.w, g.rowptr_t, g.col_t,
                                                            g.w_t) + a * x0
            x = z.view(N, B, -1).transpose(0, 1).reshape(B * N, -1)
        ei = self._batched_edges.get((B, dev))
        if ei is None:
            ei = _batchify_edge_index(self.edge_index_single.to(dev), N, B)
            self._batched_edges[(B, dev)] = ei
        ew = None
        if self.learn_edge_weight:
            ew = self._per_edge_weights(dev).repeat(B)  # column b*E + e is edge e; autograd to edge_log_weight
        elif self.weighted:
            src = self.edge_weight
            hit = self._batched_weights.get((B, dev))
            if hit is None or hit[0] != (src.data_ptr(), src._version):
                hit = ((src.data_ptr(), src._version), self._per_edge_weights(dev).repeat(B))
                self._batched_weights[(B, dev)] = hit
            ew = hit[1]
        ln = self.norm == "layer"
        for l, conv in enumerate(self.convs):
            xin = self.norms[l](x) if ln else x
            br = F.dropout(F.relu(conv(xin, ei) if ew is None else conv(xin, ei, ew)), p, self.training)
            x = x + br if self.skip == "residual" else br
        if ln:  # the heads read the normalised stream
            x = self.norms[len(self.convs)](x)
        h_nodes = x.view(B, N, -1)
        ends = inc.ends.long()
        pipe_logits = self.edge_head(h_nodes[:, ends[:, 0]], h_nodes[:, ends[:, 1]])     # (B, P)
        pooled = global_mean_pool(x, torch.arange(B, device=dev).repeat_interleave(N), size=B)
        return torch.cat([pipe_logits, self.noleak_head(pooled).unsqueeze(-1)], dim=-1)

    def forward(self, residual: torch.Tensor, tfeat: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not residual.is_cuda:
            raise RuntimeError("LeakDetector runs on a ROCm GPU only (libleakgnn has no CPU path)")
        if not self._widths_tiled():
            return self._forward_general(residual, tfeat)
        B, L, S = residual.shape
        graph, inc, slot, sensor_idx, slot_live, nonsensor = self._device_state(residual.device)
        f = ops._f32
        Wn, bn = f(self.sensor_to_node.weight), f(self.sensor_to_node.bias)  # (D, Ds+1), (D,)
        N, D = len(self.node_names), Wn.shape[0]
        skip = self.skip == "residual"
        hops = self.diffuse_hops
        dkw = {"hops": hops, "alpha": self.diffuse_alpha} if hops else {}  # absent at 0: the op as before
        # a skip or diffusion model takes the node-major layout at every B, as the bf16 tier does
        nm = ops.use_node_major(B, N, D, bf16=self.mlp_dtype == "bf16" or skip or hops > 0)
        drop = self.training and float(self.dropout.p) > 0.0
        g = graph
        bf16 = self.mlp_dtype == "bf16"
        enc = self.sensor_encoder
        edge_w = None
        if self.weighted:
            self._sync_edge_weights(g, residual.device)
            if self.learn_edge_weight and torch.is_grad_enabled() and self.edge_log_weight.requires_grad:
                edge_w = _EdgeWeightAnchor.apply(self.edge_log_weight, g)
        if enc.use_time and tfeat is None:
            raise ValueError("tfeat required when use_time=True")
        if self._fused_encoder(residual, tfeat, B, N, D, nm):
            # encoder + node init + layers as one op (library.encoder_trunk)
            mk = self._x0marks(g, slot)
            gw = [f(t) for t in (enc.gru.weight_ih_l0, enc.gru.weight_hh_l0, enc.gru.bias_ih_l0, enc.gru.bias_hh_l0)]
            cw, cb = [f(c.lin.weight) for c in self.convs], [f(c.bias) for c in self.convs]
            save = torch.is_grad_enabled() and (edge_w is not None or any(t.requires_grad for t in gw + [Wn, bn] + cw + cb))
            tf = f(tfeat).contiguous() if enc.use_time else None
            trunk = library.trunk_fields("encoder_trunk", torch.ops.leakgnn.encoder_trunk(
                f(residual), tf, *gw, Wn, bn, cw, cb, slot, sensor_idx, slot_live, g.nodetab, g.pairs, g.nodetab_t,
                g.pairs_t, mk.nodetab_s, mk.pairs_s, mk.pos_slot_t, float(self.dropout.p) if drop else 0.0,
                library.seed_tensor(residual.device) if drop else _NO_SEED, save, edge_w,
                g.rowptr if edge_w is not None else None, g.col if edge_w is not None else None, bf16=bf16))
        else:
            h_s = self.sensor_encoder(residual, tfeat)                        # (B, S, Ds)
            if self.capture is not None and torch.is_grad_enabled():
                if h_s.requires_grad:
                    h_s.retain_grad()
                self.capture["h_s"] = h_s
            # sensor_to_node (rows with a sensor: [h_s, 1] W^T + b; without: b) folded into node init
            mk = (self._x0marks(g, slot)
                  if (nm and self.compress_x0 and len(self.convs) > 1 and not skip and not hops) else None)
            if self.norm == "layer":
                trunk = library.trunk_fields("gnn_trunk_norm", torch.ops.leakgnn.gnn_trunk_norm(
                    h_s, Wn, bn, [f(c.lin.weight) for c in self.convs], [f(c.bias) for c in self.convs],
                    [f(n.weight) for n in self.norms], [f(n.bias) for n in self.norms], slot, sensor_idx, nonsensor,
                    slot_live, g.nodetab, g.pairs, g.rowptr, g.col, g.nodetab_t, g.pairs_t,
                    float(self.dropout.p) if drop else 0.0, float(self.norms[0].eps),
                    library.seed_tensor(residual.device) if drop else _NO_SEED, edge_w, **dkw), hops > 0)
            else:
                trunk = library.trunk_fields("gnn_trunk", torch.ops.leakgnn.gnn_trunk(
                    h_s, Wn, bn, [f(c.lin.weight) for c in self.convs], [f(c.bias) for c in self.convs], slot, sensor_idx,
                    nonsensor, slot_live, g.nodetab, g.pairs, g.rowptr, g.col, g.w, g.nodetab_t, g.pairs_t, g.rowptr_t,
                    g.col_t, g.w_t, float(self.dropout.p) if drop else 0.0, nm,
                    library.seed_tensor(residual.device) if drop else _NO_SEED,
                    mk.nodetab_s if mk is not None else None, mk.pairs_s if mk is not None else None,
                    mk.pos_slot_t if mk is not None else None, edge_w, bf16=bf16, **({"skip": True} if skip else {}),
                    **dkw), hops > 0)
        # xs: x_0 (its sensor rows while x0bits is non-empty) .. x_L; xns: under norm="layer" xn_0 .. xn_L
        xs, xns, ymask, x0bits = trunk.xs, trunk.xns, trunk.ymask, trunk.x0bits
        # (N, B, D) node-major, else (B, N, D); under norm="layer" the last norm's output
        h_nodes = trunk.h
        if self.keep_boundary:
            self.boundary = h_nodes
        mlp = self.edge_head.mlp     # Linear(3D,128), ReLU, Dropout, Linear(128,1)
        nmlp = self.noleak_head.mlp  # Linear(D,128), ReLU, Dropout, Linear(128,1)
        pe = float(mlp[2].p) if self.training else 0.0
        pn = float(nmlp[2].p) if self.training else 0.0
        hw = [f(t) for t in (mlp[0].weight, mlp[0].bias, mlp[3].weight, mlp[3].bias,
                             nmlp[0].weight, nmlp[0].bias, nmlp[3].weight, nmlp[3].bias)]
        keep = torch.is_grad_enabled() and (h_nodes.requires_grad or any(t.requires_grad for t in hw))
        seed = library.seed_tensor(residual.device) if (pe > 0.0 or pn > 0.0) else _NO_SEED
        # (B, P+1): pipe logits, then the no-leak logit of the mean-pooled window (:206-218)
        sched, sched_hdr = inc.schedule(D)
        out = torch.ops.leakgnn.detector_heads(h_nodes, *hw, inc.ends, inc.rowptr, inc.item, pe, pn, nm, keep, seed,
                                               sched, sched_hdr, bf16=bf16)
        if self.capture is not None:
            if x0bits is not None and x0bits.numel() > 0:  # x_0 compressed: materialise it for the diagnostics
                xs = [library.expand_x0(xs[0], x0bits, slot, bn, N, float(self.dropout.p) if drop else 0.0)] + xs[1:]
            self.capture.update(xs=xs, node_major=nm, edge_hidden=out[1], noleak_hidden=out[3])
            if skip:  # the branches' keep decisions [f > 0], which xs[l] > 0 no longer is
                nl = len(self.convs)
                self.capture["fmask"] = [_unpack_mask(w, N, B, D) for w in ymask.view(nl, -1)] if nl else []
            if self.norm == "layer":  # the branches' inputs and the heads' (xs stays the residual stream)
                self.capture["xns"] = xns
            if hops:  # the diffused node init z_K: layer 0's input, or the residual stream's start
                self.capture["z"] = trunk.z
        return out[0]


_NO_SEED = torch.zeros(1, dtype=torch.long)  # seed argument of an op that draws no dropout mask


def _unpack_mask(words: torch.Tensor, N: int, B: int, D: int) -> torch.Tensor:
    """The mask words of lg_gcn_fwd_nm_bits / _skip (include/leakgnn.h) as a bool (N, B, D) tensor:
    per node and 16-window tile 64 lanes, bit 4k + i of lane l = row 16g + (64 / (D/4)) k + l // (D/4),
    channel 4 (l % (D/4)) + i.  Diagnostics only (LeakDetector.capture)."""
    assert words.numel() == library.mask_words(N, B)
    T, lpr = words.numel() // (64 * N), D // 4  # 16-window tiles per node
    rpp = 64 // lpr
    w = words.view(N, T, rpp, lpr).to(torch.int32) & 0xFFFF                     # [n][g][l // lpr][l % lpr]
    sh = (4 * torch.arange(16 // rpp, device=words.device).view(-1, 1) + torch.arange(4, device=words.device)).view(-1)
    bits = ((w.unsqueeze(-1) >> sh.to(torch.int32)) & 1).bool()                 # [n][g][lr][lc][k * 4 + i]
    bits = bits.view(N, T, rpp, lpr, 16 // rpp, 4).permute(0, 1, 4, 2, 3, 5)   # [n][g][k][lr][lc][i]
    return bits.reshape(N, T * 16, D)[:, :B].contiguous()


def detector_from_args(inp_path: str | Path, sensor_ids: Sequence[str], pipe_ids_in_order: Sequence[str],
                       args: Optional[dict] = None, cls=None, **kwargs) -> LeakDetector:
    """The LeakDetector of the training CLI (train_detector.py:250-254 of the reference: widths 64,
    two layers, dropout 0.1), its edge-weight options read from `args`: the CLI's vars(namespace)
    or a checkpoint's ckpt["args"].  "edge_weight" in {none, ones, length, inv_length, conductance}
    (utils.link_edge_weights) and "learn_edge_weight"; a missing key is the unweighted detector.
    "gnn_layers" (default 2) and "skip" in {none, residual} (default none): a missing key is the
    two-layer plain trunk, so checkpoints from before these flags load as before.  "norm" in {none,
    layer} (default none) likewise, and so are "diffuse_hops" (default 0) and "diffuse_alpha" (0.1).
    cls: the class to build (the caller's own LeakDetector name; default: this module's)."""
    args = args or {}
    mode = args.get("edge_weight") or "none"
    ew = link_edge_weights(inp_path, mode=mode) if mode != "none" else None
    skip = args.get("skip") or "none"
    norm = args.get("norm") or "none"
    hops = int(args.get("diffuse_hops") or 0)
    alpha = args.get("diffuse_alpha")
    dkw = {"diffuse_hops": hops, "diffuse_alpha": 0.1 if alpha is None else float(alpha)} if hops else {}
    return (cls or LeakDetector)(inp_path, sensor_ids, pipe_ids_in_order, sensor_hidden=64, node_hidden=64,
                                 gnn_layers=int(args.get("gnn_layers") or 2), dropout=0.1, use_time=True,
                                 edge_weight=ew, learn_edge_weight=bool(args.get("learn_edge_weight", False)),
                                 **({"skip": skip} if skip != "none" else {}),
                                 **({"norm": norm} if norm != "none" else {}), **dkw, **kwargs)


def detector_from_checkpoint(ckpt: dict, inp_path: str | Path, **kwargs) -> LeakDetector:
    """The detector a checkpoint of train_detector describes, its state loaded strictly (a weighted
    checkpoint carries `edge_weight` or `edge_log_weight`, which ckpt["args"] announces)."""
    det = detector_from_args(inp_path, ckpt["sensor_ids"], ckpt["pipe_ids_in_order"], ckpt.get("args"), **kwargs)
    det.load_state_dict(ckpt["detector_state"], strict=True)
    return det
