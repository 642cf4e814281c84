"""MeshGraphNet baseline of the Navier-Stokes benchmark (src/nsbench/models/mgn/meshgraphnet.py) on the graph kernels
(graph_ops): constructor keywords, `forward` signature and `state_dict` keys are the reference's, so its checkpoints load with
`load_state_dict(strict=True)`.

DGL is a graph container in the reference, not arithmetic: on the fixed mesh the model is three kinds of row MLP with indexed
operand loads.  Every MLP (Linear/ReLU chain, LayerNorm, residual) is ONE launch forward; `cat(e, v[src], v[dst])` and
`cat(agg, v)` are never written.  The mesh comes from mgn_graph.build_graph (numpy), with the reference's edge features.  The
edge encoder's input is the same for every time step: it runs once per `forward`.
"""
import torch
import torch.nn as nn

from .. import lib as L
from .. import mgn_graph
from ..graph_ops import AGGREGATIONS, Graph, edge_block, graph_mlp, node_block
from ..rollout_ops import ns_rollout
from .convlstm import _Slot


class MeshGraphMLP(nn.Module):
    """`model` = Sequential(Linear, slot, [Linear, slot, ...] Linear [, LayerNorm]) with the reference's indices (a parameter-free
    slot stands where it has the activation: ReLU, or SiLU in GraphCast); `forward` on rows is graph_ops.graph_mlp."""

    def __init__(self, input_dim, output_dim, hidden_dim, hidden_layers, norm=True, act="relu"):
        super().__init__()
        layers = [nn.Linear(input_dim, hidden_dim), _Slot()]
        for _ in range(hidden_layers - 1):
            layers += [nn.Linear(hidden_dim, hidden_dim), _Slot()]
        layers.append(nn.Linear(hidden_dim, output_dim))
        if norm:
            layers.append(nn.LayerNorm(output_dim))
        self.model = nn.Sequential(*layers)
        self.hidden_layers, self.has_norm, self.act = hidden_layers, norm, act

    def params(self):
        return [p for m in self.model if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]

    def norm(self):
        return (self.model[-1].weight, self.model[-1].bias) if self.has_norm else None

    def forward(self, x):
        return graph_mlp(x, self.params(), self.norm(), act=self.act)


class MeshEdgeBlock(nn.Module):
    def __init__(self, dim, hidden_layers, act="relu"):
        super().__init__()
        self.edge_mlp = MeshGraphMLP(3 * dim, dim, dim, hidden_layers, act=act)

    def forward(self, e, v, graph):
        return edge_block(e, v, graph, self.edge_mlp.params(), self.edge_mlp.norm(), act=self.edge_mlp.act), v


class MeshNodeBlock(nn.Module):
    def __init__(self, aggregation, dim, hidden_layers, act="relu"):
        super().__init__()
        self.aggregation = aggregation
        self.node_mlp = MeshGraphMLP(2 * dim, dim, dim, hidden_layers, act=act)

    def forward(self, e, v, graph):
        return e, node_block(e, v, graph, self.node_mlp.params(), self.node_mlp.norm(), self.aggregation, act=self.node_mlp.act)


class MeshGraphNetProcessor(nn.Module):
    """`processor_layers` = edge block, node block, edge block, ... (the reference's interleaved ModuleList)"""

    def __init__(self, processor_size, dim, num_layers_node, num_layers_edge, aggregation, act="relu"):
        super().__init__()
        layers = []
        for _ in range(processor_size):
            layers += [MeshEdgeBlock(dim, num_layers_edge, act), MeshNodeBlock(aggregation, dim, num_layers_node, act)]
        self.processor_layers = nn.ModuleList(layers)

    def forward(self, v, e, graph):
        for m in self.processor_layers:
            e, v = m(e, v, graph)
        return v


def _graph_spec(graph):
    """(height, width, periodic) of the `graph=` keyword: an object with these attributes (the reference's config node) or a dict"""
    if graph is None:
        raise ValueError("MeshGraphNet needs graph= (height, width, periodic): the mesh is built at construction")
    get = graph.get if isinstance(graph, dict) else lambda k, d=None: getattr(graph, k, d)      # noqa: E731
    h, w = get("height"), get("width")
    if h is None or w is None:
        raise ValueError("graph= needs height and width")
    p = get("periodic", True)
    return int(h), int(w), (bool(p) if isinstance(p, (bool, int)) else tuple(bool(q) for q in p))


def check_limits(widths, depths, aggregation, do_concat_trick, num_processor_checkpoint_segments):
    """The refusals every model on the graph kernels shares (widths, depths: keyword -> value)"""
    if do_concat_trick:
        raise NotImplementedError("do_concat_trick=True splits the first edge Linear into three parameters (lin_efeat, lin_src, "
                                  "lin_dst): other state_dict keys, not built")
    if num_processor_checkpoint_segments and int(num_processor_checkpoint_segments) > 0:
        raise NotImplementedError("num_processor_checkpoint_segments > 0 (gradient checkpointing of the processor) is not built")
    if aggregation not in AGGREGATIONS:
        raise ValueError(f"aggregation must be 'sum' or 'mean', not {aggregation!r}")
    for k, d in widths.items():
        if int(d) < 1:
            raise ValueError(f"{k} = {d} must be positive")
        if int(d) > L.GRAPH_MAX_WIDTH:
            raise NotImplementedError(f"{k} = {d}: the graph kernels take widths up to {L.GRAPH_MAX_WIDTH}")
    for k, d in depths.items():
        if int(d) < 1:
            raise ValueError(f"{k} = {d} must be at least 1")
        if int(d) > L.GRAPH_MAX_HIDDEN_LAYERS:
            raise NotImplementedError(f"{k} = {d}: the graph kernels take up to {L.GRAPH_MAX_HIDDEN_LAYERS} hidden layers")


class MeshGraphNetBase(nn.Module):
    """What the two benchmarks' classes share: the refusals, the mesh, the four sub-networks (registered in the reference's
    order: edge_encoder, node_encoder, node_decoder, processor) and one network call."""

    def _build(self, input_dim_nodes, input_dim_edges, output_dim, processor_size, message_passing_steps, num_layers_node_processor,
               num_layers_edge_processor, hidden_dim_processor, hidden_dim_node_encoder, num_layers_node_encoder,
               hidden_dim_edge_encoder, num_layers_edge_encoder, hidden_dim_node_decoder, num_layers_node_decoder, aggregation,
               do_concat_trick, num_processor_checkpoint_segments, graph_type, graph, cylinder, device):
        check_limits({}, {}, "sum", do_concat_trick, num_processor_checkpoint_segments)
        if graph_type not in mgn_graph.GRAPH_TYPES:
            raise ValueError(f"graph_type is '{graph_type}' but should be any of {list(mgn_graph.GRAPH_TYPES)}.")
        if aggregation not in AGGREGATIONS:
            raise ValueError(f"aggregation must be 'sum' or 'mean', not {aggregation!r}")
        if int(input_dim_edges) != mgn_graph.EDGE_FEATURES[graph_type]:
            raise ValueError(f"input_dim_edges = {input_dim_edges}, but the edges of a '{graph_type}' graph carry "
                             f"{mgn_graph.EDGE_FEATURES[graph_type]} features")
        widths = dict(input_dim_nodes=input_dim_nodes, input_dim_edges=input_dim_edges, output_dim=output_dim,
                      hidden_dim_processor=hidden_dim_processor, hidden_dim_node_encoder=hidden_dim_node_encoder,
                      hidden_dim_edge_encoder=hidden_dim_edge_encoder, hidden_dim_node_decoder=hidden_dim_node_decoder)
        depths = dict(num_layers_node_processor=num_layers_node_processor, num_layers_edge_processor=num_layers_edge_processor,
                      num_layers_node_encoder=num_layers_node_encoder, num_layers_edge_encoder=num_layers_edge_encoder,
                      num_layers_node_decoder=num_layers_node_decoder)
        check_limits(widths, depths, aggregation, False, 0)
        if int(processor_size) < 1 or int(message_passing_steps) < 1:
            raise ValueError("processor_size and message_passing_steps must be at least 1")
        self.message_passing_steps, self.graph_type = int(message_passing_steps), graph_type
        self.height, self.width, self.periodic = _graph_spec(graph)
        mesh = mgn_graph.build_graph(graph_type, self.height, self.width, self.periodic, cylinder=cylinder)
        self.graph = Graph.from_mesh(mesh)
        self._edge_features = torch.from_numpy(mesh.edge_features)
        self._batched = (None, None)
        self.edge_encoder = MeshGraphMLP(input_dim_edges, hidden_dim_processor, hidden_dim_edge_encoder, num_layers_edge_encoder)
        self.node_encoder = MeshGraphMLP(input_dim_nodes, hidden_dim_processor, hidden_dim_node_encoder, num_layers_node_encoder)
        self.node_decoder = MeshGraphMLP(hidden_dim_processor, output_dim, hidden_dim_node_decoder, num_layers_node_decoder, norm=False)
        self.processor = MeshGraphNetProcessor(processor_size, hidden_dim_processor, num_layers_node_processor,
                                               num_layers_edge_processor, aggregation)
        if device is not None:
            self.to(device)

    def _check_grid(self, H, W):
        if (H, W) != (self.height, self.width):
            raise ValueError(f"the mesh was built for a {self.height} x {self.width} grid, the input is {H} x {W}")

    def batched_edge_features(self, B, device):
        """the mesh's edge features repeated for B samples `[B * E, F]` (the most recent batch size and device is kept)"""
        key = (B, str(device))
        if self._batched[0] != key:
            self._batched = (key, self._edge_features.to(device).repeat(B, 1))
        return self._batched[1]

    def encode_edges(self, B, device):
        return self.edge_encoder(self.batched_edge_features(B, device))

    def network(self, x_t, e0):
        """one network call: channels-first `[B, C, H, W]` in (one permute copy to rows "(b h w) d"), channels-first view out"""
        B, C, H, W = x_t.shape
        v = self.node_encoder(x_t.permute(0, 2, 3, 1).reshape(B * H * W, C))
        for _ in range(self.message_passing_steps):
            v = self.processor(v, e0, self.graph)
        return self.node_decoder(v).view(B, H, W, -1).permute(0, 3, 1, 2)


class MeshGraphNet(MeshGraphNetBase):
    """`forward(x [B, T, D, H, W], teacher_forcing_steps)` -> `[B, T, D, H, W]`; the rollout is the one of the other nsbench
    models (rollout_ops.ns_rollout), so `output_dim` must equal `input_dim_nodes`.  `graph`: an object or dict with `height`,
    `width`, `periodic`; `graph_type`: "grid_2d", "grid_2d_8stencil" (3 edge features) or "delaunay".  Refused:
    `do_concat_trick`, processor checkpointing, widths above 128, more than 3 hidden layers (NotImplementedError); unknown
    `graph_type` / `aggregation`, an `input_dim_edges` that is not the graph type's feature count (ValueError).  Extra keywords
    (`type`, `name`, ...) are ignored; `device` moves the parameters."""

    def __init__(self, input_dim_nodes, input_dim_edges, output_dim, context_size=5, processor_size=15, message_passing_steps=1,
                 num_layers_node_processor=2, num_layers_edge_processor=2, hidden_dim_processor=128, hidden_dim_node_encoder=128,
                 num_layers_node_encoder=2, hidden_dim_edge_encoder=128, num_layers_edge_encoder=2, hidden_dim_node_decoder=128,
                 num_layers_node_decoder=2, aggregation="sum", do_concat_trick=False, num_processor_checkpoint_segments=0,
                 graph_type="grid_2d", graph=None, device=None, **kwargs):
        super().__init__()
        if int(context_size) < 1:
            raise ValueError("context_size must be >= 1")
        self.context_size, self.output_dim = int(context_size), int(output_dim)
        self._build(int(input_dim_nodes) * self.context_size, input_dim_edges, output_dim, processor_size, message_passing_steps,
                    num_layers_node_processor, num_layers_edge_processor, hidden_dim_processor, hidden_dim_node_encoder,
                    num_layers_node_encoder, hidden_dim_edge_encoder, num_layers_edge_encoder, hidden_dim_node_decoder,
                    num_layers_node_decoder, aggregation, do_concat_trick, num_processor_checkpoint_segments, graph_type, graph,
                    False, device)

    def forward(self, x, teacher_forcing_steps=15):
        self._check_grid(x.shape[-2], x.shape[-1])
        e0 = self.encode_edges(x.shape[0], x.device)
        return ns_rollout(lambda x_t: self.network(x_t, e0), x, teacher_forcing_steps, self.context_size)
