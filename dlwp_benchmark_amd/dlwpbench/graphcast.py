"""GraphCast baseline of the weather benchmark (src/dlwpbench/models/graphcast/graph_cast_net.py, GraphCastNet) on the wide,
bipartite graph kernels (graph_ops.wide_*; csrc/graph_wide.hip): the reference's constructor keywords,
`forward(constants, prescribed, prognostic)` and `state_dict` keys in its registration order, so its checkpoints load with
`load_state_dict(strict=True)`.

The model lives on three graphs built from an icosphere file (gc_mesh, numpy): grid -> mesh (g2m), the multimesh, mesh -> grid
(m2g).  One network call: the grid-node embedder, the encoder (g2m edge MLP, mesh nodes += MLP(cat(agg, mesh)), grid nodes +=
MLP(grid)), `processor_encoder` (1 layer), `processor` (processor_layers - 2), `processor_decoder` (1), the decoder (m2g edge MLP,
grid nodes += MLP(cat(agg, grid))) and `finale`.  DGL is a container in the reference; on the fixed graphs every sub-network is a row
MLP whose operand rows are assembled through an index, and `cat(e, v_src[src], v_dst[dst])` / `cat(agg, v)` are never written.  The
embeddings of the static inputs -- mesh node features and the three edge feature sets -- depend on the parameters only: they run
once per `forward`, not once per lead time.

Differences from the reference, all on purpose:
* the rollout is the working on-device form shared by the dlwpbench models (rollout.py); the reference's loop calls `.to()` on a
  Python list at the second lead time and moves every prediction to the host;
* B > 1 is B independent samples on the same graphs (the reference refuses it);
* the input channel order of a step is the reference's `prescribed | prognostic | constants`, which is not the other dlwpbench
  models' (`constants | prescribed | prognostic`);
* `activation_fn` "relu" is ReLU in every MLP.
"""
import torch
import torch.nn as nn

from .. import gc_mesh
from .. import lib as L
from ..graph_ops import AGGREGATIONS, BipartiteGraph, wide_edge_block, wide_graph_mlp, wide_node_block
from ..nsbench.graphcast import _activation
from ..nsbench.meshgraphnet import MeshGraphMLP
from .rollout import rollout


class WideMLP(MeshGraphMLP):
    """MeshGraphMLP's modules and keys (`model.0`, `model.2`, ..., LayerNorm last) on the wide kernels"""

    def forward(self, x, residual=False):
        return wide_graph_mlp(x, self.params(), self.norm(), act=self.act, residual=residual)

    def edges(self, e, v_src, v_dst, graph, residual):
        return wide_edge_block(e, v_src, v_dst, graph, self.params(), self.norm(), residual=residual, act=self.act)

    def nodes(self, e, v_dst, graph, aggregation):
        return wide_node_block(e, v_dst, graph, self.params(), self.norm(), aggregation=aggregation, residual=True, act=self.act)


class _EncoderEmbedder(nn.Module):
    def __init__(self, grid_dim, mesh_dim, edge_dim, dim, layers, act):
        super().__init__()
        self.grid_node_mlp = WideMLP(grid_dim, dim, dim, layers, act=act)
        self.mesh_node_mlp = WideMLP(mesh_dim, dim, dim, layers, act=act)
        self.mesh_edge_mlp = WideMLP(edge_dim, dim, dim, layers, act=act)
        self.grid2mesh_edge_mlp = WideMLP(edge_dim, dim, dim, layers, act=act)


class _DecoderEmbedder(nn.Module):
    def __init__(self, edge_dim, dim, layers, act):
        super().__init__()
        self.mesh2grid_edge_mlp = WideMLP(edge_dim, dim, dim, layers, act=act)


class _Encoder(nn.Module):
    def __init__(self, dim, layers, act):
        super().__init__()
        self.edge_mlp = WideMLP(3 * dim, dim, dim, layers, act=act)
        self.src_node_mlp = WideMLP(dim, dim, dim, layers, act=act)
        self.dst_node_mlp = WideMLP(2 * dim, dim, dim, layers, act=act)


class _Decoder(nn.Module):
    def __init__(self, dim, layers, act):
        super().__init__()
        self.edge_mlp = WideMLP(3 * dim, dim, dim, layers, act=act)
        self.node_mlp = WideMLP(2 * dim, dim, dim, layers, act=act)


class _EdgeBlock(nn.Module):
    def __init__(self, dim, layers, act):
        super().__init__()
        self.edge_mlp = WideMLP(3 * dim, dim, dim, layers, act=act)


class _NodeBlock(nn.Module):
    def __init__(self, dim, layers, act):
        super().__init__()
        self.node_mlp = WideMLP(2 * dim, dim, dim, layers, act=act)


class _Processor(nn.Module):
    """`processor_layers` = edge block, node block, edge block, ... (the reference's interleaved ModuleList)"""

    def __init__(self, n, dim, layers, act, aggregation):
        super().__init__()
        self.aggregation = aggregation
        self.processor_layers = nn.ModuleList([m for _ in range(n) for m in (_EdgeBlock(dim, layers, act), _NodeBlock(dim, layers, act))])

    def forward(self, e, v, graph):
        for m in self.processor_layers:
            if isinstance(m, _EdgeBlock):
                e = m.edge_mlp.edges(e, v, v, graph, True)
            else:
                v = m.node_mlp.nodes(e, v, graph, self.aggregation)
        return e, v


class GraphCastNet(nn.Module):
    """`forward(constants [B, 1, Cc, H, W] | None, prescribed [B, T, Cp, H, W] | None, prognostic [B, T, Cg, H, W])` ->
    `[B, T - context_size, Cg, H, W]`: each frame is the newest prognostic frame plus one network call on
    `cat(prescribed window, prognostic window, constants)`.

    `meshgraph_path`: an icosphere file in the reference's JSON schema; gc_mesh.write_icospheres(path, level) writes one (the
    reference ships none).  Refused with NotImplementedError, naming the keyword: `use_cugraphops_encoder / _processor /
    _decoder`, `do_concat_trick`, `partition_size > 1`, a `norm_type` other than "LayerNorm", activations other than silu / relu,
    `hidden_dim > 512`, `hidden_layers > 3`.  ValueError: `processor_layers <= 2` (as the reference), an unknown `aggregation`,
    `input_dim_mesh_nodes != 3`, `input_dim_edges != 4` (the graphs carry these features), an input that does not fit the grid.
    `recompute_activation` is accepted with either value: a memory choice with the same arithmetic.  Extra keywords (`type`,
    `name`, `static_dataset_path`, `partition_group_name`, ...) are ignored; `device` moves parameters and graphs."""

    def __init__(self, meshgraph_path, input_height=721, input_width=1440, constant_channels=4, prescribed_channels=1,
                 prognostic_channels=8, input_dim_mesh_nodes=3, input_dim_edges=4, processor_layers=16, hidden_layers=1, hidden_dim=512,
                 aggregation="sum", activation_fn="silu", norm_type="LayerNorm", use_cugraphops_encoder=False,
                 use_cugraphops_processor=False, use_cugraphops_decoder=False, do_concat_trick=False, recompute_activation=False,
                 partition_size=1, partition_group_name=None, expect_partitioned_input=False, produce_aggregated_output=True,
                 context_size=1, device=None, **kwargs):
        super().__init__()
        for name, value in (("use_cugraphops_encoder", use_cugraphops_encoder), ("use_cugraphops_processor", use_cugraphops_processor),
                            ("use_cugraphops_decoder", use_cugraphops_decoder)):
            if value:
                raise NotImplementedError(f"{name}=True (cugraph-ops kernels) is not built: the graph kernels are the library's own")
        if do_concat_trick:
            raise NotImplementedError("do_concat_trick=True splits the first edge Linear into three parameters (lin_efeat, lin_src, "
                                      "lin_dst): other state_dict keys, not built")
        if int(partition_size or 1) > 1:
            raise NotImplementedError("partition_size > 1 (a graph distributed over several devices) is not built")
        if norm_type != "LayerNorm":
            raise NotImplementedError(f"norm_type = {norm_type!r}: the graph kernels have LayerNorm")
        act = _activation(activation_fn)
        if int(hidden_dim) > L.GRAPH_WIDE_MAX_WIDTH:
            raise NotImplementedError(f"hidden_dim = {hidden_dim}: the wide graph kernels take widths up to {L.GRAPH_WIDE_MAX_WIDTH}")
        if int(hidden_layers) > L.GRAPH_MAX_HIDDEN_LAYERS:
            raise NotImplementedError(f"hidden_layers = {hidden_layers}: the graph kernels take up to {L.GRAPH_MAX_HIDDEN_LAYERS} "
                                      "hidden layers")
        if int(hidden_dim) < 1 or int(hidden_layers) < 1:
            raise ValueError("hidden_dim and hidden_layers must be at least 1")
        if int(processor_layers) <= 2:
            raise ValueError("Expected at least 3 processor layers")
        if aggregation not in AGGREGATIONS:
            raise ValueError(f"aggregation must be 'sum' or 'mean', not {aggregation!r}")
        if int(input_dim_mesh_nodes) != 3 or int(input_dim_edges) != 4:
            raise ValueError(f"input_dim_mesh_nodes = {input_dim_mesh_nodes}, input_dim_edges = {input_dim_edges}: the mesh nodes carry 3 "
                             "features and the edges 4")
        if int(context_size) < 1:
            raise ValueError("context_size must be >= 1: the first frame needs an initial condition")
        self.context_size = int(context_size)
        self.constant_channels, self.prognostic_channels = int(constant_channels), int(prognostic_channels)
        self.input_dim_grid_nodes = self.constant_channels + (int(prescribed_channels) + self.prognostic_channels) * self.context_size
        if not 1 <= self.input_dim_grid_nodes <= L.GRAPH_WIDE_MAX_WIDTH or self.prognostic_channels < 1:
            raise NotImplementedError(f"{self.input_dim_grid_nodes} input channels per grid node: the wide graph kernels take 1.."
                                      f"{L.GRAPH_WIDE_MAX_WIDTH}")
        self.output_dim_grid_nodes = self.prognostic_channels
        self.height, self.width = int(input_height), int(input_width)
        self.aggregation = aggregation
        self.expect_partitioned_input, self.produce_aggregated_output = expect_partitioned_input, produce_aggregated_output
        try:
            ico, max_order = gc_mesh.load_icospheres(meshgraph_path)
        except FileNotFoundError:
            raise FileNotFoundError(f"{meshgraph_path}: no icosphere file (gc_mesh.write_icospheres(path, level) writes one)") from None
        g = gc_mesh.build_graphs(ico, max_order, self.height, self.width)
        self.graphs = {k: BipartiteGraph(g[k].src, g[k].dst, g[k].num_src, g[k].num_dst) for k in ("g2m", "mesh", "m2g")}
        # the static inputs: moved with the module, not part of a checkpoint
        self.register_buffer("mesh_ndata", torch.from_numpy(g["mesh_node_features"]), persistent=False)
        for k in ("g2m", "mesh", "m2g"):
            self.register_buffer(f"{k}_edata", torch.from_numpy(g[k].edge_features), persistent=False)
        dim, nl = int(hidden_dim), int(hidden_layers)
        self.encoder_embedder = _EncoderEmbedder(self.input_dim_grid_nodes, 3, 4, dim, nl, act)
        self.decoder_embedder = _DecoderEmbedder(4, dim, nl, act)
        self.encoder = _Encoder(dim, nl, act)
        self.processor_encoder = _Processor(1, dim, nl, act, aggregation)
        self.processor = _Processor(int(processor_layers) - 2, dim, nl, act, aggregation)
        self.processor_decoder = _Processor(1, dim, nl, act, aggregation)
        self.decoder = _Decoder(dim, nl, act)
        self.finale = WideMLP(dim, self.output_dim_grid_nodes, dim, nl, norm=False, act=act)
        if device is not None:
            self.to(device)

    def to(self, *args, **kwargs):
        super().to(*args, **kwargs)
        device = torch._C._nn._parse_to(*args, **kwargs)[0]
        if device is not None:
            for g in self.graphs.values():
                g.to(device)
        return self

    def embed_static(self, B):
        """the embedded mesh node features and g2m / mesh / m2g edge features, each repeated for B samples"""
        emb = self.encoder_embedder
        rows = (emb.mesh_node_mlp(self.mesh_ndata), emb.grid2mesh_edge_mlp(self.g2m_edata), emb.mesh_edge_mlp(self.mesh_edata),
                self.decoder_embedder.mesh2grid_edge_mlp(self.m2g_edata))
        return rows if B == 1 else tuple(r.repeat(B, 1) for r in rows)

    def network(self, x_t, static):
        """one network call on channels-first `[B, C, H, W]` in the order constants | prescribed | prognostic (rollout.py's): the
        constants move behind the rest (the reference's order) in the copy that makes the rows "(b h w) c"."""
        B, C, H, W = x_t.shape
        cc = self.constant_channels
        if cc:
            x_t = torch.cat([x_t[:, cc:], x_t[:, :cc]], dim=1)
        mesh_n, g2m_e, mesh_e, m2g_e = static
        g2m, mesh, m2g = self.graphs["g2m"], self.graphs["mesh"], self.graphs["m2g"]
        grid = self.encoder_embedder.grid_node_mlp(x_t.permute(0, 2, 3, 1).reshape(B * H * W, C))
        e = self.encoder.edge_mlp.edges(g2m_e, grid, mesh_n, g2m, False)
        mesh_n = self.encoder.dst_node_mlp.nodes(e, mesh_n, g2m, self.aggregation)
        grid = self.encoder.src_node_mlp(grid, residual=True)
        mesh_e, mesh_n = self.processor_encoder(mesh_e, mesh_n, mesh)
        mesh_e, mesh_n = self.processor(mesh_e, mesh_n, mesh)
        _, mesh_n = self.processor_decoder(mesh_e, mesh_n, mesh)
        e = self.decoder.edge_mlp.edges(m2g_e, mesh_n, grid, m2g, False)
        grid = self.decoder.node_mlp.nodes(e, grid, m2g, self.aggregation)
        return self.finale(grid).view(B, H, W, -1).permute(0, 3, 1, 2)

    def forward(self, constants=None, prescribed=None, prognostic=None):
        if prognostic.shape[1] <= self.context_size:
            raise ValueError(f"prognostic has {prognostic.shape[1]} frames: more than context_size = {self.context_size} are needed")
        if tuple(prognostic.shape[-2:]) != (self.height, self.width):
            raise ValueError(f"the graphs were built for a {self.height} x {self.width} grid, the input is "
                             f"{prognostic.shape[-2]} x {prognostic.shape[-1]}")
        channels = (0 if constants is None else constants.shape[2]) + self.context_size * (
            (0 if prescribed is None else prescribed.shape[2]) + prognostic.shape[2])
        if channels != self.input_dim_grid_nodes or (constants is None) != (self.constant_channels == 0):
            raise ValueError(f"the inputs make {channels} channels per grid node, the model was built for {self.input_dim_grid_nodes} "
                             f"({self.constant_channels} of them constants)")
        static = self.embed_static(prognostic.shape[0])
        return rollout(lambda x_t: self.network(x_t, static), self.context_size, constants, prescribed, prognostic)
