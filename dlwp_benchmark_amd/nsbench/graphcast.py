"""GraphCast baseline of the Navier-Stokes benchmark (src/nsbench/models/graphcast/graph_cast_net_ns.py, GraphCastNetNS) on the
graph kernels (graph_ops): constructor keywords, `forward` signature and `state_dict` keys are the reference's, so its
checkpoints load with `load_state_dict(strict=True)`.

The model is MeshGraphNet's three blocks (nsbench/meshgraphnet.py, with SiLU in place of ReLU) on another mesh: the periodic grid
plus n-hop shortcut edges with [dir_y, dir_x, dist] features (mgn_graph.build_nhop_grid, numpy).  The sub-networks are registered
in the reference's order here -- node_encoder, edge_encoder, processor, node_decoder --, which is not MeshGraphNet's.  The edge
encoder's input is the same for every time step: it runs once per `forward`.

The dlwpbench GraphCastNet (icosphere mesh file, bipartite grid-to-mesh and mesh-to-grid graphs, hidden_dim 512) is another model on
another kernel family: dlwpbench/graphcast.py.
"""
import torch
import torch.nn as nn

from .. import mgn_graph
from ..graph_ops import Graph
from ..rollout_ops import ns_rollout
from .meshgraphnet import MeshGraphMLP, MeshGraphNetBase, MeshGraphNetProcessor, check_limits

# the names of the reference's ACT2FN (models/graphcast/utils/activations.py); the kernels have the first two
ACTIVATIONS = ("silu", "relu")
OTHER_ACTIVATIONS = ("leaky_relu", "prelu", "relu6", "elu", "selu", "gelu", "sigmoid", "logsigmoid", "softplus", "softshrink",
                     "softsign", "tanh", "tanhshrink", "threshold", "hardtanh", "identity", "stan", "squareplus")


def _activation(name):
    act = name.lower()
    if act in ACTIVATIONS:
        return act
    if act in OTHER_ACTIVATIONS:
        raise NotImplementedError(f"activation_fn = '{act}': the graph kernels have {list(ACTIVATIONS)}")
    raise KeyError(f"Activation function {act} not found. Available options are: {list(ACTIVATIONS + OTHER_ACTIVATIONS)}")


class GraphCastNetNS(MeshGraphNetBase):
    """`forward(x [B, T, D, H, W], teacher_forcing_steps)` -> `[B, T, D, H, W]` with (H, W) = (input_height, input_width) //
    downscale_factor, the grid the mesh is built for (`downscale_factor=None` is taken as 1; the reference raises a TypeError).
    The rollout is the one of the other nsbench models (rollout_ops.ns_rollout), so `output_dim` must equal `input_dim_nodes`; its
    residual is the whole newest frame, which is the reference's for one channel.  B > 1 is B independent samples on the same
    graph (the reference never batches its graph and fails there).

    `activation_fn`: "silu" or "relu" in any case; the reference's other names raise NotImplementedError, unknown ones KeyError.
    `norm_type` must be "LayerNorm".  `recompute_activation` is accepted with either value: a memory choice with the same
    arithmetic (the reference's True path needs nvfuser; here the activations are stored either way).  Refused as in MeshGraphNet:
    `do_concat_trick`, processor checkpointing, widths above 128, more than 3 hidden layers (NotImplementedError); also
    `partition_size > 1`.  The reference's `perm_idcs` are unused there and not reproduced.  Extra keywords (`type`, `name`,
    `partition_group_name`, ...) are ignored; `device` moves the parameters."""

    def __init__(self, input_height=32, input_width=32, downscale_factor=None, context_size=1, nhop_neighbors=(2,),
                 input_dim_nodes=1, input_dim_edges=3, output_dim=1, processor_layers=16, num_layers_node_processor=2,
                 num_layers_edge_processor=2, hidden_dim_processor=32, hidden_dim_node_encoder=32, num_layers_node_encoder=2,
                 hidden_dim_edge_encoder=32, num_layers_edge_encoder=2, hidden_dim_node_decoder=32, num_layers_node_decoder=2,
                 aggregation="sum", activation_fn="silu", norm_type="LayerNorm", do_concat_trick=False,
                 num_processor_checkpoint_segments=0, recompute_activation=False, expect_partitioned_input=False,
                 produce_aggregated_output=True, device=None, **kwargs):
        super().__init__()
        if int(context_size) < 1:
            raise ValueError("context_size must be >= 1")
        act = _activation(activation_fn)
        if norm_type != "LayerNorm":
            raise NotImplementedError(f"norm_type = {norm_type!r}: the graph kernels have LayerNorm")
        if int(kwargs.get("partition_size") or 1) > 1:
            raise NotImplementedError("partition_size > 1 (a graph distributed over several devices) is not built")
        if int(input_dim_edges) != 3:
            raise ValueError(f"input_dim_edges = {input_dim_edges}, but the edges of the n-hop grid carry 3 features")
        if int(output_dim) != int(input_dim_nodes):
            raise ValueError(f"output_dim = {output_dim} must equal input_dim_nodes = {input_dim_nodes}: the rollout feeds the output back")
        self.context_size, self.output_dim = int(context_size), int(output_dim)
        self.expect_partitioned_input, self.produce_aggregated_output = expect_partitioned_input, produce_aggregated_output
        in_nodes = int(input_dim_nodes) * self.context_size
        check_limits(dict(input_dim_nodes=in_nodes, output_dim=output_dim, hidden_dim_processor=hidden_dim_processor,
                          hidden_dim_node_encoder=hidden_dim_node_encoder, hidden_dim_edge_encoder=hidden_dim_edge_encoder,
                          hidden_dim_node_decoder=hidden_dim_node_decoder),
                     dict(num_layers_node_processor=num_layers_node_processor, num_layers_edge_processor=num_layers_edge_processor,
                          num_layers_node_encoder=num_layers_node_encoder, num_layers_edge_encoder=num_layers_edge_encoder,
                          num_layers_node_decoder=num_layers_node_decoder),
                     aggregation, do_concat_trick, num_processor_checkpoint_segments)
        if int(processor_layers) < 1:
            raise ValueError("processor_layers must be at least 1")
        scale = 1 if downscale_factor is None else int(downscale_factor)
        if scale < 1:
            raise ValueError(f"downscale_factor = {downscale_factor} must be positive")
        self.height, self.width = int(input_height) // scale, int(input_width) // scale
        self.nhop_neighbors = tuple(int(n) for n in nhop_neighbors)
        self.message_passing_steps = 1
        mesh = mgn_graph.build_nhop_grid(self.height, self.width, self.nhop_neighbors)
        self.graph = Graph.from_mesh(mesh)
        self._edge_features = torch.from_numpy(mesh.edge_features)
        self._batched = (None, None)
        self.node_encoder = MeshGraphMLP(in_nodes, hidden_dim_processor, hidden_dim_node_encoder, num_layers_node_encoder, act=act)
        self.edge_encoder = MeshGraphMLP(input_dim_edges, hidden_dim_processor, hidden_dim_edge_encoder, num_layers_edge_encoder, act=act)
        self.processor = MeshGraphNetProcessor(processor_layers, hidden_dim_processor, num_layers_node_processor,
                                               num_layers_edge_processor, aggregation, act=act)
        self.node_decoder = MeshGraphMLP(hidden_dim_processor, output_dim, hidden_dim_node_decoder, num_layers_node_decoder, norm=False,
                                         act=act)
        if device is not None:
            self.to(device)

    def forward(self, x, teacher_forcing_steps=10):
        self._check_grid(x.shape[-2], x.shape[-1])
        e0 = self.encode_edges(x.shape[0], x.device)
        return ns_rollout(lambda x_t: self.network(x_t, e0), x, teacher_forcing_steps, self.context_size)
