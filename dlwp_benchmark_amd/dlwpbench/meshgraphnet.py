"""MeshGraphNet baseline of the weather benchmark (src/dlwpbench/models/mgn/meshgraphnet.py) on the graph kernels: the reference's
constructor keywords, `forward(constants, prescribed, prognostic)` and `state_dict` keys.  The network is the nsbench one
(../nsbench/meshgraphnet.py); what differs is the input of a step (constants | prescribed window | prognostic window), the
per-axis default of `periodic`, and the Delaunay mesh, which here triangulates H x (W + 1) points and closes the longitude only.

The rollout is the clean on-device form shared by the dlwpbench models (rollout.py): the reference's own loop calls `.to()` on a
Python list at the second lead time and raises, so only T = context_size + 1 can be compared with it.
"""
from ..nsbench.meshgraphnet import MeshGraphNetBase
from .rollout import rollout


class MeshGraphNet(MeshGraphNetBase):
    """The input of a step is `cat(constants, prescribed window, prognostic window)`, both windows `context_size` frames long
    and flattened over (time, channel); the output is a residual to the newest prognostic frame.  Returns the frames from
    `context_size` on: `[B, T - context_size, C, H, W]`.  Keywords, refusals and `graph=` as in nsbench.MeshGraphNet."""

    def __init__(self, constant_channels=4, prescribed_channels=0, prognostic_channels=1, input_dim_edges=2, context_size=5,
                 processor_size=15, message_passing_steps=1, num_layers_node_processor=2, num_layers_edge_processor=2,
                 hidden_dim_processor=128, hidden_dim_node_encoder=128, num_layers_node_encoder=2, hidden_dim_edge_encoder=128,
                 num_layers_edge_encoder=2, hidden_dim_node_decoder=128, num_layers_node_decoder=2, aggregation="sum",
                 do_concat_trick=False, num_processor_checkpoint_segments=0, graph_type="grid_2d", graph=None, device=None, **kwargs):
        super().__init__()
        if int(context_size) < 1:
            raise ValueError("context_size must be >= 1: the first frame needs an initial condition")
        self.context_size, self.prognostic_channels = int(context_size), int(prognostic_channels)
        input_dim_nodes = int(constant_channels) + (int(prescribed_channels) + int(prognostic_channels)) * self.context_size
        self._build(input_dim_nodes, input_dim_edges, prognostic_channels, processor_size, message_passing_steps,
                    num_layers_node_processor, num_layers_edge_processor, hidden_dim_processor, hidden_dim_node_encoder,
                    num_layers_node_encoder, hidden_dim_edge_encoder, num_layers_edge_encoder, hidden_dim_node_decoder,
                    num_layers_node_decoder, aggregation, do_concat_trick, num_processor_checkpoint_segments, graph_type, graph,
                    True, device)

    def forward(self, constants=None, prescribed=None, prognostic=None):
        """constants [B, 1, C, H, W] | None, prescribed [B, T, C, H, W] | None, prognostic [B, T, C, H, W]"""
        if prognostic.shape[1] <= self.context_size:
            raise ValueError(f"prognostic has {prognostic.shape[1]} frames: more than context_size = {self.context_size} are needed")
        self._check_grid(prognostic.shape[-2], prognostic.shape[-1])
        e0 = self.encode_edges(prognostic.shape[0], prognostic.device)
        return rollout(lambda x_t: self.network(x_t, e0), self.context_size, constants, prescribed, prognostic)
