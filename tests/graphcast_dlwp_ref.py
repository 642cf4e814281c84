"""Plain-torch restatement of the dlwpbench GraphCastNet (src/dlwpbench/models/graphcast/graph_cast_net.py) in any dtype, on the
index arrays of gc_mesh: every MLP from elementary operations, the concatenations written out, the rollout as dlwpbench/rollout.py
defines it.  It takes a state_dict with the reference's keys, so it runs a reference checkpoint, the golden parameters and the
parameters of the model under test alike.  CASES are the golden cases of tests/golden/make_graphcast_dlwp_golden.py."""
import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = "graphcast_dlwp_golden.npz"

# name -> (icosphere level, constructor keywords without meshgraph_path, frames T): B = 1 and T = context_size + 1, all the
# reference's own loop can run.  The grids have an even height and an odd width: a latitude 0 or longitude 0 lies exactly on a mirror
# plane of the icosahedron, where two face centroids (mesh vertices) are equally near and sklearn's choice between them is not
# ours.  Level 2 on 10 x 15, not 8 x 15: there the last mesh vertex has no grid-to-mesh edge, and DGL (like the fixture's stub)
# sizes a node type by the largest id in an edge, so the reference cannot run
CASES = {
    "l1_sum": (1, dict(input_height=8, input_width=15, constant_channels=4, prescribed_channels=0, prognostic_channels=2,
                       processor_layers=3, hidden_layers=1, hidden_dim=16, aggregation="sum", context_size=1), 2),
    "l2_mean_ctx2": (2, dict(input_height=10, input_width=15, constant_channels=2, prescribed_channels=1, prognostic_channels=3,
                             processor_layers=3, hidden_layers=2, hidden_dim=16, aggregation="mean", context_size=2), 3),
}


def rel_gap(a, b):
    """max |a - b| relative to the max norm of b (float64)"""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def make_inputs(cfg, T, gen, B=1):
    H, W = cfg["input_height"], cfg["input_width"]
    rn = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    inp = {"prognostic": rn(B, T, cfg["prognostic_channels"], H, W)}
    if cfg["constant_channels"]:
        inp["constants"] = rn(B, 1, cfg["constant_channels"], H, W)
    if cfg["prescribed_channels"]:
        inp["prescribed"] = rn(B, T, cfg["prescribed_channels"], H, W)
    target = rn(B, T - cfg["context_size"], cfg["prognostic_channels"], H, W)
    return inp, target


class RefGraphCast:
    """graphs: gc_mesh.build_graphs' dict; sd: state_dict (any dtype; used as given, so leaves with requires_grad get gradients)"""

    def __init__(self, graphs, sd, cfg, act="silu"):
        self.g, self.sd, self.cfg, self.act = graphs, sd, cfg, act
        self.dtype = next(iter(sd.values())).dtype
        dev = next(iter(sd.values())).device
        t = lambda a: torch.from_numpy(np.asarray(a)).to(dev)      # noqa: E731
        self.idx = {k: (t(graphs[k].src.astype(np.int64)), t(graphs[k].dst.astype(np.int64))) for k in ("g2m", "mesh", "m2g")}
        self.feat = {k: t(graphs[k].edge_features).to(self.dtype) for k in ("g2m", "mesh", "m2g")}
        self.mesh_ndata = t(graphs["mesh_node_features"]).to(self.dtype)

    def mlp(self, prefix, x):
        keys = sorted({int(k[len(prefix) + 7:].split(".")[0]) for k in self.sd if k.startswith(prefix + ".model.")})
        lin = [i for i in keys if self.sd[f"{prefix}.model.{i}.weight"].dim() == 2]
        for j, i in enumerate(lin):
            x = F.linear(x, self.sd[f"{prefix}.model.{i}.weight"], self.sd[f"{prefix}.model.{i}.bias"])
            if j + 1 < len(lin):
                x = x * torch.sigmoid(x) if self.act == "silu" else torch.clamp(x, min=0)
        if len(keys) > len(lin):
            i = keys[-1]
            c = x - x.mean(dim=1, keepdim=True)
            x = c / torch.sqrt((c * c).mean(dim=1, keepdim=True) + 1e-5) * self.sd[f"{prefix}.model.{i}.weight"] + \
                self.sd[f"{prefix}.model.{i}.bias"]
        return x

    def agg(self, e, dst, n, B, E):
        idx = torch.cat([dst + b * n for b in range(B)])
        out = torch.zeros(B * n, e.shape[1], dtype=e.dtype, device=e.device).index_add(0, idx, e)
        if self.cfg["aggregation"] == "mean":
            out = out / torch.bincount(idx, minlength=B * n).clamp(min=1).to(e.dtype)[:, None]
        return out

    def edge(self, prefix, e, vs, vd, name, B):
        src, dst = self.idx[name]
        ns, nd = self.g[name].num_src, self.g[name].num_dst
        si, di = torch.cat([src + b * ns for b in range(B)]), torch.cat([dst + b * nd for b in range(B)])
        return self.mlp(prefix, torch.cat([e, vs[si], vd[di]], dim=1))

    def node(self, prefix, e, vd, name, B):
        _, dst = self.idx[name]
        return vd + self.mlp(prefix, torch.cat([self.agg(e, dst, self.g[name].num_dst, B, len(dst)), vd], dim=1))

    def network(self, x_t, static):
        B, C, H, W = x_t.shape
        mesh_n, g2m_e, mesh_e, m2g_e = (s.repeat(B, 1) for s in static)
        grid = self.mlp("encoder_embedder.grid_node_mlp", x_t.permute(0, 2, 3, 1).reshape(B * H * W, C))
        e = self.edge("encoder.edge_mlp", g2m_e, grid, mesh_n, "g2m", B)
        mesh_n = self.node("encoder.dst_node_mlp", e, mesh_n, "g2m", B)
        grid = grid + self.mlp("encoder.src_node_mlp", grid)
        blocks = [("processor_encoder", 1), ("processor", self.cfg["processor_layers"] - 2), ("processor_decoder", 1)]
        for name, n in blocks:
            for i in range(n):
                mesh_e = mesh_e + self.edge(f"{name}.processor_layers.{2 * i}.edge_mlp", mesh_e, mesh_n, mesh_n, "mesh", B)
                mesh_n = self.node(f"{name}.processor_layers.{2 * i + 1}.node_mlp", mesh_e, mesh_n, "mesh", B)
        e = self.edge("decoder.edge_mlp", m2g_e, mesh_n, grid, "m2g", B)
        grid = self.node("decoder.node_mlp", e, grid, "m2g", B)
        return self.mlp("finale", grid).view(B, H, W, -1).permute(0, 3, 1, 2)

    def __call__(self, constants=None, prescribed=None, prognostic=None):
        ctx, T = self.cfg["context_size"], prognostic.shape[1]
        static = (self.mlp("encoder_embedder.mesh_node_mlp", self.mesh_ndata),
                  self.mlp("encoder_embedder.grid2mesh_edge_mlp", self.feat["g2m"]),
                  self.mlp("encoder_embedder.mesh_edge_mlp", self.feat["mesh"]),
                  self.mlp("decoder_embedder.mesh2grid_edge_mlp", self.feat["m2g"]))
        frames, outs = [prognostic[:, i] for i in range(ctx)], []
        for t in range(ctx, T):
            parts = []
            if prescribed is not None:
                parts.append(prescribed[:, t - ctx:t].flatten(1, 2))
            parts.append(torch.stack(frames[-ctx:], dim=1).flatten(1, 2))
            if constants is not None:
                parts.append(constants[:, 0])
            out = frames[-1] + self.network(torch.cat(parts, dim=1), static)
            frames.append(out)
            outs.append(out)
        return torch.stack(outs, dim=1)


def run_ref(graphs, sd, cfg, inputs, target, dtype, device="cpu"):
    """-> (y, loss, {name: gradient}) of the restatement in `dtype`"""
    sd = {k: v.detach().to(device=device, dtype=dtype).requires_grad_(True) for k, v in sd.items()}
    net = RefGraphCast(graphs, sd, cfg)
    inp = {k: v.to(device=device, dtype=dtype) for k, v in inputs.items()}
    y = net(inp.get("constants"), inp.get("prescribed"), inp["prognostic"])
    loss = F.mse_loss(y, target.to(device=device, dtype=dtype))
    loss.backward()
    return y.detach(), loss.detach(), {k: v.grad for k, v in sd.items()}
