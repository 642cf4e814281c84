"""Plain-torch restatement of the nsbench GraphCast baseline (helper module for the tests, not a conftest): the network of
tests/mgn_ref.py with the hidden layers' activation chosen per case, on the n-hop grid mesh; CPU or GPU torch ops only,
dtype-generic, written from the model's description:

* an MLP is Linear, act, [Linear, act, ...] Linear, then (except in the decoder) LayerNorm over the output width; act is SiLU
  `x * sigmoid(x)` (the model's default) or ReLU;
* one network call: v = node_encoder(node rows "(b h w) d"), e = edge_encoder(edge features, repeated per sample); for every
  processor pair  e = e + edge_mlp(cat(e, v[src], v[dst])),  v = v + node_mlp(cat(agg, v))  with agg[i] the sum (or mean) of e
  over the edges whose dst is i; finally node_decoder(v);
* the mesh (src, dst, [dir_y, dir_x, dist]) comes from dlwp_benchmark_amd.mgn_graph.build_nhop_grid for the grid
  (input_height // downscale_factor, input_width // downscale_factor) unless the caller passes the fixture's own;
* the rollout is mgn_ref.ns_forward (the one of every nsbench model).

`params` is a state_dict-like mapping with the reference's keys; the layer structure is read from the keys.
"""
import torch
import torch.nn.functional as F

from mgn_ref import _indices, ns_forward, rel_gap  # noqa: F401  (rel_gap re-exported for the tests)

ACTS = {"silu": F.silu, "relu": F.relu}


def mlp(params, prefix, x, act):
    idx = _indices(params, prefix)
    linears = [i for i in idx if params[f"{prefix}{i}.weight"].dim() == 2]
    for n, i in enumerate(linears):
        x = F.linear(x, params[f"{prefix}{i}.weight"], params[f"{prefix}{i}.bias"])
        if n < len(linears) - 1:
            x = act(x)
    for i in idx:
        w = params[f"{prefix}{i}.weight"]
        if w.dim() == 1:
            x = F.layer_norm(x, (w.shape[0],), w, params[f"{prefix}{i}.bias"], 1e-5)
    return x


def network(params, x, mesh, aggregation, act):
    """x [B, C, H, W] -> [B, out, H, W]; mesh = (src, dst, edge_features) of one sample (long, long, float)"""
    B, C, H, W = x.shape
    N = H * W
    src, dst, feats = mesh
    off = (torch.arange(B, device=x.device) * N)[:, None]
    srcb, dstb = (src.to(x.device)[None] + off).reshape(-1), (dst.to(x.device)[None] + off).reshape(-1)
    v = mlp(params, "node_encoder.model.", x.permute(0, 2, 3, 1).reshape(B * N, C), act)
    e = mlp(params, "edge_encoder.model.", feats.to(x).repeat(B, 1), act)
    pairs = len({k.split(".")[2] for k in params if k.startswith("processor.processor_layers.")}) // 2
    deg = torch.zeros(B * N, dtype=x.dtype, device=x.device).index_add_(0, dstb, torch.ones(len(dstb), dtype=x.dtype, device=x.device))
    for i in range(pairs):
        cat = torch.cat([e, v.index_select(0, srcb), v.index_select(0, dstb)], dim=1)
        e = e + mlp(params, f"processor.processor_layers.{2 * i}.edge_mlp.model.", cat, act)
        agg = torch.zeros(B * N, e.shape[1], dtype=e.dtype, device=e.device).index_add_(0, dstb, e)
        if aggregation == "mean":
            agg = agg / deg.clamp(min=1)[:, None]
        v = v + mlp(params, f"processor.processor_layers.{2 * i + 1}.node_mlp.model.", torch.cat([agg, v], dim=1), act)
    return mlp(params, "node_decoder.model.", v, act).view(B, H, W, -1).permute(0, 3, 1, 2)


def grid_of(cfg):
    s = cfg.get("downscale_factor") or 1
    return cfg["input_height"] // s, cfg["input_width"] // s


def build_mesh(cfg):
    """(src, dst, edge_features) of a case through mgn_graph"""
    from dlwp_benchmark_amd import mgn_graph
    m = mgn_graph.build_nhop_grid(*grid_of(cfg), cfg["nhop_neighbors"])
    return torch.from_numpy(m.src).long(), torch.from_numpy(m.dst).long(), torch.from_numpy(m.edge_features)


def run_case(params, x, target, dtype, cfg, roll, mesh=None, device="cpu"):
    """forward + mse loss + backward in `dtype`; returns (output, loss, {name: gradient}) as tensors of that dtype"""
    p = {k: v.detach().clone().to(device=device, dtype=dtype).requires_grad_(True) for k, v in params.items()}
    mesh = mesh if mesh is not None else build_mesh(cfg)
    act = ACTS[cfg.get("activation_fn", "silu").lower()]
    net = lambda x_t: network(p, x_t, mesh, cfg.get("aggregation", "sum"), act)      # noqa: E731
    y = ns_forward(p, torch.as_tensor(x).to(device=device, dtype=dtype), roll["teacher_forcing_steps"], cfg["context_size"], net)
    loss = F.mse_loss(y, torch.as_tensor(target).to(device=device, dtype=dtype))
    loss.backward()
    return y.detach(), loss.detach(), {k: v.grad for k, v in p.items()}


def _cfg(H, W, nhop, ctx, layers, proc, enc_n=None, enc_e=None, dec=None, **kw):
    cfg = dict(input_height=H, input_width=W, downscale_factor=1, context_size=ctx, nhop_neighbors=list(nhop), input_dim_nodes=1,
               input_dim_edges=3, output_dim=1, processor_layers=layers, hidden_dim_processor=proc,
               hidden_dim_node_encoder=enc_n or proc, hidden_dim_edge_encoder=enc_e or proc, hidden_dim_node_decoder=dec or proc)
    cfg.update(kw)
    return cfg


# the golden cases: name -> (constructor keywords, (B, T), rollout keywords of forward).  B = 1: the reference cannot do more
CASES = {
    "gc_6x6_hop2_c2_w8": (_cfg(6, 6, [2], 2, 2, 8), (1, 4), dict(teacher_forcing_steps=2)),
    "gc_8x8_hop24_c1_w34": (_cfg(8, 8, [2, 4], 1, 2, 34, 12, 7, 20), (1, 3), dict(teacher_forcing_steps=1)),
    "gc_4x4_hop2_mean_w5": (_cfg(4, 4, [2], 1, 1, 5, aggregation="mean", num_layers_node_processor=1, num_layers_edge_processor=3),
                            (1, 2), dict(teacher_forcing_steps=1)),
    # one hidden layer per processor MLP, and a fixture file of its own: at width 116 the parameters and gradients of this case
    # alone are 0.75 MiB (with two hidden layers 1 MiB), and no committed file may pass 1 MiB
    "gc_16x16_down2_c2_w116": (_cfg(16, 16, [2], 2, 1, 116, 16, 16, 16, downscale_factor=2, num_layers_node_processor=1,
                                    num_layers_edge_processor=1), (1, 3), dict(teacher_forcing_steps=2)),
    "gc_6x6_hop2_c2_w8_relu": (_cfg(6, 6, [2], 2, 2, 8, activation_fn="relu"), (1, 4), dict(teacher_forcing_steps=2)),
}
GOLDEN = "graphcast_ns_golden.npz"
GOLDEN_OF = {name: "graphcast_ns_w116_golden.npz" if name.endswith("_w116") else GOLDEN for name in CASES}      # case -> its file


def make_inputs(cfg, shape, gen):
    """fresh random input and target of a case (the fixtures store their own)"""
    B, T = shape
    H, W = grid_of(cfg)
    D = cfg["input_dim_nodes"]
    return torch.randn(B, T, D, H, W, generator=gen), torch.randn(B, T, D, H, W, generator=gen)


def load_case(npz, name):
    """(params, x, target, y, loss, grads, gaps, mesh) of a golden case, as torch tensors; mesh = the REFERENCE's
    (src, dst, edge_features), in its edge order"""
    pre = name + "/"
    params = {k[len(pre) + 2:]: torch.from_numpy(npz[k]) for k in npz.files if k.startswith(pre + "p_")}
    grads = {k[len(pre) + 2:]: torch.from_numpy(npz[k]) for k in npz.files if k.startswith(pre + "g_")}
    gaps = {k[len(pre) + 4:]: float(npz[k]) for k in npz.files if k.startswith(pre + "gap_")}
    mesh = (torch.from_numpy(npz[pre + "src"]).long(), torch.from_numpy(npz[pre + "dst"]).long(),
            torch.from_numpy(npz[pre + "edge_features"]))
    return (params, torch.from_numpy(npz[pre + "in_x"]), torch.from_numpy(npz[pre + "target"]), torch.from_numpy(npz[pre + "y"]),
            float(npz[pre + "loss"]), grads, gaps, mesh)
