"""Seeded ensemble forecasts and their probabilistic scores on libdlwpmi (csrc/ensemble.hip; the reference has none: the float64
restatement tests/ens_ref.py defines them).

`perturb_members` turns one initial state per sample into M members (dlwp_ens_perturb: the counter-based noise stream of the batch
kernels with the member in the counter, so a member depends on (seed, item, member, element) only).  `ensemble_diagnostics` reads a
chunk of NORMALISED member forecasts and targets once (dlwp_ens_diag) and leaves two small tables per (sample, lead time,
variable): four weighted pixel sums -- squared error of the ensemble mean, ensemble variance, mean absolute error of the members,
mean absolute difference of member pairs -- and the rank counts.  `ensemble_metrics` finishes on the host in float64: RMSE of the
mean, spread, spread-skill ratio, CRPS (fair and ensemble estimator) and the rank histogram.  `evaluate.evaluate_dlwp` /
`evaluate_ns` drive them with `ensemble=M`.

`crps_loss` / `crps_loss_and_grad` / `CrpsLoss` are the CRPS of the members as a training loss (dlwp_crps_loss_fwd_bwd: value and
gradient from one read of the members; the restatement tests/crps_ref.py defines them); `train_engine.GraphedTrainStep(loss=)` and
`train_loop.train_dlwp(loss="crps")` train on it.
"""
import functools

import numpy as np
import torch

from . import lib as L

MAX_MEMBERS = 64


def _check_seed(sigma_max, seed):
    """as device_data._check_noise: a perturbation needs a seed, the seed fits 64 unsigned bits"""
    if sigma_max > 0.0 and seed is None:
        raise ValueError("sigma > 0 needs a seed: the device noise stream is keyed by it")
    seed = 0 if seed is None else int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed {seed} must fit 64 unsigned bits")
    return seed


@functools.lru_cache(maxsize=16)
def _device_floats(values, device):
    """a small fp32 table (sigmas, weights) on the device, uploaded once per distinct content: a training step repeats its call"""
    return torch.tensor(values, dtype=torch.float64).float().to(device)


def _layout(x, variables):
    """(V, P): the variable count and the plane size of x [B, ..., V, H, W] or [B, ..., V, 12, n, n]"""
    s = tuple(x.shape)
    if variables is None:
        hpx = len(s) >= 5 and s[-3] == 12 and s[-1] == s[-2]
        k = 4 if hpx else 3
        if len(s) < k + 1:
            raise ValueError(f"x must be [B, ..., V, H, W] or [B, ..., V, 12, n, n], not {s}")
        return int(s[-k]), int(np.prod(s[-k + 1:]))
    V = int(variables)
    for k in (3, 4):
        if len(s) >= k + 1 and s[-k] == V:
            return V, int(np.prod(s[-k + 1:]))
    raise ValueError(f"x {s} has no axis of {V} variables in front of its [H, W] or [12, n, n] planes")


def perturb_members(x, items, members, sigma, seed, control=True, variables=None, validate_items=True):
    """x [B, ..., V, H, W] or [B, ..., V, 12, n, n] (one sample's input frames per row, NORMALISED, on the GPU) -> [B, M, ...]:
    member m of sample b is x[b] + sigma_v z with z the standard normals of (seed, items[b], m, element).

    items     B non-negative integers: the identity of each sample in the noise stream (the dataset index, not the batch position).
    members   M in 1..64.
    sigma     a scalar or one value per variable, finite and not negative, in normalised units.
    seed      0 <= seed < 2^64; needed when any sigma > 0.
    control   True: member 0 is a bit-exact copy of x and draws nothing.
    variables the size of the variable axis when the trailing axes are ambiguous (default: [..., V, 12, n, n] when they fit, else
              [..., V, H, W]).
    validate_items  False: `items` is an int32 [B] tensor on x's device whose values the caller vouches for (a row of
              `DeviceWeatherBench.epoch_table`); the kernel reads it in place -- no copy to the host, no synchronisation."""
    M = int(members)
    if not 1 <= M <= MAX_MEMBERS:
        raise ValueError(f"members = {M} must lie in 1..{MAX_MEMBERS}")
    if x.dim() < 4:
        raise ValueError(f"x must be [B, ..., V, H, W] or [B, ..., V, 12, n, n], not {tuple(x.shape)}")
    B = x.shape[0]
    V, P = _layout(x, variables)
    if validate_items:
        it = np.asarray(items.cpu() if torch.is_tensor(items) else items)
        if it.shape != (B,) or not np.issubdtype(it.dtype, np.integer):
            raise ValueError(f"items must be {B} integers, not {it.dtype} {it.shape}")
        if B and (it.min() < 0 or it.max() >= 2 ** 31):
            raise ValueError(f"items must lie in 0..2^31 - 1, found {int(it.min())}..{int(it.max())}")
    elif not (torch.is_tensor(items) and items.dtype == torch.int32 and tuple(items.shape) == (B,) and items.device == x.device):
        raise ValueError(f"validate_items=False takes an int32 [{B}] tensor on {x.device}")
    sg = np.asarray(sigma, dtype=np.float64).reshape(-1)
    if sg.size == 1:
        sg = np.repeat(sg, V)
    if sg.size != V:
        raise ValueError(f"sigma must be a scalar or have one entry per variable ({V}), not {sg.size}")
    if not (np.isfinite(sg).all() and (sg >= 0).all()):
        raise ValueError(f"sigma {sg.tolist()} must be finite and not negative")
    seed = _check_seed(float(sg.max()), seed)
    if not x.is_cuda:
        raise L.DlwpError("libdlwpmi needs CUDA/HIP tensors (no CPU fallback)")
    if x.dtype != torch.float32:
        raise L.DlwpError(f"perturb_members takes float32 tensors, not {x.dtype}")
    xc = x.contiguous()
    F = xc.numel() // B
    out = torch.empty((B, M) + tuple(x.shape[1:]), device=x.device)
    dit = torch.from_numpy(np.ascontiguousarray(it.astype(np.int32))).to(x.device) if validate_items else items.contiguous()
    dsg = _device_floats(tuple(sg.tolist()), x.device)
    L.check(L.load().dlwp_ens_perturb(L.ptr(xc), L.ptr(dit), L.ptr(dsg), B, F, P, V, M, int(bool(control)), seed, L.ptr(out), L.stream()))
    return out


def ensemble_diagnostics(members, targets, *, lats_deg=None, remap=None, state=None, t_begin=0, T=None):
    """One chunk of an ensemble rollout through dlwp_ens_diag.

    members   [Bc, M, Tc, V, H, W] (with `remap`: [Bc, M, Tc, V, 12, n, n]) NORMALISED member forecasts on the GPU; batch, member and
              time strides are free (an expanded view is read in place), the trailing axes are made dense if they are not.
    targets   [Bc, Tc, V, H, W] (with `remap`: [Bc, Tc, V, 12, n, n]), normalised.
    lats_deg  latitudes of the lat-lon rows for the cos(lat) weights of the sums (None: unweighted); the ranks are never weighted.
    remap     an hpx_remap.HEALPixRemap: members and targets go through its hpx2ll launch first and are scored on its lat-lon grid.
    state     the dictionary a previous time chunk of the SAME samples returned; t_begin / T as evaluate.rollout_diagnostics.

    Returns {"sums" [Bc, T, V, 4], "ranks" [Bc, T, V, M + 1] (int32), "members": M, "grid": (H, W), "frames"} on the GPU.  Chunks in
    time and in batch give the bits of one call."""
    if targets.dim() < 5 or members.dim() != targets.dim() + 1:
        raise ValueError(f"members must be [B, M, T, V, H, W] and targets [B, T, V, H, W] (with a remap: planes [12, n, n]), not "
                         f"{tuple(members.shape)} / {tuple(targets.shape)}")
    Bc, Tc, V = targets.shape[:3]
    M = int(members.shape[1])
    if remap is not None:
        H, W, plane = remap.H, remap.W, (12, remap.nside, remap.nside)
    else:
        plane = tuple(targets.shape[3:])
        if len(plane) != 2:
            raise ValueError(f"targets must be [B, T, V, H, W], not {tuple(targets.shape)}")
        H, W = plane
    if tuple(targets.shape[3:]) != plane:
        raise ValueError(f"targets must be [B, T, V, {', '.join(map(str, plane))}], not {tuple(targets.shape)}")
    if tuple(members.shape) != (Bc, M, Tc, V) + plane:
        raise ValueError(f"members {tuple(members.shape)} and targets {tuple(targets.shape)} differ")
    if not 2 <= M <= MAX_MEMBERS:
        raise ValueError(f"M = {M} members must lie in 2..{MAX_MEMBERS}")
    T = Tc if T is None else int(T)
    t_begin = int(t_begin)
    if t_begin < 0 or t_begin + Tc > T:
        raise ValueError(f"chunk [{t_begin}, {t_begin + Tc}) is outside the rollout of {T} frames")
    if lats_deg is not None and len(lats_deg) != H:
        raise ValueError(f"lats_deg must have {H} entries, not {len(lats_deg)}")
    if not targets.is_cuda or not members.is_cuda:
        raise L.DlwpError("libdlwpmi needs CUDA/HIP tensors (no CPU fallback)")
    dev = targets.device
    if remap is not None:
        members, targets = remap.hpx2ll(members), remap.hpx2ll(targets)
    t = targets.contiguous()
    m = members
    dense = [int(np.prod(m.shape[k + 1:])) for k in range(3, m.dim())]
    if list(m.stride()[3:]) != dense or min(m.stride()[:3]) < 0:
        m = m.contiguous()
    bs, ms, ts = m.stride()[:3]
    roww = None
    if lats_deg is not None:
        from .evaluate import lat_weights
        roww = lat_weights(lats_deg, dev).contiguous()
    if state is None:
        state = {"sums": torch.zeros(Bc, T, V, 4, device=dev), "ranks": torch.zeros(Bc, T, V, M + 1, dtype=torch.int32, device=dev),
                 "members": M, "grid": (H, W), "frames": 0}
    elif (tuple(state["sums"].shape) != (Bc, T, V, 4) or state["members"] != M or tuple(state["grid"]) != (H, W)):
        raise ValueError("state belongs to another rollout (shape, members or grid differ)")
    lib = L.load()
    ws = L.workspace(lib.dlwp_ens_diag_ws_floats, Bc, M, Tc, V, H, W, device=dev)
    L.check(lib.dlwp_ens_diag(m.data_ptr(), bs, ms, ts, L.ptr(t), L.ptr(roww), Bc, M, Tc, V, H, W, t_begin, T, L.ptr(state["sums"]),
                              L.ptr(state["ranks"]), L.ptr(ws), L.stream()))
    state["frames"] += Tc
    return state


def concat_ensemble(parts):
    """The tables of batch chunks (each a finished `ensemble_diagnostics` state) joined along the sample axis, on the host."""
    first = parts[0]
    for p in parts[1:]:
        if p["members"] != first["members"] or tuple(p["grid"]) != tuple(first["grid"]):
            raise ValueError("the parts belong to different ensembles (members or grid differ)")
    return {"sums": torch.cat([p["sums"].cpu() for p in parts], 0), "ranks": torch.cat([p["ranks"].cpu() for p in parts], 0),
            "members": first["members"], "grid": tuple(first["grid"]), "frames": first["frames"]}


def ensemble_metrics(diag, scale=None):
    """From the tables of `ensemble_diagnostics` (or `concat_ensemble`), in float64 on the host, folded over the samples in index order
    with n = B H W as `evaluate.diag_metrics`; [T, V] each:
      rmse_mean     scale sqrt(S0 / n)                     the RMSE of the ensemble mean
      spread        scale sqrt(S1 / n)                     the root of the mean ensemble variance
      spread_skill  sqrt((M + 1) / M) spread / rmse_mean   1 for a reliable ensemble
      crps          scale (S2 - S3) / n                    the fair estimator
      crps_ens      scale (S2 - (M - 1) / M S3) / n        the estimator that treats the M members as the whole distribution
      mae_members   scale S2 / n
      rank_hist     [T, V, M + 1] frequencies
    scale: per variable, physical = x scale + shift (the shift cancels in every score)."""
    s = diag["sums"].double().cpu()
    r = diag["ranks"].cpu().to(torch.int64)
    B, T, V, _ = s.shape
    M = int(diag["members"])
    H, W = diag["grid"]
    tot, cnt = torch.zeros(T, V, 4, dtype=torch.float64), torch.zeros(T, V, M + 1, dtype=torch.int64)
    for b in range(B):                                        # samples in index order
        tot += s[b]
        cnt += r[b]
    sc = torch.ones(V, dtype=torch.float64)
    if scale is not None:
        sc = torch.as_tensor(scale, dtype=torch.float64).reshape(-1).abs()
        if sc.numel() != V:
            raise ValueError(f"scale must have one entry per variable ({V}), not {sc.numel()}")
    n = float(B * H * W)
    rmse, spread = sc * torch.sqrt(tot[..., 0] / n), sc * torch.sqrt(tot[..., 1] / n)
    return {"rmse_mean": rmse, "spread": spread, "spread_skill": float(np.sqrt((M + 1) / M)) * spread / rmse,
            "crps": sc * (tot[..., 2] - tot[..., 3]) / n, "crps_ens": sc * (tot[..., 2] - (M - 1) / M * tot[..., 3]) / n,
            "mae_members": sc * tot[..., 2] / n, "rank_hist": cnt.double() / n}


# ---- the CRPS as a training loss (dlwp_crps_loss_fwd_bwd) ---------------------------------------------------------------------------
def pair_coefficient(alpha, members):
    """lambda = 1 - (1 - alpha) / M of the "almost fair" CRPS: alpha = 1 the fair estimator, alpha = 0 the ensemble estimator"""
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:                              # (a NaN fails both comparisons)
        raise ValueError(f"alpha = {alpha} must lie in [0, 1]")
    return 1.0 - (1.0 - alpha) / int(members)


def _crps_weights(plane, lats_deg, var_weights, V, device):
    """(H, W, row weights [H] or None, variable weights [V] or None) for planes [H, W] or [12, n, n] (equal-area pixels: H = 12 n,
    W = n, no row weights)"""
    if len(plane) == 3:
        if plane[0] != 12 or plane[1] != plane[2]:
            raise ValueError(f"planes must be [H, W] or [12, n, n], not {list(plane)}")
        if lats_deg is not None:
            raise ValueError("lats_deg with HEALPix planes [12, n, n]: their pixels have equal area, there are no row weights")
        H, W = 12 * plane[1], plane[2]
    elif len(plane) == 2:
        H, W = plane
    else:
        raise ValueError(f"planes must be [H, W] or [12, n, n], not {list(plane)}")
    roww = varw = None
    if lats_deg is not None:
        lats = tuple(float(v) for v in np.asarray(lats_deg, dtype=np.float64).reshape(-1))
        if len(lats) != H:
            raise ValueError(f"lats_deg must have {H} entries, not {len(lats)}")
        from .evaluate import lat_weights
        roww = _device_floats(tuple(lat_weights(lats).tolist()), device)
    if var_weights is not None:
        vw = np.asarray(var_weights, dtype=np.float64).reshape(-1)
        if vw.size != V:
            raise ValueError(f"var_weights must have one entry per variable ({V}), not {vw.size}")
        if not (np.isfinite(vw).all() and (vw >= 0).all()):
            raise ValueError(f"var_weights {vw.tolist()} must be finite and not negative")
        varw = _device_floats(tuple(vw.tolist()), device)
    return int(H), int(W), roww, varw


def _crps_launch(members, target, loss_out, want_grad, alpha, lats_deg, var_weights, held=None):
    """(loss, gradient or None): the checks and the one call behind crps_loss and crps_loss_and_grad.  held: a dictionary in which the
    caller keeps the weight tables alive (a captured step replays their addresses)"""
    if target.dim() not in (5, 6) or members.dim() != target.dim() + 1:
        raise ValueError(f"members must be [B, M, T, V, H, W] and target [B, T, V, H, W] (or planes [12, n, n]), not "
                         f"{tuple(members.shape)} / {tuple(target.shape)}")
    B, T, V = (int(n) for n in target.shape[:3])
    M = int(members.shape[1])
    plane = tuple(target.shape[3:])
    if tuple(members.shape) != (B, M, T, V) + plane:
        raise ValueError(f"members {tuple(members.shape)} and target {tuple(target.shape)} differ")
    if not 2 <= M <= MAX_MEMBERS:
        raise ValueError(f"M = {M} members must lie in 2..{MAX_MEMBERS}")
    lam = pair_coefficient(alpha, M)
    if members.dtype != torch.float32 or target.dtype != torch.float32:
        raise L.DlwpError(f"crps_loss takes float32 tensors, not {members.dtype} / {target.dtype}")
    if not target.is_cuda or not members.is_cuda:
        raise L.DlwpError("libdlwpmi needs CUDA/HIP tensors (no CPU fallback)")
    dev = target.device
    if held is None or (dev, plane) not in held:
        tables = _crps_weights(plane, lats_deg, var_weights, V, dev)
        if held is not None:
            held[(dev, plane)] = tables
    else:
        tables = held[(dev, plane)]
    H, W, roww, varw = tables
    m = members.detach()
    dense = [int(np.prod(m.shape[k + 1:])) for k in range(3, m.dim())]
    if list(m.stride()[3:]) != dense or min(m.stride()[:3]) < 0:
        m = m.contiguous()
    bs, ms, ts = m.stride()[:3]
    if loss_out is None:
        loss_out = torch.empty(1, device=dev)
    elif loss_out.numel() != 1 or loss_out.dtype != torch.float32 or loss_out.device != dev:
        raise L.DlwpError(f"loss_out must be one float32 on {dev}, not {loss_out.dtype} {tuple(loss_out.shape)} on {loss_out.device}")
    grad = torch.empty(members.shape, device=dev) if want_grad else None
    lib = L.load()
    ws = L.workspace(lib.dlwp_crps_loss_ws_floats, B, M, T, V, H, W, device=dev)
    L.check(lib.dlwp_crps_loss_fwd_bwd(m.data_ptr(), bs, ms, ts, L.ptr(target.detach().contiguous()), L.ptr(roww), L.ptr(varw), B, M, T, V,
                                       H, W, lam, L.ptr(loss_out), L.ptr(grad), L.ptr(ws), L.stream()))
    return loss_out.reshape(()), grad


def crps_loss_and_grad(members, target, loss_out=None, *, alpha=1.0, lats_deg=None, var_weights=None):
    """(the loss of `crps_loss`, its gradient with respect to members) from the one dlwp_crps_loss_fwd_bwd call, for a caller that
    seeds the backward pass itself (train_engine.mse_loss_and_grad's counterpart).  loss_out: a one-element fp32 tensor that
    receives the loss (written, not accumulated)."""
    return _crps_launch(members, target, loss_out, True, alpha, lats_deg, var_weights)


class _Crps(torch.autograd.Function):
    @staticmethod
    def forward(ctx, members, target, alpha, lats_deg, var_weights):
        want = ctx.needs_input_grad[0]                       # False under no_grad: the loss alone (grad = NULL), as validation does
        loss, g = _crps_launch(members, target, None, want, alpha, lats_deg, var_weights)
        if want:
            ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, gl):
        (g,) = ctx.saved_tensors
        return g * gl, None, None, None, None


def crps_loss(members, target, *, alpha=1.0, lats_deg=None, var_weights=None):
    """The CRPS of M members against the target as one differentiable scalar (0-d), value and gradient from the same kernel:

        loss = mean over [B, T, V, H, W] of r_h c_v ((1 / M) sum_i |x_i - y| - lambda / (M (M - 1)) sum_{i<j} |x_i - x_j|),
        lambda = 1 - (1 - alpha) / M

    members      [B, M, T, V, H, W] or [B, M, T, V, 12, n, n] fp32 on the GPU (HEALPix planes: equal-area pixels, scored as H = 12 n,
                 W = n); batch, member and time strides are read in place, the trailing axes are made dense if they are not.
    target       the same shape without M.
    alpha        1: the fair CRPS (`ensemble_metrics`' "crps"); 0: the ensemble estimator ("crps_ens"); between: "almost fair".
    lats_deg     latitudes of the H rows: the weights r = `evaluate.lat_weights`; not with HEALPix planes (ValueError).
    var_weights  one weight c per variable.
    The sub-gradient is torch's: sgn(0) = 0, members that tie contribute nothing to each other.  Where members needs no gradient
    (torch.no_grad()) the kernel skips the gradient."""
    return _Crps.apply(members, target, alpha, lats_deg, var_weights)


class CrpsLoss:
    """The loss object of `train_engine.GraphedTrainStep(..., loss=)`: the model's output [B M, T, V, ...] holds the M members of
    each of the B samples next to each other (sample-major, the `repeat_interleave` order in which `evaluate_dlwp` folds the members
    into the batch); the target has B rows."""

    def __init__(self, members, alpha=1.0, lats_deg=None, var_weights=None):
        self.members = int(members)
        if not 2 <= self.members <= MAX_MEMBERS:
            raise ValueError(f"members = {self.members} must lie in 2..{MAX_MEMBERS}")
        pair_coefficient(alpha, self.members)
        self.alpha, self.lats_deg, self.var_weights = float(alpha), lats_deg, var_weights
        self._held = {}

    def _view(self, out, target):
        if out.dim() != target.dim() or out.shape[0] != target.shape[0] * self.members or out.shape[1:] != target.shape[1:]:
            raise ValueError(f"output {tuple(out.shape)} is not {self.members} members of the target {tuple(target.shape)}")
        return out.reshape(target.shape[0], self.members, *out.shape[1:])

    def loss_and_grad(self, out, target, loss_out=None):
        """(loss, d loss / d out in out's shape)"""
        loss, g = _crps_launch(self._view(out, target), target, loss_out, True, self.alpha, self.lats_deg, self.var_weights, self._held)
        return loss, g.reshape(out.shape)

    def loss(self, out, target):
        """the loss alone (validation)"""
        return _crps_launch(self._view(out, target), target, None, False, self.alpha, self.lats_deg, self.var_weights, self._held)[0]
