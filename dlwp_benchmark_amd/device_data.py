"""Training batches assembled on the GPU from device-resident datasets (csrc/batch_ops.hip, docs/kernels/data.md).

The host paths build every sample on the CPU (ddp.ns_sample: two clones and a generator per sample; WeatherBenchArrays.__getitem__:
a subtract, a divide and a stack per variable, a float64 normal draw of the whole window), stack the batch and copy it to the
device.  Here the dataset is uploaded ONCE, an epoch's index table is uploaded with one copy, and a batch is one kernel launch
that may write straight into the buffers the captured step reads (`model.io_buffers()`).

What is the same as the host path, bit for bit: which samples and crop windows a rank sees (ddp.shard_indices / ddp.crop_start,
the functions the host path uses) and, with noise == 0, every value of every tensor (copies, and the fp32 z-score
(a - mean) / std with a correctly rounded division).  What differs: with noise > 0 the perturbation comes from the library's own
counter-based stream (Philox4x32-10 keyed by the seed, counter (element >> 2, item, epoch, tag)) instead of torch's / numpy's host
generators, which a kernel cannot reproduce; like theirs it depends on (seed, epoch, item) only, not on the batch or the ranks.

Tables are validated with numpy before they are uploaded; the kernels additionally skip any row that is out of range.
"""
import numpy as np
import torch

from . import ddp
from . import lib as L


def validate_ns_table(table, n_samples, t_file, length):
    """[..., 2] (sample index, crop start) rows as a contiguous int32 array; ValueError for a row outside the data."""
    if int(length) < 2:
        raise ValueError(f"sequence_length {length} must be at least 2 (x and y are sequence_length - 1 frames)")
    if int(length) > int(t_file):
        raise ValueError(f"sequence_length {length} is longer than the trajectories ({t_file} frames)")
    t = np.asarray(table)
    if t.ndim < 1 or t.shape[-1] != 2 or t.size == 0 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"a table of integer (sample index, crop start) rows [..., 2] is needed, got {t.dtype} {t.shape}")
    i, r = t[..., 0], t[..., 1]
    if i.min() < 0 or i.max() >= n_samples:
        raise ValueError(f"sample index outside [0, {n_samples}): min {i.min()}, max {i.max()}")
    if r.min() < 0 or r.max() > t_file - length:
        raise ValueError(f"crop start outside [0, {t_file - length}] (T {t_file}, sequence_length {length}): min {r.min()}, max {r.max()}")
    return np.ascontiguousarray(t, dtype=np.int32)


def validate_wb_items(items, n_items):
    """[...] item indices as a contiguous int32 array; ValueError for an item outside [0, n_items)."""
    t = np.asarray(items)
    if t.size == 0 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"integer item indices are needed, got {t.dtype} {t.shape}")
    if t.min() < 0 or t.max() >= n_items:
        raise ValueError(f"item outside [0, {n_items}): min {t.min()}, max {t.max()}")
    return np.ascontiguousarray(t, dtype=np.int32)


def _check_noise(noise, seed):
    noise = float(noise)
    if not (0.0 <= noise < float("inf")):
        raise ValueError(f"noise {noise} must be finite and not negative")
    if noise > 0.0 and seed is None:
        raise ValueError("noise > 0 needs a seed: the device noise stream is keyed by it")
    seed = 0 if seed is None else int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed {seed} must fit 64 unsigned bits")
    return noise, seed


def _device_table(table, upload, what):
    """A table row for a launch: tensors on the device come from epoch_table() / upload() (validated there); anything on the
    host is validated and uploaded here."""
    if torch.is_tensor(table) and table.is_cuda:
        if table.dtype != torch.int32 or not table.is_contiguous():
            raise ValueError(f"{what}: a contiguous int32 device tensor is needed (epoch_table() / upload() give one)")
        return table
    return upload(table.numpy() if torch.is_tensor(table) else table)


class DeviceTrajectories:
    """Navier-Stokes trajectories u [N, T, D, H, W] resident on the device; batches as ddp.ns_sample + torch.stack give them."""

    def __init__(self, u, sequence_length, noise=0.0, seed=1234, device="cuda"):
        u = torch.as_tensor(u)
        if u.dim() != 5 or u.dtype != torch.float32:
            raise ValueError(f"u must be a float32 [N, T, D, H, W] array, got {u.dtype} {tuple(u.shape)}")
        self.sequence_length = int(sequence_length)
        self.noise, self.seed = _check_noise(noise, seed)
        self.shape = tuple(u.shape)
        validate_ns_table(np.zeros((1, 2), dtype=np.int64), self.shape[0], self.shape[1], self.sequence_length)
        self.device = torch.device(device)
        self.u = u.to(self.device).contiguous()          # the one upload

    @classmethod
    def generate(cls, sequence_length, noise=0.0, seed=1234, device="cuda", **generate_data_kwargs):
        """Trajectories generated on the device and wrapped where they lie: nsdata.generate_data(rng="philox", solver="kernels",
        to_device=True, seed=seed, device=device, **generate_data_kwargs) -- no file, no host copy, no upload.  The one seed names
        the dataset (Philox tag of dlwp_ns2d_grf) and keys the batch noise (tag of dlwp_ns_batch): two streams.  `.u` is the tensor
        generate_data returned; train_ns(model, d.u[:k], d.u[k:], device_data=True) trains on it."""
        from . import nsdata
        for fixed in ("rng", "solver", "to_device", "seed", "device"):
            if fixed in generate_data_kwargs:
                raise ValueError(f"DeviceTrajectories.generate sets {fixed} itself")
        data = nsdata.generate_data(rng="philox", solver="kernels", to_device=True, seed=seed, device=device, **generate_data_kwargs)
        return cls(data["u"], sequence_length, noise=noise, seed=seed, device=data["u"].device)

    def upload(self, table):
        """A host table [..., 2] of (sample index, crop start) rows -> validated, int32, on the device (one copy)."""
        t = validate_ns_table(table, self.shape[0], self.shape[1], self.sequence_length)
        return torch.from_numpy(t).to(self.device)

    def epoch_table(self, epoch, rank=0, world=1, batch_size=4):
        """[n_iters, B, 2] int32 on the device: the samples ddp.shard_indices gives this rank in `epoch`, each with the crop start
        of ddp.crop_start -- what the host path draws sample by sample -- uploaded with one copy."""
        idx = ddp.shard_indices(self.shape[0], epoch, rank, world, batch_size, self.seed)
        t = np.empty(idx.shape + (2,), dtype=np.int64)
        t[..., 0] = idx
        t[..., 1] = [[ddp.crop_start(int(i), epoch, self.shape[1], self.sequence_length, self.seed) for i in row] for row in idx]
        if t.size == 0:
            return torch.empty((0, batch_size, 2), dtype=torch.int32, device=self.device)
        return self.upload(t)

    def batch(self, table_row, epoch, out=None):
        """(x, y) [B, L-1, D, H, W] of the rows [B, 2] of a table; out = (x, y) buffers to write into (e.g. io_buffers())."""
        row = _device_table(table_row, self.upload, "DeviceTrajectories.batch")
        if row.dim() != 2 or row.shape[1] != 2:
            raise ValueError(f"a table row [B, 2] is needed, got {tuple(row.shape)}")
        N, T, D, H, W = self.shape
        B, shape = row.shape[0], (row.shape[0], self.sequence_length - 1, D, H, W)
        if out is None:
            x, y = torch.empty(shape, device=self.device), torch.empty(shape, device=self.device)
        else:
            x, y = out
            for t in (x, y):
                if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != self.u.device:
                    raise ValueError(f"out buffers must be float32 {shape} on {self.u.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        L.check(L.load().dlwp_ns_batch(L.ptr(self.u), N, T, D * H * W, L.ptr(row), B, self.sequence_length, self.noise, self.seed,
                                       int(epoch), L.ptr(x), L.ptr(y), L.stream()))
        return x, y


class DeviceWeatherBench:
    """The training branch of a wbdata.WeatherBenchArrays resident on the device: every series uploaded once, batches as
    to_device_batch([dataset[i] for i in items]) gives them (None for absent groups)."""

    def __init__(self, dataset, device="cuda"):
        if getattr(dataset, "init_dates", None) is not None:
            raise ValueError("a dataset with init_dates is the evaluation branch: it stays on the host")
        self.noise, self.seed = _check_noise(dataset.noise, dataset.seed)
        self.sequence_length, self.context_size = int(dataset.sequence_length), int(dataset.context_size)
        if self.sequence_length < 2 or not 0 <= self.context_size < self.sequence_length:
            raise ValueError(f"sequence_length {self.sequence_length} must be at least 2 and context_size {self.context_size} below it")
        self.n_time, self.n_items = int(dataset.n_time), len(dataset)
        self.device = torch.device(device)
        norm = bool(dataset.normalize)
        groups = ([(np.asarray(dataset.fields[c]), dataset.stats[c], 2) for c in dataset.constant_names],
                  [(np.asarray(dataset.fields[p]), dataset.stats[p], 3) for p in dataset.prescribed_variable_names], [])
        for p, levels in dataset.prognostic_variable_names_and_levels.items():
            if levels:
                groups[2].extend((np.asarray(dataset.fields[p][l]), dataset.stats[p]["level"][l], 3) for l in levels)
            else:
                groups[2].append((np.asarray(dataset.fields[p]), dataset.stats[p], 3))
        self.counts = tuple(len(g) for g in groups)
        self.plane, self._series, chans = None, [], []
        for a, st, ndim in (e for g in groups for e in g):
            if a.dtype != np.float32 or a.ndim != ndim:
                raise ValueError(f"the device path keeps float32 series ([time, lat, lon]; constants [lat, lon]), got {a.dtype} {a.shape}")
            if self.plane is None:
                self.plane = tuple(a.shape[-2:])
            if tuple(a.shape[-2:]) != self.plane or (ndim == 3 and a.shape[0] < self.n_time):
                raise ValueError(f"series {a.shape} does not match the grid {self.plane} and the record of {self.n_time} frames")
            t = torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            self._series.append(t)                                       # keeps the storage behind the descriptors alive
            chans.append(L.WbChannel(t.data_ptr(), float(st["mean"]), float(st["std"]), int(norm)))
        raw = np.frombuffer(bytes((L.WbChannel * len(chans))(*chans)), dtype=np.uint8).copy()
        self.channels = torch.from_numpy(raw).to(self.device)

    def __len__(self):
        return self.n_items

    def upload(self, items):
        """Host item indices [...] -> validated, int32, on the device (one copy)."""
        return torch.from_numpy(validate_wb_items(items, self.n_items)).to(self.device)

    def epoch_table(self, epoch, rank=0, world=1, batch_size=4, seed=1234):
        """[n_iters, B] int32 on the device: wbdata.shard_batches' items of this rank in `epoch`, uploaded with one copy."""
        idx = ddp.shard_indices(self.n_items, epoch, rank, world, batch_size, seed=seed)
        if idx.size == 0:
            return torch.empty((0, batch_size), dtype=torch.int32, device=self.device)
        return self.upload(idx)

    def batch(self, items, epoch, out=None):
        """(constants [B,1,C,H,W], prescribed [B,L,P,H,W], prognostic [B,L,G,H,W], target [B,L-context,G,H,W]) of the items [B];
        out: four buffers to write into (None where a group is absent)."""
        row = _device_table(items, self.upload, "DeviceWeatherBench.batch")
        if row.dim() != 1:
            raise ValueError(f"item indices [B] are needed, got {tuple(row.shape)}")
        B, Ls, ctx, (H, W), (nC, nP, nG) = row.shape[0], self.sequence_length, self.context_size, self.plane, self.counts
        shapes = ((B, 1, nC, H, W), (B, Ls, nP, H, W), (B, Ls, nG, H, W), (B, Ls - ctx, nG, H, W))
        if out is None:
            out = [torch.empty(s, device=self.device) if s[2] else None for s in shapes]
        for t, s in zip(out, shapes):
            if (t is None) != (s[2] == 0) or (t is not None and (tuple(t.shape) != s or t.dtype != torch.float32
                                                                 or t.device != self.channels.device)):
                raise ValueError(f"out buffers must be float32 {[s for s in shapes]} on {self.channels.device} (None for an absent group)")
        c, p, g, t = out
        L.check(L.load().dlwp_wb_batch(L.ptr(self.channels), nC, nP, nG, L.ptr(row), B, Ls, ctx, self.n_time, H * W, self.noise,
                                       self.seed, int(epoch), L.ptr(c), L.ptr(p), L.ptr(g), L.ptr(t), L.stream()))
        return c, p, g, t
