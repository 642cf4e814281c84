"""dlwp_ns_batch through device_data.DeviceTrajectories: exact against ddp.ns_sample + torch.stack without noise, against the
float64 reference of the noise stream (tests/batch_ref.py) with it.

Shapes: a frame of 2 x 6 x 10 = 120 floats (rows of 40 bytes; 16-byte pieces), 2 x 6 x 7 = 84 floats (rows of 28 bytes, pieces that
straddle rows), 1 x 5 x 7 = 35 floats (no multiple of 4: the scalar form), an output view that starts 4 bytes off a 16-byte
boundary (the scalar form by alignment), 32 x 32 into a model's io_buffers() (the FNO plans need W % 16 == 0), and
384 x 512 = 196608 floats, where 12 source frames x 192 pieces exceed the grid cap and the workgroups stride.
The table has a repeated sample, a crop start of 0 and one of T - L."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_ref  # noqa: E402

pytestmark = pytest.mark.gpu

L_SEQ, SEED = 4, 1234
TABLE = [[3, 0], [1, 5], [3, 2]]          # repeated sample 3; crop starts 0 and T - L = 5
SHAPES = {"w10": (5, 9, 2, 6, 10), "w7": (5, 9, 2, 6, 7), "odd": (5, 9, 1, 5, 7)}


def make_u(shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def host_batch(u, table, epoch, monkeypatch):
    """torch.stack of ddp.ns_sample with the table's crop starts (crop_start is seeded per sample: it is pinned to the table)."""
    from dlwp_benchmark_amd import ddp
    xs, ys = [], []
    for i, r in table:
        monkeypatch.setattr(ddp, "crop_start", lambda *a, _r=r, **k: _r)
        x, y = ddp.ns_sample(u, i, epoch, L_SEQ, 0.0, SEED)
        xs.append(x), ys.append(y)
    monkeypatch.undo()
    return torch.stack(xs), torch.stack(ys)


def noise_bound(noise, x):
    # 4x the fp32 error of the element-to-normal map (argument rounding 2 pi 2^-24 |r| <= 2.2e-6, a few ulp of logf / sqrtf),
    # plus the rounding of the final add
    return noise * 2e-5 + 2.0 ** -23 * float(np.abs(x).max())


def check_noisy(x, u, table, epoch, noise, seed=SEED):
    """|x - (window + noise z_ref)| within the bound, per row of the table; returns the largest error in units of noise."""
    x = x.double().cpu().numpy()
    worst = 0.0
    for b, (i, r) in enumerate(table):
        win = u[i, r:r + L_SEQ - 1].double().numpy()
        z = batch_ref.normals(seed, epoch, i, win.size, batch_ref.TAG_NS).reshape(win.shape)
        err = np.abs(x[b] - (win + noise * z))
        print(f"row {b}: max noise error {err.max():.3e} (bound {noise_bound(noise, x):.3e})")
        assert (err <= noise_bound(noise, x)).all(), (b, err.max())
        worst = max(worst, err.max() / noise)
    return worst


@pytest.mark.parametrize("case", list(SHAPES))
def test_without_noise_equals_the_host_path(cuda, monkeypatch, case):
    from dlwp_benchmark_amd.device_data import DeviceTrajectories
    u = make_u(SHAPES[case])
    xr, yr = host_batch(u, TABLE, 0, monkeypatch)
    dd = DeviceTrajectories(u, L_SEQ, device=cuda)
    x, y = dd.batch(TABLE, epoch=0)
    assert torch.equal(x.cpu(), xr) and torch.equal(y.cpu(), yr)
    x2, y2 = dd.batch(dd.upload(TABLE), epoch=3)                       # a device table; without noise the epoch changes nothing
    assert torch.equal(x2, x) and torch.equal(y2, y)


def test_unaligned_output_views_take_the_scalar_form(cuda, monkeypatch):
    from dlwp_benchmark_amd.device_data import DeviceTrajectories
    u = make_u(SHAPES["w10"])
    xr, yr = host_batch(u, TABLE, 0, monkeypatch)
    dd = DeviceTrajectories(u, L_SEQ, device=cuda)
    n = xr.numel()
    flat = torch.full((2 * n + 8,), float("nan"), device=cuda)
    x, y = flat[1:1 + n].view(xr.shape), flat[n + 5:2 * n + 5].view(yr.shape)      # 4 bytes past a 16-byte boundary
    assert x.data_ptr() % 16 == 4 and y.data_ptr() % 16 == 4
    dd.batch(TABLE, 0, out=(x, y))
    assert torch.equal(x.cpu(), xr) and torch.equal(y.cpu(), yr)
    guard = torch.cat([flat[:1], flat[1 + n:n + 5], flat[2 * n + 5:]])
    assert torch.isnan(guard).all()                                     # nothing written around the views
    x3, _ = DeviceTrajectories(u, L_SEQ, noise=0.1, device=cuda).batch(TABLE, 2, out=(x, y))
    xa, _ = DeviceTrajectories(u, L_SEQ, noise=0.1, device=cuda).batch(TABLE, 2)
    assert torch.equal(x3, xa)                                          # the scalar and the vector form draw the same noise


def test_into_the_io_buffers_of_a_model(cuda, monkeypatch):
    from dlwp_benchmark_amd import nsbench
    from dlwp_benchmark_amd.device_data import DeviceTrajectories
    torch.manual_seed(7)
    model = nsbench.TFNO2DModule(n_modes=[8, 8], in_channels=1, hidden_channels=16, lifting_channels=32, projection_channels=32,
                                 out_channels=1, n_layers=2, context_size=2).to(cuda)
    u = make_u((5, 9, 1, 32, 32))
    xr, yr = host_batch(u, TABLE, 0, monkeypatch)
    bx, by = model.io_buffers(len(TABLE), L_SEQ - 1, 32, 32, 2)
    x, y = DeviceTrajectories(u, L_SEQ, device=cuda).batch(TABLE, 0, out=(bx, by))
    assert x.data_ptr() == bx.data_ptr() and y.data_ptr() == by.data_ptr()
    assert torch.equal(bx.cpu(), xr) and torch.equal(by.cpu(), yr)
    opt = model.make_optimizer(lr=1e-3)
    model.train_step(bx, by, 2, optimizer=opt)                          # the step reads the buffers in place
    torch.manual_seed(7)
    ref = nsbench.TFNO2DModule(n_modes=[8, 8], in_channels=1, hidden_channels=16, lifting_channels=32, projection_channels=32,
                               out_channels=1, n_layers=2, context_size=2).to(cuda)
    ref.train_step(xr.to(cuda), yr.to(cuda), 2, optimizer=ref.make_optimizer(lr=1e-3))
    assert torch.equal(model.flat_params.data, ref.flat_params.data)


@pytest.mark.parametrize("case", list(SHAPES))
def test_noise_follows_the_reference_stream(cuda, case):
    from dlwp_benchmark_amd.device_data import DeviceTrajectories
    u, noise, epoch = make_u(SHAPES[case]), 0.05, 2
    dd = DeviceTrajectories(u, L_SEQ, noise=noise, seed=SEED, device=cuda)
    x, y = dd.batch(TABLE, epoch)
    worst = check_noisy(x, u, TABLE, epoch, noise)
    print(f"{case}: largest noise error {worst:.3e} x noise")
    clean = DeviceTrajectories(u, L_SEQ, device=cuda).batch(TABLE, epoch)
    assert torch.equal(y, clean[1])                                     # y is never perturbed
    assert not torch.equal(x, clean[0])


def test_noise_with_a_seed_above_32_bits(cuda):
    from dlwp_benchmark_amd.device_data import DeviceTrajectories
    u, noise, seed = make_u(SHAPES["w10"]), 0.05, (0x9abcdef0 << 32) | 0x12345678
    x, _ = DeviceTrajectories(u, L_SEQ, noise=noise, seed=seed, device=cuda).batch(TABLE, 1)
    check_noisy(x, u, TABLE, 1, noise, seed=seed)


def test_noise_depends_on_seed_epoch_item_and_element_only(cuda):
    from dlwp_benchmark_amd.device_data import DeviceTrajectories
    u = make_u(SHAPES["w10"])
    dd = DeviceTrajectories(u, L_SEQ, noise=0.1, seed=SEED, device=cuda)
    x, _ = dd.batch([[3, 2], [1, 5], [0, 0]], 4)
    x2, _ = dd.batch([[2, 1], [4, 4], [3, 2], [3, 2], [1, 0]], 4)       # another batch size, composition and position
    assert torch.equal(x[0], x2[2]) and torch.equal(x2[2], x2[3])
    z = lambda t, b, i, r: (t[b].cpu() - u[i, r:r + L_SEQ - 1]) / 0.1   # noqa: E731
    za = z(x, 1, 1, 5)
    assert (z(x2, 4, 1, 0) - za).abs().max() < 1e-4                     # the same item at another crop start: the same perturbation
    x3, _ = dd.batch([[3, 2], [1, 5], [0, 0]], 5)                       # another epoch
    assert (z(x3, 1, 1, 5) - za).abs().mean() > 0.5                     # independent draws: E|z - z'| = 2 / sqrt(pi) = 1.13
    assert (z(x, 0, 3, 2) - za).abs().mean() > 0.5                      # another item
    other = DeviceTrajectories(u, L_SEQ, noise=0.1, seed=SEED + 1, device=cuda).batch([[3, 2], [1, 5], [0, 0]], 4)[0]
    assert (z(other, 1, 1, 5) - za).abs().mean() > 0.5                  # another seed


def test_strided_grid_exact_and_noisy(cuda, monkeypatch):
    """12 source frames x 192 pieces of 256 x 16 bytes: above the cap of the grid, so every workgroup strides."""
    from dlwp_benchmark_amd.device_data import DeviceTrajectories
    u = make_u((2, 5, 1, 384, 512), seed=1)
    table = [[1, 0], [0, 1], [1, 1]]
    xr, yr = host_batch(u, table, 0, monkeypatch)
    x, y = DeviceTrajectories(u, L_SEQ, device=cuda).batch(table, 0)
    assert torch.equal(x.cpu(), xr) and torch.equal(y.cpu(), yr)
    xn, yn = DeviceTrajectories(u, L_SEQ, noise=0.05, device=cuda).batch(table, 1)
    check_noisy(xn, u, table, 1, 0.05)
    assert torch.equal(yn, y)


def test_gpu_normals_have_the_moments_of_a_standard_normal(cuda):
    """2^17 elements: one sample of two 256 x 256 frames of zeros, so x / noise is the stream itself."""
    from dlwp_benchmark_amd.device_data import DeviceTrajectories
    n, noise = 2 ** 17, 0.5
    u = torch.zeros(1, 3, 1, 256, 256)
    x, y = DeviceTrajectories(u, 3, noise=noise, seed=SEED, device=cuda).batch([[0, 0]], 1)
    z = (x.double().cpu().numpy() / noise).reshape(-1)
    assert z.size == n and (y == 0).all()
    print(f"mean {z.mean():.5f} var {z.var():.5f} max |z| {np.abs(z).max():.4f}")
    assert abs(z.mean()) <= 5 / np.sqrt(n)
    assert abs(z.var() - 1) <= 5 * np.sqrt(2 / n)
    assert np.abs(z).max() <= batch_ref.Z_MAX * (1 + 1e-6)             # fp32 logf / sqrtf: a few ulp (6e-8 each) above the exact bound
    ref = batch_ref.normals(SEED, 1, 0, n, batch_ref.TAG_NS)
    assert np.abs(z - ref).max() <= 2e-5
