"""Training on the CRPS of perturbed members: GraphedTrainStep(..., loss=CrpsLoss(M)) against eager torch autograd through a
plain-torch CRPS, and train_dlwp(loss="crps") on the synthetic WeatherBench case of tests/test_gpu_train_loop.py."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _afno():
    """the model of tests/test_gpu_train_engine.py"""
    from dlwp_benchmark_amd import nsbench
    torch.manual_seed(3)
    return nsbench.AFNONet(img_height=16, img_width=16, patch_size=(2, 2), in_chans=1, out_chans=1, embed_dim=32, depth=2,
                           mlp_ratio=2.0, num_blocks=4, context_size=2)


def torch_crps(out, target, M):
    """the fair CRPS in plain torch, broadcast form: out [B M, ...] holds the members of a sample next to each other"""
    o = out.reshape(target.shape[0], M, *target.shape[1:])
    mae = (o - target[:, None]).abs().mean(dim=1)
    pair = (o[:, :, None] - o[:, None, :]).abs().sum(dim=(1, 2)) / 2
    return (mae - pair / (M * (M - 1))).mean()


def test_graphed_crps_step_matches_eager_autograd(cuda):
    """four steps, eager and captured, against torch autograd + torch.optim.Adam: the margins tests/test_gpu_train_engine.py uses for
    the MSE step"""
    from dlwp_benchmark_amd.ensemble import CrpsLoss
    from dlwp_benchmark_amd.train_engine import GraphedTrainStep
    M = 3
    g = torch.Generator().manual_seed(11)
    u = torch.randn(2, 7, 1, 16, 16, generator=g).to(cuda)
    x, y = u[:, :-1].contiguous(), u[:, 1:].contiguous()
    xm = (x.repeat_interleave(M, dim=0) + 0.1 * torch.randn(2 * M, 6, 1, 16, 16, generator=g).to(cuda)).contiguous()
    call = lambda m, kw: m(kw["x"], 2)   # noqa: E731
    ref = _afno().to(cuda).train()
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    ref_losses = []
    for _ in range(4):
        opt.zero_grad(set_to_none=True)
        loss = torch_crps(ref(xm, 2), y, M)
        loss.backward()
        opt.step()
        ref_losses.append(loss.item())
    for use_graph in (False, True):
        model = _afno().to(cuda).train()
        step = GraphedTrainStep(model, {"x": xm}, y, lr=1e-3, use_graph=use_graph, call=call, loss=CrpsLoss(M))
        losses = [step().item() for _ in range(4)]
        print(use_graph, losses, ref_losses)
        for a, b in zip(losses, ref_losses):
            assert abs(a - b) <= 2e-4 * abs(b), (use_graph, losses, ref_losses)
        for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
            assert (p - q).abs().max().item() <= 2e-4, (use_graph, n)


def wb_case(cuda, n_train=100, n_val=28):
    """the synthetic WeatherBench case of tests/test_gpu_train_loop.py (16 x 32, two prognostic channels, an SFNO2DModule)"""
    from dlwp_benchmark_amd import dlwpbench, wbdata
    fields, prog, presc, const = wbdata.synthetic_fields(n_train + n_val, 16, 32, prognostic={"t2m": [], "z": [500]}, seed=5)
    kw = dict(prognostic_variable_names_and_levels=prog, prescribed_variable_names=presc, constant_names=const,
              sequence_length=4, normalize=True, context_size=1)

    def cut(lo, hi):
        return {k: (v[lo:hi] if not isinstance(v, dict) and v.ndim == 3 else
                    ({l: a[lo:hi] for l, a in v.items()} if isinstance(v, dict) else v)) for k, v in fields.items()}
    train, val = wbdata.WeatherBenchArrays(cut(0, n_train), **kw), wbdata.WeatherBenchArrays(cut(n_train, None), **kw)
    torch.manual_seed(3)
    model = dlwpbench.SFNO2DModule(constant_channels=4, prescribed_channels=1, prognostic_channels=2, grid="equiangular",
                                   num_layers=2, scale_factor=1, embed_dim=16, context_size=1, height=16, width=32,
                                   big_skip=True, pos_embed=True, use_mlp=True, normalization_layer="none").to(cuda)
    return model, train, val


CRPS_KW = dict(loss="crps", ensemble=3, ensemble_sigma=0.05, ensemble_seed=7)


@pytest.mark.parametrize("accumulation", [1, 2])
def test_train_dlwp_on_the_crps(cuda, tmp_path, accumulation):
    from dlwp_benchmark_amd import train_loop
    model, train, val = wb_case(cuda)
    log = train_loop.train_dlwp(model, train, val, name="c", epochs=4, batch_size=4, learning_rate=2e-3, out_dir=str(tmp_path),
                                gradient_accumulation_steps=accumulation, **CRPS_KW)
    print(log)
    assert len(log) == 4 and all(set(e) == {"epoch", "lr", "train_crps", "val_mse", "val_crps"} for e in log)
    assert all(math.isfinite(e["train_crps"]) and math.isfinite(e["val_crps"]) and math.isfinite(e["val_mse"]) for e in log)
    assert log[-1]["train_crps"] < log[0]["train_crps"] and log[-1]["val_crps"] < log[0]["val_crps"], log
    assert all(0 < e["val_crps"] for e in log)
    ck = torch.load(os.path.join(str(tmp_path), "c", "checkpoints", "c_last.ckpt"), weights_only=False)
    assert ck["epoch"] == 4 and ck["iteration"] == 4 * (len(train) // 4)
    assert ck["best_val_error"] <= log[0]["val_mse"]                      # the MSE of the unperturbed forecast selects `_best`


def test_train_dlwp_crps_device_data_equals_the_host_path(cuda):
    """the same items, the same members (the noise is keyed by the dataset index, not by where the batch was assembled) and the same
    kernels: tests/test_gpu_train_device_data.py asks its noisy case for finite values; without dataset noise the two logs are equal"""
    from dlwp_benchmark_amd import train_loop
    kw = dict(epochs=2, batch_size=4, learning_rate=2e-3, save_model=False, **CRPS_KW)
    model, train, val = wb_case(cuda, 40, 16)
    host = train_loop.train_dlwp(model, train, val, **kw)
    model, train, val = wb_case(cuda, 40, 16)
    dev = train_loop.train_dlwp(model, train, val, device_data=True, **kw)
    assert len(host) == len(dev) == 2
    for a, b in zip(host, dev):
        print(a, b)
        assert all(math.isfinite(v) for v in b.values())
        assert a["train_crps"] == b["train_crps"] and a["val_crps"] == b["val_crps"] and a["val_mse"] == b["val_mse"], (host, dev)


def test_default_call_keeps_its_keys(cuda):
    from dlwp_benchmark_amd import train_loop
    model, train, val = wb_case(cuda, 40, 16)
    log = train_loop.train_dlwp(model, train, val, epochs=1, batch_size=4, learning_rate=2e-3, save_model=False)
    assert [set(e) for e in log] == [{"epoch", "lr", "train_mse", "val_mse"}]
    model, train, val = wb_case(cuda, 40, 16)
    same = train_loop.train_dlwp(model, train, val, epochs=1, batch_size=4, learning_rate=2e-3, save_model=False, loss="mse")
    assert same == log
