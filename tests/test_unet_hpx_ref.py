"""The HEALPix U-Net on a CPU-only box: the model helper (tests/unet_hpx_ref.py) against the golden vectors of the reference's
UNetHPX (tests/golden/make_unet_hpx_golden.py), the one-pixel face (n = 1) in the helper's padding, in the package's numpy
geometry and in the closed form the kernels run, the fold rows of the face-packed input gradient, and the interface and
refusals of `dlwpbench.UNetHEALPix`.

Bounds: those of tests/test_hpx_ref.py.  The padding is compared EXACTLY.  The model helper in float64 sits within twice the gap
the fixture stores for each array, in fp32 within 1e-5 (output, loss) / 5e-5 (every gradient tensor), what the fixture maker
asserts of the reference.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from unet_hpx_ref import CASES, GOLDEN, PAD_KEY, hpx_pad1, load_case, pad_input, rel_gap, run_case

HERE = os.path.dirname(os.path.abspath(__file__))


def golden():
    return np.load(os.path.join(HERE, "golden", GOLDEN))


@pytest.fixture(scope="module")
def h():
    from dlwp_benchmark_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def test_one_pixel_faces_pad_like_the_reference(h):
    """n = 1: the helper's padding, `hpx_halo_map(1)` and `dlwp_hpx_halo_sources(1)` against the reference's padded output"""
    from dlwp_benchmark_amd import conv_ops
    ref = golden()[PAD_KEY]
    x = pad_input(1)
    assert ref.shape == (12, 1, 3, 3) and ref.dtype == np.float64
    assert np.array_equal(hpx_pad1(x).numpy(), ref)
    assert np.array_equal(hpx_pad1(torch.cat([x, x + 1000.0], 0))[12:].numpy(), ref + 1000.0)      # a second sphere
    cells, src = conv_ops.hpx_halo_map(1)
    assert cells.shape == (12, 8, 2) and src.shape == (12, 8, 2, 4)
    xs = x[:, 0].numpy()
    out = np.zeros((12, 3, 3))
    out[:, 1, 1] = xs[:, 0, 0]
    for f in range(12):
        for (pr, pc), sources in zip(cells[f], src[f]):
            out[f, pr, pc] = sum(w * xs[int(sf), int(y), int(xx)] for sf, y, xx, w in sources if w > 0)
    assert np.array_equal(out, ref[:, 0])
    got = np.full((12, 8, 2), -7, dtype=np.int32)
    assert h.dlwp_hpx_halo_sources(1, got.ctypes.data_as(ctypes.c_void_p)) == 0
    want = np.where(src[..., 3] > 0, src[..., 0] + src[..., 1] + src[..., 2], -1).astype(np.int32)      # y = x = 0: the pixel is the face
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 8])
def test_fold_rows_are_the_transpose_of_the_halo_map(n):
    from dlwp_benchmark_amd import conv_ops
    cells, src = conv_ops.hpx_halo_map(n)
    table = conv_ops.hpx_fold_rows(n)
    R = 10 if n == 1 else 4
    assert table.shape == (12, n * n, R) and table.dtype == np.int32
    assert (table >= 0).sum() == 12 * 4 * (n + 1) + 8
    assert int((table >= 0).sum(axis=2).max()) == R                # at n = 1 one pixel is read by up to 10 ring cells
    PT = np.zeros((12, n, n, 12, n + 2, n + 2))
    for f in range(12):
        for p in range(n * n):
            row = table[f, p]
            ents = row[row >= 0]
            assert np.array_equal(row[:len(ents)], ents) and np.all(row[len(ents):] == -1)      # padded with -1 at the end
            assert list(ents) == sorted(ents)                                                   # a fixed, ascending order
            for e in ents:
                cf, rem = divmod(int(e) >> 1, (n + 2) * (n + 2))
                PT[f, p // n, p % n, cf, rem // (n + 2), rem % (n + 2)] += 0.5 if e & 1 else 1.0
    P = np.zeros_like(PT)
    for f in range(12):
        for (pr, pc), sources in zip(cells[f], src[f]):
            for sf, y, x, wt in sources:
                if wt > 0:
                    P[int(sf), int(y), int(x), f, pr, pc] += wt
    assert np.array_equal(P, PT)
    if n >= 2:      # the same readers in the same order as the table of the unpacked kernels
        old = conv_ops.hpx_fold_table(n)
        pix = ([(0, x) for x in range(n)] + [(n - 1, x) for x in range(n)] + [(y, 0) for y in range(1, n - 1)]
               + [(y, n - 1) for y in range(1, n - 1)])
        for pi, (y, x) in enumerate(pix):
            assert np.array_equal(old[:, pi], table[:, y * n + x])


@pytest.mark.parametrize("name", list(CASES))
def test_model_helper_matches_the_reference(name):
    cfg, n, B, T = CASES[name]
    params, inputs, target, y, loss, grads, gaps = load_case(golden(), name)
    assert inputs["prognostic"].shape == (B, T, cfg["prognostic_channels"], 12, n, n)
    assert y.shape == (B, T - cfg["context_size"], cfg["prognostic_channels"], 12, n, n)
    assert set(grads) == set(params) and n >> (len(cfg["hidden_channels"]) - 1) == (1 if name == "unet_f8" else 2)
    for dtype, bound in ((torch.float64, None), (torch.float32, (1e-5, 5e-5))):
        hy, hloss, hg = run_case(params, inputs, target, dtype, cfg)
        assert hy.shape == y.shape
        lim = lambda key, i: max(2.0 * gaps[key], 1e-12) if bound is None else bound[i]      # noqa: E731
        g = rel_gap(hy, y)
        print(f"{name} {dtype}: output {g:.2e} (<= {lim('y', 0):.2e})")
        assert g <= lim("y", 0)
        g = rel_gap(hloss, loss)
        assert g <= lim("loss", 0), (g, lim("loss", 0))
        for k in grads:
            g = rel_gap(hg[k], grads[k])
            assert g <= lim("g_" + k, 1), (k, g, lim("g_" + k, 1))


@pytest.mark.parametrize("name", list(CASES))
def test_cpu_built_model_has_the_golden_keys_and_shapes(name):
    from dlwp_benchmark_amd import dlwpbench
    assert "UNetHEALPix" in dlwpbench.__all__ and "model_class" in dlwpbench.__all__
    cfg = CASES[name][0]
    params = load_case(golden(), name)[0]
    net = dlwpbench.UNetHEALPix(device=torch.device("cpu"), type="UNetHPX", name="unet_hpx", **cfg)
    sd = net.state_dict()
    assert list(sd) == list(params)                      # the reference's keys in the reference's order
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in params.items()}
    net.load_state_dict(params, strict=True)
    assert all(torch.equal(net.state_dict()[k], params[k]) for k in params)
    levels = len(cfg["hidden_channels"])
    assert [k for k in sd if k.startswith("encoder.layers.0.")][0] == "encoder.layers.0.0.layers.1.weight"
    assert f"encoder.layers.{levels - 1}.1.layers.1.weight" in sd          # below the top the pool takes slot 0


def test_model_class_maps_the_reference_type_names():
    from dlwp_benchmark_amd import dlwpbench
    assert dlwpbench.model_class("UNetHPX") is dlwpbench.UNetHEALPix
    assert dlwpbench.model_class("UNet") is dlwpbench.UNet
    assert dlwpbench.model_class("ConvLSTMHPX") is dlwpbench.ConvLSTMHPX
    with pytest.raises(ValueError, match="NoSuchModel"):
        dlwpbench.model_class("NoSuchModel")
    for make in (lambda: dlwpbench.UNetHPX(), lambda: dlwpbench.UNet(mesh="healpix")):      # the names that keep raising say where to go
        with pytest.raises(NotImplementedError, match="UNetHEALPix") as e:
            make()
        assert "dgl" not in str(e.value)


def test_level_dispatch():
    from dlwp_benchmark_amd import conv_ops
    from dlwp_benchmark_amd.dlwpbench import unet
    assert [unet.packs_faces(n) for n in (1, 2, 4)] == [True] * 3          # the unpacked kernels refuse n = 1
    assert not any(unet.packs_faces(n) for n in (3, 6, 12, 16, 32))        # no packed kernel / faces that fill a tile
    assert unet.packs_faces(8) == (unet.PACK_FACES_UP_TO >= 8)
    net = unet.UNetHEALPix(constant_channels=0, prognostic_channels=2, hidden_channels=[4, 4, 4], device="cpu")
    net._dispatch(16)
    flags = lambda layer: {m.pack_faces for m in layer.modules() if isinstance(m, conv_ops.Conv3x3)}      # noqa: E731
    assert [flags(layer) for layer in net.encoder.layers] == [{False}, {unet.packs_faces(8)}, {True}]
    assert [flags(layer) for layer in net.decoder.layers] == [{True}, {unet.packs_faces(8)}, {False}]


def test_refusals():
    from dlwp_benchmark_amd import conv_ops, dlwpbench
    net = dlwpbench.UNetHEALPix(constant_channels=0, prescribed_channels=0, prognostic_channels=2, hidden_channels=[4, 4, 4],
                                device="cpu")
    with pytest.raises(ValueError, match="12.*6, 4, 4"):
        net(prognostic=torch.zeros(1, 3, 2, 6, 4, 4))            # a face count other than 12
    with pytest.raises(ValueError, match="12"):
        net(prognostic=torch.zeros(1, 3, 2, 8, 16))              # an equirectangular tensor
    with pytest.raises(ValueError, match="square.*4 x 8"):
        net(prognostic=torch.zeros(1, 3, 2, 12, 4, 8))
    with pytest.raises(ValueError, match="6 x 6.*3 levels.*divisible by 4"):
        net(prognostic=torch.zeros(1, 3, 2, 12, 6, 6))           # 6 -> 3 -> 1.5
    with pytest.raises(ValueError, match="context_size"):
        net(prognostic=torch.zeros(1, 1, 2, 12, 4, 4))
    with pytest.raises(ValueError, match="context_size"):
        dlwpbench.UNetHEALPix(context_size=0)
    with pytest.raises(ValueError, match="n_convolutions"):
        dlwpbench.UNetHEALPix(hidden_channels=[4, 8], n_convolutions=1)
    with pytest.raises(NotImplementedError, match="activation"):
        dlwpbench.UNetHEALPix(activation="th.nn.GELU()")
    with pytest.raises(NotImplementedError, match="UNet"):
        dlwpbench.UNetHEALPix(mesh="equirectangular")
    # pack_faces is the HEALPix padding on small faces
    with pytest.raises(ValueError, match="healpix"):
        conv_ops.Conv3x3(4, 4, pad_modes=("zeros", "circular"), pack_faces=True)
    w = torch.zeros(4, 4, 3, 3)
    with pytest.raises(ValueError, match="healpix"):
        conv_ops.conv3x3(torch.zeros(12, 4, 4, 4), w, padding="circular", pack_faces=True)
    with pytest.raises(ValueError, match="16 x 16"):
        conv_ops.conv3x3(torch.zeros(12, 16, 16, 4), w, padding="healpix", pack_faces=True)
    with pytest.raises(ValueError, match="3"):
        conv_ops.conv3x3(torch.zeros(12, 3, 3, 4), w, padding="healpix", pack_faces=True)
    assert conv_ops.Conv3x3(4, 4, pad_modes=("healpix", "healpix")).pack_faces is False


def test_packed_entry_points_refuse_bad_arguments(h):
    FAKE = 0x1000      # a non-NULL pointer value: validation must fail before it is ever dereferenced
    INVALID, UNSUPPORTED = -1, -3
    err = lambda: h.dlwp_last_error().decode()      # noqa: E731
    fwd = lambda B, H, W: h.dlwp_conv3x3_hpxp_fwd(FAKE, None, FAKE, None, FAKE, None, B, H, W, 4, 0, 4, 0, 0, None)      # noqa: E731
    dgrad = lambda B, n, R=4: h.dlwp_conv3x3_hpxp_dgrad(FAKE, FAKE, FAKE, R, FAKE, FAKE, None, B, n, 4, 4, 0, None)      # noqa: E731
    wgrad = lambda B, n: h.dlwp_conv3x3_hpxp_wgrad(FAKE, None, FAKE, FAKE, FAKE, None, B, n, 4, 0, 4, None)             # noqa: E731
    for call in (lambda: fwd(10, 4, 4), lambda: fwd(12, 4, 2), lambda: fwd(12, 0, 0), lambda: dgrad(7, 4), lambda: wgrad(12, 0),
                 lambda: dgrad(12, 4, R=0)):
        assert call() == INVALID, err()
    for call in (lambda: fwd(12, 3, 3), lambda: fwd(12, 16, 16), lambda: dgrad(12, 5), lambda: wgrad(24, 6), lambda: wgrad(12, 9)):
        assert call() == UNSUPPORTED and "1, 2, 4 and 8" in err(), err()
    assert h.dlwp_conv3x3_hpxp_dgrad_ws_floats(12, 1, 5) == 12 * 9 * 5
    assert h.dlwp_conv3x3_hpxp_dgrad_ws_floats(10, 1, 5) < 0
    assert h.dlwp_conv3x3_hpxp_wgrad_ws_floats(24, 2, 17, 57) > 0 and h.dlwp_conv3x3_hpxp_wgrad_ws_floats(24, 3, 17, 57) < 0
