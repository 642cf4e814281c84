"""HEALPix on a CPU-only box: the padding helper (tests/hpx_ref.py), the numpy geometry of the package
(`conv_ops.hpx_halo_map`, the fold table derived from it, and the closed form the kernels run, `dlwp_hpx_halo_sources`) against
the reference's own padded output (tests/golden/make_hpx_golden.py), the model helper against the golden vectors of the
reference's ConvLSTMHPX, and the interface and refusals of `dlwpbench.ConvLSTMHPX` and of the entry points.

Bounds: the padding is compared EXACTLY (the fixture is integer-valued float64; the 0.5 / 0.5 cells are exact).  The model
helper in float64 sits within twice the gap the fixture stores for each array (the rule of tests/test_convlstm_ref.py), in fp32
within 1e-5 (output, loss) / 5e-5 (every gradient tensor), what the fixture maker asserts of the reference.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from hpx_ref import CASES, GOLDEN, PAD_GOLDEN, PAD_SIZES, hpx_pad1, load_case, pad_input, rel_gap, run_case

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = 0x1000      # a non-NULL pointer value: validation must fail before it is ever dereferenced


def golden(name):
    return np.load(os.path.join(HERE, "golden", name))


def apply_map(n, x):
    """the padding of x [12, n, n] by `conv_ops.hpx_halo_map` in numpy"""
    from dlwp_benchmark_amd import conv_ops
    cells, src = conv_ops.hpx_halo_map(n)
    assert cells.shape == (12, 4 * (n + 1), 2) and src.shape == (12, 4 * (n + 1), 2, 4)
    out = np.zeros((12, n + 2, n + 2))
    out[:, 1:-1, 1:-1] = x
    for f in range(12):
        for (pr, pc), sources in zip(cells[f], src[f]):
            out[f, pr, pc] = sum(w * x[int(sf), int(y), int(xx)] for sf, y, xx, w in sources if w > 0)
    return out


@pytest.mark.parametrize("n", PAD_SIZES)
def test_padding_helper_and_halo_map_reproduce_the_reference_exactly(n):
    ref = golden(PAD_GOLDEN)[f"n{n}"]
    x = pad_input(n)
    assert ref.shape == (12, 1, n + 2, n + 2) and ref.dtype == np.float64
    assert np.array_equal(hpx_pad1(x).numpy(), ref)
    assert np.array_equal(hpx_pad1(torch.cat([x, x + 1000.0], 0))[12:].numpy(), ref + 1000.0)      # a second sphere
    assert np.array_equal(apply_map(n, x[:, 0].numpy()), ref[:, 0])


@pytest.mark.parametrize("n", PAD_SIZES + (24,))
def test_halo_map_properties_and_fold_table(n):
    from dlwp_benchmark_amd import conv_ops
    cells, src = conv_ops.hpx_halo_map(n)
    w = src[..., 3]
    assert np.array_equal(w.sum(axis=2), np.ones((12, 4 * (n + 1))))              # every cell's weights sum to 1
    two = (w[:, :, 1] > 0)
    assert two.sum() == 8 and set(np.nonzero(two)[0]) == {4, 5, 6, 7}             # 8 two-source cells, on the equatorial faces
    assert set(np.unique(w)) <= {0.0, 0.5, 1.0}
    ring = {(r, c) for r in range(n + 2) for c in range(n + 2) if r in (0, n + 1) or c in (0, n + 1)}
    assert all({tuple(rc) for rc in cells[f]} == ring for f in range(12))         # the whole ring, each cell once
    reads = {}
    for f in range(12):
        for ci in range(cells.shape[1]):
            for sf, y, x, wt in src[f, ci]:
                if wt > 0:
                    assert 0 <= sf < 12 and sf != f and 0 <= y < n and 0 <= x < n
                    reads[(int(sf), int(y), int(x))] = reads.get((int(sf), int(y), int(x)), 0) + 1
    assert max(reads.values()) <= 4                                               # no pixel is read by more than 4 ring cells
    assert all(y in (0, n - 1) or x in (0, n - 1) for _, y, x in reads)           # only border pixels are read
    if n < 2:
        return
    # the table the fold kernel reads is the transpose of the map: applying it to a one-hot ring reproduces P^T
    table = conv_ops.hpx_fold_table(n)
    assert table.shape == (12, 4 * n - 4, 4) and table.dtype == np.int32
    assert (table >= 0).sum() == 12 * 4 * (n + 1) + 8
    pix = ([(0, x) for x in range(n)] + [(n - 1, x) for x in range(n)] + [(y, 0) for y in range(1, n - 1)]
           + [(y, n - 1) for y in range(1, n - 1)])
    PT = np.zeros((12, n, n, 12, n + 2, n + 2))
    for f in range(12):
        for pi, (y, x) in enumerate(pix):
            ents = table[f, pi][table[f, pi] >= 0]
            assert list(ents) == sorted(ents)                                     # a fixed, ascending order
            for e in ents:
                cf, rem = divmod(int(e) >> 1, (n + 2) * (n + 2))
                PT[f, y, x, cf, rem // (n + 2), rem % (n + 2)] += 0.5 if e & 1 else 1.0
    P = np.zeros_like(PT)
    for f in range(12):
        for (pr, pc), sources in zip(cells[f], src[f]):
            for sf, y, x, wt in sources:
                if wt > 0:
                    P[int(sf), int(y), int(x), f, pr, pc] += wt
    assert np.array_equal(P, PT)


@pytest.fixture(scope="module")
def h():
    from dlwp_benchmark_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


@pytest.mark.parametrize("n", PAD_SIZES + (24,))
def test_the_kernels_closed_form_is_the_halo_map(h, n):
    """dlwp_hpx_halo_sources runs, on the host, the function the kernels resolve a ring cell with"""
    from dlwp_benchmark_amd import conv_ops
    cells, src = conv_ops.hpx_halo_map(n)
    out = np.full((12, 4 * (n + 1), 2), -7, dtype=np.int32)
    assert h.dlwp_hpx_halo_sources(n, out.ctypes.data_as(ctypes.c_void_p)) == 0
    want = np.where(src[..., 3] > 0, (src[..., 0] * n + src[..., 1]) * n + src[..., 2], -1).astype(np.int32)
    assert np.array_equal(out, want)             # the library's ring order is hpx_halo_map's


@pytest.mark.parametrize("name", list(CASES))
def test_model_helper_matches_the_reference(name):
    cfg, B, T = CASES[name]
    params, inputs, target, y, loss, grads, gaps = load_case(golden(GOLDEN), name)
    n = cfg["height"]
    assert inputs["prognostic"].shape == (B, T, cfg["prognostic_channels"], 12, n, n)
    assert set(grads) == set(params) and len(params) >= 12
    for dtype, bound in ((torch.float64, None), (torch.float32, (1e-5, 5e-5))):
        hy, hloss, hg = run_case(params, inputs, target, dtype, cfg["context_size"])
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
    assert "ConvLSTMHPX" in dlwpbench.__all__
    cfg, B, T = CASES[name]
    params = load_case(golden(GOLDEN), name)[0]
    net = dlwpbench.ConvLSTMHPX(batch_size=B, device=torch.device("cpu"), type="ConvLSTMHPX", name="clstm_hpx", **cfg)
    sd = net.state_dict()
    assert list(sd) == list(params)                      # the reference's keys in the reference's order
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in params.items()}
    net.load_state_dict(params, strict=True)
    assert all(torch.equal(net.state_dict()[k], params[k]) for k in params)


def test_refusals():
    from dlwp_benchmark_amd import conv_ops, dlwpbench
    with pytest.raises(ValueError, match="equal"):
        dlwpbench.ConvLSTMHPX(hidden_sizes=[8, 16])
    net = dlwpbench.ConvLSTMHPX(constant_channels=0, prescribed_channels=0, prognostic_channels=2, hidden_sizes=[4], device="cpu")
    with pytest.raises(ValueError, match="12"):
        net(prognostic=torch.zeros(1, 3, 2, 6, 4, 4))            # a face count other than 12
    with pytest.raises(ValueError, match="12"):
        net(prognostic=torch.zeros(1, 3, 2, 8, 16))              # an equirectangular tensor
    with pytest.raises(ValueError, match="square"):
        net(prognostic=torch.zeros(1, 3, 2, 12, 4, 8))
    with pytest.raises(ValueError, match="context_size"):
        net(prognostic=torch.zeros(1, 1, 2, 12, 4, 4))
    # the classes that stay unbuilt on this mesh keep saying so
    for make in (lambda: dlwpbench.ConvLSTM(mesh="healpix"), lambda: dlwpbench.UNet(mesh="healpix"), lambda: dlwpbench.UNetHPX()):
        with pytest.raises(NotImplementedError) as e:
            make()
        assert "dgl" not in str(e.value)
    with pytest.raises(NotImplementedError, match="ConvLSTMHPX"):
        dlwpbench.ConvLSTM(mesh="healpix")
    # padding pairs
    assert conv_ops._pad_codes("healpix") == (2, 2) and conv_ops._pad_codes(("healpix", "healpix")) == (2, 2)
    for bad in (("healpix", "zeros"), ("circular", "healpix")):
        with pytest.raises(ValueError, match="both axes"):
            conv_ops._pad_codes(bad)
        with pytest.raises(ValueError, match="both axes"):
            conv_ops.Conv3x3(4, 4, pad_modes=bad)
    assert conv_ops.Conv3x3(4, 4, pad_modes=("healpix", "healpix")).pad_modes == ("healpix", "healpix")
    with pytest.raises(ValueError):
        conv_ops.hpx_fold_table(1)


def test_no_cpu_path():
    from dlwp_benchmark_amd import dlwpbench, lib as L
    net = dlwpbench.ConvLSTMHPX(constant_channels=0, prescribed_channels=0, prognostic_channels=2, hidden_sizes=[4], device="cpu")
    with pytest.raises(L.DlwpError):
        net(prognostic=torch.zeros(1, 3, 2, 12, 4, 4))


def err(h):
    return h.dlwp_last_error().decode()


def test_entry_points_refuse_bad_healpix_arguments(h):
    HP = 2
    # fwd: x1, x2, wimg, bias, y1, y2, B, H, W, C1, C2, N1, N2, pad_h, pad_w, act, stream
    fwd = lambda B, H, W, ph, pw: h.dlwp_conv3x3_fwd(FAKE, None, FAKE, None, FAKE, None, B, H, W, 4, 0, 4, 0, ph, pw, 0, None)      # noqa: E731
    cellf = lambda B, H, W, ph, pw: h.dlwp_convlstm_cell_fwd(FAKE, None, FAKE, None, None, FAKE, FAKE, None, B, H, W, 4, 4, ph, pw,  # noqa: E731
                                                             None)
    wgrad = lambda B, H, W, ph, pw: h.dlwp_conv3x3_wgrad(FAKE, None, FAKE, FAKE, FAKE, None, B, H, W, 4, 0, 4, ph, pw, None)         # noqa: E731
    for fn in (fwd, cellf, wgrad):
        for ph, pw in ((HP, 0), (1, HP)):
            assert fn(12, 8, 8, ph, pw) < 0
            assert "both axes" in err(h)
        for B, H, W in ((11, 8, 8), (1, 8, 8), (12, 8, 16), (12, 1, 1)):
            assert fn(B, H, W, HP, HP) < 0
            assert "12 square faces" in err(h)
        assert fn(12, 8, 8, 3, 3) < 0 and "padding" in err(h)
    # input gradient: dz, wimg, table, ws, g1, g2, B, n, Cout, C1, C2, stream
    dgrad = h.dlwp_conv3x3_hpx_dgrad
    assert dgrad(FAKE, FAKE, None, FAKE, FAKE, None, 12, 8, 4, 4, 0, None) < 0 and "NULL" in err(h)
    assert dgrad(FAKE, FAKE, FAKE, FAKE, None, None, 12, 8, 4, 4, 0, None) < 0 and "NULL" in err(h)
    assert dgrad(FAKE, FAKE, FAKE, FAKE, FAKE, None, 13, 8, 4, 4, 0, None) < 0 and "12 square faces" in err(h)
    assert dgrad(FAKE, FAKE, FAKE, FAKE, FAKE, None, 12, 1, 4, 4, 0, None) < 0 and "12 square faces" in err(h)
    assert dgrad(FAKE, FAKE, FAKE, FAKE, FAKE, None, 12, 8, 0, 4, 0, None) < 0 and "bad shape" in err(h)
    assert dgrad(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 12, 8, 4, 4, 0, None) < 0 and "destination" in err(h)
    assert h.dlwp_conv3x3_hpx_dgrad_ws_floats(24, 8, 5) == 24 * 10 * 10 * 5
    assert h.dlwp_conv3x3_hpx_dgrad_ws_floats(10, 8, 5) < 0 and h.dlwp_conv3x3_hpx_dgrad_ws_floats(12, 1, 5) < 0
    assert h.dlwp_hpx_halo_sources(0, FAKE) < 0 and h.dlwp_hpx_halo_sources(4, None) < 0
