"""ConvLSTM on a CPU-only box: the plain-torch helper (tests/convlstm_ref.py) against the golden vectors of the reference's own
classes (tests/golden/make_convlstm_golden.py), the model classes' interface, and the host-side argument validation of the
dlwp_conv3x3_* / dlwp_convlstm_* entry points.

Bounds (all `rel_gap`: max |difference| relative to the max norm of the reference array):
* helper in float64 vs the golden fp32 arrays: twice the gap the fixture stores for that array -- the helper's float64 result
  IS the reference's float64 result up to 1e-12 if it restates the model correctly, and the stored gap is the reference's own
  fp32-vs-float64 distance (a floor of 1e-12 for an array whose stored gap is exactly zero);
* helper in fp32: 1e-5 for output and loss, 5e-5 for every gradient tensor -- what the golden script asserts of the reference.
"""
import os

import numpy as np
import pytest
import torch

from convlstm_ref import CASES, GOLDEN, load_case, rel_gap, run_case

HERE = os.path.dirname(os.path.abspath(__file__))


def golden(kind):
    return np.load(os.path.join(HERE, "golden", GOLDEN[kind]))


@pytest.mark.parametrize("name", list(CASES))
def test_helper_matches_the_reference(name):
    kind, cfg, B, T, roll = CASES[name]
    params, inputs, target, y, loss, grads, gaps = load_case(golden(kind), name)
    assert inputs[{"ns": "x", "dlwp": "prognostic"}[kind]].shape[:2] == (B, T)
    assert set(grads) == set(params) and len(params) >= 8
    for dtype, bound in ((torch.float64, None), (torch.float32, (1e-5, 5e-5))):
        hy, hloss, hg = run_case(kind, params, inputs, target, dtype, **roll)
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


def test_registries_export_convlstm():
    from dlwp_benchmark_amd import dlwpbench, nsbench
    assert "ConvLSTM" in nsbench.__all__ and "ConvLSTM" in dlwpbench.__all__
    assert nsbench.ConvLSTM is not dlwpbench.ConvLSTM


@pytest.mark.parametrize("name", list(CASES))
def test_cpu_built_model_has_the_golden_keys_and_shapes(name):
    from dlwp_benchmark_amd import dlwpbench, nsbench
    kind, cfg, B, T, roll = CASES[name]
    params = load_case(golden(kind), name)[0]
    cls = nsbench.ConvLSTM if kind == "ns" else dlwpbench.ConvLSTM
    net = cls(batch_size=B, device=torch.device("cpu"), type="ConvLSTM", name="convlstm", **cfg)
    sd = net.state_dict()
    assert list(sd) == list(params)                      # same keys in the same order
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in params.items()}
    net.load_state_dict(params, strict=True)
    assert all(torch.equal(net.state_dict()[k], params[k]) for k in params)


def test_unequal_hidden_sizes_and_healpix_are_refused():
    from dlwp_benchmark_amd import dlwpbench, nsbench
    with pytest.raises(ValueError, match="equal"):
        nsbench.ConvLSTM(batch_size=2, input_size=1, hidden_sizes=[8, 16], height=8, width=8, device="cpu")
    with pytest.raises(ValueError, match="equal"):
        dlwpbench.ConvLSTM(hidden_sizes=[8, 16])
    with pytest.raises(NotImplementedError):
        dlwpbench.ConvLSTM(mesh="healpix")
    net = nsbench.ConvLSTM(batch_size=1, input_size=1, hidden_sizes=[4], height=8, width=8, device="cpu")
    with pytest.raises(ValueError, match="teacher_forcing_steps"):
        net(torch.zeros(1, 3, 1, 8, 8), teacher_forcing_steps=0)


def test_no_cpu_path():
    """the model runs on the library only: a CPU tensor is refused, never computed on by torch"""
    from dlwp_benchmark_amd import lib as L, nsbench
    net = nsbench.ConvLSTM(batch_size=1, input_size=1, hidden_sizes=[4], height=8, width=8, device="cpu")
    with pytest.raises(L.DlwpError):
        net(torch.zeros(1, 3, 1, 8, 8), teacher_forcing_steps=2)


FAKE = 0x1000      # a non-NULL pointer value: validation must fail before it is ever dereferenced


@pytest.fixture(scope="module")
def h():
    from dlwp_benchmark_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def err(h):
    return h.dlwp_last_error().decode()


def test_conv_entry_points_reject_bad_arguments(h):
    # fwd: x1, x2, wimg, bias, y1, y2, B, H, W, C1, C2, N1, N2, pad_h, pad_w, act, stream
    assert h.dlwp_conv3x3_fwd(None, None, FAKE, None, FAKE, None, 1, 8, 8, 4, 0, 4, 0, 0, 0, 0, None) < 0
    assert "NULL" in err(h)
    assert h.dlwp_conv3x3_fwd(FAKE, None, FAKE, None, None, None, 1, 8, 8, 4, 0, 4, 0, 0, 0, 0, None) < 0
    assert h.dlwp_conv3x3_fwd(FAKE, None, FAKE, None, FAKE, None, 1, 0, 8, 4, 0, 4, 0, 0, 0, 0, None) < 0
    assert "bad shape" in err(h)
    assert h.dlwp_conv3x3_fwd(FAKE, None, FAKE, None, FAKE, None, 1, 8, 8, 0, 0, 4, 0, 0, 0, 0, None) < 0
    assert h.dlwp_conv3x3_fwd(FAKE, None, FAKE, None, FAKE, None, 1, 8, 8, 4, 3, 4, 0, 0, 0, 0, None) < 0      # C2 without x2
    assert "second input" in err(h)
    assert h.dlwp_conv3x3_fwd(FAKE, None, FAKE, None, FAKE, None, 1, 8, 8, 4, 0, 4, 0, 2, 0, 0, None) < 0
    assert "padding" in err(h)
    assert h.dlwp_conv3x3_fwd(FAKE, None, FAKE, None, FAKE, None, 1, 8, 8, 4, 0, 4, 0, 0, 1, 3, None) < 0
    assert "activation" in err(h)
    # pack / image size
    assert h.dlwp_conv3x3_image_floats(0, 4, 0) < 0 and h.dlwp_conv3x3_image_floats(4, 4, 3) < 0
    assert h.dlwp_conv3x3_image_floats(8, 6, 1) < 0                   # a cell weight has 4 * hidden output channels
    assert h.dlwp_conv3x3_image_floats(5, 5, 0) == 9 * 16 * 16 and h.dlwp_conv3x3_image_floats(114, 228, 1) == 4 * 8 * 9 * 16 * 64
    assert h.dlwp_conv3x3_pack(None, FAKE, 4, 4, 0, None) < 0
    assert h.dlwp_conv3x3_pack(FAKE, FAKE, 4, 4, 7, None) < 0
    assert "kind" in err(h)
    assert h.dlwp_conv3x3_pack(FAKE, FAKE, 4, -1, 0, None) < 0
    # cell forward: x, h_prev, wimg, bias, c_prev, h, c, gates, B, H, W, Cx, hid, pad_h, pad_w, stream
    assert h.dlwp_convlstm_cell_fwd(FAKE, None, FAKE, None, None, None, FAKE, None, 1, 8, 8, 4, 4, 1, 1, None) < 0
    assert "NULL" in err(h)
    assert h.dlwp_convlstm_cell_fwd(FAKE, None, FAKE, None, None, FAKE, FAKE, None, 1, 8, 8, 4, 0, 1, 1, None) < 0
    assert h.dlwp_convlstm_cell_fwd(FAKE, None, FAKE, None, None, FAKE, FAKE, None, 1, 8, 8, 4, 4, 1, -1, None) < 0
    assert "padding" in err(h)
    # gate backward: dh, dc, gates, c_prev, c, dz, dc_prev, npix, hid, stream
    assert h.dlwp_convlstm_gate_bwd(None, None, FAKE, None, FAKE, FAKE, FAKE, 64, 4, None) < 0
    assert h.dlwp_convlstm_gate_bwd(FAKE, None, FAKE, None, FAKE, FAKE, FAKE, 0, 4, None) < 0
    assert h.dlwp_conv3x3_act_bwd(FAKE, FAKE, FAKE, 16, 0, None) < 0
    assert "activation" in err(h)
    assert h.dlwp_conv3x3_act_bwd(FAKE, None, FAKE, 16, 1, None) < 0
    # weight gradient: x1, x2, dz, ws, gw, gb, B, H, W, C1, C2, Cout, pad_h, pad_w, stream
    assert h.dlwp_conv3x3_wgrad(FAKE, None, FAKE, None, FAKE, None, 1, 8, 8, 4, 0, 4, 0, 0, None) < 0
    assert "NULL" in err(h)
    assert h.dlwp_conv3x3_wgrad(FAKE, None, FAKE, FAKE, FAKE, None, 1, 8, 8, 4, 0, 0, 0, 0, None) < 0
    assert h.dlwp_conv3x3_wgrad(FAKE, None, FAKE, FAKE, FAKE, None, 1, 8, 8, 4, 0, 4, 0, 5, None) < 0
    assert h.dlwp_conv3x3_wgrad_ws_floats(1, 8, 8, 0, 4) < 0
    assert h.dlwp_conv3x3_wgrad_ws_floats(1, 8, 8, 4, 4) == 9 * 16 * 64
