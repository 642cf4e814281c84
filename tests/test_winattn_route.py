"""The routes of the window-attention entries (csrc/winattn_route.h; dlwp_winattn_route_fwd / _bwd in csrc/winattn_small.hip) on the
CPU: dlwp_window_attn_route_name asks the routing functions and the name formatter the launches use, reads host state only (shape,
precision mode, tuning knobs) and needs no device.  The cases, knobs and expected accounting names are those of
test_gpu_winattn_paths.py (imported, not copied): what that test asserts a GPU launched, this one asserts the route names.

The slab fold (winattn_fold_kernel) and the table packing (pack_table_kernel) are launched for the caller's buffers (slab != NULL,
a packed table), not by a route: they are left out of the expected lists.  No case is skipped."""
import ctypes as C
import os

import pytest

from test_gpu_winattn_paths import CASES, E_UNSUPPORTED, FOLD, PACK, UNSUPPORTED, fuzz_case, knobs

TOKENS, FILL, IO_BF16 = 1, 2, 4             # layout bits (include/dlwpmi.h: dlwp_window_attn_route_name)


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from dlwp_benchmark_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def route_names(direction, layout, N, d, TB, pairs, qr=None):
    """(0, sorted names) of the launch, or (error code, the refusal's text)"""
    from dlwp_benchmark_amd import lib as L
    lib = L.load()
    buf = C.create_string_buffer(256)
    lo, hi = qr or (0, N)
    rc = lib.dlwp_window_attn_route_name(direction, layout, N, d, TB, pairs, lo, hi, buf, len(buf))
    return (rc, sorted(buf.value.decode().split(";"))) if rc == 0 else (rc, lib.dlwp_last_error().decode())


def check_case(c):
    layout = {"qrange": 0, "wide": 0, "bf16": IO_BF16, "tokens": TOKENS | FILL | (IO_BF16 if c["io"] else 0), "tokens_bwd": TOKENS}[c["entry"]]
    shape = (c["N"], c["d"], c["TB"], c["M"] * c["ntypes"] * c["heads"], c["qr"])
    with knobs(c["mode"], c["knob"]):
        fwd, bwd = route_names(0, layout, *shape), route_names(1, layout, *shape)
    if c["entry"] == "wide":                # head dims above 64 have no fused kernel: window_attention_core takes the GEMM form
        assert fwd[0] == bwd[0] == E_UNSUPPORTED and "head_dim" in fwd[1] and "head_dim" in bwd[1], (fwd, bwd)
        return
    if c["entry"] != "tokens_bwd":          # (window-layout operands with token-layout gradients: a backward entry only)
        assert fwd == (0, [n for n in c["fwd"] if n != PACK]), (fwd, c["fwd"])
    assert bwd == (0, [n for n in c["bwd"] if n not in (FOLD, PACK)]), (bwd, c["bwd"])
    if layout == 0:                         # the tiled backward reads rows that only the tiled forward writes
        assert fwd[1][0].startswith("winattn_fwd_kernel") == bwd[1][0].startswith("winattn_bwd_"), (fwd, bwd)


@pytest.mark.parametrize("cid", list(CASES))
def test_route_names_the_expected_instantiations(cid):
    check_case(CASES[cid])


@pytest.mark.parametrize("family", ["tiled", "wave", "lds2", "onepass", "tok_fwd"])
def test_route_names_of_the_fuzz_draws(family):
    for seed in range(10):
        check_case(fuzz_case(family, seed))


@pytest.mark.parametrize("what", list(UNSUPPORTED))
def test_unsupported_shapes_are_refused_by_the_route(what):
    """the refusals of test_unsupported_launches_nothing: the route answers DLWP_E_UNSUPPORTED with the entry's text"""
    N, d, H, B_ = UNSUPPORTED[what]
    direction = 1 if what.startswith("bwd") else 0
    layout = IO_BF16 if "_bf16_" in what else TOKENS | FILL if "_tokens_" in what else 0
    with knobs("fp32" if what.endswith("fp32_mode") else "bf16", {}):
        rc, text = route_names(direction, layout, N, d, 169, B_ * H)
    assert rc == E_UNSUPPORTED, (rc, text)
    entry = {"fwd_bf16": "window_attn_fwd_bf16", "fwd_d65": "head_dim above 64", "fwd_tokens": "window_attn_fwd_tokens",
             "bwd_tokens": "window_attn_bwd_tokens"}[next(k for k in ("fwd_bf16", "fwd_d65", "fwd_tokens", "bwd_tokens") if what.startswith(k))]
    assert entry in text and f"(N {N}, d {d}" in text, text


def test_supported_queries_follow_the_routes():
    """the three *_supported entries answer what the routes answer (one rule, asked from Python and from the launch)"""
    from dlwp_benchmark_amd import lib as L
    lib = L.load()
    for mode in ("fp32", "bf16"):
        for knob in ({}, {"WINATTN_TILED": 1}, {"WINATTN_BWD2PASS": 1}, {"WINATTN_BWD1P_SMALL": 1}, {"WINATTN_NOLDS": 1}):
            with knobs(mode, knob):
                for N in (16, 49, 64, 65, 98, 128, 129):
                    for d in (8, 10, 16, 24, 32, 36, 48, 52):
                        for pairs in (1023, 1024, 2047, 2048):
                            for TB in (169, 2548):
                                ok = lambda direction, layout: route_names(direction, layout, N, d, TB, pairs)[0] == 0      # noqa: E731
                                assert lib.dlwp_window_attn_io_bf16_supported(N, d, TB, pairs) == ok(0, IO_BF16) == ok(1, IO_BF16)
                                assert bool(lib.dlwp_window_attn_bwd_tokens_supported(N, d, TB)) == ok(1, TOKENS | FILL) == ok(1, TOKENS)
                                assert bool(lib.dlwp_window_attn_fwd_tokens_supported(N, d, pairs)) == ok(0, TOKENS | FILL)


def test_bad_arguments_are_refused():
    from dlwp_benchmark_amd import lib as L
    lib = L.load()
    buf = C.create_string_buffer(64)
    assert lib.dlwp_window_attn_route_name(0, 0, 49, 16, 169, 100, 10, 5, buf, 64) == -1 and b"query range" in lib.dlwp_last_error()
    assert lib.dlwp_window_attn_route_name(2, 0, 49, 16, 169, 100, 0, 49, buf, 64) == -1
    assert lib.dlwp_window_attn_route_name(0, 0, 49, 16, 169, 100, 0, 49, None, 64) == -1
