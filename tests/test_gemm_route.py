"""The routes of the token GEMM entries (csrc/gemm_route.h: dlwp_gemm_route) on the CPU: dlwp_gemm_route_name asks the route function
and the name formatter the launches use, reads host state only (shape, leading dimensions, alignments, precision and tile256 modes,
tuning knobs) and needs no device.  The cases, knobs, fuzz draws and expected accounting names are those of test_gpu_gemm_paths.py
(imported, not copied): what that test asserts a GPU launched, this one asserts the route names.  Arrays are taken to lie at 256-byte
aligned addresses, as the allocator's do.  No case is skipped."""
import ctypes as C
import os

import pytest

from test_gpu_gemm_paths import (CASES, ENTRY_PLAIN, FUZZ_FAMILIES, REDUCE, WGRAD_CASES, fuzz_draw, knobs, product_call, queue_products,
                                 route_of, wgrad_call)

ADDR = 1 << 20


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from dlwp_benchmark_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def product_route(M, N, K, layout, epi, knob=None, mode="bf16", arrays=None, cpad=8, ldpad=0, queue=False, **_):
    from dlwp_benchmark_amd import lib as L
    call = product_call(M, N, K, layout, epi, *([arrays] if arrays else []), cpad=cpad, ldpad=ldpad, queue=queue)
    e = call["e"]
    with L.gemm_precision(mode), knobs(**(knob or {})):
        return route_of(call, A=ADDR, B=2 * ADDR, C=3 * ADDR, bias=4 * ADDR if e["bias"] else 0, preact=5 * ADDR if e["pre"] else 0,
                        residual=6 * ADDR if e["res"] else 0)


def fields(plan):
    return dict(kv.split("=") for kv in plan.split())


def wgrad_route(M, N, K, acc, rowsum, knob=None, **_):
    from dlwp_benchmark_amd import lib as L
    with L.gemm_precision("bf16"), knobs(**(knob or {})):
        return route_of(wgrad_call(M, N, K, acc, rowsum), A=ADDR, B=2 * ADDR, C=3 * ADDR)


@pytest.mark.parametrize("case", list(CASES))
def test_route_names_the_expected_instantiation(case):
    M, N, K, layout, epi, expect, knob, kw = CASES[case]
    names, plan = product_route(M, N, K, layout, epi, knob=knob, **kw)
    assert names == expect, (names, plan)
    assert fields(plan)["splits"] == "1" and fields(plan)["zero"] == "0", plan      # an epilogue, or K under 256: the entry does not cut K


@pytest.mark.parametrize("case", list(WGRAD_CASES))
def test_route_names_the_expected_weight_gradient_kernels(case):
    M, N, K, acc, rowsum, expect, knob, _ = WGRAD_CASES[case]
    names, plan = wgrad_route(M, N, K, acc, rowsum, knob=knob)
    assert names == sorted(expect), (names, plan)
    assert int(fields(plan)["splits"]) > 1 and fields(plan)["zero"] == str(int(not acc)), plan      # the entry cuts K and zeroes C unless it accumulates


@pytest.mark.parametrize("family", FUZZ_FAMILIES)
def test_route_names_of_the_fuzz_draws(family):
    for seed in range(12):
        kind, kw = fuzz_draw(family, seed)
        names, plan = (product_route if kind == "product" else wgrad_route)(**kw)
        assert names == kw["expect"], (seed, names, plan)


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_group_queue_parks_the_small_products(mode):
    """test_gemm_group_queue: with a queue open the four small products wait for gemm_group_any_kernel, the 5 GFLOP one launches on its own
    kernel; with no queue open each names a kernel of its own"""
    grp = f"gemm_group_any_kernel<{'true' if mode == 'bf16' else 'false'}>"
    single = f"gemm_kernel<true, true, 3, 1, {'true' if mode == 'bf16' else 'false'}, 0>"
    prods = queue_products(mode)
    for i, (M, N, K, tA, tB, da, db, epi) in enumerate(prods):
        layout = "nt"[tA] + "nt"[tB]
        names, _ = product_route(M, N, K, layout, epi, mode=mode, arrays=(da, db), queue=True)
        assert names == ([grp] if i < 4 else [single]), (i, names)
        names, _ = product_route(M, N, K, layout, epi, mode=mode, arrays=(da, db), queue=False)
        assert len(names) == 1 and names[0].startswith("gemm_kernel<"), (i, names)


def test_plan_of_a_sliced_weight_gradient():
    """AFNO's fc1 weight gradient (3072 x 768 over 16200 tokens): the entry cuts K for 512 workgroups, the TN kernel plans its own slices"""
    M, N, K, acc, rowsum, expect, knob, _ = WGRAD_CASES["tn_default_afno_fc1_gw"]
    names, plan = wgrad_route(M, N, K, acc, rowsum, knob=knob)
    f = fields(plan)
    assert names == sorted(expect)
    assert int(f["kchunk"]) % 32 == 0 and int(f["splits"]) == -(-K // int(f["kchunk"])) > 1
    assert int(f["kernel_kchunk"]) % 32 == 0 and f["grid"] == f"{24 * 6},{-(-K // int(f['kernel_kchunk']))}" and f["lds"] == str(32768)


def test_bad_arguments_are_refused():
    from dlwp_benchmark_amd import lib as L
    lib = L.load()
    buf = C.create_string_buffer(256)
    addr = (C.c_ulonglong * 6)(ADDR, 2 * ADDR, 3 * ADDR, 0, 0, 0)
    ok = lambda *a: lib.dlwp_gemm_route_name(*a)      # noqa: E731
    assert ok(ENTRY_PLAIN, 64, 64, 64, 64, 64, 64, 0, 1, 1, None, 0, addr, 0, 0, 0, buf, 256) == 0
    assert ok(4, 64, 64, 64, 64, 64, 64, 0, 1, 1, None, 0, addr, 0, 0, 0, buf, 256) == -1 and b"gemm_route_name" in lib.dlwp_last_error()
    assert ok(ENTRY_PLAIN, 0, 64, 64, 64, 64, 64, 0, 1, 1, None, 0, addr, 0, 0, 0, buf, 256) == -1
    assert ok(ENTRY_PLAIN, 64, 64, 64, 64, 64, 64, 0, 1, 1, None, 16, addr, 0, 0, 0, buf, 256) == -1 and b"dtypes" in lib.dlwp_last_error()
    assert ok(ENTRY_PLAIN, 64, 64, 64, 64, 64, 64, 0, 1, 1, None, 0, None, 0, 0, 0, buf, 256) == -1
    assert ok(ENTRY_PLAIN, 64, 64, 64, 64, 64, 64, 0, 1, 1, None, 0, addr, 0, 0, 0, None, 256) == -1
    assert ok(3, 64, 64, 64, 64, 64, 64, 1, 0, 1, None, 0, addr, 0, 0, 0, buf, 256) == -1 and b"per_product" in lib.dlwp_last_error()
    addr[2] = 0
    assert ok(ENTRY_PLAIN, 64, 64, 64, 64, 64, 64, 0, 1, 1, None, 0, addr, 0, 0, 0, buf, 256) == -1 and b"must not be 0" in lib.dlwp_last_error()
