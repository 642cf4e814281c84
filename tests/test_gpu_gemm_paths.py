"""Every kernel the token GEMM entries (csrc/token_ops.hip: dlwp_gemm_mixed / dlwp_gemm_batched_mixed, routed by csrc/gemm_route.h) can
launch, each case pinned to the instantiation it must reach through lib.kernel_accounting (and to what dlwp_gemm_route_name answers for the
same call) and held to a float64 product of the bf16-rounded operands:
per output tile of the kernel under test (edge tiles reported on their own), with sentinel rows after M and sentinel columns between N
and ldc that must come back bit for bit, and bit-identical repeated launches wherever the kernel adds its K slices in a fixed order.

Case table (test_gemm_path[<case id>]; "default" = no knob, the dispatcher's own shape rules at a step shape):

    kernel instantiation                      cases
    gemm_glds_kernel<true, 32, 128>           glds_nt_kd32_n128, glds_nt_kd32_ragged_k, glds_nt_default_afno_fc1
    gemm_glds_kernel<true, 32, 96>            glds_nt_kd32_n96, glds_nt_default_swin_fc2
    gemm_glds_kernel<true, 64, 128>           glds_nt_kd64_n128
    gemm_glds_kernel<true, 64, 96>            glds_nt_kd64_n96, glds_nt_default_pangu_fc2
    gemm_glds_kernel<false, 32, 128>          glds_nn_kd32_n128, glds_nn_kd32_ragged_k, glds_nn_default_afno_fc2_gx
    gemm_glds_kernel<false, 32, 96>           glds_nn_kd32_n96
    gemm_glds_kernel<false, 64, 128>          glds_nn_kd64_n128
    gemm_glds_kernel<false, 64, 96>           glds_nn_kd64_n96, glds_nn_default_pangu_fc1_gx
    gemm_p8_kernel<true, true, true>          p8_nt_direct_wide_k64, p8_nt_direct_wide, p8_nt_default_afno_fc2
    gemm_p8_kernel<true, false, true>         p8_nn_direct_wide, p8_nn_default_afno_fc1_gx
    gemm_p8_kernel<true, true, false>         p8_nt_direct_narrow
    gemm_p8_kernel<true, false, false>        p8_nn_direct_narrow
    gemm_p8_kernel<false, true, false>        p8_nt_staged
    gemm_p8_kernel<false, false, false>       p8_nn_staged
    gemm_glds_tn_kernel<32> + slab reduce     tn_kd32_slab, tn_default_afno_fc1_gw
    gemm_glds_tn_kernel<64> + slab reduce     tn_kd64_slab_ragged_k
    gemm_glds_tn_kernel<32> (atomic)          tn_kd32_atomic
    gemm_glds_tn_kernel<64> (atomic)          tn_kd64_atomic_few_tiles, tn_default_pangu_gw
    gemm_p8_tn_kernel + slab reduce           p8tn_ragged_k, p8tn_edges, p8tn_fourcastnet_gw (forced: never taken by shape)
    gemm_kernel<true, true, 3, 1, false, 0>   generic_t1_fp32_arrays
    gemm_kernel<false, false, 3, 1, true, 0>  generic_t1_fp32_arrays_bf16_mode
    gemm_kernel<true, false, 3, 1, true, 3>   generic_t1_bf16_arrays_nn
    gemm_kernel<true, true, 3, 1, true, 3>    generic_t1_default_afno
    gemm_kernel<true, true, 3, 2, false, 0>   generic_t2_fp32_arrays
    gemm_kernel<true, true, 3, 2, true, 3>    generic_t2_default_bf16_arrays
    gemm_group_any_kernel<true> / <false>     test_gemm_group_queue[bf16] / [fp32]

test_fast_path_fuzz draws twelve products per family (glds, p8, glds_tn, p8_tn) inside the family's applicability region and asserts the
instantiation the draw must reach."""
import contextlib
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LAM = 0.5                  # soft-shrink threshold (exact in fp32)
PAD_ROWS = 3               # sentinel rows after row M of every output buffer
ACTS = {"gelu": 1, "relu": 2, "shrink": 3, "dgelu": 4, "drelu": 5, "dshrink": 6, "gelu_d": 7, "mul": 8}


@contextlib.contextmanager
def knobs(tile256=None, **kw):
    """tuning overrides (lib.set_tuning) and the 256 x 256 kernel mode for the body, released afterwards"""
    from dlwp_benchmark_amd import lib as L
    try:
        for k, v in kw.items():
            L.set_tuning(k, v)
        if tile256 is not None:
            L.set_gemm_tile256(tile256)
        yield
    finally:
        for k in kw:
            L.set_tuning(k, None)
        if tile256 is not None:
            L.set_gemm_tile256(0)


def gemm_names(fn):
    """the GEMM rows of the accounting of one eager call"""
    from dlwp_benchmark_amd import lib as L
    with L.kernel_accounting() as acc:
        fn()
        torch.cuda.synchronize()
    return sorted(r["name"] for r in acc.rows if r["name"].startswith("gemm"))


def tile_of(name):
    """output tile (rows, columns) of a kernel, from its accounting name"""
    if name.startswith("gemm_glds_kernel<"):
        return 128, int(name.split(",")[2].split(">")[0])
    if name.startswith(("gemm_p8_kernel<", "gemm_p8_tn_kernel")):
        return 256, 256
    if name.startswith("gemm_glds_tn_kernel<"):
        return 128, 128
    if name.startswith("gemm_kernel<"):
        t = int(name.split(",")[3])
        return 64 * t, 64 * t
    return 64, 64


def fp32_tol(K):
    # fp32 accumulation: the rounding errors of K partial sums grow like sqrt(K) against an output of unit scale; 2e-5 holds with a wide
    # margin up to K = 4096 (the LDS-DMA tests' bound), beyond that it widens with sqrt(K)
    return 2e-5 * max(1.0, math.sqrt(K / 4096))


def check_tiles(what, got, want, tile, tol, bf16_out):
    """Error per output tile of the kernel under test: max |got - want| over the tile against the tile's max |want| (floored at 1/16 of
    the whole output's, so that a corner tile of a few small elements is not held to a relative bound of its own).  A bf16 output may
    in addition differ by its own rounding, 2^-8 |want| per element (round to nearest); anything beyond that counts against tol."""
    want = want.double()
    err = (got.double() - want).abs()
    if bf16_out:
        err = (err - 2.0 ** -8 * want.abs()).clamp_min(0)
    M, N = want.shape
    tm, tn = tile
    mt, nt = -(-M // tm), -(-N // tn)

    def tilemax(t):
        p = torch.zeros(mt * tm, nt * tn, dtype=t.dtype, device=t.device)
        p[:M, :N] = t
        return p.view(mt, tm, nt, tn).amax(dim=(1, 3))
    floor = max(want.abs().max().item() / 16, 1e-30)
    r = (tilemax(err) / tilemax(want.abs()).clamp_min(floor)).cpu()
    em, en = M % tm != 0, N % tn != 0
    inner = r[:mt - em, :nt - en]
    edge = torch.cat([r[mt - 1, :].reshape(-1) if em else r.new_zeros(0), r[:, nt - 1].reshape(-1) if en else r.new_zeros(0)])
    worst = lambda t: f"{t.max().item():.3g}" if t.numel() else "-"      # noqa: E731
    assert r.max().item() <= tol, (f"{what}: tile error {worst(r)} > {tol:.3g} (interior tiles {worst(inner)}, edge tiles {worst(edge)}; "
                                   f"worst tile {divmod(int(r.argmax()), nt)} of {mt} x {nt} tiles {tm} x {tn})")


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def guarded(M, N, ldc, dtype, g, cuda):
    """[M + PAD_ROWS][ldc] buffer of random values: [:M, :N] the output, the rest sentinels"""
    return torch.randn(M + PAD_ROWS, ldc, generator=g).to(cuda).to(dtype)


def check_guards(what, buf, before, M, N):
    assert torch.equal(bits(buf[M:]), bits(before[M:])), f"{what}: rows after M were written"
    assert torch.equal(bits(buf[:M, N:]), bits(before[:M, N:])), f"{what}: columns between N and ldc were written"


def gelu_d(v):
    """GELU'(v) of the exact (erf) GELU"""
    return 0.5 * (1 + torch.erf(v / math.sqrt(2))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)


def parse_epi(epi):
    toks = set(epi.split("+")) if epi else set()
    act = [ACTS[t] for t in toks if t in ACTS]
    e = dict(bias="bias" in toks, act=act[0] if act else 0, pre="pre" in toks or "gelu_d" in toks,
             res="res16" if "res16" in toks else ("res32" if "res32" in toks else None), res_pre="respre" in toks,
             acc="acc" in toks, out=BF if "bf16out" in toks else torch.float32)
    assert not (e["acc"] and e["out"] == BF)
    assert e["act"] not in (4, 5, 6, 8) or (e["res"] and not e["pre"])
    return e


def epi_reference(prod, e, bias, res, c0):
    """(output, pre-activation output or None) of the epilogue on the float64 product"""
    v = prod + (bias.double() if e["bias"] else 0)
    r = res[:, :prod.shape[1]].double() if res is not None else None
    act, pre = e["act"], None
    if act in (4, 5, 6, 8):
        y = {4: lambda: v * gelu_d(r), 5: lambda: v * (r > 0), 6: lambda: v * (r.abs() > LAM), 8: lambda: v * r}[act]()
    else:
        if r is not None and e["res_pre"]:
            v = v + r
        pre = gelu_d(v) if act == 7 else v
        y = {0: v, 1: F.gelu(v), 2: F.relu(v), 3: F.softshrink(v, LAM), 7: F.gelu(v)}[act]
        if r is not None and not e["res_pre"]:
            y = y + r
    if e["acc"]:
        y = y + c0
    return y, (pre if e["pre"] else None)


ENTRY_PLAIN, ENTRY_BATCHED = 0, 1      # dlwp_gemm_route_name's entry (include/dlwpmi.h)
FLAG_ACT, FLAG_ROWSUM, FLAG_ACC, FLAG_QUEUE = 1, 8, 32, 128
ADDRS = ("A", "B", "C", "bias", "preact", "residual")


def route_of(call, **addr):
    """(sorted accounting names, plan text) that dlwp_gemm_route_name answers for a call (product_call / wgrad_call) whose arrays lie at
    the given addresses (name = address; 0 or missing: absent).  Host state only."""
    from dlwp_benchmark_amd import lib as L
    buf = ctypes.create_string_buffer(512)
    a = (ctypes.c_ulonglong * 6)(*[addr.get(k) or 0 for k in ADDRS])
    L.check(L.load().dlwp_gemm_route_name(call["entry"], call["M"], call["N"], call["K"], call["lda"], call["ldb"], call["ldc"], call["tA"],
                                          call["tB"], 1, None, call["dt"], a, call["flags"], 0, 0, buf, len(buf)))
    names, plan = buf.value.decode().split("|")
    return sorted(names.split(";")), plan


def product_call(M, N, K, layout, epi, arrays=(BF, BF), cpad=8, ldpad=0, queue=False):
    """the call arguments run_product makes for a product (layout flags, leading dimensions, storage mask, route flags) and the parsed
    epilogue under "e"; entry: dlwp_gemm_batched_mixed with one batch"""
    e = parse_epi(epi)
    tA, tB = int(layout[0] == "t"), int(layout[1] == "t")
    dt = (1 if arrays[0] == BF else 0) | (2 if arrays[1] == BF else 0) | (4 if e["out"] == BF else 0) | (8 if e["res"] == "res16" else 0)
    flags = (FLAG_ACT if e["act"] else 0) | (FLAG_ACC if e["acc"] else 0) | (FLAG_QUEUE if queue else 0)
    return dict(entry=ENTRY_BATCHED, M=M, N=N, K=K, tA=tA, tB=tB, lda=(M if tA else K) + ldpad, ldb=(K if tB else N) + ldpad,
                ldc=-(-N // 8) * 8 + cpad, dt=dt, flags=flags, e=e, arrays=arrays)


def wgrad_call(M, N, K, acc, rowsum):
    """the call arguments run_wgrad makes: dlwp_gemm_mixed with transA, both operands bf16 arrays"""
    return dict(entry=ENTRY_PLAIN, M=M, N=N, K=K, tA=1, tB=0, lda=M, ldb=N, ldc=N + 8, dt=3,
                flags=(FLAG_ACC if acc else 0) | (FLAG_ROWSUM if rowsum else 0))


def ptrs(**tensors):
    return {k: (v.data_ptr() if v is not None else 0) for k, v in tensors.items()}


def run_product(cuda, M, N, K, layout, epi, expect, seed, knob=None, mode="bf16", arrays=(BF, BF), cpad=8, ldpad=0, reps=1):
    """C (+)= epilogue(op(A) op(B)) through dlwp_gemm_batched_mixed with layout "nt" (y = x W^T), "nn" (gx = g W) or "tn"
    (A given as [K][M]); asserts the launched kernels (and that the route names them), the tile-local error of every output and the
    guard regions."""
    from dlwp_benchmark_amd import lib as L
    from dlwp_benchmark_amd.token_ops import _gemm_batched
    call = product_call(M, N, K, layout, epi, arrays, cpad, ldpad)
    e, tA, tB, lda, ldb, ldc = (call[k] for k in ("e", "tA", "tB", "lda", "ldb", "ldc"))
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(K if tA else M, lda, generator=g).to(cuda).to(arrays[0])
    B = (torch.randn(N if tB else K, ldb, generator=g) / math.sqrt(K)).to(cuda).to(arrays[1])
    opA = A[:, :M].double().T if tA else A[:, :K].double()
    opB = B[:, :K].double().T if tB else B[:, :N].double()
    if mode == "bf16":       # the matrix units read bf16-rounded operands whatever the array type
        opA, opB = opA.to(BF).double(), opB.to(BF).double()
    prod = opA @ opB
    bias = torch.randn(N, generator=g).to(cuda) if e["bias"] else None
    res = torch.randn(M, ldc, generator=g).to(cuda).to(BF if e["res"] == "res16" else torch.float32) if e["res"] else None
    C0 = guarded(M, N, ldc, e["out"], g, cuda)
    P0 = guarded(M, N, ldc, e["out"], g, cuda) if e["pre"] else None
    want, pre_want = epi_reference(prod, e, bias, res, C0[:M, :N].double())
    outs = []
    with L.gemm_precision(mode), knobs(**(knob or {})):
        for rep in range(reps):
            C = C0.clone()
            P = P0.clone() if P0 is not None else None

            def launch():
                _gemm_batched(A, B, C, M, N, K, lda, ldb, ldc, tA, tB, bias=bias, act=e["act"], act_param=LAM, preact=P, residual=res,
                              res_pre=int(e["res_pre"]), accumulate=int(e["acc"]))
            names = gemm_names(launch)
            assert names == expect, (names, expect)
            routed = route_of(call, **ptrs(A=A, B=B, C=C, bias=bias, preact=P, residual=res))
            assert routed[0] == names, (routed, names)
            outs.append((C, P))
    tile = tile_of(expect[0])
    tol = fp32_tol(K)
    C, P = outs[0]
    check_guards("C", C, C0, M, N)
    check_tiles("C", C[:M, :N], want, tile, tol, e["out"] == BF)
    if P is not None:
        check_guards("preact", P, P0, M, N)
        check_tiles("preact", P[:M, :N], pre_want, tile, tol, e["out"] == BF)
    for Cr, Pr in outs[1:]:
        assert torch.equal(bits(Cr), bits(C)), "repeated launch differs"
        if P is not None:
            assert torch.equal(bits(Pr), bits(P)), "repeated launch differs (preact)"


def run_wgrad(cuda, M, N, K, acc, rowsum, expect, seed, knob=None, reps=1):
    """gW (+)= g^T x with both operands bf16 arrays [K][M], [K][N] (dlwp_gemm_mixed, transA): the weight-gradient kernels, with the bias
    gradient (row sums of g^T) as a by-product; guard regions around gW and the bias gradient"""
    from dlwp_benchmark_amd import lib as L
    from dlwp_benchmark_amd.token_ops import _gemm
    gen = torch.Generator().manual_seed(seed)
    call = wgrad_call(M, N, K, acc, rowsum)
    ldc = call["ldc"]
    gm = torch.randn(K, M, generator=gen).to(cuda).to(BF)
    x = torch.randn(K, N, generator=gen).to(cuda).to(BF)
    W0 = guarded(M, N, ldc, torch.float32, gen, cuda)
    b0 = torch.randn(M + 8, generator=gen).to(cuda) if rowsum else None
    want = gm.double().T @ x.double() + (W0[:M, :N].double() if acc else 0)
    outs = []
    with L.gemm_precision("bf16"), knobs(**(knob or {})):
        for _ in range(reps):
            W = W0.clone()
            b = b0.clone() if rowsum else None
            names = gemm_names(lambda: _gemm(gm, x, W, M, N, K, M, N, ldc, 1, 0, accumulate=int(acc), rowsum=b))
            assert names == expect, (names, expect)
            routed = route_of(call, **ptrs(A=gm, B=x, C=W))
            assert routed[0] == names, (routed, names)
            outs.append((W, b))
    W, b = outs[0]
    check_guards("gW", W, W0, M, N)
    check_tiles("gW", W[:M, :N], want, tile_of(expect[0]), fp32_tol(K), False)
    if rowsum:
        assert torch.equal(b[M:], b0[M:]), "bias gradient written past M"
        want_b = b0[:M].double() + gm.double().sum(0)
        assert ((b[:M].double() - want_b).abs().max() / want_b.abs().max()).item() <= fp32_tol(K)
    for Wr, _ in outs[1:]:
        assert torch.equal(bits(Wr), bits(W)), "repeated launch differs"


FORCE = {"GEMM_GLDS_FORCE": 1}
P8 = dict(FORCE, tile256=1)
GLDS = "gemm_glds_kernel<{}, {}, {}>"
P8K = "gemm_p8_kernel<{}, {}, {}>"
REDUCE = "gemm_slab_reduce_kernel"
T, Fa = "true", "false"

# id: (M, N, K, layout, epilogue, [kernel names], knobs, extra keyword arguments).  Edge tiles: M and N = whole tiles + 1 / + (edge - 8)
# (N + 4 / + 8 where the layout needs N % 4 / N % 8); K at the family's minimum and ragged where it may be.
CASES = {
    # ---- 128 x (128 | 96) LDS-DMA kernels: forced down to small shapes (GEMM_GLDS_FORCE), K-step depth and tile width by knob
    "glds_nt_kd32_n128": (129, 132, 32, "nt", "bias+gelu+pre+bf16out", [GLDS.format(T, 32, 128)], FORCE, {}),
    "glds_nt_kd32_n96": (248, 192, 96, "nt", "bias+res32+acc", [GLDS.format(T, 32, 96)], dict(FORCE, GEMM_GLDS_N96=2), {}),
    "glds_nt_kd64_n128": (300, 248, 64, "nt", "bias+relu+pre+res16+respre", [GLDS.format(T, 64, 128)], dict(FORCE, GEMM_GLDS_KD=64), {}),
    "glds_nt_kd64_n96": (385, 288, 192, "nt", "bias+gelu_d+res32+bf16out", [GLDS.format(T, 64, 96)],
                         dict(FORCE, GEMM_GLDS_KD=64, GEMM_GLDS_N96=2), dict(ldpad=8)),
    "glds_nt_kd32_ragged_k": (1000, 380, 160, "nt", "shrink+pre+res32", [GLDS.format(T, 32, 128)], FORCE, {}),
    "glds_nn_kd32_n128": (129, 136, 32, "nn", "dgelu+res16+bf16out", [GLDS.format(Fa, 32, 128)], FORCE, {}),
    "glds_nn_kd32_n96": (248, 288, 96, "nn", "mul+res32", [GLDS.format(Fa, 32, 96)], dict(FORCE, GEMM_GLDS_N96=2), {}),
    "glds_nn_kd64_n128": (300, 248, 128, "nn", "bias+gelu+acc", [GLDS.format(Fa, 64, 128)], dict(FORCE, GEMM_GLDS_KD=64), dict(ldpad=8)),
    "glds_nn_kd64_n96": (257, 192, 64, "nn", "dshrink+res16+bf16out", [GLDS.format(Fa, 64, 96)],
                         dict(FORCE, GEMM_GLDS_KD=64, GEMM_GLDS_N96=2), {}),
    "glds_nn_kd32_ragged_k": (513, 520, 96, "nn", "bias+gelu_d+bf16out", [GLDS.format(Fa, 32, 128)], FORCE, {}),
    # by shape: AFNO 16200 x 3072 x 768 (fc1) and its input gradient through fc2, Swin C4 stage-2 fc2, Pangu C4 fc2 / fc1 input gradient
    "glds_nt_default_afno_fc1": (16200, 3072, 768, "nt", "bias+gelu_d+bf16out", [GLDS.format(T, 32, 128)], None, {}),
    "glds_nn_default_afno_fc2_gx": (16200, 3072, 768, "nn", "mul+res16+bf16out", [GLDS.format(Fa, 32, 128)], None, {}),
    "glds_nt_default_swin_fc2": (16384, 192, 768, "nt", "bias+res32", [GLDS.format(T, 32, 96)], None, {}),
    "glds_nt_default_pangu_fc2": (8192, 384, 1536, "nt", "bias+res32", [GLDS.format(T, 64, 96)], None, {}),
    "glds_nn_default_pangu_fc1_gx": (8192, 384, 1536, "nn", "dgelu+res16+bf16out", [GLDS.format(Fa, 64, 96)], None, {}),
    # ---- 256 x 256 two-group kernel: forced (set_gemm_tile256(1) + GEMM_GLDS_FORCE), register epilogue wide (128-byte rows) or narrow
    # (N % 8 != 0, ldc % 8 != 0), or the LDS-staged epilogue (GEMM_P8_STAGED); repeated launches must agree bit for bit
    "p8_nt_direct_wide_k64": (513, 264, 64, "nt", "bias+gelu_d+bf16out", [P8K.format(T, T, T)], P8, dict(reps=2)),
    "p8_nt_direct_wide": (504, 760, 192, "nt", "bias+relu+pre+res16+respre", [P8K.format(T, T, T)], P8, dict(reps=2)),
    "p8_nn_direct_wide": (300, 520, 128, "nn", "dgelu+res16+bf16out", [P8K.format(T, Fa, T)], P8, dict(reps=2)),
    "p8_nt_direct_narrow": (257, 260, 128, "nt", "bias+res32+acc", [P8K.format(T, T, Fa)], P8, dict(reps=2)),
    "p8_nn_direct_narrow": (520, 264, 256, "nn", "mul+res16+bf16out", [P8K.format(T, Fa, Fa)], P8, dict(reps=2, cpad=4)),
    "p8_nt_staged": (300, 300, 64, "nt", "bias+shrink+pre", [P8K.format(Fa, T, Fa)], dict(P8, GEMM_P8_STAGED=1), dict(reps=2)),
    "p8_nn_staged": (513, 264, 320, "nn", "drelu+res32", [P8K.format(Fa, Fa, Fa)], dict(P8, GEMM_P8_STAGED=1), dict(reps=2)),
    # by shape: AFNO fc2 16200 x 768 x 3072 and the fc1 input gradient of the same size (K >= 2048, 192 tiles = 75 % of a round)
    "p8_nt_default_afno_fc2": (16200, 768, 3072, "nt", "bias+res32", [P8K.format(T, T, T)], None, dict(reps=2)),
    "p8_nn_default_afno_fc1_gx": (16200, 768, 3072, "nn", "mul+res16+bf16out", [P8K.format(T, Fa, T)], None, {}),
    # ---- register-staged 64 T x 64 T kernel
    "generic_t1_fp32_arrays": (193, 130, 100, "nt", "bias+relu+pre+res32", ["gemm_kernel<true, true, 3, 1, false, 0>"], None,
                               dict(mode="fp32", arrays=(torch.float32, torch.float32))),
    "generic_t1_fp32_arrays_bf16_mode": (300, 200, 96, "tn", "acc", ["gemm_kernel<false, false, 3, 1, true, 0>"], None,
                                         dict(arrays=(torch.float32, torch.float32))),
    "generic_t1_bf16_arrays_nn": (200, 136, 72, "nn", "dgelu+res16+bf16out", ["gemm_kernel<true, false, 3, 1, true, 3>"], None, {}),
    "generic_t2_fp32_arrays": (2049, 1796, 68, "nt", "bias+gelu_d", ["gemm_kernel<true, true, 3, 2, false, 0>"], {"GEMM_TILE": 128},
                               dict(mode="fp32", arrays=(torch.float32, torch.float32))),
    # by shape: AFNO 721 x 1440's 18540 x 768 x 728 (K not a multiple of 32: no LDS-DMA kernel), and a bf16-array product with K >= 768
    # that the LDS-DMA kernels refuse (K % 32 != 0), where the 128 x 128 tile is taken
    "generic_t1_default_afno": (18540, 768, 728, "nt", "bias", ["gemm_kernel<true, true, 3, 1, true, 3>"], None, {}),
    "generic_t2_default_bf16_arrays": (8192, 768, 776, "nt", "bias+res32", ["gemm_kernel<true, true, 3, 2, true, 3>"], None, {}),
}

# id: (M, N, K, accumulate, row sums, [kernel names], knobs, repetitions).  M, N multiples of 8 (the kernels' rule); K = tokens, ragged.
WGRAD_CASES = {
    "tn_kd32_slab": (1032, 264, 1024, True, True, ["gemm_glds_tn_kernel<32>", REDUCE], {"GEMM_GLDS_TN_KD": 32}, 2),
    "tn_kd64_slab_ragged_k": (760, 776, 1027, False, False, ["gemm_glds_tn_kernel<64>", REDUCE], {"GEMM_GLDS_TN_KD": 64}, 2),
    "tn_kd32_atomic": (264, 1032, 2000, True, True, ["gemm_glds_tn_kernel<32>"], {"GEMM_TN_ATOMIC": 1, "GEMM_GLDS_TN_KD": 32}, 1),
    "tn_kd64_atomic_few_tiles": (264, 264, 1100, True, True, ["gemm_glds_tn_kernel<64>"], None, 1),
    # by shape: AFNO fc1 weight gradient 3072 x 768 over 16200 tokens (144 tiles: 32 deep, slab); Pangu 768 x 384 over 8192 (18 tiles:
    # 64 deep, float atomics)
    "tn_default_afno_fc1_gw": (3072, 768, 16200, True, True, ["gemm_glds_tn_kernel<32>", REDUCE], None, 2),
    "tn_default_pangu_gw": (768, 384, 8192, True, False, ["gemm_glds_tn_kernel<64>"], None, 1),
    # 256 x 256 weight-gradient kernel (set_gemm_tile256(1)): slices end inside a K-tile, edge tiles of 8 and 248
    "p8tn_ragged_k": (520, 264, 1027, True, True, ["gemm_p8_tn_kernel", REDUCE], {"tile256": 1}, 2),
    "p8tn_edges": (760, 504, 4100, False, False, ["gemm_p8_tn_kernel", REDUCE], {"tile256": 1}, 2),
    "p8tn_fourcastnet_gw": (768, 3072, 4100, True, True, ["gemm_p8_tn_kernel", REDUCE], {"tile256": 1}, 2),
}


@pytest.mark.parametrize("case", list(CASES))
def test_gemm_path(cuda, case):
    M, N, K, layout, epi, expect, knob, kw = CASES[case]
    run_product(cuda, M, N, K, layout, epi, expect, seed=sum(map(ord, case)), knob=knob, **kw)


@pytest.mark.parametrize("case", list(WGRAD_CASES))
def test_weight_gradient_path(cuda, case):
    M, N, K, acc, rowsum, expect, knob, reps = WGRAD_CASES[case]
    run_wgrad(cuda, M, N, K, acc, rowsum, expect, seed=sum(map(ord, case)), knob=knob, reps=reps)


def _draw_epi(rng, allow_acc=True):
    """a valid epilogue drawn at random; never the bare fp32 product (which the dispatcher may cut along K: float atomics)"""
    out16 = bool(rng.integers(0, 2))
    act = str(rng.choice(["", "gelu", "relu", "shrink", "dgelu", "drelu", "dshrink", "gelu_d", "mul"]))
    toks = [act] if act else []
    if act in ("dgelu", "drelu", "dshrink", "mul"):
        toks.append(str(rng.choice(["res16", "res32"])))
    else:
        if act == "gelu_d" or rng.integers(0, 2):
            toks.append("pre")
        if rng.integers(0, 2):
            toks.append(str(rng.choice(["res16", "res32"])))
            if rng.integers(0, 2):
                toks.append("respre")
    if rng.integers(0, 2):
        toks.append("bias")
    if out16:
        toks.append("bf16out")
    elif allow_acc and rng.integers(0, 2):
        toks.append("acc")
    if not out16 and not [t for t in toks if t != "acc"]:
        toks.append("bias")
    return "+".join(toks)


FUZZ_FAMILIES = ["glds", "p8", "glds_tn", "p8_tn"]


def fuzz_draw(family, seed):
    """the product test_fast_path_fuzz runs for (family, seed): ("product", keyword arguments of run_product) or ("wgrad", those of
    run_wgrad), the expected kernels among them"""
    rng = np.random.default_rng(7000 + 100 * FUZZ_FAMILIES.index(family) + seed)
    if family in ("glds", "p8"):
        nn = bool(rng.integers(0, 2))
        if family == "glds":
            kd, n96 = int(rng.choice([32, 64])), int(rng.choice([0, 2]))
            M = int(rng.integers(128, 700))
            N = 96 * int(rng.integers(1, 7)) if n96 and rng.integers(0, 2) else (8 if nn else 4) * int(rng.integers(16, 176))
            K = kd * int(rng.integers(1, 1024 // kd))            # a multiple of the forced depth (32: ragged against 64)
            gn = 96 if (n96 == 2 and N % 96 == 0) else 128
            expect = [GLDS.format(Fa if nn else T, kd, gn)]
            knob = dict(FORCE, GEMM_GLDS_KD=kd, GEMM_GLDS_N96=n96)
            cpad = 8
        else:
            staged = bool(rng.integers(0, 2))
            M = int(rng.integers(256, 800))
            N = 8 * int(rng.integers(32, 100)) if nn else 4 * int(rng.integers(64, 200))
            K = 64 * int(rng.integers(1, 9))
            cpad = int(rng.choice([4, 8]))
            ldc = -(-N // 8) * 8 + cpad
            wide = not staged and N % 8 == 0 and ldc % 8 == 0
            expect = [P8K.format(Fa if staged else T, Fa if nn else T, T if wide else Fa)]
            knob = dict(P8, GEMM_P8_STAGED=int(staged))
        epi = _draw_epi(rng)
        return "product", dict(M=M, N=N, K=K, layout="nn" if nn else "nt", epi=epi, expect=expect, seed=seed, knob=knob, cpad=cpad,
                               reps=2 if family == "p8" else 1)
    M, N = 8 * int(rng.integers(32 if family == "p8_tn" else 16, 120)), 8 * int(rng.integers(32 if family == "p8_tn" else 16, 120))
    K = int(rng.integers(1024, 3000))
    acc = bool(rng.integers(0, 2))
    rowsum = acc and bool(rng.integers(0, 2))
    if family == "p8_tn":
        return "wgrad", dict(M=M, N=N, K=K, acc=acc, rowsum=rowsum, expect=["gemm_p8_tn_kernel", REDUCE], seed=seed, knob={"tile256": 1}, reps=2)
    kd, atomic = int(rng.choice([32, 64])), int(rng.integers(0, 2))
    slab = not atomic and (-(-M // 128)) * (-(-N // 128)) >= 24
    expect = [f"gemm_glds_tn_kernel<{kd}>"] + ([REDUCE] if slab else [])
    return "wgrad", dict(M=M, N=N, K=K, acc=acc, rowsum=rowsum, expect=sorted(expect), seed=seed,
                         knob={"GEMM_GLDS_TN_KD": kd, "GEMM_TN_ATOMIC": atomic}, reps=2 if slab else 1)


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("family", FUZZ_FAMILIES)
def test_fast_path_fuzz(cuda, family, seed):
    kind, kw = fuzz_draw(family, seed)
    (run_product if kind == "product" else run_wgrad)(cuda, **kw)


def queue_products(mode):
    """test_gemm_group_queue's products: (M, N, K, tA, tB, A array type, B array type, epilogue)"""
    lowp = BF if mode == "bf16" else torch.float32          # the fp32 mode reads fp32 arrays
    return [(100, 72, 64, 0, 1, lowp, lowp, "bias+gelu+pre+bf16out" if mode == "bf16" else "bias+gelu+pre"),
            (96, 132, 200, 1, 0, torch.float32, lowp, "acc"),
            (77, 64, 48, 0, 0, lowp, torch.float32, "relu+res32"),
            (132, 40, 36, 1, 1, torch.float32, torch.float32, "bias+res32+respre"),
            (4096, 1024, 600, 0, 1, torch.float32, torch.float32, "bias")]       # 5 GFLOP: not parked


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_gemm_group_queue(cuda, mode):
    """lib.gemm_group(): three small independent products of mixed layouts, array types and ragged shapes go out as ONE
    gemm_group_any_kernel launch; a fourth flushes the full queue first and leaves in a second group launch when the group closes; a
    product over the size limit (2.2 GFLOP) launches at once on its own kernel.  Every result against float64, guards included."""
    from dlwp_benchmark_amd import lib as L
    from dlwp_benchmark_amd.token_ops import _gemm_batched
    g = torch.Generator().manual_seed(11 if mode == "bf16" else 12)
    prods = queue_products(mode)
    runs = []
    for M, N, K, tA, tB, da, db, epi in prods:
        e = parse_epi(epi)
        lda, ldb, ldc = (M if tA else K), (K if tB else N), -(-N // 8) * 8 + 8
        A = torch.randn(K if tA else M, lda, generator=g).to(cuda).to(da)
        B = (torch.randn(N if tB else K, ldb, generator=g) / math.sqrt(K)).to(cuda).to(db)
        opA, opB = (A.double().T if tA else A.double()), (B.double().T if tB else B.double())
        if mode == "bf16":
            opA, opB = opA.to(BF).double(), opB.to(BF).double()
        bias = torch.randn(N, generator=g).to(cuda) if e["bias"] else None
        res = torch.randn(M, ldc, generator=g).to(cuda) if e["res"] else None
        C0 = guarded(M, N, ldc, e["out"], g, cuda)
        P0 = guarded(M, N, ldc, e["out"], g, cuda) if e["pre"] else None
        want, pre_want = epi_reference(opA @ opB, e, bias, res, C0[:M, :N].double())
        runs.append(dict(args=(A, B, M, N, K, lda, ldb, ldc, tA, tB), e=e, bias=bias, res=res, C0=C0, P0=P0, C=C0.clone(),
                         P=P0.clone() if P0 is not None else None, want=want, pre_want=pre_want))
    with L.gemm_precision(mode), L.kernel_accounting() as acc:
        with L.gemm_group():
            for r in runs:
                A, B, M, N, K, lda, ldb, ldc, tA, tB = r["args"]
                _gemm_batched(A, B, r["C"], M, N, K, lda, ldb, ldc, tA, tB, bias=r["bias"], act=r["e"]["act"], act_param=LAM,
                              preact=r["P"], residual=r["res"], res_pre=int(r["e"]["res_pre"]), accumulate=int(r["e"]["acc"]))
        torch.cuda.synchronize()
    rows = {x["name"]: x for x in acc.rows if x["name"].startswith("gemm")}
    grp = f"gemm_group_any_kernel<{'true' if mode == 'bf16' else 'false'}>"
    single = f"gemm_kernel<true, true, 3, 1, {'true' if mode == 'bf16' else 'false'}, 0>"
    assert sorted(rows) == sorted([grp, single]), sorted(rows)
    assert rows[grp]["calls"] == 2 and rows[single]["calls"] == 1
    assert rows[grp]["flops"] == pytest.approx(sum(2.0 * p[0] * p[1] * p[2] for p in prods[:4]))
    for i, r in enumerate(runs):
        M, N, K = r["args"][2:5]
        tile = (64, 64)
        check_guards(f"product {i}", r["C"], r["C0"], M, N)
        check_tiles(f"product {i}", r["C"][:M, :N], r["want"], tile, fp32_tol(K), r["e"]["out"] == BF)
        if r["P"] is not None:
            check_guards(f"product {i} preact", r["P"], r["P0"], M, N)
            check_tiles(f"product {i} preact", r["P"][:M, :N], r["pre_want"], tile, fp32_tol(K), r["e"]["out"] == BF)
