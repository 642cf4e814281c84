"""Every kernel the normalisation entries (csrc/norm_ops.hip: dlwp_layernorm_fwd_ex, layernorm_bwd_impl behind dlwp_layernorm_bwd / _res /
_ex / _lowp; csrc/instnorm.hip; dlwp_colsum_*; dlwp_act_bwd) can launch, each case pinned through lib.kernel_accounting to the
instantiation it must reach and held to the float64 closed forms of tests/norm_ref.py.  Every array sits in a larger allocation: PAD rows
of NaN after the inputs' row T (a masked lane that leaks into a reduction shows as NaN in a live row), PAD rows of a sentinel bit pattern
after the outputs' (they must come back bit for bit).  The column gradients start from random contents (the engine's fused accumulation
relies on +=); repeated launches must agree bit for bit in gx and its bf16 copy.

Case table ("default" = no knob, the dispatcher's own shape rules):

    kernel instantiation                         cases
    layernorm_fwd_vec_kernel<8>                  test_fwd_path[vec8_c{4,20,32}_t{1,33}]
    layernorm_fwd_vec_kernel<16>                 test_fwd_path[vec16_c{36,64}_t17]  (c64: 1e3 row offset)
    layernorm_fwd_vec_kernel<32>                 test_fwd_path[vec32_c{68,128}_t9], [default_below_threshold_c96_t43690]
    layernorm_fwd_vec_kernel<64>                 test_fwd_path[vec64_c{132,256}_t5]
    layernorm_fwd_wide_kernel<2>                 test_fwd_path[wide2_c{260,512}_t5]
    layernorm_fwd_wide_kernel<3>                 test_fwd_path[wide3_c{516,768}_t5]  (c768: 1e3 row offset)
    layernorm_fwd_wide_kernel<4>                 test_fwd_path[wide4_c{772,1024}_t5]
    layernorm_fwd_kernel (by shape)              test_fwd_path[scalar_c{1,7,63,65,250,1028,2052}_t6]  (c250: 1e3 row offset)
    layernorm_fwd_kernel (by alignment)          test_fwd_path[scalar_c{96,384}_{x4,gamma4,y2}]
    layernorm_fwd_vecn_kernel<8|16|32|64, 3>     test_fwd_path[vecn_c{96,192,384,768}_t{2048,2049}] (LN_FWD_V3=2; c96_t2049: 1e3 row offset),
                                                 [default_vecn_c96_t43691] (<8, 3>), [default_vecn_c768_t5462] (<64, 3>)
    layernorm_bwd_vec_kernel<8|16|32|64, 4>      test_bwd_path[vec4_c{4,20|36,64|100,128|132,256}_t{1,37,301,303}], test_bwd_partitions[vec4_*]
    layernorm_bwd_vec_kernel<8|16|32|64, 8>      test_bwd_path[vec8w_c{...}_t{1,37,301,303}] (LN_BWD_NW=8)
    layernorm_bwd_vecn_kernel<8|16|32, 3, 8, 4>  test_bwd_path[vecn_c{96,192,384}_t{2048,2049,2051}], test_bwd_partitions[vecn_c{96,192,384}]
    layernorm_bwd_vecn_kernel<64, 3, 8, 2>       test_bwd_path[vecn_c768_t2051], test_bwd_partitions[vecn_c768] (LN_BWD_V3=2)
    layernorm_bwd_wide_kernel<2>                 test_bwd_path[wide_c{260,512}_t{5,129,130}], [wide_c384_t50], test_bwd_partitions[wide_c260]
    layernorm_bwd_wide_kernel<3>                 test_bwd_path[wide_c{516,768}_t{5,129,130}], test_bwd_partitions[wide_c516]
    layernorm_bwd_wide_kernel<4>                 test_bwd_path[wide_c{772,1024}_t{5,129,130}], test_bwd_partitions[wide_c1024]
    layernorm_bwd_kernel<1|2|4|8|16|32>          test_bwd_path[scalar_c{1,63|65,127|129,250|258,510|514,1022|1026,2048}_t{6,70}],
                                                 test_bwd_partitions[scalar_c{63,514}]  (the name carries no NQ: C is inside that NQ's range)
    layernorm_bwd_kernel (LN_BWD_NOWIDE)         test_bwd_path[scalar_nowide_c512]
    layernorm_bwd_kernel (by alignment)          test_bwd_path[scalar_c{96,384}_{x4,gadd4,gy2}]
    none (DLWP_E_UNSUPPORTED)                    test_bwd_refuses_c2049

Notes on the case list.  The sample-scale table with B = 3 needs T % 3 == 0, which none of the row counts 1 / 37 / 301 / 5 / 130 / 2048 /
2051 offers: every family carries one more row count for it (303, 129, 2049; the scalar kernel's 6 divides already).  LN_BWD_WANT does not
reach the eight-wave one-chunk kernels (their rows per workgroup come from T / 256 alone) and the three-chunk kernels need T >= 2048, so
their partition cases run at T = 2051.  Each shape carries one flag combination, one shape per instantiation carries all six (FLAGS).

InstanceNorm: a channel that is constant over P has zero variance: rstd == eps ** -0.5 and y == beta (+ residual) there.  Its gx is NOT
zero: with xhat == 0 the closed form leaves gx = rstd gamma (gy - mean(gy)), which is what torch autograd of the definition gives too
(tests/test_norm_ref.py), so the channel is held to the float64 closed form like the others, against its own max norm (it is rstd = 1e3
times larger than its neighbours and would hide them in a common one).

Bounds (ceilings from the project's float64 tests and from the summation depth, never from the results): bound_* below.  TIGHT holds the
factors by which a bound was tightened after the first run on an MI355X (largest observed error under a tenth of the bound -> four times
the observed value); docs/kernels/gemm_norm_train.md has the table of observed errors.  The bf16 output of the forward kernels equals
the rounded fp32 output of the same instantiation in every element of every case (0 differ), so that is asserted."""
import contextlib
import ctypes
import json
import math
import os

import pytest
import torch

import norm_ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
PAD = 8                       # rows after row T of every array: the rows of one wave group of the widest vector kernel
SENT32, SENT16 = 0x4B1DFACE, 0x4B1D
U = 2.0 ** -23                # fp32 unit in the last place of 1
E_UNSUPPORTED = -3

RECORD = {}                   # (family, quantity) -> largest observed error / untightened bound
# (family, quantity) -> factor on the bound, from the first MI355X run: 4 x the largest observed ratio where that was below 0.1
TIGHT = {
    ("bwd_kernel", "gbeta"): 0.008,
    ("bwd_kernel", "ggamma"): 0.014,
    ("bwd_kernel", "gx"): 0.046,
    ("bwd_kernel", "gx_bf16"): 0.0015,
    ("bwd_vec", "gbeta"): 0.012,
    ("bwd_vec", "ggamma"): 0.027,
    ("bwd_vec", "gx"): 0.059,
    ("bwd_vec", "gx_bf16"): 0.0044,
    ("bwd_vecn", "gbeta"): 0.0019,
    ("bwd_vecn", "ggamma"): 0.0025,
    ("bwd_vecn", "gx"): 0.062,
    ("bwd_vecn", "gx_bf16"): 0.0042,
    ("bwd_wide", "gbeta"): 0.0082,
    ("bwd_wide", "ggamma"): 0.014,
    ("bwd_wide", "gx"): 0.048,
    ("bwd_wide", "gx_bf16"): 0.0029,
    ("colsum", "bf16 array"): 0.022,
    ("colsum", "fp32 array"): 0.22,
    ("fwd_kernel", "mean"): 0.085,
    ("fwd_kernel", "rstd"): 0.32,
    ("fwd_kernel", "y"): 0.036,
    ("fwd_vec", "mean"): 0.11,
    ("fwd_vec", "y"): 0.046,
    ("fwd_vec", "y_bf16"): 0.0034,
    ("fwd_vecn", "mean"): 0.11,
    ("fwd_vecn", "y"): 0.051,
    ("fwd_vecn", "y_bf16"): 0.0084,
    ("fwd_wide", "mean"): 0.046,
    ("fwd_wide", "rstd"): 0.33,
    ("fwd_wide", "y"): 0.037,
    ("instnorm", "gbeta"): 0.0077,
    ("instnorm", "ggamma"): 0.0023,
    ("instnorm", "gx"): 0.041,
    ("instnorm", "gx (constant channel)"): 0.031,
    ("instnorm", "mean"): 0.31,
    ("instnorm", "y"): 0.37,
    ("instnorm", "y (constant channel)"): 0.018,
    ("instnorm_1e3", "gbeta"): 0.0077,
    ("instnorm_1e3", "ggamma"): 0.0029,
    ("instnorm_1e3", "gx"): 0.045,
    ("instnorm_1e3", "gx (constant channel)"): 0.031,
    ("instnorm_1e3", "y (constant channel)"): 0.018,
}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("DLWP_NORM_PATHS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({f"{k[0]}/{k[1]}": v for k, v in sorted(RECORD.items())}, f, indent=1)


@contextlib.contextmanager
def knobs(**kw):
    """tuning overrides (lib.set_tuning) for the body, released afterwards"""
    from dlwp_benchmark_amd import lib as L
    try:
        for k, v in kw.items():
            L.set_tuning(k, v)
        yield
    finally:
        for k in kw:
            L.set_tuning(k, None)


def ln_names(fn):
    """the layernorm_* rows of the accounting of one eager call"""
    from dlwp_benchmark_amd import lib as L
    with L.kernel_accounting() as acc:
        fn()
        torch.cuda.synchronize()
    return sorted(r["name"] for r in acc.rows if r["name"].startswith("layernorm_"))


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def raw(cuda, n, dtype, off=0):
    """n elements that start `off` bytes into a 16-byte aligned allocation"""
    es = torch.empty((), dtype=dtype).element_size()
    assert off % es == 0
    base = torch.empty(n + off // es + 8, dtype=dtype, device=cuda)
    assert base.data_ptr() % 16 == 0
    out = base[off // es: off // es + n]
    assert out.data_ptr() % 16 == off
    return out


def inbuf(cuda, live, dtype=F32, off=0):
    """an input array: `live` ([rows] or [rows][cols]) followed by PAD rows of NaN"""
    rows, tail = live.shape[0], tuple(live.shape[1:])
    b = raw(cuda, (rows + PAD) * math.prod(tail), dtype, off).view(rows + PAD, *tail)
    b[:rows] = live.to(cuda).to(dtype)
    b[rows:] = float("nan")
    return b


def outbuf(cuda, rows, cols=0, dtype=F32, off=0):
    """an output array of rows (+ PAD) rows, every element the sentinel bit pattern"""
    b = raw(cuda, (rows + PAD) * max(cols, 1), dtype, off)
    b = b.view(rows + PAD, cols) if cols else b
    bits(b).fill_(SENT16 if dtype == BF else SENT32)
    return b


def pad_intact(what, b, rows):
    assert bool((bits(b[rows:]) == (SENT16 if b.dtype == BF else SENT32)).all()), f"{what}: rows after {rows} were written"


def accbuf(cuda, n, g):
    """an accumulated output ([n] live, PAD sentinels): random non-zero contents; returns (buffer, its initial copy)"""
    b = raw(cuda, n + PAD, F32)
    b.copy_(torch.randn(n + PAD, generator=g))
    return b, b.clone()


def hold(family, qty, err, bound, what):
    """err <= bound everywhere (tensors or numbers; TIGHT applied); records the worst ratio to the untightened bound"""
    err, bound = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(bound, dtype=torch.float64)
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    if not ratio <= RECORD.get((family, qty), 0.0):
        RECORD[(family, qty)] = ratio
    f = TIGHT.get((family, qty), 1.0)
    assert ratio <= f, f"{what}: {qty} error is {ratio:.3g} of its bound (allowed: {f:.3g})"


def bound_out(want):
    """gx, y (fp32): 1e-5 of the output's max norm (test_gpu_round6.py, test_gpu_fft.py)"""
    return 1e-5 * want.abs().max().item()


def excess16(got, want):
    """error of a bf16 output beyond its own rounding, 2^-8 |want| per element (check_tiles in test_gpu_gemm_paths.py)"""
    return ((got.double() - want).abs() - 2.0 ** -8 * want.abs()).clamp_min(0)


def bound_colgrad(want, rows):
    """ggamma, gbeta: 2e-5 sqrt(rows) of their max norm (test_gpu_round6.py)"""
    return 2e-5 * math.sqrt(rows) * want.abs().max().item()


def bound_mean(x, C):
    """Row mean in fp32.  A sum of n terms added at depth d carries at most d u sum|x_i| of rounding error (u = 2^-24); the kernels add
    at most 4 ceil(C / 256) ... 12 (vector kernels: four elements per 16-byte chunk) or ceil(C / 64) (scalar kernel) values in a lane,
    then at most six shuffle levels, then one division (or the product with a rounded 1 / C: two roundings): d <= 2 (ceil(C / 64) + 8) for
    every instantiation (largest: wide<4> at C = 1024, 15 + 6 + 2 = 23 <= 48), and sum|x_i| / C <= max|x_row|.  Per row:
    (ceil(C / 64) + 8) 2^-23 max|x_row|."""
    return (-(-C // 64) + 8) * U * x.double().abs().amax(1)


def bound_rstd(x, C, want_rstd):
    """rstd = rsqrt(var + eps) in fp32, relative.  var is a sum of squares (all positive, so the depth bound of bound_mean holds
    relatively, the two roundings of each square included in its factor two), taken around a mean that is off by at most
    bound_mean = mb: sum (x - mu - mb)^2 / C = var + mb^2 exactly, relative mb^2 rstd^2.  Half of that (square root), plus rsqrtf: the
    guides state no bound; torch.rsqrt in fp32 on the CPU is within 0.75 2^-23 of the float64 value over 2 M arguments in [1e-6, 1e4],
    times 4 = 3 2^-23."""
    mb = bound_mean(x, C)
    return want_rstd * (0.5 * ((-(-C // 64) + 8) * U + (mb * want_rstd) ** 2) + 3 * U)


def ln_inputs(T, C, seed, offset=False):
    g = torch.Generator().manual_seed(seed)
    x = 2 * torch.randn(T, C, generator=g) + 0.5
    if offset:
        x = x + 1e3                     # mean >> standard deviation: only a two-pass variance survives
    return g, x, 1 + 0.1 * torch.randn(C, generator=g), torch.randn(C, generator=g)


def eps32(eps):
    """the float the C ABI receives"""
    return ctypes.c_float(eps).value


# ------------------------------------------------------------------------------------------------------------------ forward
def run_fwd(cuda, C, T, expect, family, knob=None, offset=False, eps=1e-5, mis=None, seed=0):
    """dlwp_layernorm_fwd_ex with fp32 and with bf16 output; mis: "x4" / "gamma4" (that array starts 4 bytes into its allocation) or "y2"
    (the bf16 output starts 2 bytes in; the fp32 output of that case 4 bytes in)"""
    from dlwp_benchmark_amd import lib as L
    lib = L.load()
    g, x, gamma, beta = ln_inputs(T, C, seed, offset)
    xb = inbuf(cuda, x, off=4 if mis == "x4" else 0)
    gmb = inbuf(cuda, gamma, off=4 if mis == "gamma4" else 0)
    btb = inbuf(cuda, beta)
    want_y, want_m, want_r = norm_ref.layernorm_fwd(xb[:T], gmb[:C], btb[:C], eps32(eps))
    ys = {}
    for y16 in (0, 1):
        what = f"C={C} T={T} {'bf16' if y16 else 'fp32'}"
        yb = outbuf(cuda, T, C, BF if y16 else F32, ((2 if y16 else 4) if mis == "y2" else 0))
        mb, rb = outbuf(cuda, T), outbuf(cuda, T)

        def call():
            L.check(lib.dlwp_layernorm_fwd_ex(L.ptr(xb), L.ptr(gmb), L.ptr(btb), L.ptr(yb), L.ptr(mb), L.ptr(rb), T, C, eps, y16, L.stream()))
        with knobs(**(knob or {})):
            names = ln_names(call)
        assert names == [expect], (what, names, expect)
        for name, b in (("y", yb), ("mean", mb), ("rstd", rb)):
            pad_intact(f"{what} {name}", b, T)
        y = yb[:T]
        hold(family, "y_bf16" if y16 else "y", excess16(y, want_y) if y16 else (y.double() - want_y).abs(), bound_out(want_y), what)
        hold(family, "mean", (mb[:T].double() - want_m).abs(), bound_mean(xb[:T], C), what)
        hold(family, "rstd", (rb[:T].double() - want_r).abs(), bound_rstd(xb[:T], C, want_r), what)
        if C == 1 and not y16:          # zero variance: y == beta exactly, rstd == eps ** -0.5 (held above: want_r is just that)
            assert torch.equal(y, btb[:C].expand(T, C))
        ys[y16] = y
    # both branches form the same fp32 value and the bf16 one rounds it: 0 differing elements expected
    differ = int((bits(ys[0].to(BF)) != bits(ys[1])).sum())
    RECORD[(family, "bf16 != rounded fp32 (elements)")] = RECORD.get((family, "bf16 != rounded fp32 (elements)"), 0) + differ
    assert differ == 0, f"C={C} T={T}: {differ} of {T * C} bf16 outputs differ from the rounded fp32 output"


V3 = {"LN_FWD_V3": 2}
FVEC, FVECN, FWIDE, FSCAL = ("layernorm_fwd_vec_kernel<{}>", "layernorm_fwd_vecn_kernel<{}, 3>", "layernorm_fwd_wide_kernel<{}>",
                             "layernorm_fwd_kernel")
# id: (C, T, kernel, family, keyword arguments)
FWD_CASES = {}
for lpr, cs, ts in ((8, (4, 20, 32), (1, 33)), (16, (36, 64), (17,)), (32, (68, 128), (9,)), (64, (132, 256), (5,))):
    for c in cs:
        for t in ts:
            FWD_CASES[f"vec{lpr}_c{c}_t{t}"] = (c, t, FVEC.format(lpr), "fwd_vec", dict(offset=(c == 64)))
for nv, cs in ((2, (260, 512)), (3, (516, 768)), (4, (772, 1024))):
    for c in cs:
        FWD_CASES[f"wide{nv}_c{c}_t5"] = (c, 5, FWIDE.format(nv), "fwd_wide", dict(offset=(c == 768)))
for c in (1, 7, 63, 65, 250, 1028, 2052):
    FWD_CASES[f"scalar_c{c}_t6"] = (c, 6, FSCAL, "fwd_kernel", dict(offset=(c == 250)))
for c in (96, 384):
    for mis in ("x4", "gamma4", "y2"):
        FWD_CASES[f"scalar_c{c}_{mis}"] = (c, 6, FSCAL, "fwd_kernel", dict(mis=mis))
for lpr, c in ((8, 96), (16, 192), (32, 384), (64, 768)):
    for t in (2048, 2049):
        FWD_CASES[f"vecn_c{c}_t{t}"] = (c, t, FVECN.format(lpr), "fwd_vecn", dict(knob=V3, offset=(c == 96 and t == 2049)))
# by default: the first T with T C >= 4 << 20, and the last one below it (the only large cases: 17 MB each)
FWD_CASES["default_vecn_c96_t43691"] = (96, 43691, FVECN.format(8), "fwd_vecn", {})
FWD_CASES["default_vecn_c768_t5462"] = (768, 5462, FVECN.format(64), "fwd_vecn", {})
FWD_CASES["default_below_threshold_c96_t43690"] = (96, 43690, FVEC.format(32), "fwd_vec", {})


@pytest.mark.parametrize("case", list(FWD_CASES))
def test_fwd_path(cuda, case):
    C, T, expect, family, kw = FWD_CASES[case]
    i = list(FWD_CASES).index(case)
    run_fwd(cuda, C, T, expect, family, eps=(1e-5, 1e-6)[i % 2], seed=1000 + i, **kw)


# ----------------------------------------------------------------------------------------------------------------- backward
# flag combinations the kernels branch on: bf16 upstream gradient, residual gradient, the scaled bf16 second output (off / a scale per
# sample for B samples / row_scale == NULL, which means 1).  The entry follows: dlwp_layernorm_bwd, _res, _ex, _lowp.
FLAGS = {
    "plain": dict(gy16=False, gadd=False, lowp=None),
    "res": dict(gy16=False, gadd=True, lowp=None),
    "ex16": dict(gy16=True, gadd=False, lowp=None),
    "lowp_b3": dict(gy16=True, gadd=True, lowp=3),
    "lowp_null": dict(gy16=False, gadd=False, lowp=0),
    "lowp_b1": dict(gy16=False, gadd=True, lowp=1),
}
SCALES = {1: [0.75], 3: [1.25, 0.0, 0.75]}


def run_bwd(cuda, C, T, expect, family, flags, knob=None, mis=None, eps=1e-5, seed=0, reps=2):
    """The backward entry that `flags` select, `reps` times on the same inputs; mean and rstd are the fp32 arrays the forward kernel
    wrote, the reference widens them.  mis: "x4" / "gadd4" / "gy2" (that array starts 4 / 4 / 2 bytes into its allocation).  Returns
    {flag set: (gx, bf16 gx or None)}."""
    from dlwp_benchmark_amd import lib as L
    lib = L.load()
    g, x, gamma, _ = ln_inputs(T, C, seed)
    gy, gadd = torch.randn(T, C, generator=g), torch.randn(T, C, generator=g)
    xb = inbuf(cuda, x, off=4 if mis == "x4" else 0)
    gmb = inbuf(cuda, gamma)
    xa, ya, ma, ra = xb[:T].clone(), torch.empty(T, C, device=cuda), torch.empty(T, device=cuda), torch.empty(T, device=cuda)
    L.check(lib.dlwp_layernorm_fwd_ex(L.ptr(xa), L.ptr(gmb), L.ptr(gmb), L.ptr(ya), L.ptr(ma), L.ptr(ra), T, C, eps, 0, L.stream()))
    meanb, rstdb = inbuf(cuda, ma), inbuf(cuda, ra)
    gyb = {False: inbuf(cuda, gy, off=4 if mis == "gy2" else 0), True: inbuf(cuda, gy, BF, off=2 if mis == "gy2" else 0)}
    gab = inbuf(cuda, gadd, off=4 if mis == "gadd4" else 0)
    outs = {}
    for fl in flags:
        f = FLAGS[fl]
        what = f"C={C} T={T} {fl}"
        lowp = f["lowp"]
        if lowp == 3 and T % 3:
            lowp = 1                      # no three whole samples in T rows
        gyu, gau = gyb[f["gy16"]], (gab if f["gadd"] else None)
        want_x, want_g, want_b = norm_ref.layernorm_bwd(xb[:T], gmb[:C], meanb[:T], rstdb[:T], gyu[:T], gau[:T] if gau is not None else None)
        scale = torch.tensor(SCALES[lowp], device=cuda) if lowp else None
        first = None
        for rep in range(reps):
            gxb = outbuf(cuda, T, C)
            lowb = outbuf(cuda, T, C, BF) if lowp is not None else None
            (ggb, gg0), (gbb, gb0) = accbuf(cuda, C, g), accbuf(cuda, C, g)
            a = [L.ptr(xb), L.ptr(gmb), L.ptr(meanb), L.ptr(rstdb), L.ptr(gyu)]
            o = [L.ptr(gxb), L.ptr(ggb), L.ptr(gbb), T, C]

            def call():
                if lowp is not None:
                    L.check(lib.dlwp_layernorm_bwd_lowp(*a, int(f["gy16"]), L.ptr(gau), *o, L.ptr(lowb), L.ptr(scale), T // max(lowp, 1), L.stream()))
                elif f["gy16"]:
                    L.check(lib.dlwp_layernorm_bwd_ex(*a, 1, L.ptr(gau), *o, L.stream()))
                elif f["gadd"]:
                    L.check(lib.dlwp_layernorm_bwd_res(*a, L.ptr(gau), *o, L.stream()))
                else:
                    L.check(lib.dlwp_layernorm_bwd(*a, *o, L.stream()))
            with knobs(**(knob or {})):
                names = ln_names(call)
            assert names == [expect], (what, names, expect)
            pad_intact(f"{what} gx", gxb, T)
            for name, b, b0 in (("ggamma", ggb, gg0), ("gbeta", gbb, gb0)):
                assert torch.equal(bits(b[C:]), bits(b0[C:])), f"{what}: {name} written past C"
            hold(family, "gx", (gxb[:T].double() - want_x).abs(), bound_out(want_x), what)
            wg, wb = gg0[:C].double() + want_g, gb0[:C].double() + want_b
            hold(family, "ggamma", (ggb[:C].double() - wg).abs(), bound_colgrad(wg, T), what)
            hold(family, "gbeta", (gbb[:C].double() - wb).abs(), bound_colgrad(wb, T), what)
            if lowb is not None:
                pad_intact(f"{what} bf16 gx", lowb, T)
                rs = scale.repeat_interleave(T // lowp)[:, None] if lowp else 1.0
                want_l = want_x * (rs.double() if lowp else 1.0)
                hold(family, "gx_bf16", excess16(lowb[:T], want_l), bound_out(want_l), what)
                # the kernels round the product of the stored gx and the fp32 scale: exactly that
                assert torch.equal(bits(lowb[:T]), bits((gxb[:T] * rs).to(BF))), f"{what}: bf16 gx is not bf16(gx * scale)"
            if first is None:
                first = (gxb[:T], lowb[:T] if lowb is not None else None)
            else:
                assert torch.equal(bits(first[0]), bits(gxb[:T])), f"{what}: repeated launch differs in gx"
                assert lowb is None or torch.equal(bits(first[1]), bits(lowb[:T])), f"{what}: repeated launch differs in the bf16 gx"
        outs[fl] = first
    return outs


BVEC, BVECN, BWIDE, BSCAL = ("layernorm_bwd_vec_kernel<{}, {}>", "layernorm_bwd_vecn_kernel<{}, 3, 8, {}>", "layernorm_bwd_wide_kernel<{}>",
                             "layernorm_bwd_kernel")
ALL = tuple(FLAGS)
ONE = [f for f in FLAGS if f != "lowp_b3"]            # the flag sets a shape without three whole samples takes turns with
# id: (C, T, kernel, family, flag sets, keyword arguments)
BWD_CASES = {}


def _add(cid, C, T, kernel, family, full, b3, **kw):
    n = len(BWD_CASES)
    flags = ALL if full else (("lowp_b3",) if b3 else (ONE[n % len(ONE)],))
    BWD_CASES[cid] = (C, T, kernel, family, flags, kw)


for nw in (4, 8):
    for lpr, cs in ((8, (4, 20)), (16, (36, 64)), (32, (100, 128)), (64, (132, 256))):
        for c in cs:
            for t in (1, 37, 301, 303):
                _add(f"vec{'4' if nw == 4 else '8w'}_c{c}_t{t}", c, t, BVEC.format(lpr, nw), "bwd_vec", full=(c == cs[1] and t == 301),
                     b3=(t == 303), knob={"LN_BWD_NW": 8} if nw == 8 else None)
for lpr, c in ((8, 96), (16, 192), (32, 384)):
    for t in (2048, 2049, 2051):
        _add(f"vecn_c{c}_t{t}", c, t, BVECN.format(lpr, 4), "bwd_vecn", full=(t == 2051), b3=(t == 2049))
_add("vecn_c768_t2051", 768, 2051, BVECN.format(64, 2), "bwd_vecn", full=True, b3=False, knob={"LN_BWD_V3": 2})
for nv, cs in ((2, (260, 512)), (3, (516, 768)), (4, (772, 1024))):
    for c in cs:
        for t in (5, 129, 130):
            _add(f"wide_c{c}_t{t}", c, t, BWIDE.format(nv), "bwd_wide", full=(c == cs[1] and t == 130), b3=(t == 129))
_add("wide_c384_t50", 384, 50, BWIDE.format(2), "bwd_wide", full=False, b3=False)        # below the three-chunk kernel's 2048 rows
for cs in ((1, 63), (65, 127), (129, 250), (258, 510), (514, 1022), (1026, 2048)):       # NQ 1, 2, 4, 8, 16, 32
    for c in cs:
        for t in (6, 70):
            _add(f"scalar_c{c}_t{t}", c, t, BSCAL, "bwd_kernel", full=(c == cs[1] and t == 6), b3=False)
_add("scalar_nowide_c512", 512, 6, BSCAL, "bwd_kernel", full=True, b3=False, knob={"LN_BWD_NOWIDE": 1})
for c in (96, 384):
    for mis, fl in (("x4", "res"), ("gadd4", "lowp_b3"), ("gy2", "ex16")):
        BWD_CASES[f"scalar_c{c}_{mis}"] = (c, 6, BSCAL, "bwd_kernel", (fl,), dict(mis=mis))


@pytest.mark.parametrize("case", list(BWD_CASES))
def test_bwd_path(cuda, case):
    C, T, expect, family, flags, kw = BWD_CASES[case]
    i = list(BWD_CASES).index(case)
    run_bwd(cuda, C, T, expect, family, flags, eps=(1e-5, 1e-6)[i % 2], seed=2000 + i, **kw)


# id: (C, T, kernel, family, partition knob, other knobs).  Knob values 1, 3, 64: one workgroup for all rows, several with a short last
# one, more slots than row groups.
PARTITIONS = {f"vec4_c{c}": (c, 301, BVEC.format(lpr, 4), "bwd_vec", "LN_BWD_WANT", {}) for lpr, c in ((8, 20), (16, 36), (32, 100), (64, 132))}
PARTITIONS.update({f"scalar_c{c}": (c, 301, BSCAL, "bwd_kernel", "LN_BWD_WANT", {}) for c in (63, 514)})
PARTITIONS.update({f"wide_c{c}": (c, 301, BWIDE.format(nv), "bwd_wide", "LN_BWD_WGS", {}) for nv, c in ((2, 260), (3, 516), (4, 1024))})
PARTITIONS.update({f"vecn_c{c}": (c, 2051, BVECN.format(lpr, 4), "bwd_vecn", "LN_BWD_WGS", {}) for lpr, c in ((8, 96), (16, 192), (32, 384))})
PARTITIONS["vecn_c768"] = (768, 2051, BVECN.format(64, 2), "bwd_vecn", "LN_BWD_WGS", {"LN_BWD_V3": 2})


@pytest.mark.parametrize("case", list(PARTITIONS))
def test_bwd_partitions(cuda, case):
    """the rows-per-workgroup partition does not change a row's arithmetic: gx and its bf16 copy agree bit for bit across three
    partitions of the same instantiation; the column gradients meet their float64 bound in each"""
    C, T, expect, family, knob, other = PARTITIONS[case]
    seed = 3000 + list(PARTITIONS).index(case)
    outs = [run_bwd(cuda, C, T, expect, family, ("lowp_b1",), knob=dict(other, **{knob: v}), seed=seed, reps=1)["lowp_b1"] for v in (1, 3, 64)]
    for gx, low in outs[1:]:
        assert torch.equal(bits(gx), bits(outs[0][0])) and torch.equal(bits(low), bits(outs[0][1]))


def test_bwd_refuses_c2049(cuda):
    """C = 2049: DLWP_E_UNSUPPORTED, no launch, every output untouched"""
    from dlwp_benchmark_amd import lib as L
    lib = L.load()
    T, C = 6, 2049
    g, x, gamma, _ = ln_inputs(T, C, 77)
    xb, gmb, gyb = inbuf(cuda, x), inbuf(cuda, gamma), inbuf(cuda, torch.randn(T, C, generator=g))
    mb, rb = inbuf(cuda, x.mean(1)), inbuf(cuda, (x.var(1, unbiased=False) + 1e-5).rsqrt())
    gxb, lowb = outbuf(cuda, T, C), outbuf(cuda, T, C, BF)
    (ggb, gg0), (gbb, gb0) = accbuf(cuda, C, g), accbuf(cuda, C, g)
    rcs = []

    def call():
        rcs.append(lib.dlwp_layernorm_bwd_lowp(L.ptr(xb), L.ptr(gmb), L.ptr(mb), L.ptr(rb), L.ptr(gyb), 0, None, L.ptr(gxb), L.ptr(ggb),
                                               L.ptr(gbb), T, C, L.ptr(lowb), None, T, L.stream()))
        rcs.append(lib.dlwp_layernorm_bwd(L.ptr(xb), L.ptr(gmb), L.ptr(mb), L.ptr(rb), L.ptr(gyb), L.ptr(gxb), L.ptr(ggb), L.ptr(gbb), T, C,
                                          L.stream()))
    assert ln_names(call) == [] and rcs == [E_UNSUPPORTED, E_UNSUPPORTED]
    pad_intact("gx", gxb, 0)
    pad_intact("bf16 gx", lowb, 0)
    assert torch.equal(bits(ggb), bits(gg0)) and torch.equal(bits(gbb), bits(gb0))


# ------------------------------------------------------------------------------------------------------------- InstanceNorm
def bound_in_stats(x, mean, rstd, eps):
    """(mean bound, rstd bound) [B][C] of csrc/instnorm.hip's shifted sums: with K = x[b][0][c] and d = x - K the kernels form m1 = sum d / P,
    m2 = sum d^2 / P, mean = K + m1, var = max(m2 - m1^2, 0).  A thread adds at most 8 of its slab's 128 rows, four threads' partials and
    ceil(P / 128) slabs follow (float atomics), then the division: depth D = ceil(P / 128) + 12, so |m1 error| <= D 2^-23 max|d| (as
    bound_mean) and the last sum rounds once more, 2^-24 |mean|.  m2 and m1^2 carry D 2^-23 relative each and var is their difference:
    D 2^-23 (m2 + m1^2) = D 2^-23 (var + 2 m1^2) absolute, half of it relative to var + eps in rstd, plus 3 2^-23 for rsqrtf
    (bound_rstd).  The shift keeps m1 at the size of the standard deviation whatever the channel's offset."""
    x = x.double()
    P = x.shape[1]
    D = (-(-P // 128) + 12) * U
    d = x - x[:, :1, :]
    m1 = mean - x[:, 0, :]
    var = rstd ** -2 - eps
    return D * d.abs().amax(1) + U / 2 * mean.abs(), rstd * (0.5 * D * (var + 2 * m1 * m1) * rstd ** 2 + 3 * U)


@pytest.mark.parametrize("offset", [0.0, 1e3])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("B,P,C", [(1, 1, 5), (2, 127, 64), (2, 129, 65), (3, 300, 130)])
def test_instnorm_paths(cuda, B, P, C, residual, offset):
    """dlwp_instnorm_fwd / _bwd through the C ABI: P inside one 128-row slab, one short of it, one past it and three slabs with a ragged
    tail, C ragged against the 64 lanes; a per-channel offset (0 or 1e3) that the shifted sums must absorb; channel C // 2 constant over
    P (per sample), where the variance clamp decides."""
    from dlwp_benchmark_amd import lib as L
    lib = L.load()
    eps = 1e-6 if C % 2 else 1e-5
    g = torch.Generator().manual_seed(B + P + C)
    cc = C // 2
    x = 2 * torch.randn(B, P, C, generator=g) + 0.5 + offset * (1 - 2 * (torch.arange(C) % 2))        # +-1e3 by channel
    x[:, :, cc] = (3.25 + torch.arange(B) + offset)[:, None]
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), torch.randn(C, generator=g)
    res = torch.randn(B, P, C, generator=g) if residual else None
    gy = torch.randn(B, P, C, generator=g)
    flat = lambda t: t.reshape(B * P, C)                      # noqa: E731  (pad rows after the last sample's last token)
    xb, gmb, btb, gyb = inbuf(cuda, flat(x)), inbuf(cuda, gamma), inbuf(cuda, beta), inbuf(cuda, flat(gy))
    rsb = inbuf(cuda, flat(res)) if residual else None
    yb, gxb = outbuf(cuda, B * P, C), outbuf(cuda, B * P, C)
    stb, wkb = outbuf(cuda, B * C, 2), outbuf(cuda, B * C, 2)
    (ggb, gg0), (gbb, gb0) = accbuf(cuda, C, g), accbuf(cuda, C, g)
    L.check(lib.dlwp_instnorm_fwd(L.ptr(xb), L.ptr(gmb), L.ptr(btb), L.ptr(rsb), L.ptr(yb), L.ptr(stb), B, P, C, eps, L.stream()))
    L.check(lib.dlwp_instnorm_bwd(L.ptr(xb), L.ptr(gmb), L.ptr(stb), L.ptr(gyb), L.ptr(gxb), L.ptr(ggb), L.ptr(gbb), L.ptr(wkb), B, P, C,
                                  L.stream()))
    torch.cuda.synchronize()
    what = f"B={B} P={P} C={C} residual={residual} offset={offset}"
    for name, b, rows in (("y", yb, B * P), ("gx", gxb, B * P), ("stats", stb, B * C), ("work", wkb, B * C)):
        pad_intact(f"{what} {name}", b, rows)
    for name, b, b0 in (("ggamma", ggb, gg0), ("gbeta", gbb, gb0)):
        assert torch.equal(bits(b[C:]), bits(b0[C:])), f"{what}: {name} written past C"
    x3, gy3 = xb[:B * P].view(B, P, C), gyb[:B * P].view(B, P, C)
    r3 = rsb[:B * P].view(B, P, C) if residual else None
    want_y, want_m, want_r = norm_ref.instnorm_fwd(x3, gmb[:C], btb[:C], eps32(eps), r3)
    mean, rstd = stb[:B * C].view(B, C, 2)[..., 0], stb[:B * C].view(B, C, 2)[..., 1]
    fam = "instnorm" if offset == 0 else "instnorm_1e3"
    bm, br = bound_in_stats(x3, want_m, want_r, eps32(eps))
    hold(fam, "mean", (mean.double() - want_m).abs(), bm, what)
    hold(fam, "rstd", (rstd.double() - want_r).abs(), br, what)
    want_gx, want_gg, want_gb = norm_ref.instnorm_bwd(x3, gmb[:C], mean, rstd, gy3)
    y, gx = yb[:B * P].view(B, P, C), gxb[:B * P].view(B, P, C)
    others = [c for c in range(C) if c != cc]
    hold(fam, "y", (y.double() - want_y).abs()[..., others], bound_out(want_y[..., others]), what)
    if P > 1:
        hold(fam, "gx", (gx.double() - want_gx).abs()[..., others], bound_out(want_gx[..., others]), what)
    # the constant channel: mean == x, rstd == eps ** -0.5 (bounds above), y == beta (+ residual) and gx against the closed form, by itself
    hold(fam, "y (constant channel)", (y.double() - want_y).abs()[..., cc], bound_out(want_y[..., cc]), what)
    if P > 1:
        hold(fam, "gx (constant channel)", (gx.double() - want_gx).abs()[..., cc], bound_out(want_gx[..., cc]), what)
    else:
        assert not gx.any(), f"{what}: gx of a one-token sample is zero"
    assert torch.equal(mean[:, cc], x3[:, 0, cc])
    wg, wb = gg0[:C].double() + want_gg, gb0[:C].double() + want_gb
    hold(fam, "ggamma", (ggb[:C].double() - wg).abs(), bound_colgrad(wg, P), what)
    hold(fam, "gbeta", (gbb[:C].double() - wb).abs(), bound_colgrad(wb, P), what)


# -------------------------------------------------------------------------------------------------------------- column sums
# fp32 arrays 2e-6, bf16 arrays 1e-5 of the max norm (test_gpu_token_ops.py: test_colsum_accumulates_the_column_sums,
# test_colsum_of_a_bf16_array)
@pytest.mark.parametrize("T,N,off", [(17, 7, 0), (33, 1028, 0), (300, 1030, 0), (40, 64, 2)])
def test_colsum_bf16_paths(cuda, T, N, off):
    """dlwp_colsum_bf16: 8-byte loads (N % 4 == 0, aligned) and the scalar bf16 branch (odd N; an aligned width on an array 2 bytes in)"""
    from dlwp_benchmark_amd import lib as L
    g = torch.Generator().manual_seed(T + N)
    xb = inbuf(cuda, torch.randn(T, N, generator=g), BF, off)
    out, out0 = accbuf(cuda, N, g)
    L.check(L.load().dlwp_colsum_bf16(L.ptr(xb), L.ptr(out), T, N, L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(out[N:]), bits(out0[N:]))
    want = out0[:N].double() + xb[:T].double().sum(0)
    hold("colsum", "bf16 array", (out[:N].double() - want).abs(), 1e-5 * want.abs().max().item(), f"T={T} N={N}")


@pytest.mark.parametrize("T,N,overwrite", [(17, 7, 1), (257, 1030, 1), (16, 7, 0), (16, 7, 1), (1, 5, 0), (1, 5, 1)])
def test_colsum_ex_paths(cuda, T, N, overwrite):
    """dlwp_colsum_ex: the tall form (T > 16) overwriting an output full of NaN at odd widths; the flat form adding and overwriting"""
    from dlwp_benchmark_amd import lib as L
    g = torch.Generator().manual_seed(T + N + overwrite)
    xb = inbuf(cuda, torch.randn(T, N, generator=g))
    out, out0 = accbuf(cuda, N, g)
    if overwrite:
        out[:N] = float("nan")
    L.check(L.load().dlwp_colsum_ex(L.ptr(xb), L.ptr(out), T, N, overwrite, L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(out[N:]), bits(out0[N:]))
    want = xb[:T].double().sum(0) + (0 if overwrite else out0[:N].double())
    hold("colsum", "fp32 array", (out[:N].double() - want).abs(), 2e-6 * want.abs().max().item(), f"T={T} N={N} overwrite={overwrite}")


# ------------------------------------------------------------------------------------------------------ activation backward
@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 3])
@pytest.mark.parametrize("act", [1, 2, 3])
def test_act_bwd_paths(cuda, act, n):
    """dlwp_act_bwd: gz = gy act'(z).  ReLU (2) and soft-shrink (3) are strict inequalities, exact at 0, lam, -lam and their fp32
    neighbours; GELU (1) against the float64 derivative of the exact (erf) GELU, the form common.hip.h's gelu_both evaluates.  Its
    bound: Abramowitz-Stegun 7.1.26 leaves 1.5e-7 in erfc, 0.75e-7 in the distribution function; about twelve fp32 roundings (and the
    1-ulp v_rcp_f32 / v_exp_f32) of terms that are at most 1 follow, 2^-24 each: 1e-6 absolute on the derivative, times |gy|, plus the
    product's own rounding.  n: one element, one short of / one past a workgroup, three past the 2048-workgroup grid's first round."""
    from dlwp_benchmark_amd import lib as L
    g = torch.Generator().manual_seed(act + n)
    lam = torch.tensor(0.3, dtype=F32)
    inf = torch.tensor(float("inf"))
    base = torch.stack([torch.zeros(()), lam, -lam])
    special = torch.cat([base, torch.nextafter(base, inf), torch.nextafter(base, -inf), -torch.zeros(1)])
    z = torch.randn(n, generator=g)
    z[::2] = special[(torch.arange(n)[::2] // 2) % special.numel()]
    z[-1] = lam if n > 1 else 0.0
    on = ((z > 0) if act == 2 else ((z > lam) | (z < -lam))).to(cuda)           # on the CPU: shares nothing with the kernel
    zb, gyb, gzb = inbuf(cuda, z), inbuf(cuda, torch.randn(n, generator=g)), outbuf(cuda, n)
    L.check(L.load().dlwp_act_bwd(L.ptr(zb), L.ptr(gyb), L.ptr(gzb), n, act, lam.item(), L.stream()))
    torch.cuda.synchronize()
    pad_intact("gz", gzb, n)
    zz, gy, gz = zb[:n], gyb[:n], gzb[:n]
    if act == 1:
        zd = zz.double()
        d = 0.5 * (1 + torch.erf(zd / math.sqrt(2))) + zd * torch.exp(-0.5 * zd * zd) / math.sqrt(2 * math.pi)
        want = gy.double() * d
        hold("act_bwd", "gelu", (gz.double() - want).abs(), 1e-6 * gy.double().abs() + U * want.abs() + 1e-30, f"n={n}")
    else:
        assert torch.equal(gz, gy * on)
