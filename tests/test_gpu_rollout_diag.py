"""csrc/rollout_diag.hip on the MI355X: dlwp_rollout_diag on lat-lon and HPX planes (staged and direct), dlwp_group_mean, their wrappers
in evaluate.py and the driver evaluate_dlwp, against the float64 restatement tests/rollout_diag_ref.py.

Every source sits in a buffer followed by GUARD planes of NaN (a lane that reads past its chunk shows as NaN), every result in a
buffer followed by a tail of a sentinel bit pattern that must come back untouched.  Fields carry a large offset (shift 5e4, scale
3e3 for variable 0), so a sum or a difference taken in physical units would show at once.

Bounds (from the arithmetic, not from results; u = 2^-24).  A fixed-order fp32 sum of n terms is within (n + 1) u sum|x_i| of the
float64 sum of the same terms, asserted with a factor 2:
  window sum  (normalised; n = frames in the window)   2 (n + 1) u sum_t |x_t|
  zonal mean  (de-normalised: sum / W * scale + shift)  2 (W + 1) u sum_w |x_w| |scale| / W for the sum, + u |scale| sum|x| / W for the
              rounded division, + u |result| for the rounded fma
  HPX         each interpolated value is four products and three additions of a convex combination: 7 u max|plane| per value
              (tests/test_gpu_hpx_remap.py), added per term
  climatology forecast  each value is (c - shift) * (1 / scale) in fp32: three roundings, 3 u |x| per term
physical_soundness is a root of a mean of squares of differences of means of those table entries: the RMS of a perturbed vector moves
by at most the largest perturbation of an entry, so its bound is the sum of the two largest entry bounds (output + target).  The per-lead rmse / acc use the tolerances of tests/test_gpu_evaluate.py (rmse rtol 2e-5, acc atol 2e-5).  Bit equality
(torch.equal): two runs; one call against two time chunks x two batch chunks; the persistence view against its copy; the climatology
forecast against its materialised gather."""
import contextlib

import numpy as np
import pytest
import torch

import hpx_remap_ref as HR
import rollout_diag_ref as R

pytestmark = pytest.mark.gpu

GUARD = 2
SENT = 0x4B1DFACE
U24 = 2.0 ** -24
DT = 6                                       # hours between frames
LL_SHAPES = [(1, 1, 1, 4, 8), (2, 5, 3, 5, 12), (3, 7, 2, 32, 64)]
HPX_SHAPES = [(1, 4, 8), (2, 8, 16), (8, 32, 64)]
HPX_BTV = (2, 5, 3)


@contextlib.contextmanager
def knobs(**kw):
    from dlwp_benchmark_amd import lib as L
    try:
        for k, v in kw.items():
            L.set_tuning(k, v)
        yield
    finally:
        for k in kw:
            L.set_tuning(k, None)


def launched(fn):
    from dlwp_benchmark_amd import lib as L
    with L.kernel_accounting() as acc:
        out = fn()
        torch.cuda.synchronize()
    return out, sorted(r["name"] for r in acc.rows)


def guarded(x, dev):
    """x [B, ...] float32 numpy -> the first B entries of a device buffer whose GUARD further entries are NaN"""
    buf = torch.full((x.shape[0] + GUARD,) + x.shape[1:], float("nan"), device=dev)
    buf[:x.shape[0]] = torch.from_numpy(x).to(dev)
    return buf[:x.shape[0]]


def canary(shape, dev, zero=False):
    """(view of `shape`, whole buffer): the view is followed by a sentinel tail of one leading slice's size, at least 64 words"""
    n = int(np.prod(shape))
    tail = max(64, GUARD * (n // shape[0]))
    full = torch.full((n + tail,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
    view = full[:n].view(shape)
    if zero:
        view.zero_()
    return view, full


def check_canary(view, full, all_written=True):
    n = view.numel()
    assert (full[n:].view(torch.int32) == SENT).all(), "the words behind the result were written"
    if all_written:
        assert not (view.reshape(-1).view(torch.int32) == SENT).any(), "part of the result was not written"


def new_state(B, T, V, H, W, window, dev):
    m, mf = canary((B, T, V, 5), dev)
    z, zf = canary((2, B, T, V, H), dev)
    w, wf = canary((2, B, V, H, W), dev, zero=True)
    return {"moments": m, "zonal": z, "wsum": w, "window": tuple(window), "frames": 0}, [(m, mf), (z, zf), (w, wf)]


class Case:
    """seeded normalised outputs / targets [B, T, V, plane], per-variable scale / shift, a physical climatology and months"""

    def __init__(self, B, T, V, H, W, n=None, seed=0):
        rng = np.random.default_rng([seed, B, T, V, H, W, n or 0])
        self.B, self.T, self.V, self.H, self.W, self.n = B, T, V, H, W, n
        self.plane = (H, W) if n is None else (12, n, n)
        self.o = rng.standard_normal((B, T, V) + self.plane).astype(np.float32)
        self.t = rng.standard_normal((B, T, V) + self.plane).astype(np.float32)
        self.scale = (3.0e3 * (1 + 0.25 * np.arange(V))).astype(np.float32)
        self.shift = (5.0e4 - 7.0e3 * np.arange(V)).astype(np.float32)
        self.clim = (self.shift[None, :, None, None]
                     + self.scale[None, :, None, None] * 0.5 * rng.standard_normal((12, V, H, W))).astype(np.float32)
        self.months = rng.integers(0, 12, (B, T))
        self.lats = R.lat_coordinate(H)
        # the window: labels (i + 1) DT hours between 12 h and 24 h -> frames 1..3 where they exist; a single frame is its own window
        self.window = (0, 1) if T == 1 else (1, min(4, T))

    def latlon(self, x, remap):
        """float64 [B, T, V, H, W] of a normalised array: itself, or hpx2ll with the float32 weights the device holds"""
        if remap is None:
            return np.asarray(x, dtype=np.float64)
        idx, w = remap._hpx2ll.idx.cpu().numpy().reshape(-1, 4), remap._hpx2ll.w.cpu().numpy().reshape(-1, 4)
        return HR.apply_table(idx, w, x.reshape(x.shape[:3] + (-1,))).reshape(x.shape[:3] + (self.H, self.W))


def reference(case, xo, xt, *, with_ss, with_w, with_clim, gather_o=0.0, gather_t=0.0, clim_forecast=False):
    """xo / xt float64 normalised lat-lon values.  Returns the restatement's results and the table bounds of the module docstring."""
    B, T, V, H, W = xo.shape
    scale, shift = (case.scale.astype(np.float64), case.shift.astype(np.float64)) if with_ss else (np.ones(V), np.zeros(V))
    sc5 = scale.reshape(1, 1, V, 1, 1)
    po, pt = R.denormalise(xo, scale, shift), R.denormalise(xt, scale, shift)
    lats = case.lats if with_w else None
    c = R.climatology_forecast(case.clim, case.months) if with_clim else None
    ref = R.rmse_acc(po, pt, lats, c)
    w0, w1 = case.window
    nwin = w1 - w0
    ref["zonal"] = np.stack([po.mean(axis=4), pt.mean(axis=4)])
    ref["wsum"] = np.stack([xo[:, w0:w1].sum(axis=1), xt[:, w0:w1].sum(axis=1)])
    per_term = [gather_o + (3 * U24 * np.abs(xo) if clim_forecast else 0.0), gather_t + 0.0 * xt]
    ztol, wtol = [], []
    for x, p, e in zip((xo, xt), (po, pt), per_term):
        sabs = np.abs(x).sum(axis=4)
        eterm = np.broadcast_to(e, x.shape)
        ztol.append((2 * (W + 1) * U24 * sabs + U24 * sabs + eterm.sum(axis=4)) * np.abs(sc5[..., 0]) / W + U24 * np.abs(p.mean(axis=4)))
        wtol.append(2 * (nwin + 1) * U24 * np.abs(x[:, w0:w1]).sum(axis=1) + eterm[:, w0:w1].sum(axis=1))
    ref["zonal_tol"], ref["wsum_tol"] = np.stack(ztol), np.stack(wtol)
    # the window in days for the restatement's label slice: labels (w0 + 1) DT .. w1 DT hours
    ps = R.physical_soundness(po, pt, case.lats, DT, (w0 + 1) * DT / 24.0, w1 * DT / 24.0)
    assert ps["window_frames"].tolist() == list(range(w0, w1))
    ref["soundness"] = ps
    zt = ref["zonal_tol"].max(axis=(1, 2, 4))                                 # [2, V]: the largest entry bound per variable
    ref["zonal_rmse_tol"] = zt[0] + zt[1]
    wt = ref["wsum_tol"].max(axis=(1, 3, 4))
    ref["window_rmse_tol"] = (wt[0] + wt[1]) / max(nwin, 1) * np.abs(scale)
    return ref


def run(case, dev, *, remap=None, with_ss=True, with_w=True, with_clim=True, outputs="given", state=None, bsl=slice(None), tsl=slice(None),
        src=None):
    """one rollout_diagnostics call on the chunk [bsl, tsl] of the case; `src` = (outputs, targets) device tensors of the whole case"""
    from dlwp_benchmark_amd import evaluate
    o_dev, t_dev = src
    o = None if outputs == "clim" else o_dev[bsl, tsl]
    clim = torch.from_numpy(case.clim).to(dev) if with_clim else None
    return evaluate.rollout_diagnostics(o, t_dev[bsl, tsl], scale=case.scale if with_ss else None, shift=case.shift if with_ss else None,
                                        lats_deg=case.lats if with_w else None, remap=remap, climatology=clim,
                                        months=case.months[bsl, tsl] if with_clim else None, window=case.window, state=state,
                                        t_begin=tsl.start or 0, T=case.T)


def check_tables(state, ref, with_clim, label):
    from dlwp_benchmark_amd import evaluate
    z, w = state["zonal"].cpu().numpy().astype(np.float64), state["wsum"].cpu().numpy().astype(np.float64)
    assert np.isfinite(z).all() and np.isfinite(w).all() and torch.isfinite(state["moments"]).all(), "a guard plane was read"
    zr = (np.abs(z - ref["zonal"]) / ref["zonal_tol"]).max()
    wr = (np.abs(w - ref["wsum"]) / np.maximum(ref["wsum_tol"], 1e-300)).max()
    print(f"{label}: zonal err / bound {zr:.3f}, window-sum err / bound {wr:.3f} (allowed 1: the bounds carry the factor 2)")
    assert (np.abs(z - ref["zonal"]) <= ref["zonal_tol"]).all()
    assert (np.abs(w - ref["wsum"]) <= ref["wsum_tol"]).all()
    got = evaluate.diag_metrics(state)
    assert set(got) == ({"rmse", "acc"} if with_clim else {"rmse"})
    print(f"   rmse rel err {np.abs(got['rmse'].numpy() / ref['rmse'] - 1).max():.2e}")
    np.testing.assert_allclose(got["rmse"].numpy(), ref["rmse"], rtol=2e-5)
    if with_clim:
        print(f"   acc abs err {np.abs(got['acc'].numpy() - ref['acc']).max():.2e}")
        np.testing.assert_allclose(got["acc"].numpy(), ref["acc"], rtol=0, atol=2e-5)


def check_soundness(diag, ref, lats, nwin, label):
    from dlwp_benchmark_amd import evaluate
    got = evaluate.physical_soundness(diag, lats, nwin)
    ps = ref["soundness"]
    for k in ("rmse_global", "rmse_trade_winds", "rmse_south_westerlies", "rmse_window"):
        g, r = got[k].numpy(), ps[k]
        tol = (ref["window_rmse_tol"] if k == "rmse_window" else ref["zonal_rmse_tol"]) + 1e-12 * np.abs(r)
        sel = np.isfinite(r)                                                  # (a band without rows on a small grid: nan on both sides)
        assert np.array_equal(np.isfinite(g), sel), (label, k, g, r)
        print(f"{label}: {k} err / bound {(np.abs(g - r)[sel] / tol[sel]).max() if sel.any() else 0.0:.3f}")
        assert (np.abs(g - r)[sel] <= tol[sel]).all(), (label, k, g, r, tol)


VARIANTS = [dict(with_ss=True, with_w=True, with_clim=True), dict(with_ss=False, with_w=False, with_clim=False),
            dict(with_ss=True, with_w=False, with_clim=False), dict(with_ss=False, with_w=True, with_clim=True)]


@pytest.mark.parametrize("variant", VARIANTS, ids=["all", "plain", "scaled", "weights+clim"])
@pytest.mark.parametrize("B,T,V,H,W", LL_SHAPES)
def test_latlon_against_restatement(cuda, B, T, V, H, W, variant):
    case = Case(B, T, V, H, W)
    src = (guarded(case.o, cuda), guarded(case.t, cuda))
    state, bufs = new_state(B, T, V, H, W, case.window, cuda)
    state, names = launched(lambda: run(case, cuda, src=src, state=state, **variant))
    assert names == ["rollout_diag_fold", "rollout_diag_ll"]
    for view, full in bufs:
        check_canary(view, full)
    ref = reference(case, case.latlon(case.o, None), case.latlon(case.t, None), **variant)
    label = f"lat-lon {B}x{T}x{V}x{H}x{W}"
    check_tables(state, ref, variant["with_clim"], label)
    check_soundness(state, ref, case.lats, case.window[1] - case.window[0], label)
    if not variant["with_clim"]:
        assert not state["moments"][..., 2:].any()


@pytest.mark.parametrize("path", ["staged", "direct"])
@pytest.mark.parametrize("with_clim", [True, False])
@pytest.mark.parametrize("n,H,W", HPX_SHAPES)
def test_hpx_against_restatement(cuda, n, H, W, with_clim, path):
    from dlwp_benchmark_amd.hpx_remap import HEALPixRemap
    B, T, V = HPX_BTV
    remap = HEALPixRemap(latitudes=H, longitudes=W, nside=n, device=cuda)
    case = Case(B, T, V, H, W, n=n)
    src = (guarded(case.o, cuda), guarded(case.t, cuda))
    variant = dict(with_ss=True, with_w=True, with_clim=with_clim)
    state, bufs = new_state(B, T, V, H, W, case.window, cuda)
    with knobs(**({"DIAG_PATH": 2} if path == "direct" else {})):
        state, names = launched(lambda: run(case, cuda, remap=remap, src=src, state=state, **variant))
    assert names == ["rollout_diag_fold", "rollout_diag_hpx_direct" if path == "direct" else "rollout_diag_hpx_lds"]
    for view, full in bufs:
        check_canary(view, full)
    g_o, g_t = 7 * U24 * np.abs(case.o).max(), 7 * U24 * np.abs(case.t).max()
    ref = reference(case, case.latlon(case.o, remap), case.latlon(case.t, remap), gather_o=g_o, gather_t=g_t, **variant)
    label = f"hpx n={n} {H}x{W} {path}"
    check_tables(state, ref, with_clim, label)
    check_soundness(state, ref, case.lats, case.window[1] - case.window[0], label)


def test_hpx_natural_direct_path_and_equal_bits(cuda):
    """HPX32 planes (two of 48 KiB) do not fit the LDS budget: the dispatcher takes the direct kernel by itself; at HPX8 the forced
    direct kernel gives the bits of the staged one (the same arithmetic on the same values)"""
    from dlwp_benchmark_amd.hpx_remap import HEALPixRemap
    remap = HEALPixRemap(latitudes=32, longitudes=64, nside=32, device=cuda)
    case = Case(1, 2, 1, 32, 64, n=32)
    src = (guarded(case.o, cuda), guarded(case.t, cuda))
    state, names = launched(lambda: run(case, cuda, remap=remap, src=src))
    assert names == ["rollout_diag_fold", "rollout_diag_hpx_direct"]
    ref = reference(case, case.latlon(case.o, remap), case.latlon(case.t, remap), with_ss=True, with_w=True, with_clim=True,
                    gather_o=7 * U24 * np.abs(case.o).max(), gather_t=7 * U24 * np.abs(case.t).max())
    check_tables(state, ref, True, "hpx n=32 natural direct")
    remap8 = HEALPixRemap(latitudes=32, longitudes=64, nside=8, device=cuda)
    case8 = Case(2, 3, 2, 32, 64, n=8)
    src8 = (guarded(case8.o, cuda), guarded(case8.t, cuda))
    a = run(case8, cuda, remap=remap8, src=src8)
    with knobs(DIAG_PATH=2):
        b = run(case8, cuda, remap=remap8, src=src8)
    for k in ("moments", "zonal", "wsum"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("mesh", ["latlon", "hpx"])
def test_two_runs_and_chunked_runs_give_the_same_bits(cuda, mesh):
    from dlwp_benchmark_amd.hpx_remap import HEALPixRemap
    remap = HEALPixRemap(latitudes=32, longitudes=64, nside=8, device=cuda) if mesh == "hpx" else None
    case = Case(3, 7, 2, 32, 64, n=8 if mesh == "hpx" else None)
    assert case.window == (1, 4)
    src = (guarded(case.o, cuda), guarded(case.t, cuda))
    one, again = run(case, cuda, remap=remap, src=src), run(case, cuda, remap=remap, src=src)
    for k in ("moments", "zonal", "wsum"):
        assert torch.equal(one[k], again[k]), k
    parts = []
    for bsl in (slice(0, 2), slice(2, 3)):                    # two batch chunks x two time chunks; the window [1, 4) spans the cut at 3
        st = run(case, cuda, remap=remap, src=src, bsl=bsl, tsl=slice(0, 3))
        st = run(case, cuda, remap=remap, src=src, bsl=bsl, tsl=slice(3, 7), state=st)
        assert st["frames"] == 7
        parts.append(st)
    assert torch.equal(torch.cat([p["moments"] for p in parts], 0), one["moments"])
    assert torch.equal(torch.cat([p["zonal"] for p in parts], 1), one["zonal"])
    assert torch.equal(torch.cat([p["wsum"] for p in parts], 1), one["wsum"])


def test_odd_shape_in_chunks(cuda):
    """(2, 5, 3, 5, 12) cut at frame 2: the time-sliced outputs are a strided view read in place"""
    case = Case(2, 5, 3, 5, 12)
    src = (guarded(case.o, cuda), guarded(case.t, cuda))
    one = run(case, cuda, src=src)
    st = run(case, cuda, src=src, tsl=slice(0, 2))
    st = run(case, cuda, src=src, tsl=slice(2, 5), state=st)
    for k in ("moments", "zonal", "wsum"):
        assert torch.equal(one[k], st[k]), k


def test_persistence_view_equals_its_copy(cuda):
    from dlwp_benchmark_amd import evaluate
    case = Case(3, 7, 2, 32, 64)
    inits = guarded(case.o[:, 0], cuda)                       # [B, V, H, W]
    t_dev = guarded(case.t, cuda)
    view = evaluate.persistence_forecast(inits, case.T)
    assert view.stride()[1] == 0 and view.data_ptr() == inits.data_ptr()
    a = run(case, cuda, src=(view, t_dev))
    b = run(case, cuda, src=(view.contiguous(), t_dev))
    for k in ("moments", "zonal", "wsum"):
        assert torch.equal(a[k], b[k]), k
    xo = np.broadcast_to(case.o[:, :1], case.o.shape).astype(np.float64)
    ref = reference(case, xo, case.latlon(case.t, None), with_ss=True, with_w=True, with_clim=True)
    check_tables(a, ref, True, "persistence")


def test_climatology_forecast_equals_its_gather(cuda):
    """outputs=None reads the monthly map per frame; the materialised forecast is the same fp32 arithmetic, (c - shift) * (1 / scale),
    spelled out with torch on the device (1 / scale rounded once on the host, as an IEEE division)"""
    case = Case(3, 7, 2, 32, 64)
    t_dev = guarded(case.t, cuda)
    a = run(case, cuda, src=(None, t_dev), outputs="clim")
    inv = torch.from_numpy(np.float32(1.0) / case.scale).to(cuda).view(1, 1, -1, 1, 1)
    sh = torch.from_numpy(case.shift).to(cuda).view(1, 1, -1, 1, 1)
    gathered = torch.from_numpy(case.clim).to(cuda)[torch.from_numpy(case.months).to(cuda)]      # [B, T, V, H, W] physical
    mat = (gathered - sh) * inv
    b = run(case, cuda, src=(mat, t_dev))
    for k in ("moments", "zonal", "wsum"):
        assert torch.equal(a[k], b[k]), k
    assert not a["moments"][..., 3].any()                     # the forecast IS the climatology: its anomaly is zero
    sc5, sh5 = case.scale.astype(np.float64).reshape(1, 1, -1, 1, 1), case.shift.astype(np.float64).reshape(1, 1, -1, 1, 1)
    xo = (R.climatology_forecast(case.clim, case.months) - sh5) / sc5
    ref = reference(case, xo, case.latlon(case.t, None), with_ss=True, with_w=True, with_clim=False, clim_forecast=True)
    z, w = a["zonal"].cpu().numpy().astype(np.float64), a["wsum"].cpu().numpy().astype(np.float64)
    assert (np.abs(z - ref["zonal"]) <= ref["zonal_tol"]).all() and (np.abs(w - ref["wsum"]) <= ref["wsum_tol"]).all()
    from dlwp_benchmark_amd import evaluate
    np.testing.assert_allclose(evaluate.diag_metrics(a)["rmse"].numpy(), ref["rmse"], rtol=2e-5)


@pytest.mark.parametrize("N,P,empty", [(1, 300, None), (37, 300, 4), (37, 2048, 4)])
def test_group_mean(cuda, N, P, empty):
    from dlwp_benchmark_amd import lib as L
    rng = np.random.default_rng(N + P)
    groups = np.array([g for g in range(12) if g != empty])
    m = groups[rng.integers(0, len(groups), N)].astype(np.int32) if N > 1 else np.array([7], dtype=np.int32)
    x = (5.0e4 + 3.0e3 * rng.standard_normal((N, P))).astype(np.float32)
    src = guarded(x, cuda)
    mean, mfull = canary((12, P), cuda)
    count, cfull = canary((12,), cuda)
    g = torch.from_numpy(m).to(cuda)
    _, names = launched(lambda: L.check(L.load().dlwp_group_mean(src.data_ptr(), g.data_ptr(), mean.data_ptr(), count.data_ptr(), N, P, 12,
                                                                 L.stream())))
    assert names == ["group_mean"]
    check_canary(mean, mfull)
    check_canary(count, cfull)
    ref, cnt = R.monthly_climatology(x, m)
    assert count.view(torch.int32).cpu().numpy().tolist() == cnt.tolist()
    got = mean.cpu().numpy().astype(np.float64)
    sabs = np.stack([np.abs(x[m == k].astype(np.float64)).sum(axis=0) for k in range(12)])
    tol = 2 * (cnt[:, None] + 1) * U24 * sabs / np.maximum(cnt[:, None], 1) + U24 * np.abs(ref)      # the sum, then the rounded division
    print(f"group_mean N={N} P={P}: max err / bound {(np.abs(got - ref) / np.maximum(tol, 1e-300)).max():.3f}")
    assert (np.abs(got - ref) <= tol).all()
    if empty is not None:
        assert cnt[empty] == 0 and not got[empty].any()


def test_monthly_climatology_wrapper(cuda):
    from dlwp_benchmark_amd import evaluate
    rng = np.random.default_rng(3)
    x, m = rng.standard_normal((20, 2, 4, 8)).astype(np.float32), rng.integers(0, 12, 20)
    mean, count = evaluate.monthly_climatology(torch.from_numpy(x).to(cuda), m)
    ref, cnt = R.monthly_climatology(x, m)
    assert tuple(mean.shape) == (12, 2, 4, 8) and count.cpu().numpy().tolist() == cnt.tolist()
    np.testing.assert_allclose(mean.cpu().numpy(), ref, rtol=0, atol=20 * U24 * np.abs(x).max())


def dated_dataset(H, W, fields_map=None):
    """synthetic fields on a 6-hourly time axis across the January / February boundary, three initialisation dates"""
    from dlwp_benchmark_amd import wbdata
    n_time = 48
    fields, prognostic, prescribed, constants = wbdata.synthetic_fields(n_time, H, W)
    times = np.datetime64("2017-01-27T00", "h") + np.timedelta64(DT, "h") * np.arange(n_time)
    inits = times[[0, 9, 17]]
    use = fields if fields_map is None else fields_map(fields)
    ds = wbdata.WeatherBenchArrays(use, prognostic, prescribed, constants, sequence_length=6, normalize=True, context_size=1, seed=0,
                                   times=times, init_dates=inits, timedelta=DT)
    phys = np.stack([a for p, levels in prognostic.items() for a in ([fields[p][l] for l in levels] if levels else [fields[p]])], axis=1)
    months = (times.astype("datetime64[M]").astype(np.int64) % 12)
    return ds, phys, months


def e2e_reference(ds, outs, tars, clim, lats, to_latlon):
    from dlwp_benchmark_amd import evaluate
    scale, shift = evaluate.dataset_scale_shift(ds)
    xo, xt = to_latlon(outs), to_latlon(tars)
    po, pt = R.denormalise(xo, scale, shift), R.denormalise(xt, scale, shift)
    T = xo.shape[1]
    months = R.forecast_months(ds.init_dates, T, DT)
    ref = R.rmse_acc(po, pt, lats, R.climatology_forecast(clim, months))
    ref["soundness"] = R.physical_soundness(po, pt, lats, DT, 0.5, 1)
    return ref, xo, xt, np.asarray(scale, dtype=np.float64)


def check_e2e(res, ref, xo, xt, scale, gather=0.0):
    np.testing.assert_allclose(res["rmse"].numpy(), ref["rmse"], rtol=2e-5)
    np.testing.assert_allclose(res["acc"].numpy(), ref["acc"], rtol=0, atol=2e-5)
    ps = ref["soundness"]
    assert res["window"] == (int(ps["window_frames"][0]), int(ps["window_frames"][-1]) + 1)
    W, nwin = xo.shape[4], len(ps["window_frames"])
    w0, w1 = res["window"]
    ztol = wtol = 0.0
    for x in (xo, xt):                                                        # the entry bounds of the module docstring, per variable
        sabs = np.abs(x).sum(axis=4)
        phys_max = np.abs(res["diag"]["zonal"].numpy()).max(axis=(0, 1, 2, 4))
        ztol = ztol + ((2 * (W + 1) + 1) * U24 * sabs.max(axis=(0, 1, 3)) + W * gather) * scale / W + U24 * phys_max
        wtol = wtol + (2 * (nwin + 1) * U24 * np.abs(x[:, w0:w1]).sum(axis=1).max(axis=(0, 2, 3)) + nwin * gather) / nwin * scale
    for k in ("rmse_global", "rmse_trade_winds", "rmse_south_westerlies", "rmse_window"):
        g, r = res[k].numpy(), ps[k]
        tol = (wtol if k == "rmse_window" else ztol) + 1e-12 * np.abs(r)
        assert np.isfinite(r).all() and np.isfinite(g).all(), (k, g, r)           # (32 rows: no band is empty)
        print(f"end to end {k}: err / bound {(np.abs(g - r) / tol).max():.3f}")
        assert (np.abs(g - r) <= tol).all(), (k, g, r, tol)


def test_evaluate_dlwp_convlstm(cuda):
    from dlwp_benchmark_amd import dlwpbench, evaluate, wbdata
    ds, phys, months = dated_dataset(32, 64)
    clim, count = evaluate.monthly_climatology(torch.from_numpy(phys).to(cuda), months)
    assert count.cpu().numpy().tolist() == [20, 28] + [0] * 10
    torch.manual_seed(5)
    model = dlwpbench.ConvLSTM(constant_channels=4, prescribed_channels=1, prognostic_channels=8, hidden_sizes=[8, 8],
                               context_size=1).to(cuda)
    res = evaluate.evaluate_dlwp(model, ds, 2, climatology=clim, window_days=(0.5, 1))
    outs, tars = [], []
    with torch.no_grad():
        for items in ([0, 1], [2]):
            c, p, g, t = wbdata.to_device_batch([ds[i] for i in items], cuda)
            outs.append(model(c, p, g).cpu().numpy())
            tars.append(t.cpu().numpy())
    lats = R.lat_coordinate(32)
    ref, xo, xt, scale = e2e_reference(ds, np.concatenate(outs), np.concatenate(tars), clim.cpu().numpy(), lats,
                                       lambda a: np.asarray(a, dtype=np.float64))
    assert tuple(res["rmse"].shape) == (6, 8)
    check_e2e(res, ref, xo, xt, scale)
    # the baselines run through the same driver
    per = evaluate.evaluate_dlwp(model, ds, 3, forecast="persistence", climatology=clim, window_days=(0.5, 1))
    tar = np.concatenate(tars)
    prog0 = np.stack([ds[i][2][0] for i in range(3)])
    pref, pxo, pxt, _ = e2e_reference(ds, R.persistence(prog0, 6), tar, clim.cpu().numpy(), lats, lambda a: np.asarray(a, dtype=np.float64))
    check_e2e(per, pref, pxo, pxt, scale)
    cl = evaluate.evaluate_dlwp(None, ds, 3, forecast="climatology", climatology=clim, window_days=(0.5, 1), device=cuda)
    scale_, shift_ = evaluate.dataset_scale_shift(ds)
    cphys = R.climatology_forecast(clim.cpu().numpy(), R.forecast_months(ds.init_dates, 6, DT))
    cref = R.rmse_acc(cphys, R.denormalise(tar, scale_, shift_), lats)
    np.testing.assert_allclose(cl["rmse"].numpy(), cref["rmse"], rtol=2e-5)


def test_evaluate_dlwp_convlstm_hpx(cuda):
    from dlwp_benchmark_amd import dlwpbench, evaluate, wbdata
    from dlwp_benchmark_amd.hpx_remap import HEALPixRemap
    remap = HEALPixRemap(latitudes=32, longitudes=64, nside=2, device=cuda)      # (32 rows: every latitude band has members)
    ds, phys, months = dated_dataset(32, 64, fields_map=remap.remap_fields)
    clim, _ = evaluate.monthly_climatology(torch.from_numpy(phys).to(cuda), months)
    torch.manual_seed(6)
    model = dlwpbench.ConvLSTMHPX(constant_channels=4, prescribed_channels=1, prognostic_channels=8, hidden_sizes=[8, 8],
                                  context_size=1).to(cuda)
    res = evaluate.evaluate_dlwp(model, ds, 2, remap=remap, climatology=clim, window_days=(0.5, 1))
    outs, tars = [], []
    with torch.no_grad():
        for items in ([0, 1], [2]):
            c, p, g, t = wbdata.to_device_batch([ds[i] for i in items], cuda)
            outs.append(model(c, p, g).cpu().numpy())
            tars.append(t.cpu().numpy())
    idx, w = remap._hpx2ll.idx.cpu().numpy().reshape(-1, 4), remap._hpx2ll.w.cpu().numpy().reshape(-1, 4)

    def to_latlon(a):
        return HR.apply_table(idx, w, a.reshape(a.shape[:3] + (-1,))).reshape(a.shape[:3] + (32, 64))

    outs, tars = np.concatenate(outs), np.concatenate(tars)
    ref, xo, xt, scale = e2e_reference(ds, outs, tars, clim.cpu().numpy(), remap.lats_deg, to_latlon)
    assert tuple(res["rmse"].shape) == (6, 8)
    check_e2e(res, ref, xo, xt, scale, gather=7 * U24 * max(np.abs(outs).max(), np.abs(tars).max()))
