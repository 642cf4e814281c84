#!/usr/bin/env python3
"""Time of the spectra kernels (csrc/spectra.hip: dlwp_sphere_spectra, dlwp_plane_spectra) beside the torch composition they replace
and beside the HBM roof of their algorithmic bytes, in one run.

Shapes: the benchmark's one-year rollout, T = 1460 frames, V = 8 variables on 32 x 64 at --batch (default 8), analysed in time chunks
of --chunk frames through `state` (lat-lon planes, and HPX8 planes interpolated in the kernel); and Navier-Stokes vorticity rollouts
of 64 x 64 (B 16, T 50) and 256 x 256 (B 4, T 50).  Per case one JSON line:

    kernels      spectra.sphere_spectra / spectra.plane_spectra over all chunks (tables pre-allocated in the state)
    composition  torch with the SAME tables: sphere -- (HPX: HEALPixRemap.hpx2ll of both tensors,) torch.fft.rfft along longitude, the
                 first M orders times 2 pi / W, einsum with the complex image of Wf, c_m |a|^2 and the cross term summed over m;
                 plane -- torch.fft.rfft2, c |u|^2 and the cross term, torch.bincount with the shell index as bins
    roof         one read of outputs and targets at the 8 TB/s datasheet figure and at the 6.3 TB/s a float4 copy reaches

Method: device events around windows of back-to-back calls, every window at least --window seconds long (the repetition count is
found first), 3 warm-up calls each, the two routes alternating over --windows windows; median microseconds and [min, max].

    python tools/bench_spectra.py [--batch 8] [--frames 1460] [--chunk 365] [--window 0.3] [--windows 5] [--out profiles/spectra.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF_SPEC_TBS, ROOF_COPY_TBS = 8.0, 6.3


def window_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def compare(ours, base, window, windows):
    """alternating windows -> (median us ours, [min, max]), (median us baseline, [min, max])"""
    reps = []
    for fn in (ours, base):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps.append(max(3, int(window * 1e6 / max(window_us(fn, 3), 1e-3))))
    t = ([], [])
    for _ in range(windows):
        for k, fn in enumerate((ours, base)):
            t[k].append(window_us(fn, reps[k]))
    return [(statistics.median(x), [round(min(x), 1), round(max(x), 1)]) for x in t]


def report(case, shape, nbytes, ours, base, agree, kernels, args):
    (us, spread), (bus, bspread) = compare(ours, base, args.window, args.windows)
    line = {"case": case, "shape": shape, "kernels_us": round(us, 1), "kernels_us_min_max": spread, "composition_us": round(bus, 1),
            "composition_us_min_max": bspread, "composition_over_kernels": round(bus / us, 2), "algorithmic_bytes": nbytes,
            "roof_us_at_8TBs": round(nbytes / ROOF_SPEC_TBS / 1e6, 1), "roof_us_at_6.3TBs": round(nbytes / ROOF_COPY_TBS / 1e6, 1),
            "fraction_of_8TBs": round(nbytes / us / 1e6 / ROOF_SPEC_TBS, 4), "fraction_of_6.3TBs": round(nbytes / us / 1e6 / ROOF_COPY_TBS, 4),
            "kernels_one_pass": kernels, "max_rel_difference_to_composition": agree}
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=1460)
    ap.add_argument("--chunk", type=int, default=365)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_spectra: no GPU (timings on the CPU would say nothing)")
    from dlwp_benchmark_amd import hpx_remap, spectra
    from dlwp_benchmark_amd import lib as L
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())      # noqa: E731
    lines = []

    # ---- sphere: the one-year rollout in time chunks ----
    B, T, V, H, W, n = args.batch, args.frames, 8, 32, 64, 8
    rm = hpx_remap.HEALPixRemap(latitudes=H, longitudes=W, nside=n, device=dev)
    tab = spectra.sphere_tables(H, W, "midpoint", None, dev)
    Lm, M = tab["L"], tab["M"]
    cmv = torch.where(torch.arange(M, device=dev) == 0, 1.0, 2.0) / (4.0 * math.pi)
    chunks = [(t0, min(t0 + args.chunk, T)) for t0 in range(0, T, args.chunk)]
    for mesh in ("latlon", "hpx8"):
        plane = (H, W) if mesh == "latlon" else (12, n, n)
        # a chunked rollout hands over one tensor per chunk: both routes read the same pre-split chunks
        o = [torch.randn((B, t1 - t0, V) + plane, device=dev, generator=gen) for t0, t1 in chunks]
        t = [torch.randn((B, t1 - t0, V) + plane, device=dev, generator=gen) for t0, t1 in chunks]
        remap = rm if mesh != "latlon" else None
        state = {"st": None}

        def kernels():
            st = state["st"]
            for k, (t0, t1) in enumerate(chunks):
                st = spectra.sphere_spectra(o[k], t[k], remap=remap, state=st, t_begin=t0, T=T)
            st["frames"] = 0
            state["st"] = st
            return st

        def composition():
            po, pt, cr = [], [], []
            for k in range(len(chunks)):
                xo, xt = o[k], t[k]
                if remap is not None:
                    xo, xt = rm.hpx2ll(xo), rm.hpx2ll(xt)
                a = []
                for x in (xo, xt):
                    tm = torch.fft.rfft(x, dim=-1)[..., :M] * (2.0 * math.pi / W)                     # [B, Tc, V, H, M]
                    a.append(torch.einsum("mlk,btvkm->btvlm", tab["Wf"].to(tm.dtype), tm))
                po.append((a[0].abs() ** 2 * cmv).sum(-1))
                pt.append((a[1].abs() ** 2 * cmv).sum(-1))
                cr.append(((a[0] * a[1].conj()).real * cmv).sum(-1))
            return torch.cat(po, 1), torch.cat(pt, 1), torch.cat(cr, 1)

        with L.kernel_accounting() as acc:
            st = kernels()
            torch.cuda.synchronize()
        kern = {r["name"]: {"calls": r["calls"], "ms": round(r["ms"], 4)} for r in acc.rows}
        with torch.no_grad():
            po, pt, cr = composition()
            agree = {"power_out": rel(st["power"][0], po), "power_tgt": rel(st["power"][1], pt), "cross": rel(st["cross"], cr)}
            del po, pt, cr
            nbytes = 4.0 * B * T * V * int(np.prod(plane)) * 2
            lines.append(report(f"sphere_{mesh}", f"B {B}, T {T} in chunks of {args.chunk}, V {V}, {H}x{W}, L {Lm}, M {M}"
                                + (f", HPX{n}" if remap is not None else ""), nbytes, kernels, composition, agree, kern, args))
        del o, t, state
        torch.cuda.empty_cache()

    # ---- plane: Navier-Stokes vorticity rollouts ----
    for (Bn, Tn, Hn) in ((16, 50, 64), (4, 50, 256)):
        o = torch.randn(Bn, Tn, 1, Hn, Hn, device=dev, generator=gen)
        t = torch.randn(Bn, Tn, 1, Hn, Hn, device=dev, generator=gen)
        rowptr, entry, weight, K = spectra.plane_shells_host(Hn, Hn)
        shell = torch.empty(entry.size, dtype=torch.long)
        shell[torch.from_numpy(entry.astype(np.int64))] = torch.from_numpy(np.repeat(np.arange(K), np.diff(rowptr)))
        cw = torch.empty(entry.size)
        cw[torch.from_numpy(entry.astype(np.int64))] = torch.from_numpy(weight)
        shell, cw = shell.to(dev), (cw / float(Hn * Hn) ** 2).to(dev)
        nf = Bn * Tn
        bins = (torch.arange(nf, device=dev)[:, None] * K + shell[None, :]).reshape(-1)
        state = {"st": None}

        def kernels():
            st = spectra.plane_spectra(o, t, state=state["st"])
            st["frames"] = 0
            state["st"] = st
            return st

        def composition():
            uo, ut = torch.fft.rfft2(o).reshape(nf, -1), torch.fft.rfft2(t).reshape(nf, -1)
            out = []
            for z in (uo.abs() ** 2, ut.abs() ** 2, (uo * ut.conj()).real):
                out.append(torch.bincount(bins, weights=(z * cw).reshape(-1), minlength=nf * K).reshape(Bn, Tn, 1, K))
            return out

        with L.kernel_accounting() as acc:
            st = kernels()
            torch.cuda.synchronize()
        kern = {r["name"]: {"calls": r["calls"], "ms": round(r["ms"], 4)} for r in acc.rows}
        with torch.no_grad():
            po, pt, cr = composition()
            agree = {"power_out": rel(st["power"][0], po), "power_tgt": rel(st["power"][1], pt), "cross": rel(st["cross"], cr)}
            nbytes = 4.0 * nf * Hn * Hn * 2
            lines.append(report(f"plane_{Hn}", f"B {Bn}, T {Tn}, D 1, {Hn}x{Hn}, K {K}", nbytes, kernels, composition, agree, kern, args))
        del o, t, state
        torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
