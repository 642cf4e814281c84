#!/usr/bin/env python3
"""The face-packed HEALPix 3 x 3 kernels (csrc/conv3x3_hpx_packed.hip) against the default HEALPix kernels (csrc/conv3x3.hip) on
the shapes of the lower U-Net levels: 16 spheres, faces of 2, 4 and 8 pixels (and 1, which only the packed kernels take),
184 -> 184 channels and 16 + 16 -> 16 channels; forward, input gradient (product + fold) and weight gradient (product + fold)
through the raw entry points.

Method: per quantity and family three runs, ALTERNATING between the families (default, packed, default, packed, ...), each run
`--launches` back-to-back launches between two device events after a warm-up; reported per launch: the median of the three runs
and their spread (max - min).  One JSON line per shape and quantity.

    python tools/bench_conv_hpx_packed.py [--launches 300] [--out profiles/conv_hpx_packed.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPHERES = 16
SHAPES = [(184, 0, 184), (16, 16, 16)]      # (C1, C2, Cout)


def timed(fn, launches):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / launches      # microseconds per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--faces", default="1,2,4,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_hpx_packed.json"))
    a = ap.parse_args()
    from dlwp_benchmark_amd import conv_ops, lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    B = 12 * SPHERES
    lines = []
    for n in (int(v) for v in a.faces.split(",")):
        for C1, C2, Cout in SHAPES:
            g = torch.Generator().manual_seed(n * 1000 + Cout)
            r = lambda *s: torch.randn(*s, generator=g).to(dev)      # noqa: E731
            C = C1 + C2
            x1, x2 = r(B, n, n, C1), (r(B, n, n, C2) if C2 else None)
            w, b, dz = r(Cout, C, 3, 3) / (3.0 * C ** 0.5), r(Cout), r(B, n, n, Cout)
            pk = conv_ops.PackedWeight(w)
            y, g1 = torch.empty(B, n, n, Cout, device=dev), torch.empty(B, n, n, C1, device=dev)
            g2 = torch.empty(B, n, n, C2, device=dev) if C2 else None
            gw, gb = torch.zeros_like(w), torch.zeros_like(b)
            s = L.stream()
            rows = conv_ops._hpx_rows(n, dev)
            wsG = torch.empty(lib.dlwp_conv3x3_hpxp_dgrad_ws_floats(B, n, C), device=dev)
            wsWp = torch.empty(lib.dlwp_conv3x3_hpxp_wgrad_ws_floats(B, n, C, Cout), device=dev)
            P = L.ptr
            fam = {"packed": {
                "forward": lambda: L.check(lib.dlwp_conv3x3_hpxp_fwd(P(x1), P(x2), P(pk.fwd), P(b), P(y), None, B, n, n, C1, C2, Cout, 0, 2, s)),
                "input_gradient": lambda: L.check(lib.dlwp_conv3x3_hpxp_dgrad(P(dz), P(pk.dgrad), rows.data_ptr(), rows.shape[-1], P(wsG),
                                                                              P(g1), P(g2), B, n, Cout, C1, C2, s)),
                "weight_gradient": lambda: L.check(lib.dlwp_conv3x3_hpxp_wgrad(P(x1), P(x2), P(dz), P(wsWp), P(gw), P(gb), B, n, C1, C2,
                                                                               Cout, s))}}
            if n >= 2:
                table = conv_ops._hpx_table(n, dev)
                wsW = torch.empty(lib.dlwp_conv3x3_wgrad_ws_floats(B, n, n, C, Cout), device=dev)
                fam["default"] = {
                    "forward": lambda: L.check(lib.dlwp_conv3x3_fwd(P(x1), P(x2), P(pk.fwd), P(b), P(y), None, B, n, n, C1, C2, Cout, 0, 2, 2,
                                                                    2, s)),
                    "input_gradient": lambda: L.check(lib.dlwp_conv3x3_hpx_dgrad(P(dz), P(pk.dgrad), table.data_ptr(), P(wsG), P(g1), P(g2),
                                                                                 B, n, Cout, C1, C2, s)),
                    "weight_gradient": lambda: L.check(lib.dlwp_conv3x3_wgrad(P(x1), P(x2), P(dz), P(wsW), P(gw), P(gb), B, n, n, C1, C2,
                                                                              Cout, 2, 2, s))}
            for q in ("forward", "input_gradient", "weight_gradient"):
                runs = {k: [] for k in fam}
                for _ in range(3):
                    for k in sorted(fam):                          # default, packed, default, packed, ...
                        runs[k].append(timed(fam[k][q], a.launches))
                line = {"spheres": SPHERES, "face": n, "channels": f"{C1}+{C2}->{Cout}" if C2 else f"{C1}->{Cout}", "quantity": q,
                        "launches_per_run": a.launches}
                for k, v in runs.items():
                    line[k + "_us"] = round(statistics.median(v), 2)
                    line[k + "_spread_us"] = round(max(v) - min(v), 2)
                    line[k + "_runs_us"] = [round(t, 2) for t in v]
                if "default" in runs:
                    line["packed_over_default"] = round(line["packed_us"] / line["default_us"], 3)
                    line["packed_wins_beyond_default_spread"] = bool(line["default_us"] - line["packed_us"] > line["default_spread_us"])
                lines.append(line)
                print(json.dumps(line), flush=True)
                os.makedirs(os.path.dirname(a.out), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
