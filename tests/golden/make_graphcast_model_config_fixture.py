#!/usr/bin/env python3
"""Constructor kwargs of the reference's shipped nsbench GraphCast config, as a JSON fixture.

Reads src/nsbench/configs/model/graphcast_ns.yaml of the reference (a config schema is data, not code) and writes
tests/golden/shipped_graphcast_model_configs.json.  The file holds four interpolations, resolved here the way the app's default
data group does: `input_height` / `input_width` = the grid (64 x 64), `downscale_factor` = 1; `device` is dropped (the tests pass
their own).  `parameters` records the names and shapes of the reference's own class built from those keywords on a SMALL grid
(the parameters do not depend on the grid; the reference builds its edge features in a Python loop over the edges), in
state_dict order.

    python tests/golden/make_graphcast_model_config_fixture.py
"""
import json
import os
import sys

import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_graphcast_ns_golden import REF, load_reference  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shipped_graphcast_model_configs.json")
GRID = [64, 64]


def main():
    cls = load_reference()
    with open(f"{REF}/nsbench/configs/model/graphcast_ns.yaml") as f:
        cfg = yaml.safe_load(f)
    assert cfg.pop("device") == "${device}"
    assert (cfg["input_height"], cfg["input_width"], cfg["downscale_factor"]) == ("${data.height}", "${data.width}",
                                                                                   "${data.downscale_factor}")
    cfg["downscale_factor"] = 1
    net = cls(device="cpu", **dict(cfg, input_height=6, input_width=6))
    cfg["input_height"], cfg["input_width"] = GRID
    assert not any(isinstance(v, str) and "${" in v for v in cfg.values()), cfg
    out = {"nsbench/graphcast_ns": {"source": "src/nsbench/configs/model/graphcast_ns.yaml", "grid": GRID, "kwargs": cfg,
                                    "parameters": [[k, list(v.shape)] for k, v in net.state_dict().items()]}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", OUT, len(out), "configs")


if __name__ == "__main__":
    main()
