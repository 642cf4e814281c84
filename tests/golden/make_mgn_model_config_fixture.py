#!/usr/bin/env python3
"""Constructor kwargs of the reference's two shipped MeshGraphNet configs, as a JSON fixture.

Reads src/{nsbench,dlwpbench}/configs/model/meshgraphnet.yaml of the reference (a config schema is data, not code) and writes
tests/golden/shipped_mgn_model_configs.json.  The files hold three interpolations, resolved here the way the apps' default data
groups do: `graph.height` / `graph.width` = the grid (64 x 64 / 32 x 64); `device` is dropped (the tests pass their own).
`parameters` records the names and shapes of the reference's own class built from those keywords on a SMALL grid (the parameters
do not depend on the grid; the reference builds its edge features in a Python loop over the edges), in state_dict order.

    python tests/golden/make_mgn_model_config_fixture.py
"""
import json
import os
import sys

import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_mgn_golden import REF, construct, load_reference  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shipped_mgn_model_configs.json")
GRID = {"nsbench": [64, 64], "dlwpbench": [32, 64]}


def main():
    out, classes = {}, load_reference()
    for app, grid in GRID.items():
        with open(f"{REF}/{app}/configs/model/meshgraphnet.yaml") as f:
            cfg = yaml.safe_load(f)
        assert cfg.pop("device") == "${device}" and cfg["graph"] == {"height": "${data.height}", "width": "${data.width}", "periodic": True}
        assert not any(isinstance(v, str) and "${" in v for v in cfg.values()), cfg
        net = construct(classes["ns" if app == "nsbench" else "dlwp"], dict(cfg, graph=dict(height=4, width=8, periodic=True)))
        cfg["graph"] = {"height": grid[0], "width": grid[1], "periodic": True}
        out[f"{app}/meshgraphnet"] = {"source": f"src/{app}/configs/model/meshgraphnet.yaml", "grid": grid, "kwargs": cfg,
                                      "parameters": [[k, list(v.shape)] for k, v in net.state_dict().items()]}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", OUT, len(out), "configs")


if __name__ == "__main__":
    main()
