#!/usr/bin/env python3
"""Constructor kwargs of the reference's two shipped U-Net configs, as a JSON fixture.

Reads src/{nsbench,dlwpbench}/configs/model/unet.yaml of the reference (a config schema is data, not code) and writes
tests/golden/shipped_unet_model_configs.json with the grid of each app's default data group (64 x 64 / 32 x 64) next to the
keywords; tests/test_unet_ref.py and tests/test_gpu_unet.py build the classes from it the way train.py does
(`eval(cfg.model.type)(**cfg.model)`).  Neither file has an interpolation to resolve.  `parameters` records the names and shapes
of the reference's own class built from those keywords (imported as in make_unet_golden.py), in state_dict order.

    python tests/golden/make_unet_model_config_fixture.py
"""
import json
import os
import sys

import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_unet_golden import load_reference  # noqa: E402

REF = "/root/reference/src"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shipped_unet_model_configs.json")
GRID = {"nsbench": [64, 64], "dlwpbench": [32, 64]}


def main():
    out, classes = {}, load_reference()
    for app, grid in GRID.items():
        with open(f"{REF}/{app}/configs/model/unet.yaml") as f:
            cfg = yaml.safe_load(f)
        assert not any(isinstance(v, str) and "${" in v for v in cfg.values()), cfg
        net = classes["ns" if app == "nsbench" else "dlwp"](**cfg)
        out[f"{app}/unet"] = {"source": f"src/{app}/configs/model/unet.yaml", "grid": grid, "kwargs": cfg,
                              "parameters": [[k, list(v.shape)] for k, v in net.state_dict().items()]}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", OUT, len(out), "configs")


if __name__ == "__main__":
    main()
