#!/usr/bin/env python3
"""Constructor kwargs of the reference's shipped configs of the convolutional baselines, as a JSON fixture.

Reads src/{nsbench,dlwpbench}/configs/model/convlstm.yaml of the reference (a config schema is data, not code), resolves the
`${...}` interpolations against the default groups of each app (data: 64 x 64 / 32 x 64; training/default.yaml: batch_size 16;
config.yaml: device cuda:0) and writes tests/golden/shipped_conv_model_configs.json, which tests/test_gpu_convlstm.py builds
the classes from the way train.py does (`eval(cfg.model.type)(**cfg.model)`).

    python tests/golden/make_conv_model_config_fixture.py
"""
import json
import os

import yaml

REF = "/root/reference/src"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shipped_conv_model_configs.json")
MODELS = {"nsbench": ["convlstm"], "dlwpbench": ["convlstm"]}
ENV = {"nsbench": {"data.height": 64, "data.width": 64, "training.batch_size": 16, "device": "cuda:0"},
       "dlwpbench": {"data.height": 32, "data.width": 64, "training.batch_size": 16, "device": "cuda:0"}}


def resolve(v, env):
    if isinstance(v, str) and v.startswith("${") and v.endswith("}"):
        return env[v[2:-1]]
    return v


def main():
    out = {}
    for app, names in MODELS.items():
        for name in names:
            with open(f"{REF}/{app}/configs/model/{name}.yaml") as f:
                cfg = yaml.safe_load(f)
            out[f"{app}/{name}"] = {"source": f"src/{app}/configs/model/{name}.yaml",
                                    "kwargs": {k: resolve(v, ENV[app]) for k, v in cfg.items()}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", OUT, len(out), "configs")


if __name__ == "__main__":
    main()
