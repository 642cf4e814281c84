#!/usr/bin/env python3
"""Constructor kwargs of the reference's shipped dlwpbench GraphCast config, as a JSON fixture.

Reads src/dlwpbench/configs/model/graphcast.yaml of the reference (a config schema is data, not code) and writes
tests/golden/shipped_graphcast_dlwp_model_config.json.  `meshgraph_path` names a file the reference does not ship
(models/graphcast/icospheres_l3.json): the fixture records its level, 3, and the tests write the file themselves.  `parameters`
records the names and shapes of the reference's own class built from those keywords on a SMALL grid and a level-1 file (the
parameters depend on neither), in state_dict order.

    python tests/golden/make_graphcast_dlwp_config_fixture.py
"""
import json
import os
import sys
import tempfile

import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_graphcast_dlwp_golden import REF, gc_mesh, load_reference  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shipped_graphcast_dlwp_model_config.json")


def main():
    _, cls = load_reference()
    with open(f"{REF}/dlwpbench/configs/model/graphcast.yaml") as f:
        cfg = yaml.safe_load(f)
    assert cfg["meshgraph_path"] == "models/graphcast/icospheres_l3.json"
    assert not any(isinstance(v, str) and "${" in v for v in cfg.values()), cfg
    grid = [cfg["input_height"], cfg["input_width"]]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "icospheres_l1.json")
        gc_mesh.write_icospheres(path, 1)
        net = cls(**dict(cfg, meshgraph_path=path, input_height=8, input_width=15))
    out = {"dlwpbench/graphcast": {"source": "src/dlwpbench/configs/model/graphcast.yaml", "grid": grid, "icosphere_level": 3,
                                   "kwargs": cfg, "parameters": [[k, list(v.shape)] for k, v in net.state_dict().items()]}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", OUT, len(out["dlwpbench/graphcast"]["parameters"]), "parameters")


if __name__ == "__main__":
    main()
