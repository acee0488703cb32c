"""Fixtures of tests/test_engine_host.py and tests/test_engine_gpu.py: the `model:` sections of the reference's six
configs (gcd-model/configs/*.yaml) as tests/golden/configs/<name>.yaml, and the distinct `target:` strings they name as
tests/golden/configs/targets.txt.  Settings only: the `data:` and `lightning:` sections (dataset paths, logger and
trainer options) are dropped, comments go with the re-serialisation.  Run where the reference tree is present:

    python tools/make_golden_engine.py [path to gcd-model]
"""
from __future__ import annotations

import sys
from pathlib import Path

import yaml

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "configs"
NAMES = ("infer_kubric", "infer_pardom", "train_kubric_max90", "train_kubric_max180", "train_pardom_rgb",
         "train_pardom_semantic")


def targets_of(node, found=None) -> set:
    """Every `target:` value (and the `network_wrapper` string) below `node`."""
    found = set() if found is None else found
    if isinstance(node, dict):
        for k, v in node.items():
            if k in ("target", "network_wrapper") and isinstance(v, str):
                found.add(v)
            else:
                targets_of(v, found)
    elif isinstance(node, (list, tuple)):
        for v in node:
            targets_of(v, found)
    return found


def main(ref: Path) -> None:
    OUT.mkdir(parents=True, exist_ok=True)
    found = set()
    for name in NAMES:
        with open(ref / "configs" / f"{name}.yaml") as f:
            model = yaml.safe_load(f)["model"]
        found |= targets_of(model)
        with open(OUT / f"{name}.yaml", "w") as f:
            yaml.safe_dump({"model": model}, f, sort_keys=False, default_flow_style=None)
        print(f"{name}: {len(targets_of(model))} targets -> {OUT / (name + '.yaml')}")
    (OUT / "targets.txt").write_text("".join(t + "\n" for t in sorted(found)))
    print(f"{len(found)} distinct targets -> {OUT / 'targets.txt'}")


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(Path(sys.argv[1]))
    else:
        sys.path.insert(0, str(ROOT))
        from oracle.ref_shim import REF
        main(REF)
