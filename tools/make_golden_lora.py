"""Write tests/golden/lora_layers.json: which layers the reference's `ft_strategy` rules select on the reference's OWN
VideoUNet (built under the meta device through oracle.ref_shim), for the TINY and the Kubric configuration.

    python tools/make_golden_lora.py

Per configuration: `time_lora` — the (qualified name, out_features, in_features) of every nn.Linear that the walk of
sgm/models/diffusion.py:137-151 yields, in the walk's order; `time` — how many parameters keep requires_grad under the
rule of diffusion.py:127-133, and how many there are; `dummy` — the names left trainable by diffusion.py:159-168.
The file holds names and numbers only.  Needs the reference tree; tests read the file, never the tree."""
import json
import sys
from pathlib import Path

import torch
from torch import nn

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import ref_shim, svd_unet_ref as O  # noqa: E402

OUT = ROOT / "tests" / "golden" / "lora_layers.json"


def walk(net):
    for parent_name, parent_module in net.named_modules():
        for name, module in parent_module.named_children():
            if "time" in name or "time" in parent_name:
                if isinstance(module, nn.Linear):
                    yield f"{parent_name}.{name}" if parent_name else name, module


def main() -> None:
    VideoUNet = ref_shim.reference_classes()[0]
    out = {}
    for label, cfg in (("TINY", O.TINY), ("KUBRIC", O.KUBRIC)):
        with torch.device("meta"):
            net = VideoUNet(**cfg.as_reference_kwargs())
        layers = [[n, m.out_features, m.in_features] for n, m in walk(net)]
        names = [n for n, _ in net.named_parameters()]
        out[label] = {
            "time_lora": layers,
            "adapted_parameters": sum(N * K for _, N, K in layers),
            "parameters": sum(p.numel() for p in net.parameters()),
            "time": {"trainable": sum("time" in n for n in names), "tensors": len(names)},
            "dummy": [n for n in names if "output_blocks.11.1.time_mixer.mix_factor" in n],
        }
        print(label, len(layers), "adapted Linears,", out[label]["adapted_parameters"], "of", out[label]["parameters"], "parameters;",
              "time:", out[label]["time"])
    OUT.write_text(json.dumps(out, indent=0) + "\n")
    print("wrote", OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
