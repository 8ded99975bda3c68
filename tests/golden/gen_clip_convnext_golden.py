"""Writes tests/golden/ref_state_shapes_clip_convnext.json: names and shapes of the state dict of the CLIP backbone
(ov_dvis/backbones/clip.py: ``clip_model.*``) for the two ConvNeXt rows of the model table, taken from the LITERAL timm / open_clip
composition of tests/convnext_cases.py built on the meta device (no weights are allocated or stored).

    python tests/golden/gen_clip_convnext_golden.py

Neither open_clip nor timm is available where this was written, so the literal model — and with it this fixture — is written from
their published definitions and is UNVERIFIED against a real laion2b_s29b_b131k_ft_soup checkpoint.  An integrator who
has open_clip can regenerate the fixture from ``open_clip.create_model(name).state_dict()`` and compare."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import convnext_cases as K      # noqa: E402

# open_clip model configs: timm trunk dims / depths, embed_dim, timm_proj, text width / heads / layers
MODELS = {
    "convnext_base_w": dict(dims=(128, 256, 512, 1024), depths=(3, 3, 27, 3), embed=640, head="linear", text=(640, 10, 12)),
    "convnext_large_d_320": dict(dims=(192, 384, 768, 1536), depths=(3, 3, 27, 3), embed=768, head="mlp", text=(768, 12, 16)),
}

if __name__ == "__main__":
    out = {}
    for name, mc in MODELS.items():
        with torch.device("meta"):
            model = K.LitCLIP(**mc, context=77, vocab=49408)
        out[name] = {"clip_model." + k: list(v.shape) for k, v in sorted(model.state_dict().items())}
    with open(os.path.join(HERE, "ref_state_shapes_clip_convnext.json"), "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(name) + ": {\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in sd.items())
                                   + "\n}" for name, sd in sorted(out.items())) + "\n}\n")       # one key per line
    print({k: len(v) for k, v in out.items()})
