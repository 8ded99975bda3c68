"""Generate the g21 Swin fixtures from the reference's own D2SwinTransformer (BUILD CONTAINER ONLY, like gen_golden.py):

    python tests/golden/gen_swin_golden.py

writes tests/golden/g21_swin_w7.npz, g21_swin_w12.npz (image, res2..res5, stage 1's block-0 / block-1 outputs, meta) and
ref_state_shapes_swin.json (names and shapes of the reference's state dict).  No weights are stored: swin_cases.fill_weights
fills them from one seeded generator, here and in the tests alike.  Stubs beyond _ref_import's: un-vendored third-party names only
(timm.models.layers, detectron2.modeling) and an empty parent package, so no ``__init__`` of the reference runs."""
import collections.abc
import importlib
import itertools
import json
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_import as R                     # noqa: E402
import swin_cases as S                      # noqa: E402

MAX_BYTES = 1 << 20


def ref_swin():
    R.install()

    class DropPath(nn.Identity):
        def __init__(self, drop_prob=0.0):
            super().__init__()

    def to_2tuple(x):
        return tuple(x) if isinstance(x, collections.abc.Iterable) and not isinstance(x, str) else tuple(itertools.repeat(x, 2))

    tl = R._mod("timm.models.layers", DropPath=DropPath, to_2tuple=to_2tuple, trunc_normal_=nn.init.trunc_normal_)
    tm = R._mod("timm.models", layers=tl)
    R._mod("timm", models=tm)
    d2m = sys.modules["detectron2.modeling"]
    d2m.BACKBONE_REGISTRY = R._Registry("BACKBONE")
    d2m.Backbone = nn.Module
    d2m.ShapeSpec = R._ShapeSpec
    pkg = types.ModuleType("mask2former.modeling.backbone")
    pkg.__path__ = [f"{R.REF}/mask2former/modeling/backbone"]
    sys.modules["mask2former.modeling.backbone"] = pkg
    return importlib.import_module("mask2former.modeling.backbone.swin")


def main():
    swin = ref_swin()
    shapes = None
    for name in S.FIXTURES:
        ws, _ = S.FIXTURE_SPECS[name]
        cfg = S.swin_cfg(ws)
        model = S.fill_weights(swin.D2SwinTransformer(cfg, None), S.SEED)
        model.eval()                                # (the reference's train() returns None)
        image = S.fixture_image(name)
        got, hooks = {}, []
        for i, blk in enumerate(model.layers[0].blocks):
            hooks.append(blk.register_forward_hook(lambda mod, args, out, i=i: got.__setitem__(f"block{i}", out.detach())))
        with torch.no_grad():
            got.update(model(image))
        for h in hooks:
            h.remove()
        assert sorted(got) == ["block0", "block1", "res2", "res3", "res4", "res5"], sorted(got)
        maxes = {k: float(v.abs().max()) for k, v in got.items()}
        for k, v in maxes.items():
            assert 0.1 <= v <= 50, (name, k, v)         # so that an absolute 1e-3 bound means something
        s = cfg.MODEL.SWIN
        meta = {"cfg": {"WINDOW_SIZE": s.WINDOW_SIZE, "EMBED_DIM": s.EMBED_DIM, "DEPTHS": list(s.DEPTHS), "NUM_HEADS": list(s.NUM_HEADS)},
                "seed": S.SEED, "max_abs": maxes, "shapes": {k: list(v.shape) for k, v in got.items()}}
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, image=image.numpy(), meta=np.array(json.dumps(meta)), **{k: v.numpy() for k, v in got.items()})
        assert os.path.getsize(path) < MAX_BYTES, (path, os.path.getsize(path))
        print(name, os.path.getsize(path), "bytes", {k: round(v, 3) for k, v in maxes.items()})
        sd = {k: list(v.shape) for k, v in model.state_dict().items()}
        if shapes is None:
            shapes = {}
        shapes[name] = sd
    with open(os.path.join(HERE, "ref_state_shapes_swin.json"), "w") as f:
        json.dump(shapes, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
