"""Drop-in check of INTEGRATION.md §2, run in a fresh interpreter by tests/test_registry_dropin.py (CPU).

Self-contained: the host framework is stood in for here, with what the check depends on recorded from the reference
under tests/golden/ (state_dict_shapes.json: the name and shape of every state_dict entry of the reference's pixel
decoder and decoder; pixdec.npz / decoder.npz: their inputs and outputs).

The order is the one the documented recipe produces: the host's registry module
(maskformer_transformer_decoder.py:16) and its own decoder / pixel decoder classes register first, then bm2f's
classes are imported -- as the edited ``__init__.py`` files would import them -- and replace those entries.
Then the host's builders, ``build_pixel_decoder`` (pixel_decoder/fpn.py:21-33) and
``build_transformer_decoder`` (maskformer_transformer_decoder.py:22-27) -- a registry lookup by the name in the
config, then ``Cls(cfg, ...)`` -- are called with a config; they must return the bm2f classes.  A reference
state_dict (the recorded names and shapes, filled by tests/golden/filler.py as the fixtures were made) loads strictly
into each, and the outputs match the reference's golden fixtures on CPU (the oracle's MSDA / decoder restatements
stand in for the HIP kernels here).

The stand-ins mirror the host's behaviour where the check depends on it: the registry raises on a duplicate name
like detectron2's Registry, ``configurable`` routes a cfg through ``from_config``, and the host's registry module
sits in ``sys.modules`` under the reference's module name, holding classes with the reference's names.
"""
import functools
import os
import sys
import types
from collections import namedtuple

import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE, os.path.join(HERE, "golden")]


def install_detectron2_standins():
    class Registry:
        def __init__(self, name):
            self._name, self._obj_map = name, {}

        def _do_register(self, name, obj):
            if name in self._obj_map:  # detectron2/fvcore Registry behaviour
                raise AssertionError(f"An object named '{name}' was already registered in '{self._name}' registry!")
            self._obj_map[name] = obj

        def register(self, obj=None):
            if obj is None:
                def deco(o):
                    self._do_register(o.__name__, o)
                    return o
                return deco
            self._do_register(obj.__name__, obj)
            return obj

        def get(self, name):
            return self._obj_map[name]

    def configurable(init_func=None, *, from_config=None):
        def wrap(init):
            @functools.wraps(init)
            def wrapped(self, *args, **kwargs):
                if args and hasattr(args[0], "MODEL"):
                    init(self, **type(self).from_config(*args, **kwargs))
                else:
                    init(self, *args, **kwargs)
            return wrapped
        return wrap(init_func) if init_func is not None else wrap

    class Conv2d(nn.Conv2d):
        def __init__(self, *args, **kwargs):
            norm, activation = kwargs.pop("norm", None), kwargs.pop("activation", None)
            super().__init__(*args, **kwargs)
            self.norm, self.activation = norm, activation

        def forward(self, x):
            x = F.conv2d(x, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups)
            if self.norm is not None:
                x = self.norm(x)
            if self.activation is not None:
                x = self.activation(x)
            return x

    def get_norm(norm, out_channels):
        return None if not norm else nn.GroupNorm(32, out_channels)

    ShapeSpec = namedtuple("ShapeSpec", ["channels", "height", "width", "stride"], defaults=[None] * 4)
    mods = {n: types.ModuleType(n) for n in [
        "detectron2", "detectron2.config", "detectron2.layers", "detectron2.modeling", "detectron2.utils",
        "detectron2.utils.registry", "fvcore", "fvcore.nn", "fvcore.nn.weight_init"]}
    mods["detectron2.config"].configurable = configurable
    mods["detectron2.layers"].Conv2d = Conv2d
    mods["detectron2.layers"].ShapeSpec = ShapeSpec
    mods["detectron2.layers"].get_norm = get_norm
    mods["detectron2.layers"].DeformConv = None
    mods["detectron2.modeling"].SEM_SEG_HEADS_REGISTRY = Registry("SEM_SEG_HEADS")
    mods["detectron2.utils.registry"].Registry = Registry
    mods["fvcore.nn.weight_init"].c2_xavier_fill = lambda m: None
    mods["fvcore.nn"].weight_init = mods["fvcore.nn.weight_init"]
    sys.modules.update(mods)
    return ShapeSpec


TD_MODULE = "mask2former.modeling.transformer_decoder.maskformer_transformer_decoder"


def install_host_standins():
    """The host's registry module under the reference's name, with same-name decoder / pixel-decoder classes
    registered first, and its two builders.  Returns (module, build_pixel_decoder, build_transformer_decoder)."""
    from detectron2.modeling import SEM_SEG_HEADS_REGISTRY
    from detectron2.utils.registry import Registry
    for pkg in ("mask2former", "mask2former.modeling", "mask2former.modeling.transformer_decoder"):
        sys.modules[pkg] = types.ModuleType(pkg)
    td = types.ModuleType(TD_MODULE)
    td.TRANSFORMER_DECODER_REGISTRY = Registry("TRANSFORMER_MODULE")
    sys.modules[TD_MODULE] = td

    @td.TRANSFORMER_DECODER_REGISTRY.register()
    class MultiScaleMaskedTransformerDecoder(nn.Module):     # the host's own class, registered first
        pass

    @SEM_SEG_HEADS_REGISTRY.register()
    class MSDeformAttnPixelDecoder(nn.Module):
        pass

    def build_pixel_decoder(cfg, input_shape):
        model = SEM_SEG_HEADS_REGISTRY.get(cfg.MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME)(cfg, input_shape)
        assert callable(getattr(model, "forward_features", None))
        return model

    def build_transformer_decoder(cfg, in_channels, mask_classification=True):
        name = cfg.MODEL.MASK_FORMER.TRANSFORMER_DECODER_NAME
        return td.TRANSFORMER_DECODER_REGISTRY.get(name)(cfg, in_channels, mask_classification)

    td.HostDecoder, td.HostPixdec = MultiScaleMaskedTransformerDecoder, MSDeformAttnPixelDecoder
    return td, build_pixel_decoder, build_transformer_decoder


def reference_state_dict(which):
    """The reference module's state_dict, re-created from its recorded names and shapes by the fixtures' filler."""
    import json
    from filler import fill_value
    with open(os.path.join(HERE, "golden", "state_dict_shapes.json")) as f:
        shapes = json.load(f)[which]
    return {k: fill_value(k, shape).to(torch.float32) for k, shape in shapes.items()}


def main():
    ShapeSpec = install_detectron2_standins()
    # bm2f's module stands in for the compiled MultiScaleDeformableAttention
    import bm2f_amd.msda
    sys.modules["MultiScaleDeformableAttention"] = bm2f_amd.msda
    td, build_pixel_decoder, build_transformer_decoder = install_host_standins()
    from detectron2.modeling import SEM_SEG_HEADS_REGISTRY
    assert td.TRANSFORMER_DECODER_REGISTRY.get("MultiScaleMaskedTransformerDecoder") is td.HostDecoder
    assert SEM_SEG_HEADS_REGISTRY.get("MSDeformAttnPixelDecoder") is td.HostPixdec

    # the edited __init__.py files import bm2f's classes here
    from bm2f_amd.pixel_decoder import MSDeformAttnPixelDecoder
    from bm2f_amd.transformer_decoder import MultiScaleMaskedTransformerDecoder
    from bm2f_amd.bench_model import default_cfg

    cfg = default_cfg()
    shapes = {"res2": ShapeSpec(channels=256, stride=4), "res3": ShapeSpec(channels=512, stride=8),
              "res4": ShapeSpec(channels=1024, stride=16), "res5": ShapeSpec(channels=2048, stride=32)}
    pd = build_pixel_decoder(cfg, shapes)                           # the host's builder
    dec = build_transformer_decoder(cfg, 256, mask_classification=True)
    assert type(pd) is MSDeformAttnPixelDecoder, type(pd)
    assert type(dec) is MultiScaleMaskedTransformerDecoder, type(dec)

    from module_cases import oracle_msda, rel_err, run_decoder, run_pixdec
    from oracle.decoder_ref import torch_decoder_ops
    torch.manual_seed(0)
    pd.load_state_dict(reference_state_dict("pixdec"), strict=True)
    pd.train()
    with oracle_msda():
        g, feats, outs = run_pixdec(pd, torch.device("cpu"))
    for name, o in zip(["out_mask_features", "out_out0", "out_ms0", "out_ms1", "out_ms2"], outs):
        assert rel_err(o.detach(), g[name]) < 1e-4, name

    dec.load_state_dict(reference_state_dict("decoder"), strict=True)
    dec.train()
    with torch_decoder_ops():
        g, x, mf, logits, masks, _ = run_decoder(dec, torch.device("cpu"), "decoder.npz", False)
    assert rel_err(torch.stack([t.detach() for t in logits]), g["pred_logits"]) < 1e-4
    assert rel_err(torch.stack([t.detach() for t in masks]), g["pred_masks"]) < 1e-4
    print("registry drop-in ok")


if __name__ == "__main__":
    main()
