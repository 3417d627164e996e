"""Record tests/golden/color_aug.npz: what the colour definitions (bm2f_amd/color_aug.py) and image_views on CPU
tensors give on the cases of tests/color_aug_cases.py, beside the literal numpy expressions of detectron2's
``convert`` and ``BlendTransform``.

    python tests/golden/gen_color_aug_golden.py

The recorded outputs come from this project's own numpy definition under the numpy named in the file ("numpy"), not
from cv2 or detectron2: neither was available.  They pin the definition, so that a later change of it, of numpy's
promotion rules or of the BLAS behind ``ndarray.dot`` shows up as a difference and not as silence.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import color_aug_cases as cc  # noqa: E402
from bm2f_amd import color_aug as ca, image_views  # noqa: E402


def main():
    out = {"numpy": np.array(np.__version__)}
    small = cc.random_image(24, 32, 11)
    small[0, :, :] = np.arange(0, 256, 8, dtype=np.uint8)[:, None]          # a row of greys
    out["small"] = small
    sweep = cc.sweep_image()
    for name, aug in cc.COLOR_CASES.items():
        out[f"small_{name}"] = ca.apply_color(small, aug)
        out[f"sweep_{name}"] = np.ascontiguousarray(ca.apply_color(sweep, aug)[::cc.SWEEP_STRIDE, ::cc.SWEEP_STRIDE])
    for a, b in ((0.5, 0), (1.5, 0), (1, 32), (1, -32)):
        out[f"literal_convert_{a}_{b}"] = cc.literal_convert(small, a, b)
    for w in (0.9, 1.1):
        for n, v in cc.literal_blends(small, w).items():
            out[f"literal_{n}_{w}"] = v
    out["small_hsv"] = ca.bgr2hsv(small)
    src = torch.from_numpy(cc.random_image(*cc.GEO_SOURCE, 3))
    for vname in cc.GEO_VIEWS:
        for fam in cc.FAMILIES:
            got, _ = image_views([src], [cc.geo_view(vname, cc.COLOR_CASES[fam])], out_dtype=torch.uint8,
                                 size_divisibility=cc.GEO_PAD, pad_value=7)
            out[f"geo_{vname}_{fam}"] = got[0].numpy()
    for mname, (shape, view) in cc.MEAN_CASES.items():
        src = torch.from_numpy(cc.random_image(*shape, 17))
        for aname, aug in cc.MEAN_AUGS.items():
            import dataclasses
            got, _ = image_views([src], [dataclasses.replace(view, color=aug)], out_dtype=torch.uint8)
            out[f"mean_{mname}_{aname}"] = got[0].numpy()
    path = os.path.join(HERE, "color_aug.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
