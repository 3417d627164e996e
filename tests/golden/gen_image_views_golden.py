"""Record Pillow's outputs for the cases of tests/image_view_cases.py into tests/golden/image_views.npz.

    python tests/golden/gen_image_views_golden.py

Needs Pillow (12.2.0 where the fixture was made).  Inputs are regenerated from seeds by the tests, so only outputs are
stored: as a SHA-256 per case, whole for the few that the tests assemble into batches (image_view_cases.record)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import image_view_cases as ivc  # noqa: E402


def pil_resize(img, size):
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(img)).resize((size[1], size[0]), Image.BILINEAR))


def main():
    import PIL
    store = {"pillow_version": np.frombuffer(PIL.__version__.encode(), dtype=np.uint8)}
    for c in ivc.IMAGE_CASES:
        ivc.record(store, c["name"], ivc.pil_image(c))
    for c in ivc.LABEL_CASES:
        ivc.record(store, c["name"], ivc.pil_label(c))
    sources, _ = ivc.ragged_sources()
    for v in ivc.RAGGED_VIEWS:
        out = ivc.pil_image(v, np.ascontiguousarray(sources[v["source"]]))
        ivc.record(store, v["name"], out, full=True)
    # the sizes are literals here, worked by hand from ResizeShortestEdge's formula, not taken from the package
    img = ivc.tta_image()                                    # 20 x 30, min sizes 16 and 24, max 40
    for i, size in enumerate([(16, 24), (24, 36)]):
        ivc.record(store, f"tta{i}", np.moveaxis(pil_resize(img, size), 2, 0), full=True)
    a, b = ivc.prep_images()                                 # 20 x 30 -> 24 x 36; 31 x 18 -> 40 x 23 (41.33 > 40)
    ivc.record(store, "prep0", np.moveaxis(pil_resize(a, (24, 36)), 2, 0), full=True)
    ivc.record(store, "prep1", np.moveaxis(pil_resize(b, (40, 23)), 2, 0), full=True)
    path = os.path.join(HERE, "image_views.npz")
    np.savez_compressed(path, **ivc.finish(store))
    print(path, os.path.getsize(path), "bytes,", len(store), "entries")


if __name__ == "__main__":
    main()
