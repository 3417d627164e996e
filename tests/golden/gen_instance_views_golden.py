"""Record Pillow's outputs for the cases of tests/instance_view_cases.py into tests/golden/instance_views.npz.

    python tests/golden/gen_instance_views_golden.py

Needs Pillow (12.2.0 where the fixture was made).  The masks are regenerated from seeds by the tests, so only the
outputs are stored, one bit per pixel."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import instance_view_cases as ivc  # noqa: E402


def main():
    import PIL
    store = ivc.golden_store(ivc.pil_view)
    store["pillow_version"] = np.frombuffer(PIL.__version__.encode(), dtype=np.uint8)
    path = os.path.join(HERE, "instance_views.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes,", len(store), "entries")


if __name__ == "__main__":
    main()
