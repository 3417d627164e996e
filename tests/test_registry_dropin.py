"""INTEGRATION.md §2 end to end, in a fresh interpreter (tests/registry_dropin_check.py): the host's
build_pixel_decoder / build_transformer_decoder return the bm2f classes after the documented import, a
reference state_dict loads strictly, and the outputs match the reference's fixtures.  Self-contained: the host
framework is stood in for, and the reference's state_dict names and shapes are recorded under tests/golden/."""
import os
import subprocess
import sys


def test_registry_dropin_with_reference_builders():
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "registry_dropin_check.py")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "registry drop-in ok" in r.stdout
