"""The device forms of rt_exact.hpp (the shading code's short division, root and normalize, and the branch-free
reciprocal of ray_pre) return the bits of `/`, sqrtf and rcp_ieee: tools/exact/exact_exhaustive (built by
the Makefile from the product header) checks on the GPU
  * the root over all 2^32 bit patterns,
  * the quotient for every denominator mantissa, 4,098 numerators each plus the exponent pairs at and beyond both ends of
    the guard (4 x 10^10 quotients),
  * normalize over 2^30 vectors across its guard's ends (zero components included),
  * the reciprocal over every float of magnitude <= 2,
in about a second. tests/test_exact_forms.py checks the host forms (the algebra and the guards) without a GPU; the frames
that use them are compared with the strict kernel in tests/test_gpu_exact_frames.py.
"""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "exact", "exact_exhaustive")


def test_short_forms_equal_ieee_on_the_device():
    assert os.path.exists(BIN), "tools/exact/exact_exhaustive missing: run `make` (build() does)"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {m.group(1): (int(m.group(2)), int(m.group(3)))
           for m in re.finditer(r"^(\w+) mismatches (\d+) of (\d+)", r.stdout, re.M)}
    assert got["root"] == (0, 1 << 32), r.stdout
    assert got["quotient"][0] == 0 and got["quotient"][1] >= 1 << 30, r.stdout
    assert got["normalize"] == (0, 1 << 30), r.stdout
    assert got["rcp_small"] == (0, 2 * ((1 << 30) + 1)), r.stdout
