"""Triangle sweep queries on scenes of other magnitudes (tests/variants.py): the generated mesh tiny, far from the
origin, huge, anisotropic, and cut down to one, two and nine triangles, with 64 queries of trisweep_ref.fixture_seeded
each: kernel="strict" and kernel="fast" both give the yardstick's bits, and the fast kernel walked the wide view for
every query inside its stated domain."""
import functools

import numpy as np
import pytest

from tests import trisweep_ref as tr
from tests import variants

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["tiny", "far", "huge", "aniso", "few1", "few2", "few9"]
NQ = 64


@functools.lru_cache(maxsize=None)
def expectations(name):
    c = variants.coords(name)
    q, d = tr.fixture_seeded(c, NQ, 59)
    assert np.isfinite(q).all() and np.isfinite(d).all()
    return c, q, d, tr.expected(q, d, c)


def test_the_variants_test_something():
    for name in NAMES:
        c, q, d, want = expectations(name)
        found = int((want[0] >= 0).sum())
        print(name, "found", found, "kinds", np.bincount(want[3][want[0] >= 0], minlength=16).tolist())
        # (huge: every triple product of its coordinates overflows float32, so no candidate and no crossing test is
        # valid and every answer is empty, as the header says; what it tests is that the kernels make the same NaNs)
        assert found >= (0 if name == "huge" else 16), name
        assert tr.domain(q, d, max(16.0, float(np.abs(c).max()))).all(), name


@pytest.mark.parametrize("kernel", ["strict", "fast"])
@pytest.mark.parametrize("name", NAMES)
def test_trisweep_matches_the_yardstick(name, kernel):
    import torch
    from prt import device
    assert device.device_count() > 0, "no GPU visible"
    c, q, d, want = expectations(name)
    r = device.Renderer(0).upload(variants.scene(name))
    kind = torch.empty(NQ, dtype=torch.int32, device="cuda")
    tri, t, point = r.sweep_tris(torch.from_numpy(q.copy()).cuda(), torch.from_numpy(d.copy()).cuda(), kernel=kernel,
                                 kind=kind)
    info = r.trisweep_info()
    np.testing.assert_array_equal(tri.cpu().numpy(), want[0], err_msg=name)
    assert tr.same_bits(t.cpu().numpy(), want[1]) and tr.same_bits(point.cpu().numpy(), want[2]), name
    np.testing.assert_array_equal(kind.cpu().numpy(), want[3], err_msg=name)
    assert info["triangles"] == NQ and info["stack_overflows"] == 0 and info["found"] == int((want[0] >= 0).sum())
    if kernel == "fast":
        assert info["walked"] == NQ and info["exhaustive"] == 0, info
    else:
        assert info["exhaustive"] == NQ and info["pairs_tested"] == NQ * len(c), info
    r.close()
