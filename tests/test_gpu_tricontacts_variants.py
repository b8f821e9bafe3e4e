"""Triangle contact queries on scenes of other magnitudes (tests/variants.py): the generated mesh tiny, far from the
origin, huge, anisotropic, and cut down to one, two and nine triangles, with 64 queries of trisweep_ref.fixture_seeded
each, k = 4 with count_all: kernel="strict" and kernel="fast" both give the yardstick's bits, and the fast kernel walked
the wide view for every query inside its stated domain."""
import functools

import numpy as np
import pytest

from tests import tricontacts_ref as tc
from tests import trisweep_ref as tr
from tests import variants

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ["tiny", "far", "huge", "aniso", "few1", "few2", "few9"]
NQ = 64
K = 4


@functools.lru_cache(maxsize=None)
def expectations(name):
    c = variants.coords(name)
    q, d = tr.fixture_seeded(c, NQ, 59)
    assert np.isfinite(q).all() and np.isfinite(d).all()
    mem = tc.members(q, d, c)
    return c, q, d, mem, tc.lists(mem, q, K, count_all=True)


def test_the_variants_test_something():
    for name in NAMES:
        c, q, d, mem, want = expectations(name)
        found, full = int((mem.total > 0).sum()), int((mem.total > K).sum())
        print(name, "found", found, "more than k members", full, "members", int(mem.total.sum()))
        # (huge: every triple product of its coordinates overflows float32: every set is empty, as the header says;
        # few1 and few2 have fewer triangles than k, and few9's nine rarely give a query more than k members)
        assert found >= (0 if name == "huge" else 16), name
        assert full >= {"huge": 0, "few1": 0, "few2": 0, "few9": 1}.get(name, 8), name
        assert tr.domain(q, d, max(16.0, float(np.abs(c).max()))).all(), name


@pytest.mark.parametrize("kernel", ["strict", "fast"])
@pytest.mark.parametrize("name", NAMES)
def test_tricontacts_match_the_yardstick(name, kernel):
    import torch
    from prt import device
    assert device.device_count() > 0, "no GPU visible"
    c, q, d, mem, want = expectations(name)
    r = device.Renderer(0).upload(variants.scene(name))
    kind = torch.empty((NQ, K), dtype=torch.int32, device="cuda")
    tri, t, count, point = r.sweep_tri_contacts(torch.from_numpy(q.copy()).cuda(), torch.from_numpy(d.copy()).cuda(),
                                                k=K, count_all=True, points_out=True, kernel=kernel, kind=kind)
    info = r.tricontacts_info()
    np.testing.assert_array_equal(tri.cpu().numpy(), want[0], err_msg=name)
    assert tc.same_bits(t.cpu().numpy(), want[1]) and tc.same_bits(point.cpu().numpy(), want[2]), name
    np.testing.assert_array_equal(kind.cpu().numpy(), want[3], err_msg=name)
    np.testing.assert_array_equal(count.cpu().numpy(), want[4], err_msg=name)
    assert info["triangles"] == NQ and info["stack_overflows"] == 0 and info["found"] == int((mem.total > 0).sum())
    assert info["counted"] == int(mem.total.sum()) and info["stored"] == int(np.minimum(mem.total, K).sum()), info
    if kernel == "fast":
        assert info["walked"] == NQ and info["exhaustive"] == 0, info
    else:
        assert info["exhaustive"] == NQ and info["pairs_tested"] == NQ * len(c), info
    r.close()
