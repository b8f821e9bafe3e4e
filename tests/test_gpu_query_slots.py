"""The ten query families keep apart on one Renderer: each has its own counters, events and state (rt_ctx's query
slots, rt_hip.hip), so a query of one family changes no other family's info. Every family runs once with a count of
its own, then again, one after the other, while the other nine infos are held field for field. Also per family: an
empty query reports zeros, a refused one changes nothing. Queries come from car_only itself (triangle centroids, the
triangles, the committed camera's rays); what the queries answer is the other GPU tests' business."""
import numpy as np
import pytest

from prt import host

pytestmark = pytest.mark.gpu

W, H = 32, 16  # 512 camera rays: more than any count below
# a count per family, all different: none a multiple of 64 (a partial pass of a wave, a partial chunk), three past one
# chunk of 256; the second round's are different again, from the first round's too
FIRST = {"rays": 65, "shade": 97, "hits": 131, "nearest": 163, "neighbours": 197, "overlaps": 229, "sweep": 259,
         "contacts": 291, "cuts": 323, "clearance": 101}
SECOND = {name: n + 2 for name, n in FIRST.items()}
COUNTER = {"rays": "rays", "shade": "rays", "hits": "rays", "nearest": "points", "neighbours": "points",
           "overlaps": "boxes", "sweep": "spheres", "contacts": "spheres", "cuts": "triangles",
           "clearance": "triangles"}


def strip(info):
    return {k: v for k, v in info.items() if k != "kernel_ms"}


def same(a, b):
    return strip(a) == strip(b) and abs(a["kernel_ms"] - b["kernel_ms"]) < 1e-4


def test_the_query_families_share_no_slot():
    import torch
    from prt import device, rays
    assert device.device_count() > 0, "no GPU visible"
    scene = host.Scene.named("car_only").build_bvh(3)
    coords = scene.triangles["coords"]
    assert set(FIRST) == set(COUNTER) and len(set(FIRST.values()) | set(SECOND.values())) == 20
    assert all(65 <= n <= 330 and n % 64 for n in (*FIRST.values(), *SECOND.values()))
    assert sum(n > 256 for n in FIRST.values()) >= 2

    tris = torch.from_numpy(np.ascontiguousarray(coords[:: len(coords) // 400][:400], np.float32)).cuda()
    pts = tris.mean(dim=1).contiguous()  # centroids: points, box centres, sphere centres
    lo, hi = (pts - 0.05).contiguous(), (pts + 0.05).contiguous()
    down = torch.zeros_like(pts)
    down[:, 1] = -1.0
    o, d = rays.pinhole(host.camera(W, H), W, H)
    torch.cuda.synchronize()  # (these tensors are torch's work; the queries run on the renderer's stream)

    r = device.Renderer(0).upload(scene)
    run = {
        "rays": lambda n, **kw: r.trace_rays(o[:n], d[:n], **kw),
        "shade": lambda n, **kw: r.shade_rays(o[:n], d[:n], **kw),
        "hits": lambda n, **kw: r.trace_hits(o[:n], d[:n], max_hits=2, **kw),
        "nearest": lambda n, **kw: r.nearest(pts[:n], **kw),
        "neighbours": lambda n, **kw: r.nearest_tris(pts[:n], k=4, **kw),
        "overlaps": lambda n, **kw: r.overlaps(lo[:n], hi[:n], k=4, **kw),
        "sweep": lambda n, **kw: r.sweep(pts[:n], down[:n], 0.01, **kw),
        "contacts": lambda n, **kw: r.sweep_contacts(pts[:n], down[:n], 0.01, k=4, **kw),
        "cuts": lambda n, **kw: r.cuts(tris[:n], k=4, **kw),
        "clearance": lambda n, **kw: r.clearance(tris[:n], **kw),
    }
    info = {"rays": r.query_info, "shade": r.shade_info, "hits": r.hits_info, "nearest": r.nearest_info,
            "neighbours": r.neighbours_info, "overlaps": r.overlaps_info, "sweep": r.sweep_info,
            "contacts": r.contacts_info, "cuts": r.cuts_info, "clearance": r.clearance_info}
    names = list(FIRST)

    for name in names:  # before its first query a family has no info, whatever the families before it ran
        with pytest.raises(device.RtError, match="status -5"):
            info[name]()
        run[name](FIRST[name])
    held = {name: info[name]() for name in names}
    for name in names:
        assert held[name][COUNTER[name]] == FIRST[name], (name, held[name])
        assert held[name]["kernel_ms"] > 0 and held[name]["stack_overflows"] == 0, (name, held[name])

    def others_as_held(but):
        for other in names:
            if other != but:
                assert same(info[other](), held[other]), (but, other, info[other](), held[other])

    for name in names:
        run[name](SECOND[name])
        held[name] = info[name]()
        assert held[name][COUNTER[name]] == SECOND[name] and held[name]["kernel_ms"] > 0, (name, held[name])
        others_as_held(name)
        with pytest.raises(device.RtError, match="bad kernel"):  # a refused call leaves the family's info as it was
            run[name](SECOND[name], kernel=7)
        assert same(info[name](), held[name]), (name, info[name](), held[name])
        run[name](0)  # an empty query: RT_OK, zero counters, no kernel time
        held[name] = info[name]()
        assert all(v == 0 for v in held[name].values()), (name, held[name])
        others_as_held(name)
    r.close()

    # the slots go with their context: a second one starts with none, and makes its own
    r = device.Renderer(0).upload(scene)
    with pytest.raises(device.RtError, match="status -5"):
        r.nearest_info()
    r.nearest(pts[:70])
    assert r.nearest_info()["points"] == 70
    with pytest.raises(device.RtError, match="status -5"):
        r.clearance_info()
    r.close()
