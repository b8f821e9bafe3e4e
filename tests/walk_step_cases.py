"""The cases of tests/test_gpu_walk_step.py and the recorder of its expected counts (tests/golden/walk_step_counts.json).

The walk step's registers and waits changed; its arithmetic, the order of its tests, which lane walks
which ray and every stack operation did not. So a counting render must take the same wave steps, with the same
lane-count histogram, and visit the same nodes, leaves and triangles per ray kind as the commit before that change
did. That commit's figures were recorded once, with this file, from a library built from its tree:

    PRT_LIB_DIR=<the parent commit's lib/> python -m tests.walk_step_cases --record tests/golden/walk_step_counts.json

Shapes: dragon, car_boxed and sportscar have wide depths 8, 11 and 15 -- three stack capacities, and walks that reach
the packed stack's second array. 60 x 44 has partial tiles (lanes outside the frame that walk as pool workers) and an
even width (the centre column's degenerate rays and their strict fallbacks); 8 x 8 is one tile with fewer jobs than
`regroup` and steps where no lane is busy.
"""
import json
import sys

SCENES = ("dragon", "car_boxed", "sportscar")
SIZES = ((60, 44), (8, 8))
CAMS = (0, 7)  # frame 0 is the reference camera; frame i of the benchmark's path is moved by i * 0.02 along x
ORBIT = 0.02
VARIANTS = ("shdefer", "shpool")
SPPS = (1, 4)
BOUNCES = 4
COUNT_KEYS = ("wave_steps", "shadow_wave_steps", "steps_hist", "sh_inner", "sh_leaf", "sh_tri", "ch_inner", "ch_leaf",
              "ch_tri", "steps_lanes_16", "steps_lanes_32", "steps_lanes_48", "steps_lanes_64")
RAY_KEYS = ("primary", "reflection", "shadow", "shadow_skipped", "hits", "pixels")

_SCENES = {}


def scene(name):
    from prt import host
    if name not in _SCENES:
        _SCENES[name] = host.Scene.named(name).build_bvh(3)
    return _SCENES[name]


def camera(W, H, i):
    from prt import host
    c = host.camera(W, H)
    c.pos.x += i * ORBIT
    c.ul.x += i * ORBIT
    return c


def shapes():
    """(W, H, camera index, spp) of every frame a scene is rendered at"""
    return [(W, H, ci, spp) for (W, H) in SIZES for ci in CAMS for spp in SPPS]


def key(W, H, ci, spp, variant):
    return f"{W}x{H}/cam{ci}/spp{spp}/{variant}"


class Session:
    """one renderer with a scene uploaded, rendering small frames one after another"""

    def __init__(self, name, counters=False, flags=0):
        from prt import device
        self.r = device.Renderer(0, counters=counters, flags=flags)
        self.r.upload(scene(name))

    def render(self, W, H, ci, spp, variant):
        import torch
        rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        hit = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        t = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        bh = torch.zeros((H, W, BOUNCES), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.r.render(camera(W, H, ci), W, H, bounces=BOUNCES, spp=spp, kernel="fast", variant=variant, rgb=rgb, hit=hit,
                      t=t, bounce_hit=bh)
        self.r.sync()
        return {"rgb": rgb.cpu().numpy(), "hit": hit.cpu().numpy(), "t": t.cpu().numpy(), "bounce_hit": bh.cpu().numpy(),
                "stats": self.r.stats(), "launch": self.r.launch_info()}

    def close(self):
        self.r.close()


def counts(name):
    """{case key: the counting builds' figures}, the list hand-out and the forced cursor agreeing on every one"""
    from prt import device
    out = {}
    lst, cur = Session(name, counters=True), Session(name, counters=True, flags=device.FLAG_POOL_CURSOR)
    for W, H, ci, spp in shapes():
        for v in VARIANTS:
            a, b = lst.render(W, H, ci, spp, v)["stats"], cur.render(W, H, ci, spp, v)["stats"]
            for k in COUNT_KEYS + RAY_KEYS:
                assert a[k] == b[k], (name, key(W, H, ci, spp, v), k, a[k], b[k])
            out[key(W, H, ci, spp, v)] = {k: a[k] for k in COUNT_KEYS + RAY_KEYS}
    lst.close()
    cur.close()
    return out


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    with open(sys.argv[2], "w") as f:
        json.dump({n: counts(n) for n in SCENES}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded", sys.argv[2])
