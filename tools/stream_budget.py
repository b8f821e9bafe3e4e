#!/usr/bin/env python3
"""Where a pool kernel's instruction stream goes: the static price of its parts, all instruction classes, times how
often each part runs.

A wave's frame time is the length of its own instruction stream: about 4 cycles per instruction it
issues -- VALU, SALU, s_nop, LDS and VMEM issue alike -- plus exposed waits. This script prices the parts of one
k_persist instantiation from its assembly and multiplies them by a launch's counters.

1. The assembly, with line tables (no GPU needed):
       ISA_FLAGS=-gline-tables-only tools/isa_one.sh "4,false,false,true,4,false,true,2,true,true,2"
   (the bench instantiation; append ",false" for its cursor hand-out). Every instruction carries the source line it was
   compiled from (.loc). A line belongs to a part by the function it lies in (PARTS below) or, inside shadow_pool and
   trace_path_dfr, by the `<budget:NAME>` ... `</budget>` comments around the refill's hand-out, the ray formation, the
   list build, the closest levels' setup and the shading loop. Lines of the small vector helpers in rt_device.hpp (sub,
   dot, dvs, rcp_ieee: inlined everywhere) and of rt_exact.hpp's forms inherit the part of the instruction before them.
   A part's static count is what one pass through its code costs only as far as the code is straight-line and present
   once: the node test, the stack and the triangle tests exist once per walk kind (closest and shadow), so a step is
   priced at their sum / 2; loops inside a part (the cursor hand-out's, the face search of degenerate_ok) count once.
2. The counters: a PRT_DEFS=-DPRT_DIAG_REFILL build under RT_FLAG_COUNTERS reports refill rounds, cursor-loop
   iterations, lanes refilled and lists built in the lane-count bins (steps_lanes_16 / 32 / 48 / 64), next to the
   wave steps. `--run` renders one batch and reads them (PRT_LIB_DIR=<the diagnostics build>); `--counters FILE` takes
   a JSON object with wave_steps, rounds, iters, lanes, lists, tiles, levels (closest levels run per tile, summed)
   and shade_hits (shading-loop iterations that shade a hit; absent: one per tile). The same build counts both per
   tile and level in the histogram's slots (PRT_LEVEL_CNT, rt_kernels.hpp).

usage: tools/stream_budget.py [--asm /tmp/isa/one.s] [--kernel SUBSTR] [--run [--cursor] [--scene dragon] [--frames 4]]
                              [--counters FILE]
"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "parallel-ray-tracer_amd", "csrc", "hip")

# function -> part (rt_kernels.hpp, rt_shpool.hpp); what is not named lands in "other" and is listed
PARTS = {
    "node test": ["wide_node", "pin_q", "pin_node", "wload", "wload_at", "f4", "plane_pair", "plane_sel", "shift_in",
                  "far_sel", "max_raw", "min_raw", "max3_raw", "min3_raw", "fma_half", "fma_half_clamp", "closest_lim",
                  "own_leaf_words"],
    "triangle tests": ["hit_triangle", "hit_triangle_at", "hit_tri", "tri_load", "tri_landed", "leaf_tris", "closest_tris_packed",
                       "shadow_tris_packed", "tq_clear"],
    "stack": ["wide_next", "wide_next_tc", "top_reload", "wide_step_next"],
    "walk loop": ["closest_wide", "visible_wide", "count_step", "first_active_lane"],
    "ray formation": ["ray_pre_shadow", "shadow_reach", "shadow_reach_mag", "degenerate", "degenerate_ok", "on_face"],
    "refill hand-out": ["kth_bit", "drop_low", "mbcnt64"],
    "closest-level setup": ["closest", "ray_pre_closest", "tie_bound", "wide_for", "walk_base", "primary_dir",
                            "primary_dir_sample", "cam_of", "image_row", "opaque", "popc_wave", "trace_path_dfr",
                            "trace_path_shp", "tri_base", "tri_arr"],
    "shading": ["fold_pb"],
    "strict fallback": ["closest_walk", "visible_walk", "children", "children_out", "visit", "ref_reaches"],
    "tile loop": ["k_persist", "next_item", "lane_now", "lane_slot", "render_pixel_shp", "store_px", "clamp01", "flush",
                  "flush_u", "wave_sum", "ev_add", "ev_lds", "uni", "uni64", "pin_s"],
}
FUNC_PART = {f: p for p, fs in PARTS.items() for f in fs}
FUNC_PART["shadow_pool"] = "walk loop"  # (its lines outside the budget marks: the pool's walk loop)
NEUTRAL_FILES = ("rt_device.hpp", "rt_exact.hpp")  # (except hit_triangle)
FUNC_RE = re.compile(r"^(?:__device__|__global__|__host__|inline|static|void|template\b.*>\s*__device__)[^;]*?\b(\w+)\(")


def line_parts(path):
    """line number -> part of one source file: by enclosing function, overridden by the budget marks"""
    out, fn, mark = {}, None, None
    neutral = os.path.basename(path) in NEUTRAL_FILES
    for i, l in enumerate(open(path), 1):
        m = FUNC_RE.match(l)
        if m and not l.rstrip().endswith(";"):
            fn = m.group(1)
        mm = re.search(r"<budget:([\w -]+)>", l)
        if mm:
            mark = mm.group(1)
        part = mark or FUNC_PART.get(fn, None if neutral else "other:" + str(fn))
        if neutral and fn != "hit_triangle":
            part = mark  # (None: inherit)
        out[i] = part
        if "</budget>" in l:
            mark = None
    return out


def classify(ins):
    op = ins.split()[0]
    if op.startswith("s_nop"):
        return "nop"
    if op.startswith(("s_waitcnt", "s_barrier", "s_sleep")):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_endpgm")):
        return "branch"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("v_"):
        return "valu"
    return "other"


CLASSES = ("valu", "salu", "nop", "branch", "wait", "smem", "lds", "vmem", "other")


def price(asm, want):
    s = open(asm).read()
    files = {}
    for m in re.finditer(r'^\s*\.file\s+(\d+)\s+(?:"([^"]*)"\s+)?"([^"]*)"', s, re.M):
        files[int(m.group(1))] = os.path.basename(m.group(3))
    starts = [m.start() for m in re.finditer(r"^_ZN[^\s:]*:", s, re.M)]
    body = None
    for st in starts:
        name = s[st:s.index(":", st)]
        if want in name:
            body = s[st:s.index(".Lfunc_end", st)]
            break
    if body is None:
        raise SystemExit(f"no kernel matching {want!r} in {asm}")
    maps = {}
    counts, cur, seen_loc = {}, "tile loop", False
    for raw in body.split("\n"):
        l = raw.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", l)
        if m:
            seen_loc = True
            f = files.get(int(m.group(1)), "")
            if f not in maps:
                p = os.path.join(HIP, f)
                maps[f] = line_parts(p) if os.path.exists(p) else {}
            part = maps[f].get(int(m.group(2)))
            if part:
                cur = part
            continue
        if not l or l.startswith((";", ".")) or l.endswith(":"):
            continue
        ins = l.split(";")[0].strip()
        if not ins:
            continue
        c = counts.setdefault(cur, dict.fromkeys(CLASSES, 0))
        c[classify(ins)] += 1
    if not seen_loc:
        raise SystemExit(f"{asm} has no .loc lines: compile with ISA_FLAGS=-gline-tables-only tools/isa_one.sh ...")
    return name, counts


def run_counters(scene, frames, cursor):
    sys.path.insert(0, os.path.join(ROOT, "parallel-ray-tracer_amd"))
    import torch
    from prt import device, host
    s = host.Scene.named(scene).build_bvh(3)
    W, H = 1920, 1080
    cams = []
    for i in range(frames):
        c = host.camera(W, H)
        c.pos.x += i * 0.02
        c.ul.x += i * 0.02
        cams.append(c)
    r = device.Renderer(0, counters=True, flags=device.FLAG_POOL_CURSOR if cursor else 0)
    r.upload(s)
    px = torch.empty((frames, H, W), dtype=torch.int32, device="cuda")
    r.render_frames(cams, W, H, bgra=px, kernel="fast", variant="shdefer")
    r.sync()
    st, li = r.stats(), r.launch_info()
    r.close()
    tiles = frames * ((W + 7) // 8) * ((H + 7) // 8)
    # the diagnostics build's histogram slots (PRT_LEVEL_CNT): closest levels run, shading-loop iterations, and those
    # of them that shade a hit, one per tile (wave) and level
    h = st["steps_hist"]
    levels, shade_iters, shade_hits = (sum(h[k][l][b] for l in range(4)) for k, b in ((0, 0), (1, 0), (1, 1)))
    return {"frames": frames, "wave_steps": st["wave_steps"], "shadow_wave_steps": st["shadow_wave_steps"],
            "rounds": st["steps_lanes_16"], "iters": st["steps_lanes_32"], "lanes": st["steps_lanes_48"],
            "lists": st["steps_lanes_64"], "tiles": tiles, "shadow_rays": st["shadow"],
            "levels": levels, "shade_iters": shade_iters, "shade_hits": shade_hits,
            "levels_by_level": [h[0][l][0] for l in range(4)], "shade_hits_by_level": [h[1][l][1] for l in range(4)],
            "build_bits": li["build_bits"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", default="/tmp/isa/one.s")
    ap.add_argument("--kernel", default="k_persist")
    ap.add_argument("--run", action="store_true", help="render one batch on the GPU and read the refill counters")
    ap.add_argument("--cursor", action="store_true", help="--run: the cursor hand-out (RT_FLAG_POOL_CURSOR)")
    ap.add_argument("--scene", default="dragon")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--counters", default="", help="JSON file of counters instead of --run")
    a = ap.parse_args()
    name, counts = price(a.asm, a.kernel)
    print(f"kernel {name}")
    print(f"{'part':28s} " + " ".join(f"{c:>6s}" for c in CLASSES) + "    all")
    tot = dict.fromkeys(CLASSES, 0)
    allp = {}
    for part in sorted(counts, key=lambda p: -sum(counts[p].values())):
        c = counts[part]
        allp[part] = sum(c.values())
        for k in CLASSES:
            tot[k] += c[k]
        print(f"{part:28s} " + " ".join(f"{c[k]:6d}" for k in CLASSES) + f" {allp[part]:6d}")
    print(f"{'total':28s} " + " ".join(f"{tot[k]:6d}" for k in CLASSES) + f" {sum(tot.values()):6d}")
    ctr = None
    if a.run:
        ctr = run_counters(a.scene, a.frames, a.cursor)
    elif a.counters:
        ctr = json.load(open(a.counters))
    if not ctr:
        return
    print("counters " + json.dumps(ctr))
    g = lambda p: allp.get(p, 0)
    step = (g("node test") + g("stack") + g("triangle tests") + g("walk loop")) / 2.0
    rows = [("walk steps", ctr["wave_steps"], step),
            ("refill hand-out", ctr["rounds"] + ctr.get("iters", 0), g("refill hand-out")),
            ("ray formation", ctr["rounds"], g("ray formation")),
            ("list build", ctr.get("lists", 0), g("list build")),
            ("closest-level setup", ctr["levels"], g("closest-level setup") / 4.0),
            ("shading", ctr.get("shade_hits", ctr["tiles"]), g("shading"))]
    # (shading: the loop's body is present once and runs once per level that shades a hit; an iteration that only
    # writes a miss colour and leaves, shade_iters - shade_hits of them, is a handful of instructions and is not priced)
    # (the cursor hand-out's loop body runs once per iteration, its frame once per round: priced together per event)
    total = sum(n * p for _, n, p in rows)
    print(f"{'part':22s} {'events':>12s} {'instr/event':>12s} {'M instr':>10s} {'share':>7s}")
    for what, n, p in rows:
        print(f"{what:22s} {n:12d} {p:12.1f} {n * p / 1e6:10.1f} {100.0 * n * p / max(1.0, total):6.1f}%")
    print(f"{'total':22s} {'':12s} {'':12s} {total / 1e6:10.1f}  (x 4 cycles per instruction and wave)")


if __name__ == "__main__":
    main()
