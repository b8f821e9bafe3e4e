#!/usr/bin/env python3
"""Vertex updates against fresh uploads (rt_update_vertices): per scene and per rigid motion of half
its triangles (those with centroid x above the median: a rotation about z plus a translation, `small` and `large`),
one JSON line with
  update_ms_first   the first update after the upload (it also makes the trees' level lists: one download per view)
  update_ms         median of --runs further updates to the same coordinates (HIP events around the whole update),
  update_wall_ms    and the same updates by the host clock, call to synchronise (the plan pass's host wait included)
  ref_build_ms      the caller's bvh_build of the moved triangles, which a fresh upload needs first (host clock)
  upload_ms         the fresh upload of S' by the host clock; build_ms: the library's own share (rt_scene_info)
  frame_ms_refit    a 20-frame batch's kernel time per frame on the refitted views,
  frame_ms_fresh    and on the fresh upload of S': each the mean of two medians of --runs launches, taken refit,
                    fresh, refit, fresh after the default rule has settled (the medians themselves in *_runs)
  area_ratio        the full view's decoded child-box area against its build (rt_update_info)
  pixels_differing  pixels of one frame that differ between the two renderers. The fresh upload here is what a caller
                    without updates would do, a NEW bvh_build of the moved triangles, so its reference tree's order
                    differs from the kept one's and exact ties may fall the other way (rt_hip.h); the bit-for-bit
                    comparison with a fresh upload of the kept topology is tests/test_gpu_refit.py's
and the library's md5.
--rebuild: view rebuilds instead (rt_rebuild_views), for the `large` motion: four renderers of the same
moved scene -- refitted (update_vertices), rebuilt on the device, rebuilt on the host, and the fresh upload -- with
  frame_ms_{refit,device,host,fresh}   kernel time per frame as above, the four sides taken in turn, twice
  rebuild_{device,host}                that mode's rt_rebuild_info: rebuild_ms (HIP events, the update included), host_ms
                                       (the call's wall time), the stages, nodes and depth per view, area_before / after
  ref_build_ms, upload_ms, build_ms    what a fresh upload costs instead
  frames_to_break_even_{device,host}   rebuild host_ms / (frame_ms_refit - frame_ms_<mode>): frames after which the
                                       rebuild has paid for itself (null when its frames are not faster)
usage: python tools/refit_bench.py [--rebuild] [--scenes dragon sportscar two_cars car_boxed] [--width 1920 --height 1080]
       [--runs 7] [--out profiles/<dir>/refit.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-ray-tracer_amd"))

MOTIONS = {"small": (0.02, (0.05, -0.03, 0.02)), "large": (0.5, (3.0, 2.0, 1.0))}
FRAMES = 20


def moved(tris, angle, shift):
    import numpy as np
    from prt import host
    c = tris["coords"].astype(np.float64)
    sel = tris["centroid"][:, 0] > np.median(tris["centroid"][:, 0])
    R = np.array([[np.cos(angle), -np.sin(angle), 0.0], [np.sin(angle), np.cos(angle), 0.0], [0.0, 0.0, 1.0]])
    c[sel] = c[sel] @ R.T + np.array(shift)
    c = np.ascontiguousarray(c.astype(np.float32))
    return c, host.triangle_init(c, tris["ks"], tris["kd"], tris["kr"])


def batch_ms(r, cams, W, H, px, runs):
    """kernel ms per frame of a FRAMES-frame batch: the default rule's trial launches first, then the median"""
    for _ in range(10):
        r.render_frames(cams, W, H, bgra=px)
        r.sync()
        if r.launch_info()["settled"]:
            break
    ms = []
    for _ in range(runs):
        r.render_frames(cams, W, H, bgra=px)
        ms.append(r.sync() / len(cams))
    return statistics.median(ms), min(ms), max(ms), r.launch_info()["variant"]


def rebuild_lines(a, emit):
    import torch
    from prt import device, host
    W, H = a.width, a.height
    md5 = device.lib_md5()
    cams = [host.camera(W, H)] * FRAMES
    px = torch.zeros((FRAMES, H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    angle, shift = MOTIONS["large"]
    for name in a.scenes:
        s = host.Scene.named(name).build_bvh(3)
        coords, tris1 = moved(s.triangles, angle, shift)
        dc = torch.from_numpy(coords).cuda()
        sides, info = {}, {}
        sides["refit"] = device.Renderer(0).upload(s)
        sides["refit"].update_vertices(dc)
        area_ratio = sides["refit"].update_info()["area_ratio"]
        for mode in ("device", "host"):
            r = sides[mode] = device.Renderer(0).upload(s)
            times = []
            for _ in range(max(3, a.runs // 2)):  # (every rebuild starts from the upload's own views)
                r.upload(s)
                r.sync()
                r.rebuild_views(dc, mode=mode)
                times.append(r.rebuild_info())
            i = dict(times[-1])
            for f in ("rebuild_ms", "host_ms", "ploc_ms", "collapse_ms", "fill_ms"):
                i[f] = round(statistics.median(t[f] for t in times), 3)
            info[mode] = i
        t0 = time.perf_counter()
        s1 = host.Scene(tris1, s.lights)
        s1.amb = s.amb
        s1.build_bvh(3)
        ref_build_ms = (time.perf_counter() - t0) * 1e3
        sides["fresh"] = device.Renderer(0)
        t0 = time.perf_counter()
        sides["fresh"].upload(s1)
        upload_ms = (time.perf_counter() - t0) * 1e3
        rounds = [{k: batch_ms(r, cams, W, H, px, a.runs) for k, r in sides.items()} for _ in range(2)]
        line = {"scene": name, "motion": "large", "angle": angle, "shift": shift, "triangles": len(coords), "width": W,
                "height": H, "frames": FRAMES, "runs": a.runs, "area_ratio_refit": round(area_ratio, 4),
                "ref_build_ms": round(ref_build_ms, 2), "upload_ms": round(upload_ms, 2),
                "build_ms": round(sides["fresh"].scene_info()["build_ms"], 2), "lib_md5": md5}
        for k in sides:
            line[f"frame_ms_{k}"] = round(0.5 * (rounds[0][k][0] + rounds[1][k][0]), 4)
            line[f"frame_ms_{k}_runs"] = [round(rounds[0][k][0], 4), round(rounds[1][k][0], 4)]
            line[f"frame_ms_{k}_spread"] = [round(min(rounds[0][k][1], rounds[1][k][1]), 4),
                                            round(max(rounds[0][k][2], rounds[1][k][2]), 4)]
            line[f"variant_{k}"] = rounds[1][k][3]
        for mode in ("device", "host"):
            line[f"rebuild_{mode}"] = info[mode]
            saved = line["frame_ms_refit"] - line[f"frame_ms_{mode}"]
            line[f"frames_to_break_even_{mode}"] = round(info[mode]["host_ms"] / saved, 1) if saved > 0 else None
        emit(json.dumps(line))
        for r in sides.values():
            r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rebuild", action="store_true", help="measure view rebuilds (rt_rebuild_views) instead")
    ap.add_argument("--scenes", nargs="+", default=["dragon", "sportscar", "two_cars", "car_boxed"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()

    def emit(out):
        print(out, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(out + "\n")

    if a.rebuild:
        return rebuild_lines(a, emit)
    import torch
    from prt import device, host
    W, H = a.width, a.height
    md5 = device.lib_md5()
    cams = [host.camera(W, H)] * FRAMES
    px = torch.zeros((FRAMES, H, W), dtype=torch.int32, device="cuda")
    px2 = torch.zeros((FRAMES, H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for name in a.scenes:
        s = host.Scene.named(name).build_bvh(3)
        r = device.Renderer(0).upload(s)
        base_ms = batch_ms(r, cams, W, H, px, a.runs)[0]  # the unmoved scene, for context
        for motion, (angle, shift) in MOTIONS.items():
            coords, tris1 = moved(s.triangles, angle, shift)
            dc = torch.from_numpy(coords).cuda()
            r.upload(s)  # (every motion starts from the upload's own views)
            r.update_vertices(dc)
            first = r.update_info()
            ev, wall = [], []
            for _ in range(a.runs):
                r.sync()
                t0 = time.perf_counter()
                r.update_vertices(dc)
                r.sync()
                wall.append((time.perf_counter() - t0) * 1e3)
                ev.append(r.update_info()["update_ms"])
            info = r.update_info()
            t0 = time.perf_counter()
            s1 = host.Scene(tris1, s.lights)
            s1.amb = s.amb
            s1.build_bvh(3)
            ref_build_ms = (time.perf_counter() - t0) * 1e3
            fresh = device.Renderer(0)
            t0 = time.perf_counter()
            fresh.upload(s1)
            upload_ms = (time.perf_counter() - t0) * 1e3
            r.render_frames(cams[:1], W, H, bgra=px[:1], kernel="persist4")
            fresh.render_frames(cams[:1], W, H, bgra=px2[:1], kernel="persist4")
            r.sync(), fresh.sync()
            differ = int((px[0] != px2[0]).sum())
            # alternating, same box: refit, fresh, refit, fresh; each side reported as the mean of its two medians
            f_refit = batch_ms(r, cams, W, H, px, a.runs)
            f_fresh = batch_ms(fresh, cams, W, H, px2, a.runs)
            f_refit2 = batch_ms(r, cams, W, H, px, a.runs)
            f_fresh2 = batch_ms(fresh, cams, W, H, px2, a.runs)
            si, fi = r.scene_info(), fresh.scene_info()
            line = {"scene": name, "motion": motion, "angle": angle, "shift": shift, "triangles": len(coords),
                    "width": W, "height": H, "frames": FRAMES, "runs": a.runs, "pixels_differing": differ,
                    "update_ms_first": round(first["update_ms"], 4), "update_ms": round(statistics.median(ev), 4),
                    "update_ms_min": round(min(ev), 4), "update_ms_max": round(max(ev), 4),
                    "update_wall_ms": round(statistics.median(wall), 4), "views_refit": info["views_refit"],
                    "views_rebuilt": info["views_rebuilt"], "area_ratio": round(info["area_ratio"], 4),
                    "scene_magnitude": info["scene_magnitude"], "ref_build_ms": round(ref_build_ms, 2),
                    "upload_ms": round(upload_ms, 2), "build_ms": round(fi["build_ms"], 2),
                    "frame_ms_unmoved": round(base_ms, 4), "frame_ms_refit": round(0.5 * (f_refit[0] + f_refit2[0]), 4),
                    "frame_ms_refit_runs": [round(f_refit[0], 4), round(f_refit2[0], 4)],
                    "frame_ms_refit_spread": [round(min(f_refit[1], f_refit2[1]), 4), round(max(f_refit[2], f_refit2[2]), 4)],
                    "frame_ms_fresh": round(0.5 * (f_fresh[0] + f_fresh2[0]), 4),
                    "frame_ms_fresh_runs": [round(f_fresh[0], 4), round(f_fresh2[0], 4)],
                    "frame_ms_fresh_spread": [round(min(f_fresh[1], f_fresh2[1]), 4), round(max(f_fresh[2], f_fresh2[2]), 4)],
                    "variant_refit": f_refit[3], "variant_fresh": f_fresh[3], "wide_nodes": si["wide_nodes"],
                    "wide_nodes_fresh": fi["wide_nodes"], "lib_md5": md5}
            emit(json.dumps(line))
            fresh.close()
        r.close()


if __name__ == "__main__":
    main()
