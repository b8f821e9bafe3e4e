#!/usr/bin/env python3
"""Ray-query throughput (rt_trace_rays): per scene and ray set, `--runs` queries; one JSON line each
with Mrays/s from the median kernel_ms (HIP events around the query's launch), the spread (min / max ms), the
query's counters and the library's md5. Ray sets, each W x H rays:
  primary_rows / primary_tiles / primary_perm  the reference camera's primary rays in row-major order, in 8x8-tile
                                               order, in a fixed random permutation (CLOSEST)
  bounce_closest                               unit-length rays from the primary hit points in random directions
  bounce_occluded / bounce_occluded_perm       those rays as OCCLUDED with max_dist2 = 4, in pixel order and in the
                                               permutation (about 1 % of float32-normalised directions miss the
                                               occlusion walk's length window and walk the reference tree)
  window_occluded / window_occluded_perm       the same with every direction inside that window (in_window)
and, for context beside primary_rows, the frame kernel's own rate (stats()["rays"] / kernel_ms of a `persist` frame).
The fast and the strict kernel answer with the same bits (checked here on every set).
--mode shade times rt_shade_rays instead (shade_mode below), --mode hits rt_trace_hits beside the
closest-hit query (hits_mode below), --mode nearest rt_nearest_points (nearest_mode below),
--mode neighbours rt_nearest_tris beside rt_nearest_points (neighbours_mode below), --mode overlap
rt_overlap_boxes beside rt_nearest_tris' radius count (overlap_mode below), --mode sweep
rt_sweep_spheres beside the closest-hit query on the same rays (sweep_mode below), --mode cuts
rt_cut_triangles beside rt_overlap_boxes on the query triangles' corner boxes (cuts_mode below), --mode
contacts rt_sweep_contacts beside rt_sweep_spheres on the same sweeps (contacts_mode below), --mode
clearance rt_clearance_triangles beside rt_cut_triangles' count on the same triangles and rt_nearest_points on their
centroids (clearance_mode below), --mode proximity rt_proximity_triangles' lists beside
rt_clearance_triangles, its counts within a margin beside rt_cut_triangles' count, and its CSR form (proximity_mode
below).
usage: python tools/query_bench.py [--scenes dragon car_boxed] [--width 1920 --height 1080] [--runs 7]
       python tools/query_bench.py --mode shade [--regroups 4 16 32] [--runs 15]
       python tools/query_bench.py --mode hits [--runs 7]
       python tools/query_bench.py --mode nearest [--runs 7] [--out profiles/nearest_bench_<md5>.jsonl]
       python tools/query_bench.py --mode neighbours [--runs 7] [--out profiles/neighbours_bench_<md5>.jsonl]
       python tools/query_bench.py --mode overlap [--runs 7] [--out profiles/overlap_bench_<md5>.jsonl]
       python tools/query_bench.py --mode sweep [--runs 7] [--out profiles/sweep_bench_<md5>.jsonl]
       python tools/query_bench.py --mode cuts [--runs 5] [--out profiles/cuts_bench_<md5>.jsonl]
       python tools/query_bench.py --mode contacts [--runs 5] [--out profiles/contacts_bench_<md5>.jsonl]
       python tools/query_bench.py --mode clearance [--runs 5] [--out profiles/clearance_bench_<md5>.jsonl]
       python tools/query_bench.py --mode proximity [--runs 3] [--out profiles/proximity_bench_<md5>.jsonl]
       python tools/query_bench.py --mode trisweep [--runs 5] [--out profiles/trisweep_bench_<md5>.jsonl]
       python tools/query_bench.py --mode tricontacts [--runs 3] [--out profiles/tricontacts_bench_<md5>.jsonl]
--mode trisweep times rt_sweep_triangles beside rt_sweep_spheres with r = 0 on the same centres and motions and beside
rt_clearance_triangles on the same triangles (trisweep_mode below). --mode tricontacts times
rt_sweep_tri_contacts' lists and its swept-volume count beside rt_sweep_triangles on the same queries (tricontacts_mode
below)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-ray-tracer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["dragon", "car_boxed"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--mode", choices=["trace", "shade", "hits", "nearest", "neighbours", "overlap", "sweep", "cuts",
                                       "contacts", "clearance", "proximity", "trisweep", "tricontacts"],
                    default="trace",
                    help="trace: rt_trace_rays (above); shade: rt_shade_rays' forms beside rt_render (shade_mode); "
                         "hits: rt_trace_hits beside the closest-hit query (hits_mode); "
                         "nearest: rt_nearest_points beside the closest-hit query (nearest_mode); "
                         "neighbours: rt_nearest_tris beside rt_nearest_points (neighbours_mode); "
                         "overlap: rt_overlap_boxes beside rt_nearest_tris' radius count (overlap_mode); "
                         "sweep: rt_sweep_spheres beside the closest-hit query (sweep_mode); "
                         "cuts: rt_cut_triangles beside rt_overlap_boxes on the corner boxes (cuts_mode); "
                         "contacts: rt_sweep_contacts beside rt_sweep_spheres (contacts_mode); "
                         "clearance: rt_clearance_triangles beside rt_cut_triangles' count and rt_nearest_points "
                         "(clearance_mode); "
                         "proximity: rt_proximity_triangles beside rt_clearance_triangles and rt_cut_triangles' count "
                         "(proximity_mode); "
                         "trisweep: rt_sweep_triangles beside rt_sweep_spheres at r = 0 and rt_clearance_triangles "
                         "(trisweep_mode); "
                         "tricontacts: rt_sweep_tri_contacts' lists and swept-volume count beside rt_sweep_triangles "
                         "(tricontacts_mode)")
    ap.add_argument("--out", default=None,
                    help="nearest, neighbours, overlap, sweep, cuts, contacts: also append the raw lines to this file")
    ap.add_argument("--regroups", type=int, nargs="+", default=[4, 16, 32], help="shade: the pool form's thresholds")
    a = ap.parse_args()
    import numpy as np
    import torch
    from prt import device, host
    W, H = a.width, a.height
    md5 = device.lib_md5()
    if a.mode == "shade":
        return shade_mode(a, md5)
    if a.mode == "hits":
        return hits_mode(a, md5)
    if a.mode == "nearest":
        return nearest_mode(a, md5)
    if a.mode == "neighbours":
        return neighbours_mode(a, md5)
    if a.mode == "overlap":
        return overlap_mode(a, md5)
    if a.mode == "sweep":
        return sweep_mode(a, md5)
    if a.mode == "cuts":
        return cuts_mode(a, md5)
    if a.mode == "contacts":
        return contacts_mode(a, md5)
    if a.mode == "clearance":
        return clearance_mode(a, md5)
    if a.mode == "proximity":
        return proximity_mode(a, md5)
    if a.mode == "trisweep":
        return trisweep_mode(a, md5)
    if a.mode == "tricontacts":
        return tricontacts_mode(a, md5)
    for name in a.scenes:
        s = host.Scene.named(name).build_bvh(3)
        r = device.Renderer(0)
        r.upload(s)
        c = torch.from_numpy(host.camera_array(host.camera(W, H))).cuda()
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device="cuda"),
                                torch.arange(W, dtype=torch.float32, device="cuda"), indexing="ij")
        d = ((c[1] - c[0])[None, :] + c[2][None, :] * xs.reshape(-1, 1)) + c[3][None, :] * ys.reshape(-1, 1)
        o = c[0][None, :].expand_as(d).contiguous()
        n = W * H
        g = torch.Generator(device="cpu").manual_seed(1)
        idx = torch.arange(n).reshape(H, W)
        tiles = torch.cat([idx[y:y + 8, x:x + 8].reshape(-1) for y in range(0, H, 8) for x in range(0, W, 8)]).cuda()
        perm = torch.randperm(n, generator=g).cuda()
        hit, t = r.trace_rays(o, d, kernel="strict")
        r.sync()  # (the query runs on the renderer's stream, the tensor operations below on torch's)
        t1 = torch.where(hit >= 0, t, torch.ones_like(t))
        bo = (o + d * t1[:, None]).contiguous()
        bd = torch.randn(n, 3, generator=g)
        bd = bd / bd.norm(dim=1, keepdim=True)
        bw = in_window(bd).cuda().contiguous()
        bd = bd.cuda().contiguous()
        four = torch.full((n,), 4.0, device="cuda")
        sets = [("primary_rows", o, d, None), ("primary_tiles", o[tiles].contiguous(), d[tiles].contiguous(), None),
                ("primary_perm", o[perm].contiguous(), d[perm].contiguous(), None), ("bounce_closest", bo, bd, None),
                ("bounce_occluded", bo, bd, four),
                ("bounce_occluded_perm", bo[perm].contiguous(), bd[perm].contiguous(), four),
                ("window_occluded", bo, bw, four),
                ("window_occluded_perm", bo[perm].contiguous(), bw[perm].contiguous(), four)]
        for label, so, sd, m in sets:
            # the kind's forms, interleaved run by run: the occlusion query's pool (the default) and its lockstep form
            # (regroup = 64); the closest-hit query has the lockstep form only
            forms = [("lockstep", 64)] if m is None else [("pool", 0), ("lockstep", 64)]

            def run(kernel, regroup=0):
                if m is None:
                    out = r.trace_rays(so, sd, kernel=kernel)
                else:
                    out = (r.occluded(so, sd, m, kernel=kernel, regroup=regroup),)
                return out, r.query_info()
            ref, _ = run("strict")
            ms, info, same = {f: [] for f, _ in forms}, {}, {}
            for _ in range(a.runs):
                for f, rg in forms:
                    out, info[f] = run("fast", rg)
                    ms[f].append(info[f]["kernel_ms"])
                    same[f] = all(bool((x.view(torch.int32) == y.view(torch.int32)).all()) for x, y in zip(out, ref))
            for f, _ in forms:
                med = statistics.median(ms[f])
                line = {"scene": name, "set": label, "form": f, "rays": n, "mrays_s": round(n / med / 1e3, 1),
                        "kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(ms[f]), 4),
                        "kernel_ms_max": round(max(ms[f]), 4), "runs": a.runs, "equals_strict": same[f],
                        "info": {k: v for k, v in info[f].items() if k != "kernel_ms"}, "lib_md5": md5}
                if f != forms[-1][0]:
                    print(json.dumps(line), flush=True)
            if label == "primary_rows":  # context, not a bar: the frame kernel's rays per second on the same scene
                rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
                fm = []
                for _ in range(a.runs):
                    r.render(host.camera(W, H), W, H, kernel="persist", rgb=rgb)
                    fm.append(r.sync())
                line["frame_persist_mrays_s"] = round(r.stats()["rays"] / statistics.median(fm) / 1e3, 1)
            print(json.dumps(line), flush=True)
        r.close()


def shade_mode(a, md5):
    """--mode shade: per scene, the W x H camera's rays through rt_shade_rays in row-major order and in
    a fixed random permutation, on the lockstep form (regroup 64) and the pool form at --regroups (and, for context, in
    8x8-tile order on the lockstep form and the pool at 16, and row-major with regroup 0, the default), and beside them
    rt_render of the same camera (variant persist, and the default rule once its shape is settled): the project's
    existing way to shade those rays, on the same build. One untimed round first (and the default rule's trial
    frames); then --runs rounds with the arms interleaved; kernel_ms from the HIP events around each launch. One JSON
    line per arm: median / min / max ms, the query's counters, whether its rgb equals the strict-checked render's."""
    import torch
    from prt import device, host, rays
    W, H, n = a.width, a.height, a.width * a.height
    for name in a.scenes:
        s = host.Scene.named(name).build_bvh(3)
        r = device.Renderer(0)
        r.upload(s)
        cam = host.camera(W, H)
        o, d = rays.pinhole(cam, W, H)
        perm = torch.randperm(n, generator=torch.Generator(device="cpu").manual_seed(1)).cuda()
        po, pd = o[perm].contiguous(), d[perm].contiguous()
        frame = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        r.render(cam, W, H, kernel="strict", rgb=frame)
        r.sync()
        want = {"rows": frame.reshape(n, 3).clone()}
        want["perm"] = want["rows"][perm].contiguous()
        # (context: the same rays in 8x8-tile order, a wave's 64 rays one tile as the frame kernels deal them)
        idx = torch.arange(n).reshape(H, W)
        tiles = torch.cat([idx[y:y + 8, x:x + 8].reshape(-1) for y in range(0, H, 8) for x in range(0, W, 8)]).cuda()
        want["tiles"] = want["rows"][tiles].contiguous()
        sets = {"rows": (o, d), "perm": (po, pd), "tiles": (o[tiles].contiguous(), d[tiles].contiguous())}

        def shade(order, regroup):
            so, sd = sets[order]
            r.shade_rays(so, sd, regroup=regroup, rgb=out)
            info = r.shade_info()
            torch.cuda.synchronize()
            return info, bool((out.view(torch.int32) == want[order].view(torch.int32)).all())

        def render(variant):
            r.render(cam, W, H, kernel="fast", variant=variant, rgb=frame)
            ms = r.sync()
            return {"kernel_ms": ms, "variant_ran": r.launch_info()["variant"]}, \
                bool((frame.reshape(n, 3).view(torch.int32) == want["rows"].view(torch.int32)).all())

        arms = [(f"shade_{order}_{'lockstep' if rg == 64 else 'pool%d' % rg}", (lambda order=order, rg=rg: shade(order, rg)))
                for order in ("rows", "perm") for rg in [64] + list(a.regroups)]
        arms += [("shade_tiles_lockstep", lambda: shade("tiles", 64)),
                 ("shade_tiles_pool16", lambda: shade("tiles", 16)), ("shade_rows_default", lambda: shade("rows", 0)),
                 ("render_persist", lambda: render("persist")), ("render_default", lambda: render("default"))]
        for _ in range(64):  # the default rule's trial frames of this shape
            render("default")
            if r.launch_info()["settled"]:
                break
        for _, fn in arms:
            fn()
        ms, last, same = {k: [] for k, _ in arms}, {}, {k: True for k, _ in arms}
        for _ in range(a.runs):
            for k, fn in arms:
                last[k], eq = fn()
                ms[k].append(last[k]["kernel_ms"])
                same[k] = same[k] and eq
        for k, _ in arms:
            med = statistics.median(ms[k])
            print(json.dumps({"scene": name, "arm": k, "rays": n, "width": W, "height": H,
                              "kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(ms[k]), 4),
                              "kernel_ms_max": round(max(ms[k]), 4), "runs": a.runs, "equals_strict_render": same[k],
                              "info": {x: v for x, v in last[k].items() if x != "kernel_ms"}, "lib_md5": md5}),
                  flush=True)
        r.close()


def hits_mode(a, md5):
    """--mode hits: per scene, rt_trace_hits on the W x H camera's primary rays in row-major order
    (primary_rows) and in a fixed random permutation (primary_perm) and on unit-length rays from the primary hit points
    in random directions (bounce), with max_hits 1, 4, 8, 16 and as a pure count (max_hits 0, count_all), beside the
    unchanged closest-hit query (rt_trace_rays, fast kernel) on the same rays in the same session (and, for context, that
    query on a context with RT_FLAG_UNPACKED_TRIS: its build without packed triangle tests). One untimed round
    first; then --runs rounds with the arms interleaved; kernel_ms from the HIP events around each launch. One JSON line
    per arm: median / min / max ms, the ratio of the medians to the closest query's, the counters, and two checks: the
    rays whose first stored t is not the closest query's t (how many, how many of them have a zero direction
    component, how many the closest query missed altogether, and whether the exhaustive kernel agrees with the fast one
    on them), and whether the fast kernel equals the exhaustive one on a sample of 2,048 rays (the exhaustive kernel on
    all of them would be rays x triangles tests)."""
    import torch
    from prt import device, host
    W, H, n = a.width, a.height, a.width * a.height
    for name in a.scenes:
        s = host.Scene.named(name).build_bvh(3)
        r = device.Renderer(0)
        r.upload(s)
        # a second context whose closest query runs without packed triangle tests, as rt_trace_hits does: what part of
        # the distance between the two queries the packed tests are
        r2 = device.Renderer(0, flags=device.FLAG_UNPACKED_TRIS)
        r2.upload(s)
        c = torch.from_numpy(host.camera_array(host.camera(W, H))).cuda()
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device="cuda"),
                                torch.arange(W, dtype=torch.float32, device="cuda"), indexing="ij")
        d = ((c[1] - c[0])[None, :] + c[2][None, :] * xs.reshape(-1, 1)) + c[3][None, :] * ys.reshape(-1, 1)
        o = c[0][None, :].expand_as(d).contiguous()
        g = torch.Generator(device="cpu").manual_seed(1)
        perm = torch.randperm(n, generator=g).cuda()
        hit, t = r.trace_rays(o, d, kernel="fast")
        r.sync()
        t1 = torch.where(hit >= 0, t, torch.ones_like(t))
        bo = (o + d * t1[:, None]).contiguous()
        bd = torch.randn(n, 3, generator=g)
        bd = (bd / bd.norm(dim=1, keepdim=True)).cuda().contiguous()
        sets = [("primary_rows", o, d), ("primary_perm", o[perm].contiguous(), d[perm].contiguous()), ("bounce", bo, bd)]
        for label, so, sd in sets:
            sample = torch.randperm(n, generator=g)[:2048].cuda()
            po, pd = so[sample].contiguous(), sd[sample].contiguous()

            def closest():
                out = r.trace_rays(so, sd, kernel="fast")
                return r.query_info(), out[1]

            def hits(K, count_all=False):
                out = r.trace_hits(so, sd, max_hits=K, count_all=count_all, kernel="fast")
                return r.hits_info(), (out[1][:, 0].contiguous() if K else None)

            def sample_equal(K, count_all):
                x = r.trace_hits(po, pd, max_hits=K, count_all=count_all, kernel="fast")
                r.sync()
                y = r.trace_hits(po, pd, max_hits=K, count_all=count_all, kernel="strict")
                r.sync()
                return all(bool((p.view(torch.int32) == q.view(torch.int32)).all()) for p, q in zip(x, y))

            def closest_unpacked():  # context: the closest query's build without packed triangle tests
                out = r2.trace_rays(so, sd, kernel="fast")
                return r2.query_info(), out[1]

            arms = [("closest", closest)] + [(f"hits{K}", (lambda K=K: hits(K))) for K in (1, 4, 8, 16)]
            arms.append(("count_all", lambda: hits(0, True)))
            arms.append(("closest_unpacked_tris", closest_unpacked))
            checks = {"closest": None, "closest_unpacked_tris": None, "count_all": sample_equal(0, True)}
            for K in (1, 4, 8, 16):
                checks[f"hits{K}"] = sample_equal(K, False)
            _, tc = closest()
            r.sync()
            first = {}
            for k, fn in arms:  # the untimed round, and the first-hit check
                _, t0 = fn()
                r.sync()
                if t0 is None or k.startswith("closest"):
                    first[k] = None
                    continue
                # rays whose first stored t is not the closest query's: bvh_traverse loses hits that brute force finds
                # (DESIGN.md §3o); how many have a zero direction component, and the exhaustive kernel's word on them
                idx = torch.nonzero(t0.view(torch.int32) != tc.view(torch.int32)).reshape(-1)
                first[k] = {"rays": int(idx.numel()), "zero_component": int((sd[idx] == 0).any(1).sum()),
                            "closest_missed": int((tc[idx] == 3.4028234663852886e38).sum())}
                if idx.numel():
                    xo, xd = so[idx].contiguous(), sd[idx].contiguous()
                    torch.cuda.synchronize()
                    te = r.trace_hits(xo, xd, max_hits=1, kernel="strict")[1]
                    r.sync()
                    first[k]["exhaustive_agrees"] = bool((te[:, 0].view(torch.int32) == t0[idx].view(torch.int32)).all())
            ms, last = {k: [] for k, _ in arms}, {}
            for _ in range(a.runs):
                for k, fn in arms:
                    last[k], _ = fn()
                    ms[k].append(last[k]["kernel_ms"])
            base = statistics.median(ms["closest"])
            for k, _ in arms:
                med = statistics.median(ms[k])
                print(json.dumps({"scene": name, "set": label, "arm": k, "rays": n, "width": W, "height": H,
                                  "mrays_s": round(n / med / 1e3, 1), "kernel_ms_median": round(med, 4),
                                  "kernel_ms_min": round(min(ms[k]), 4), "kernel_ms_max": round(max(ms[k]), 4),
                                  "ratio_to_closest": round(med / base, 3), "runs": a.runs,
                                  "first_t_differs_from_closest": first[k], "sample_equals_exhaustive": checks[k],
                                  "info": {x: v for x, v in last[k].items() if x != "kernel_ms"}, "lib_md5": md5}),
                      flush=True)
        r.close()
        r2.close()


def nearest_mode(a, md5):
    """--mode nearest: per scene, rt_nearest_points on three sets of W x H points -- the camera's
    primary hit points pushed 0.05 along the ray (near the surface, coherent; a missing ray's point lies at t = 1), the
    same points in a fixed random permutation, and uniform points in the scene's box grown by a quarter -- with the fast
    kernel, beside the closest-hit query (rt_trace_rays, fast kernel) on the same count of camera rays for scale and the
    exhaustive kernel on 4,096 of the points. One untimed round first; then --runs rounds with the arms interleaved;
    kernel_ms from the HIP events around each launch. One JSON line per arm: median / min / max ms, the ratios of the
    medians to the closest query's and (per point) to the exhaustive kernel's, nodes_visited and tris_tested per point,
    the counters, and whether the fast kernel equals the exhaustive one on the 4,096 points."""
    import torch
    from prt import device, host
    W, H, n = a.width, a.height, a.width * a.height
    NS = 4096
    out = open(a.out, "a") if a.out else None
    for name in a.scenes:
        s = host.Scene.named(name).build_bvh(3)
        r = device.Renderer(0)
        r.upload(s)
        o, d, g, sets = point_sets(r, s, W, H)
        for label, pts in sets:
            sample = pts[torch.randperm(n, generator=g)[:NS].cuda()].contiguous()

            def closest():
                r.trace_rays(o, d, kernel="fast")
                return r.query_info(), n

            def fast():
                r.nearest(pts, kernel="fast")
                return r.nearest_info(), n

            def exhaustive():
                r.nearest(sample, kernel="strict")
                return r.nearest_info(), NS

            x = r.nearest(sample, kernel="fast")
            r.sync()
            y = r.nearest(sample, kernel="strict")
            r.sync()
            same = all(bool((p.view(torch.int32) == q.view(torch.int32)).all()) for p, q in zip(x, y))
            arms = [("nearest_fast", fast), ("closest", closest), ("nearest_exhaustive_4096", exhaustive)]
            for _, fn in arms:  # the untimed round
                fn()
            ms, last, cnt = {k: [] for k, _ in arms}, {}, {}
            for _ in range(a.runs):
                for k, fn in arms:
                    last[k], cnt[k] = fn()
                    ms[k].append(last[k]["kernel_ms"])
            med = {k: statistics.median(ms[k]) for k, _ in arms}
            for k, _ in arms:
                info = last[k]
                line = {"scene": name, "set": label, "arm": k, "points": cnt[k], "width": W, "height": H,
                        "mpoints_s": round(cnt[k] / med[k] / 1e3, 2), "kernel_ms_median": round(med[k], 4),
                        "kernel_ms_min": round(min(ms[k]), 4), "kernel_ms_max": round(max(ms[k]), 4),
                        "ratio_to_closest": round(med[k] / med["closest"], 3),
                        "per_point_ratio_to_exhaustive": round((med[k] / cnt[k]) / (med["nearest_exhaustive_4096"] / NS), 6),
                        "runs": a.runs, "sample_equals_exhaustive": same if k == "nearest_fast" else None,
                        "info": {x: v for x, v in info.items() if x != "kernel_ms"}, "lib_md5": md5}
                if "nodes_visited" in info:
                    line["nodes_visited_per_point"] = round(info["nodes_visited"] / cnt[k], 2)
                    line["tris_tested_per_point"] = round(info["tris_tested"] / cnt[k], 2)
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + "\n")
                    out.flush()
        r.close()
    if out:
        out.close()


def point_sets(r, s, W, H):
    """the camera's rays (o, d), the generator, and §3p's three sets of W x H points: the primary hit points pushed 0.05
    along the ray, the same in a fixed random permutation, uniform points in the scene's box grown by a quarter"""
    import numpy as np
    import torch
    from prt import host
    n = W * H
    c = torch.from_numpy(host.camera_array(host.camera(W, H))).cuda()
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device="cuda"),
                            torch.arange(W, dtype=torch.float32, device="cuda"), indexing="ij")
    d = ((c[1] - c[0])[None, :] + c[2][None, :] * xs.reshape(-1, 1)) + c[3][None, :] * ys.reshape(-1, 1)
    o = c[0][None, :].expand_as(d).contiguous()
    g = torch.Generator(device="cpu").manual_seed(1)
    perm = torch.randperm(n, generator=g).cuda()
    hit, t = r.trace_rays(o, d, kernel="fast")
    r.sync()
    t1 = torch.where(hit >= 0, t, torch.ones_like(t))
    near = (o + d * (t1 + 0.05)[:, None]).contiguous()
    co = torch.from_numpy(np.ascontiguousarray(s.triangles["coords"], np.float32).reshape(-1, 3))
    lo, hi = co.min(0).values, co.max(0).values
    grow = (hi - lo) / 4
    uni = (torch.rand(n, 3, generator=g) * (hi - lo + 2 * grow) + (lo - grow)).cuda().contiguous()
    return o, d, g, [("near_surface", near), ("near_surface_perm", near[perm].contiguous()), ("uniform_box", uni)]


def neighbours_mode(a, md5):
    """--mode neighbours: per scene, on §3p's three sets of W x H points (point_sets), rt_nearest_tris
    with k = 1, 4, 8 and 16 (tri, d2 and count), k = 1 and k = 8 with the point output as well, and the pure count
    within max_dist2 = 1e-3 (k = 0, count_all), beside the unchanged rt_nearest_points on the same points. One untimed
    round first; then --runs rounds with the arms interleaved; kernel_ms from the HIP events around each launch. One
    JSON line per arm: median / min / max ms, the ratio of the medians to rt_nearest_points', nodes_visited and
    tris_tested per point, the counters, and whether the fast kernel equals the exhaustive one on 4,096 of the points
    (every output the arm writes)."""
    import torch
    from prt import device, host
    W, H, n = a.width, a.height, a.width * a.height
    NS = 4096
    out = open(a.out, "a") if a.out else None
    for name in a.scenes:
        s = host.Scene.named(name).build_bvh(3)
        r = device.Renderer(0)
        r.upload(s)
        _, _, g, sets = point_sets(r, s, W, H)
        radius = torch.full((n,), 1e-3, dtype=torch.float32, device="cuda")
        for label, pts in sets:
            sample = pts[torch.randperm(n, generator=g)[:NS].cuda()].contiguous()

            def nearest(p=pts, kernel="fast"):
                res = r.nearest(p, kernel=kernel)
                return r.nearest_info(), res

            def tris(k, points_out=False, count=False, p=pts, kernel="fast"):
                res = r.nearest_tris(p, k=k, points_out=points_out, kernel=kernel, count_all=count,
                                     max_dist2=radius[:len(p)] if count else None)
                return r.neighbours_info(), res

            arms = [("nearest_points", nearest), ("tris1", lambda **kw: tris(1, **kw)),
                    ("tris1_points", lambda **kw: tris(1, True, **kw)), ("tris4", lambda **kw: tris(4, **kw)),
                    ("tris8", lambda **kw: tris(8, **kw)), ("tris8_points", lambda **kw: tris(8, True, **kw)),
                    ("tris16", lambda **kw: tris(16, **kw)), ("count_1e-3", lambda **kw: tris(0, count=True, **kw))]
            same = {}
            for k, fn in arms:  # the sample against the exhaustive kernel, and the untimed round
                x, y = fn(p=sample)[1], fn(p=sample, kernel="strict")[1]
                same[k] = all(bool((p.view(torch.int32) == q.view(torch.int32)).all()) for p, q in zip(x, y))
                fn()
            ms, last = {k: [] for k, _ in arms}, {}
            for _ in range(a.runs):
                for k, fn in arms:
                    last[k] = fn()[0]
                    ms[k].append(last[k]["kernel_ms"])
            med = {k: statistics.median(ms[k]) for k, _ in arms}
            for k, _ in arms:
                info = last[k]
                line = {"scene": name, "set": label, "arm": k, "points": n, "width": W, "height": H,
                        "mpoints_s": round(n / med[k] / 1e3, 2), "kernel_ms_median": round(med[k], 4),
                        "kernel_ms_min": round(min(ms[k]), 4), "kernel_ms_max": round(max(ms[k]), 4),
                        "ratio_to_nearest_points": round(med[k] / med["nearest_points"], 3), "runs": a.runs,
                        "sample_equals_exhaustive": same[k],
                        "nodes_visited_per_point": round(info["nodes_visited"] / n, 2),
                        "tris_tested_per_point": round(info["tris_tested"] / n, 2),
                        "info": {x: v for x, v in info.items() if x != "kernel_ms"}, "lib_md5": md5}
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + "\n")
                    out.flush()
        r.close()
    if out:
        out.close()


def overlap_mode(a, md5):
    """--mode overlap: per scene, rt_overlap_boxes on W x H boxes (1920 x 1080 = 2,073,600 by default)
    in two shapes: cubes centred on the hit points of the camera's primary rays (a missing ray's centre lies at t = 1)
    with half-widths of 0.1 %, 1 % and 5 % of the scene's extent (its box's longest side), and a voxel grid over the
    scene's box (prt.boxes.grid; 128 x 135 x 120 cells at the default size). Per set: the pure count (k = 0,
    count_all), k = 8 (tri and count) and the CSR form (overlaps_csr: the count, the list form and the sort; wall-clock
    ms around the call, skipped when the sets hold more than 2^27 entries in all), beside rt_nearest_tris' pure
    count within the same half-width on the same centres (a ball inside the cube: fewer triangles), and the
    exhaustive kernel's count and k = 8 on 4,096 of the boxes. One untimed round first; then --runs rounds with the
    arms interleaved; kernel_ms from the HIP events around each launch. One JSON line per arm: median / min / max ms,
    the per-box ratio to the exhaustive kernel, nodes_visited and tris_tested per box, the counters, and whether the
    fast kernel equals the exhaustive one on the 4,096 boxes."""
    import time

    import numpy as np
    import torch
    from prt import boxes, device, host
    W, H, n = a.width, a.height, a.width * a.height
    NS, CSR_CAP = 4096, 1 << 27
    out = open(a.out, "a") if a.out else None
    for name in a.scenes:
        s = host.Scene.named(name).build_bvh(3)
        r = device.Renderer(0)
        r.upload(s)
        o, d, g, _ = point_sets(r, s, W, H)
        hit, t = r.trace_rays(o, d, kernel="fast")
        r.sync()
        ctr = (o + d * torch.where(hit >= 0, t, torch.ones_like(t))[:, None]).contiguous()
        v = np.ascontiguousarray(s.triangles["coords"], np.float32).reshape(-1, 3)
        slo, shi = v.min(0), v.max(0)
        ext = float((shi - slo).max())
        dims = (128, 135, 120) if n == 2073600 else (W, H, 1)
        glo, ghi = boxes.grid(slo, shi, dims)
        sets = [(f"hit_points_{pct}pct", (ctr - ext * pct / 100).contiguous(), (ctr + ext * pct / 100).contiguous(), ctr,
                 ext * pct / 100) for pct in (0.1, 1.0, 5.0)]
        cell = float(((shi - slo) / np.array(dims, np.float32)).max()) / 2
        sets.append((f"grid_{dims[0]}x{dims[1]}x{dims[2]}", glo, ghi, ((glo + ghi) * 0.5).contiguous(), cell))
        for label, lo, hi, centres, radius in sets:
            pick = torch.randperm(n, generator=g)[:NS].cuda()
            slo_, shi_ = lo[pick].contiguous(), hi[pick].contiguous()
            md = torch.full((n,), radius * radius, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()

            def boxes_arm(k, l=lo, h=hi, kernel="fast"):
                res = r.overlaps(l, h, k=k, count_all=k == 0, kernel=kernel)
                return r.overlaps_info(), res, len(l)

            def ball_count():
                res = r.nearest_tris(centres, k=0, count_all=True, max_dist2=md)
                return r.neighbours_info(), res, n

            def csr():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = r.overlaps_csr(lo, hi)
                torch.cuda.synchronize()
                info = dict(r.overlaps_info())
                info["kernel_ms"] = (time.perf_counter() - t0) * 1e3  # (wall clock: two launches, a scan and a sort)
                return info, res, n

            total = int(boxes_arm(0)[1][1].sum(dtype=torch.int64))
            arms = [("count", lambda: boxes_arm(0)), ("k8", lambda: boxes_arm(8)), ("ball_count", ball_count),
                    ("count_exhaustive_4096", lambda: boxes_arm(0, slo_, shi_, "strict")),
                    ("k8_exhaustive_4096", lambda: boxes_arm(8, slo_, shi_, "strict"))]
            if total <= CSR_CAP:
                arms.append(("csr", csr))
            same = {}
            for k in (0, 8):  # the sample against the exhaustive kernel
                x, y = boxes_arm(k, slo_, shi_)[1], boxes_arm(k, slo_, shi_, "strict")[1]
                same["count" if k == 0 else "k8"] = all(bool((p == q).all()) for p, q in zip(x, y))
            for _, fn in arms:  # the untimed round
                fn()
            ms, last, cnt = {k: [] for k, _ in arms}, {}, {}
            for _ in range(a.runs):
                for k, fn in arms:
                    last[k], _, cnt[k] = fn()
                    ms[k].append(last[k]["kernel_ms"])
            med = {k: statistics.median(ms[k]) for k, _ in arms}
            for k, _ in arms:
                info = last[k]
                exh = "k8_exhaustive_4096" if k.startswith("k8") else "count_exhaustive_4096"
                line = {"scene": name, "set": label, "arm": k, "boxes": cnt[k], "half_width": round(radius, 6),
                        "set_entries": total, "mboxes_s": round(cnt[k] / med[k] / 1e3, 2),
                        "kernel_ms_median": round(med[k], 4), "kernel_ms_min": round(min(ms[k]), 4),
                        "kernel_ms_max": round(max(ms[k]), 4),
                        "per_box_ratio_to_exhaustive": round((med[k] / cnt[k]) / (med[exh] / NS), 6),
                        "runs": a.runs, "sample_equals_exhaustive": same.get(k),
                        "nodes_visited_per_box": round(info["nodes_visited"] / cnt[k], 2),
                        "tris_tested_per_box": round(info["tris_tested"] / cnt[k], 2),
                        "info": {x: v for x, v in info.items() if x != "kernel_ms"}, "lib_md5": md5}
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + "\n")
                    out.flush()
            if total > CSR_CAP:
                print(json.dumps({"scene": name, "set": label, "arm": "csr", "skipped": "set_entries above the cap",
                                  "set_entries": total, "cap": CSR_CAP}), flush=True)
        r.close()
    if out:
        out.close()


def sweep_mode(a, md5):
    """--mode sweep: per scene, rt_sweep_spheres on W x H sweeps (1920 x 1080 by default) whose (c, d)
    are the camera's primary rays, and the unit-length bounce rays of the trace mode (from the primary hit points in
    random directions: with r > 0 most of these touch at the start), with radii of 0, 0.1 %, 1 % and 5 % of the scene's
    extent (its box's longest side), beside rt_trace_rays' closest hit on the same rays, and the exhaustive kernel on
    4,096 of the sweeps. One untimed round first; then --runs rounds with the arms interleaved; kernel_ms from the HIP
    events around each launch. One JSON line per arm: median / min / max ms, the ratio of the medians to the
    closest-hit query's, the per-sweep ratio to the exhaustive kernel, nodes_visited and tris_tested per sweep, the
    counters, and whether the fast kernel equals the exhaustive one on the 4,096 sweeps."""
    import numpy as np
    import torch
    from prt import device, host
    W, H, n = a.width, a.height, a.width * a.height
    NS = 4096
    out = open(a.out, "a") if a.out else None
    for name in a.scenes:
        s = host.Scene.named(name).build_bvh(3)
        r = device.Renderer(0)
        r.upload(s)
        o, d, g, _ = point_sets(r, s, W, H)
        hit, t = r.trace_rays(o, d, kernel="fast")
        r.sync()
        bo = (o + d * torch.where(hit >= 0, t, torch.ones_like(t))[:, None]).contiguous()
        bd = torch.randn(n, 3, generator=g)
        bd = (bd / bd.norm(dim=1, keepdim=True)).cuda().contiguous()
        v = np.ascontiguousarray(s.triangles["coords"], np.float32).reshape(-1, 3)
        ext = float((v.max(0) - v.min(0)).max())
        for label, so, sd in (("primary", o, d), ("bounce", bo, bd)):
            pick = torch.randperm(n, generator=g)[:NS].cuda()
            po, pd = so[pick].contiguous(), sd[pick].contiguous()
            radii = {pct: torch.full((n,), ext * pct / 100, dtype=torch.float32, device="cuda")
                     for pct in (0.0, 0.1, 1.0, 5.0)}
            torch.cuda.synchronize()

            def sweep(pct, c=so, m=sd, kernel="fast"):
                res = r.sweep(c, m, radii[pct][:len(c)], kernel=kernel)
                return r.sweep_info(), res, len(c)

            def trace():
                res = r.trace_rays(so, sd, kernel="fast")
                return r.query_info(), res, n

            arms = [("trace_rays", trace)]
            for pct in radii:
                arms.append((f"sweep_{pct}pct", lambda pct=pct: sweep(pct)))
                arms.append((f"sweep_{pct}pct_exhaustive_4096", lambda pct=pct: sweep(pct, po, pd, "strict")))
            same = {}
            for pct in radii:  # the sample against the exhaustive kernel
                x, y = sweep(pct, po, pd)[1], sweep(pct, po, pd, "strict")[1]
                same[f"sweep_{pct}pct"] = all(bool((p.view(torch.int32) == q.view(torch.int32)).all())
                                              for p, q in zip(x, y))
            for _, fn in arms:  # the untimed round
                fn()
            ms, last, cnt = {k: [] for k, _ in arms}, {}, {}
            for _ in range(a.runs):
                for k, fn in arms:
                    last[k], _, cnt[k] = fn()
                    ms[k].append(last[k]["kernel_ms"])
            med = {k: statistics.median(ms[k]) for k, _ in arms}
            for k, _ in arms:
                info = last[k]
                line = {"scene": name, "set": label, "arm": k, "sweeps": cnt[k], "extent": round(ext, 4),
                        "msweeps_s": round(cnt[k] / med[k] / 1e3, 2), "kernel_ms_median": round(med[k], 4),
                        "kernel_ms_min": round(min(ms[k]), 4), "kernel_ms_max": round(max(ms[k]), 4),
                        "ratio_to_trace_rays": round((med[k] / cnt[k]) / (med["trace_rays"] / n), 3), "runs": a.runs,
                        "info": {x: v for x, v in info.items() if x != "kernel_ms"}, "lib_md5": md5}
                if k.startswith("sweep"):
                    exh = k if k.endswith("_4096") else k + "_exhaustive_4096"
                    line["per_sweep_ratio_to_exhaustive"] = round((med[k] / cnt[k]) / (med[exh] / NS), 6)
                    line["sample_equals_exhaustive"] = same.get(k)
                    line["nodes_visited_per_sweep"] = round(info["nodes_visited"] / cnt[k], 2)
                    line["tris_tested_per_sweep"] = round(info["tris_tested"] / cnt[k], 2)
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + "\n")
                    out.flush()
        r.close()
    if out:
        out.close()


def cuts_mode(a, md5):
    """--mode cuts: per scene, rt_cut_triangles on W x H query triangles (1920 x 1080 = 2,073,600 by
    default) in two shapes: triangles centred on the hit points of the camera's primary rays (a missing ray's centre
    lies at t = 1) whose corners are the centre plus size * (a standard normal 3 x 3 draw with the corner mean
    removed), with sizes of 0.1 %, 1 % and 5 % of the scene's extent (its box's longest side), and a prt.tris.sheet
    through the middle of the scene's box, tilted by a tenth of the extent along both sides (1440 x 720 cells at the
    default size). Per set: the pure count (k = 0, count_all), k = 8 (tri and count) and the CSR form with its segments
    (cuts_csr: the count, the list form and the sort; wall-clock ms around the call, skipped when the sets hold more
    than 2^26 entries in all), beside rt_overlap_boxes' pure count on the same triangles' corner boxes (the same walk
    and the same cull: the ratio prices the pair test), and the exhaustive kernel's count on 4,096 of the queries. One
    untimed round first; then --runs rounds with the arms interleaved; kernel_ms from the HIP events around each
    launch. One JSON line per arm: median / min / max ms, the ratio of the medians to the box count's, the per-query
    ratio to the exhaustive kernel, nodes_visited and pairs_tested per query, the counters, and whether the fast kernel
    equals the exhaustive one on the 4,096 queries (count, k = 8, and the CSR form with its segments' bits)."""
    import time

    import numpy as np
    import torch
    from prt import device, host, tris
    W, H, n = a.width, a.height, a.width * a.height
    NS, CSR_CAP = 4096, 1 << 26
    out = open(a.out, "a") if a.out else None
    for name in a.scenes:
        s = host.Scene.named(name).build_bvh(3)
        r = device.Renderer(0)
        r.upload(s)
        o, d, g, _ = point_sets(r, s, W, H)
        hit, t = r.trace_rays(o, d, kernel="fast")
        r.sync()
        ctr = (o + d * torch.where(hit >= 0, t, torch.ones_like(t))[:, None]).contiguous()
        v = np.ascontiguousarray(s.triangles["coords"], np.float32).reshape(-1, 3)
        slo, shi = v.min(0), v.max(0)
        ext = float((shi - slo).max())
        off = torch.randn(n, 3, 3, generator=g)
        off = (off - off.mean(dim=1, keepdim=True)).cuda()
        sets = [(f"hit_points_{pct}pct", (ctr[:, None, :] + off * (ext * pct / 100)).contiguous(), ext * pct / 100)
                for pct in (0.1, 1.0, 5.0)]
        dims = (1440, 720) if n == 2073600 else (W, max(H // 2, 1))
        mid = (slo + shi) / 2
        su = np.array([shi[0] - slo[0], 0.0, 0.1 * ext], np.float32)
        sv = np.array([0.0, shi[1] - slo[1], 0.1 * ext], np.float32)
        sheet = tris.sheet(np.array([slo[0], slo[1], mid[2] - 0.1 * ext], np.float32), su, sv, dims)
        sets.append((f"sheet_{dims[0]}x{dims[1]}", sheet, float(max(su[0] / dims[0], sv[1] / dims[1]))))
        for label, q, size in sets:
            m = len(q)
            pick = torch.randperm(m, generator=g)[:NS].cuda()
            qs = q[pick].contiguous()
            lo, hi = q.min(dim=1).values.contiguous(), q.max(dim=1).values.contiguous()
            torch.cuda.synchronize()

            def cuts(k, p=q, kernel="fast"):
                res = r.cuts(p, k=k, count_all=k == 0, kernel=kernel)
                return r.cuts_info(), res, len(p)

            def box_count():
                res = r.overlaps(lo, hi, k=0, count_all=True)
                return r.overlaps_info(), res, m

            def csr(p=q, kernel="fast"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = r.cuts_csr(p, kernel=kernel)
                torch.cuda.synchronize()
                info = dict(r.cuts_info())
                info["kernel_ms"] = (time.perf_counter() - t0) * 1e3  # (wall clock: two launches, a scan and a sort)
                return info, res, len(p)

            total = int(cuts(0)[1][1].sum(dtype=torch.int64))
            arms = [("cut_count", lambda: cuts(0)), ("cut_k8", lambda: cuts(8)), ("box_count", box_count),
                    ("cut_count_exhaustive_4096", lambda: cuts(0, qs, "strict"))]
            if total <= CSR_CAP:
                arms.append(("cut_csr", csr))
            same = {}
            for k in (0, 8):  # the sample against the exhaustive kernel
                x, y = cuts(k, qs)[1], cuts(k, qs, "strict")[1]
                same["cut_count" if k == 0 else "cut_k8"] = all(bool((p == w).all()) for p, w in zip(x, y))
            x, y = csr(qs)[1], csr(qs, "strict")[1]
            same["cut_csr"] = all(bool((p.view(torch.int32) == w.view(torch.int32)).all()) for p, w in zip(x, y))
            for _, fn in arms:  # the untimed round
                fn()
            ms, last, cnt = {k: [] for k, _ in arms}, {}, {}
            for _ in range(a.runs):
                for k, fn in arms:
                    last[k], _, cnt[k] = fn()
                    ms[k].append(last[k]["kernel_ms"])
            med = {k: statistics.median(ms[k]) for k, _ in arms}
            for k, _ in arms:
                info = last[k]
                tested = info["tris_tested"] if k == "box_count" else info["pairs_tested"]
                line = {"scene": name, "set": label, "arm": k, "queries": cnt[k], "size": round(size, 6),
                        "set_entries": total, "mqueries_s": round(cnt[k] / med[k] / 1e3, 2),
                        "kernel_ms_median": round(med[k], 4), "kernel_ms_min": round(min(ms[k]), 4),
                        "kernel_ms_max": round(max(ms[k]), 4),
                        "ratio_to_box_count": round((med[k] / cnt[k]) / (med["box_count"] / m), 3),
                        "per_query_ratio_to_exhaustive": round((med[k] / cnt[k]) /
                                                               (med["cut_count_exhaustive_4096"] / NS), 6),
                        "runs": a.runs, "sample_equals_exhaustive": same.get(k),
                        "nodes_visited_per_query": round(info["nodes_visited"] / cnt[k], 2),
                        "tests_per_query": round(tested / cnt[k], 2),
                        "info": {x: w for x, w in info.items() if x != "kernel_ms"}, "lib_md5": md5}
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + "\n")
                    out.flush()
            if total > CSR_CAP:
                print(json.dumps({"scene": name, "set": label, "arm": "cut_csr", "skipped": "set_entries above the cap",
                                  "set_entries": total, "cap": CSR_CAP}), flush=True)
        r.close()
    if out:
        out.close()


def clearance_mode(a, md5):
    """--mode clearance: per scene, rt_clearance_triangles on W x H query triangles (1920 x 1080 by
    default): cuts_mode's triangles centred on the hit points of the camera's primary rays, with sizes of 0.1 %, 1 % and
    5 % of the scene's extent, on the surface and lifted off it (the centre moved back along its ray by three times the
    size), and a prt.tris.sheet beside the mesh (parallel to the low z face of the scene's box, a twentieth of the
    extent outside it). Per set: the fast kernel, beside rt_cut_triangles' pure count on the same triangles (the walk
    that answers "does it cross") and rt_nearest_points on their centroids (the walk that answers a point), and the
    exhaustive kernel on 4,096 of the queries. One untimed round first; then --runs rounds with the arms interleaved;
    kernel_ms from the HIP events around each launch. One JSON line per arm: median / min / max ms, the ratios of the
    medians to the cut count's and to the nearest query's, the per-query ratio to the exhaustive kernel, nodes_visited,
    pairs_tested and pairs_gated per query, the share of answers that are crossings, the counters, and whether the
    fast kernel equals the exhaustive one on the 4,096 queries (every output's bits)."""
    import numpy as np
    import torch
    from prt import device, host, tris
    W, H, n = a.width, a.height, a.width * a.height
    NS = 4096
    out = open(a.out, "a") if a.out else None
    for name in a.scenes:
        s = host.Scene.named(name).build_bvh(3)
        r = device.Renderer(0)
        r.upload(s)
        sets, g, _ = triangle_sets(r, s, W, H)
        for label, q, size in sets:
            m = len(q)
            pick = torch.randperm(m, generator=g)[:NS].cuda()
            qs = q[pick].contiguous()
            cen = q.mean(dim=1).contiguous()
            kind = torch.empty(m, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def clearance(p=q, kernel="fast", kd=None):
                res = r.clearance(p, kernel=kernel, kind=kd)
                return r.clearance_info(), res, len(p)

            def cut_count():
                res = r.cuts(q, k=0, count_all=True)
                return r.cuts_info(), res, m

            def nearest():
                res = r.nearest(cen)
                return r.nearest_info(), res, m

            arms = [("clearance", lambda: clearance(kd=kind)), ("cut_count", cut_count), ("nearest_centroids", nearest),
                    ("clearance_exhaustive_4096", lambda: clearance(qs, "strict"))]
            ka, kb = (torch.empty(NS, dtype=torch.int32, device="cuda") for _ in range(2))
            x, y = clearance(qs, "fast", ka)[1], clearance(qs, "strict", kb)[1]
            same = all(bool((p.view(torch.int32) == w.view(torch.int32)).all()) for p, w in zip((*x, ka), (*y, kb)))
            for _, fn in arms:  # the untimed round
                fn()
            crossing = float((kind == 15).float().mean())
            ms, last, cnt = {k: [] for k, _ in arms}, {}, {}
            for _ in range(a.runs):
                for k, fn in arms:
                    last[k], _, cnt[k] = fn()
                    ms[k].append(last[k]["kernel_ms"])
            med = {k: statistics.median(ms[k]) for k, _ in arms}
            for k, _ in arms:
                info = last[k]
                tested = info["tris_tested"] if k == "nearest_centroids" else info["pairs_tested"]
                line = {"scene": name, "set": label, "arm": k, "queries": cnt[k], "size": round(size, 6),
                        "crossing_share": round(crossing, 4), "mqueries_s": round(cnt[k] / med[k] / 1e3, 2),
                        "kernel_ms_median": round(med[k], 4), "kernel_ms_min": round(min(ms[k]), 4),
                        "kernel_ms_max": round(max(ms[k]), 4),
                        "ratio_to_cut_count": round((med[k] / cnt[k]) / (med["cut_count"] / m), 3),
                        "ratio_to_nearest": round((med[k] / cnt[k]) / (med["nearest_centroids"] / m), 3),
                        "per_query_ratio_to_exhaustive": round((med[k] / cnt[k]) /
                                                               (med["clearance_exhaustive_4096"] / NS), 6),
                        "runs": a.runs, "sample_equals_exhaustive": same if k == "clearance" else None,
                        "nodes_visited_per_query": round(info["nodes_visited"] / cnt[k], 2),
                        "tests_per_query": round(tested / cnt[k], 2),
                        "gated_per_query": round(info.get("pairs_gated", 0) / cnt[k], 2),
                        "info": {x: w for x, w in info.items() if x != "kernel_ms"}, "lib_md5": md5}
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + "\n")
                    out.flush()
        r.close()
    if out:
        out.close()


def triangle_sets(r, s, W, H):
    """clearance_mode's query sets -> ([(label, tris [m, 3, 3] on the device, size)], the generator, the scene's extent)"""
    import numpy as np
    import torch
    from prt import tris
    n = W * H
    o, d, g, _ = point_sets(r, s, W, H)
    hit, t = r.trace_rays(o, d, kernel="fast")
    r.sync()
    t = torch.where(hit >= 0, t, torch.ones_like(t))
    v = np.ascontiguousarray(s.triangles["coords"], np.float32).reshape(-1, 3)
    slo, shi = v.min(0), v.max(0)
    ext = float((shi - slo).max())
    off = torch.randn(n, 3, 3, generator=g)
    off = (off - off.mean(dim=1, keepdim=True)).cuda()
    sets = []
    for pct in (0.1, 1.0, 5.0):
        size = ext * pct / 100
        for lift, what in ((0.0, "on"), (3.0 * size, "lifted")):
            ctr = (o + d * (t - lift / d.norm(dim=1))[:, None]).contiguous()
            sets.append((f"hit_points_{pct}pct_{what}", (ctr[:, None, :] + off * size).contiguous(), size))
    dims = (1440, 720) if n == 2073600 else (W, max(H // 2, 1))
    su = np.array([shi[0] - slo[0], 0.0, 0.0], np.float32)
    sv = np.array([0.0, shi[1] - slo[1], 0.0], np.float32)
    sheet = tris.sheet(np.array([slo[0], slo[1], slo[2] - 0.05 * ext], np.float32), su, sv, dims)
    sets.append((f"sheet_beside_{dims[0]}x{dims[1]}", sheet, float(max(su[0] / dims[0], sv[1] / dims[1]))))
    return sets, g, ext


def proximity_mode(a, md5):
    """--mode proximity: per scene, on clearance_mode's query sets (triangle_sets), rt_proximity_triangles
    with k = 1, 4, 8 and 16 (tri, d2, both points and kind written) beside rt_clearance_triangles on the same queries;
    its pure count within margins of 0.1 % and 1 % of the scene's extent beside rt_cut_triangles' pure count; and
    Renderer.proximity_csr at the 0.1 % margin (two launches and the sorts: wall time around the call, after a
    synchronise, not kernel_ms; skipped with its reason where the total does not fit). One untimed round first; then
    --runs rounds with the arms interleaved; kernel_ms from the HIP events around each launch. One JSON line per arm:
    median / min / max ms, the ratio of the median to clearance's, nodes_visited, pairs_tested and pairs_gated per
    query, stored and counted per query, the counters, and whether the fast kernel's list of 8 and count equal the
    exhaustive kernel's on 4,096 of the queries (every output's bits)."""
    import time

    import torch
    from prt import device, host
    W, H = a.width, a.height
    NS = 4096
    out = open(a.out, "a") if a.out else None
    for name in a.scenes:
        s = host.Scene.named(name).build_bvh(3)
        r = device.Renderer(0)
        r.upload(s)
        sets, g, ext = triangle_sets(r, s, W, H)
        for label, q, size in sets:
            m = len(q)
            pick = torch.randperm(m, generator=g)[:NS].cuda()
            qs = q[pick].contiguous()
            margins = {pct: torch.full((m,), (ext * pct / 100) ** 2, dtype=torch.float32, device="cuda")
                       for pct in (0.1, 1.0)}
            kinds = {k: torch.empty((m, k), dtype=torch.int32, device="cuda") for k in (1, 4, 8, 16)}
            ckind = torch.empty(m, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def clearance():
                r.clearance(q, kind=ckind)
                return r.clearance_info()

            def lists(k):
                r.proximity(q, k=k, pairs_out=True, kind=kinds[k])
                return r.proximity_info()

            def count(pct):
                r.proximity(q, k=0, count_all=True, max_dist2=margins[pct])
                return r.proximity_info()

            def cut_count():
                r.cuts(q, k=0, count_all=True)
                return r.cuts_info()

            def csr():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                try:
                    off = r.proximity_csr(q, margins[0.1])[0]
                except device.RtError as e:
                    return {"kernel_ms": float("nan"), "skipped": str(e)}
                torch.cuda.synchronize()
                info = r.proximity_info()
                info["kernel_ms"] = (time.perf_counter() - t0) * 1e3  # (wall time of the whole call)
                info["total"] = int(off[-1])
                return info

            def sample(k, **kw):
                x = [r.proximity(qs, k=k, pairs_out=k > 0, kernel=kern, **kw) for kern in ("fast", "strict")]
                r.sync()
                return all(bool((p.view(torch.int32) == w.view(torch.int32)).all()) for p, w in zip(*x))

            same = sample(8) and sample(0, count_all=True, max_dist2=margins[1.0][:NS].contiguous())
            arms = [("clearance", clearance)] + [(f"proximity_k{k}", lambda k=k: lists(k)) for k in (1, 4, 8, 16)] + \
                   [(f"count_{pct}pct", lambda pct=pct: count(pct)) for pct in (0.1, 1.0)] + \
                   [("cut_count", cut_count), ("csr_0.1pct", csr)]
            for _, fn in arms:  # the untimed round
                fn()
            ms, last = {k: [] for k, _ in arms}, {}
            for _ in range(a.runs):
                for k, fn in arms:
                    last[k] = fn()
                    ms[k].append(last[k]["kernel_ms"])
            med = {k: statistics.median(ms[k]) for k, _ in arms}
            for k, _ in arms:
                info = last[k]
                line = {"scene": name, "set": label, "arm": k, "queries": m, "size": round(size, 6),
                        "kernel_ms_median": round(med[k], 4), "kernel_ms_min": round(min(ms[k]), 4),
                        "kernel_ms_max": round(max(ms[k]), 4),
                        "ratio_to_clearance": round(med[k] / med["clearance"], 3),
                        "ratio_to_cut_count": round(med[k] / med["cut_count"], 3), "runs": a.runs,
                        "wall_time": k.startswith("csr"),
                        "sample_equals_exhaustive": same if k in ("proximity_k8", "count_1.0pct") else None,
                        "nodes_visited_per_query": round(info.get("nodes_visited", 0) / m, 2),
                        "tests_per_query": round(info.get("pairs_tested", 0) / m, 2),
                        "gated_per_query": round(info.get("pairs_gated", 0) / m, 2),
                        "stored_per_query": round(info.get("stored", 0) / m, 2),
                        "counted_per_query": round(info.get("counted", 0) / m, 2),
                        "info": {x: w for x, w in info.items() if x != "kernel_ms"}, "lib_md5": md5}
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + "\n")
                    out.flush()
        r.close()
    if out:
        out.close()


def moving_triangle_sets(r, s, W, H, NS):
    """trisweep_mode's query sets (its docstring), one after another -> (pct, "ray" / "surface", size, the centres
    [n, 3], the triangles [n, 3, 3], the motions [n, 3], t_max [n] or None, (the same three for NS of the queries))"""
    import numpy as np
    import torch
    n = W * H
    o, d, g, _ = point_sets(r, s, W, H)
    hit, t = r.trace_rays(o, d, kernel="fast")
    r.sync()
    t = torch.where(hit >= 0, t, torch.ones_like(t))
    v = np.ascontiguousarray(s.triangles["coords"], np.float32).reshape(-1, 3)
    ext = float((v.max(0) - v.min(0)).max())
    off = torch.randn(n, 3, 3, generator=g)
    off = (off - off.mean(dim=1, keepdim=True)).cuda()
    w = d / d.norm(dim=1, keepdim=True)
    up = torch.tensor([0.0, 1.0, 0.0], device="cuda").expand_as(w)
    side = torch.linalg.cross(w, up)
    side = side / side.norm(dim=1, keepdim=True).clamp_min(1e-6)
    for pct in (0.1, 1.0, 5.0):
        size = ext * pct / 100
        for what in ("ray", "surface"):
            back = 3.0 * size + (0.05 * ext if what == "ray" else 0.0)
            ctr = (o + w * (t * d.norm(dim=1) - back)[:, None]).contiguous()
            q = (ctr[:, None, :] + off * size).contiguous()
            mv = ((w if what == "ray" else side) * (0.1 * ext)).contiguous()
            tm = None if what == "ray" else torch.ones(n, dtype=torch.float32, device="cuda")
            pick = torch.randperm(n, generator=g)[:NS].cuda()
            sample = (q[pick].contiguous(), mv[pick].contiguous(), None if tm is None else tm[pick].contiguous())
            yield pct, what, size, ctr, q, mv, tm, sample


def trisweep_mode(a, md5):
    """--mode trisweep: per scene, rt_sweep_triangles on W x H query triangles (1920 x 1080 by default):
    cuts_mode's triangles of 0.1 %, 1 % and 5 % of the scene's extent, centred on the camera's primary rays, in two
    motions. "ray": the centre starts a twentieth of the extent plus three sizes before the hit point and moves along
    the view ray, a tenth of the extent per unit of t, with no bound. "surface": the centre starts three sizes before
    the hit point and moves across the ray, a tenth of the extent within t_max = 1. Per set: the fast kernel, beside
    rt_sweep_spheres with r = 0 on the same centres, motions and bounds (the walk that answers a moving point) and
    rt_clearance_triangles on the same triangles where they start (the walk that answers a triangle standing still),
    and the exhaustive kernel on 4,096 of the queries. One untimed round first; then --runs rounds with the arms
    interleaved; kernel_ms from the HIP events around each launch. One JSON line per arm: median / min / max ms, the
    ratios of the medians to the sphere sweep's and to clearance's, the per-query ratio to the exhaustive kernel,
    nodes_visited, pairs_tested and pairs_gated per query, the shares of found answers and of starts in contact, the
    counters, and whether the fast kernel equals the exhaustive one on the 4,096 queries (every output's bits)."""
    import numpy as np
    import torch
    from prt import device, host
    W, H, n = a.width, a.height, a.width * a.height
    NS = 4096
    out = open(a.out, "a") if a.out else None
    for name in a.scenes:
        s = host.Scene.named(name).build_bvh(3)
        r = device.Renderer(0)
        r.upload(s)
        for pct, what, size, ctr, q, mv, tm, (qs, ms_, ts) in moving_triangle_sets(r, s, W, H, NS):
            kind = torch.empty(n, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def trisweep(p=q, m=mv, b=tm, kernel="fast", kd=None):
                res = r.sweep_tris(p, m, t_max=b, kernel=kernel, kind=kd)
                return r.trisweep_info(), res, len(p)

            def sphere():
                res = r.sweep(ctr, mv, 0.0, t_max=tm)
                return r.sweep_info(), res, n

            def clearance():
                res = r.clearance(q)
                return r.clearance_info(), res, n

            arms = [("trisweep", lambda: trisweep(kd=kind)), ("sweep_r0", sphere), ("clearance", clearance),
                    ("trisweep_exhaustive_4096", lambda: trisweep(qs, ms_, ts, "strict"))]
            ka, kb = (torch.empty(NS, dtype=torch.int32, device="cuda") for _ in range(2))
            x, y = trisweep(qs, ms_, ts, "fast", ka)[1], trisweep(qs, ms_, ts, "strict", kb)[1]
            same = all(bool((p.view(torch.int32) == u.view(torch.int32)).all()) for p, u in zip((*x, ka), (*y, kb)))
            for _, fn in arms:  # the untimed round
                fn()
            start = float((kind == 15).float().mean())
            ms, last, cnt = {k: [] for k, _ in arms}, {}, {}
            for _ in range(a.runs):
                for k, fn in arms:
                    last[k], _, cnt[k] = fn()
                    ms[k].append(last[k]["kernel_ms"])
            med = {k: statistics.median(ms[k]) for k, _ in arms}
            for k, _ in arms:
                info = last[k]
                tested = info["tris_tested"] if k == "sweep_r0" else info["pairs_tested"]
                queries = info["spheres"] if k == "sweep_r0" else info["triangles"]
                line = {"scene": name, "set": f"hit_points_{pct}pct_{what}", "arm": k, "queries": cnt[k],
                        "size": round(size, 6), "found_share": round(info["found"] / max(queries, 1), 4),
                        "kind15_share": round(start, 4), "mqueries_s": round(cnt[k] / med[k] / 1e3, 2),
                        "kernel_ms_median": round(med[k], 4), "kernel_ms_min": round(min(ms[k]), 4),
                        "kernel_ms_max": round(max(ms[k]), 4),
                        "ratio_to_sweep_r0": round((med[k] / cnt[k]) / (med["sweep_r0"] / n), 3),
                        "ratio_to_clearance": round((med[k] / cnt[k]) / (med["clearance"] / n), 3),
                        "per_query_ratio_to_exhaustive": round((med[k] / cnt[k]) /
                                                               (med["trisweep_exhaustive_4096"] / NS), 6),
                        "runs": a.runs, "sample_equals_exhaustive": same if k == "trisweep" else None,
                        "nodes_visited_per_query": round(info["nodes_visited"] / cnt[k], 2),
                        "tests_per_query": round(tested / cnt[k], 2),
                        "gated_per_query": round(info.get("pairs_gated", 0) / cnt[k], 2),
                        "info": {x: u for x, u in info.items() if x != "kernel_ms"}, "lib_md5": md5}
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + "\n")
                    out.flush()
        r.close()
    if out:
        out.close()


def tricontacts_mode(a, md5):
    """--mode tricontacts: per scene, on trisweep_mode's six query sets (moving_triangle_sets),
    rt_sweep_tri_contacts with k = 1, 4, 8 and 16 (tri, t, point and kind written) beside rt_sweep_triangles on the same
    queries, the swept-volume count (k = 0, count_all, t_max = 1 on every set), and the exhaustive kernel with k = 8 on
    4,096 of the queries. One untimed round first; then --runs rounds with the arms interleaved; kernel_ms from the HIP
    events around each launch. One JSON line per arm: median / min / max ms, the ratio of the medians to the sweep's,
    the per-query ratio to the exhaustive kernel, nodes_visited, pairs_tested and pairs_gated per query, stored and
    counted per query, the share of starts in contact, the counters, and whether the fast kernel equals the exhaustive
    one on the 4,096 queries (k = 8 with count_all, and the swept-volume count: every output's bits)."""
    import torch
    from prt import device, host
    W, H, n = a.width, a.height, a.width * a.height
    NS = 4096
    out = open(a.out, "a") if a.out else None
    for name in a.scenes:
        s = host.Scene.named(name).build_bvh(3)
        r = device.Renderer(0)
        r.upload(s)
        for pct, what, size, ctr, q, mv, tm, (qs, ms_, ts) in moving_triangle_sets(r, s, W, H, NS):
            one = torch.ones(n, dtype=torch.float32, device="cuda")
            kind = torch.empty(n, dtype=torch.int32, device="cuda")
            kinds = {k: torch.empty((n, k), dtype=torch.int32, device="cuda") for k in (1, 4, 8, 16)}
            torch.cuda.synchronize()

            def sweep():
                r.sweep_tris(q, mv, t_max=tm, kind=kind)
                return r.trisweep_info(), n

            def lists(k):
                r.sweep_tri_contacts(q, mv, k=k, t_max=tm, points_out=True, kind=kinds[k])
                return r.tricontacts_info(), n

            def volume():
                r.sweep_tri_contacts(q, mv, k=0, t_max=one, count_all=True)
                return r.tricontacts_info(), n

            def exhaustive():
                r.sweep_tri_contacts(qs, ms_, k=8, t_max=ts, points_out=True, kernel="strict")
                return r.tricontacts_info(), NS

            def sample(k, **kw):
                x = [r.sweep_tri_contacts(qs, ms_, k=k, points_out=k > 0, kernel=kern, **kw)
                     for kern in ("fast", "strict")]
                r.sync()
                return all(bool((p.view(torch.int32) == u.view(torch.int32)).all()) for p, u in zip(*x))

            same = sample(8, t_max=ts, count_all=True) and sample(0, t_max=one[:NS].contiguous(), count_all=True)
            arms = [("trisweep", sweep)] + [(f"tricontacts_k{k}", lambda k=k: lists(k)) for k in (1, 4, 8, 16)] + \
                   [("swept_volume_count", volume), ("tricontacts_k8_exhaustive_4096", exhaustive)]
            for _, fn in arms:  # the untimed round
                fn()
            start = float((kind == 15).float().mean())
            ms, last, cnt = {k: [] for k, _ in arms}, {}, {}
            for _ in range(a.runs):
                for k, fn in arms:
                    last[k], cnt[k] = fn()
                    ms[k].append(last[k]["kernel_ms"])
            med = {k: statistics.median(ms[k]) for k, _ in arms}
            for k, _ in arms:
                info = last[k]
                line = {"scene": name, "set": f"hit_points_{pct}pct_{what}", "arm": k, "queries": cnt[k],
                        "size": round(size, 6), "found_share": round(info["found"] / max(info["triangles"], 1), 4),
                        "kind15_share": round(start, 4), "mqueries_s": round(cnt[k] / med[k] / 1e3, 2),
                        "kernel_ms_median": round(med[k], 4), "kernel_ms_min": round(min(ms[k]), 4),
                        "kernel_ms_max": round(max(ms[k]), 4),
                        "ratio_to_trisweep": round((med[k] / cnt[k]) / (med["trisweep"] / n), 3),
                        "per_query_ratio_to_exhaustive": round((med[k] / cnt[k]) /
                                                               (med["tricontacts_k8_exhaustive_4096"] / NS), 6),
                        "runs": a.runs, "sample_equals_exhaustive": same if k == "tricontacts_k8" else None,
                        "nodes_visited_per_query": round(info["nodes_visited"] / cnt[k], 2),
                        "tests_per_query": round(info["pairs_tested"] / cnt[k], 2),
                        "gated_per_query": round(info["pairs_gated"] / cnt[k], 2),
                        "stored_per_query": round(info.get("stored", 0) / cnt[k], 3),
                        "counted_per_query": round(info.get("counted", 0) / cnt[k], 3),
                        "info": {x: u for x, u in info.items() if x != "kernel_ms"}, "lib_md5": md5}
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + "\n")
                    out.flush()
        r.close()
    if out:
        out.close()


def contacts_mode(a, md5):
    """--mode contacts: per scene, rt_sweep_contacts on sweep_mode's W x H sweeps (the camera's primary
    rays, and the unit-length bounce rays from the primary hit points) at radii of 0, 0.1 %, 1 % and 5 % of the scene's
    extent: the lists of k = 1, 4, 8 and 16 contacts (tri, t and count; no points), and the pure count with t_max = 1
    (the capsule count: the triangles that the capsule from c to c + d touches), beside rt_sweep_spheres on the same
    sweeps, and the exhaustive kernel's k = 16 on 4,096 of the sweeps. One untimed round first; then --runs rounds with
    the arms interleaved; kernel_ms from the HIP events around each launch. One JSON line per arm: median / min / max
    ms, the ratio of the medians to rt_sweep_spheres', the per-sweep ratio to the exhaustive kernel, nodes_visited and
    tris_tested (toi evaluations) per sweep, the counters, and whether the fast kernel equals the exhaustive one on the
    4,096 sweeps (every output's bits, points included)."""
    import numpy as np
    import torch
    from prt import device, host
    W, H, n = a.width, a.height, a.width * a.height
    NS = 4096
    out = open(a.out, "a") if a.out else None
    for name in a.scenes:
        s = host.Scene.named(name).build_bvh(3)
        r = device.Renderer(0)
        r.upload(s)
        o, d, g, _ = point_sets(r, s, W, H)
        hit, t = r.trace_rays(o, d, kernel="fast")
        r.sync()
        bo = (o + d * torch.where(hit >= 0, t, torch.ones_like(t))[:, None]).contiguous()
        bd = torch.randn(n, 3, generator=g)
        bd = (bd / bd.norm(dim=1, keepdim=True)).cuda().contiguous()
        v = np.ascontiguousarray(s.triangles["coords"], np.float32).reshape(-1, 3)
        ext = float((v.max(0) - v.min(0)).max())
        one = torch.ones(n, dtype=torch.float32, device="cuda")
        for label, so, sd in (("primary", o, d), ("bounce", bo, bd)):
            pick = torch.randperm(n, generator=g)[:NS].cuda()
            po, pd = so[pick].contiguous(), sd[pick].contiguous()
            torch.cuda.synchronize()
            for pct in (0.0, 0.1, 1.0, 5.0):
                rad = torch.full((n,), ext * pct / 100, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()

                def sweep():
                    res = r.sweep(so, sd, rad, kernel="fast")
                    return r.sweep_info(), res, n

                def contacts(k, c=so, m=sd, kernel="fast", capsule=False, points=False):
                    res = r.sweep_contacts(c, m, rad[:len(c)], k=k, t_max=one[:len(c)] if capsule else None,
                                           count_all=k == 0, points_out=points, kernel=kernel)
                    return r.contacts_info(), res, len(c)

                arms = [("sweep_spheres", sweep)]
                arms += [(f"contacts_k{k}", lambda k=k: contacts(k)) for k in (1, 4, 8, 16)]
                arms += [("capsule_count", lambda: contacts(0, capsule=True)),
                         ("contacts_k16_exhaustive_4096", lambda: contacts(16, po, pd, "strict"))]
                same = {}
                for key, k, capsule in [(f"contacts_k{k}", k, False) for k in (1, 4, 8, 16)] + [("capsule_count", 0,
                                                                                                   True)]:
                    x = contacts(k, po, pd, capsule=capsule, points=k > 0)[1]
                    y = contacts(k, po, pd, "strict", capsule=capsule, points=k > 0)[1]
                    same[key] = all(bool((p.view(torch.int32) == q.view(torch.int32)).all()) for p, q in zip(x, y))
                for _, fn in arms:  # the untimed round
                    fn()
                ms, last, cnt = {k: [] for k, _ in arms}, {}, {}
                for _ in range(a.runs):
                    for k, fn in arms:
                        last[k], _, cnt[k] = fn()
                        ms[k].append(last[k]["kernel_ms"])
                med = {k: statistics.median(ms[k]) for k, _ in arms}
                for k, _ in arms:
                    info = last[k]
                    line = {"scene": name, "set": label, "radius_pct": pct, "arm": k, "sweeps": cnt[k],
                            "extent": round(ext, 4), "msweeps_s": round(cnt[k] / med[k] / 1e3, 2),
                            "kernel_ms_median": round(med[k], 4), "kernel_ms_min": round(min(ms[k]), 4),
                            "kernel_ms_max": round(max(ms[k]), 4),
                            "ratio_to_sweep_spheres": round((med[k] / cnt[k]) / (med["sweep_spheres"] / n), 3),
                            "per_sweep_ratio_to_exhaustive": round((med[k] / cnt[k]) /
                                                                   (med["contacts_k16_exhaustive_4096"] / NS), 6),
                            "runs": a.runs, "sample_equals_exhaustive": same.get(k),
                            "nodes_visited_per_sweep": round(info["nodes_visited"] / cnt[k], 2),
                            "tris_tested_per_sweep": round(info["tris_tested"] / cnt[k], 2),
                            "info": {x: w for x, w in info.items() if x != "kernel_ms"}, "lib_md5": md5}
                    if "tris_counted" in info:
                        line["contacts_per_sweep"] = round(info["tris_counted"] / cnt[k], 3)
                    print(json.dumps(line), flush=True)
                    if out:
                        out.write(json.dumps(line) + "\n")
                        out.flush()
        r.close()
    if out:
        out.close()


def in_window(d):
    """directions (CPU float32 [n, 3]) whose squared length, computed as the kernel computes it ((x x + y y) + z z in
    float32), lies in the occlusion walk's window [1 - 4u, 1 + 2u], u = 2^-24: rows outside are rescaled by
    1 / sqrt(l2) up to three times, and what then still fails is replaced by (1, 0, 0)"""
    import torch
    d = d.clone()
    lo, hi = 1.0 - 4 * 2.0 ** -24, 1.0 + 2 * 2.0 ** -24

    def l2(v):
        return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    for _ in range(3):
        q = l2(d)
        bad = (q < lo) | (q > hi)
        d[bad] = d[bad] / torch.sqrt(q[bad])[:, None]
    q = l2(d)
    d[(q < lo) | (q > hi)] = torch.tensor([1.0, 0.0, 0.0])
    return d


if __name__ == "__main__":
    main()
