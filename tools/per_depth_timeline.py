#!/usr/bin/env python3
"""tools/per_depth_timeline.py <kernel_trace.csv> [--pass N] — the frame per depth, from a `rocprofv3 --kernel-trace` of one render.

A fused render pass is a chain of launches per depth (wf_render_pass): "Reset queues", closest-hit walk, route hits, ray samples, escaped
rays, emitter hits, a shade and an NEE kernel per material type, the any-hit walk.  The trace has every launch's start and end on the
device clock, so this prints, per depth of one pass (the last by default: the timed one of bench.py): the launches, the sum of their
kernel times, the wall span from the depth's first start to its last end, and — for the frame scheduling of DESIGN.md 4.7 — where each
any-hit launch lies relative to the NEXT depth's closest-hit / route-hit / sample launches (the fraction of its interval inside their span).

A depth begins at a closest-hit launch of the whole queue (k_closest_fast / k_intersect_closest; the two-class scheme's second launch and
the near-tie re-trace belong to the depth that is open).  A pass begins at k_gen_camera_rays."""
import csv
import sys


def load(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name") or r.get("KernelName") or r.get("Name")
            a = r.get("Start_Timestamp") or r.get("BeginNs") or r.get("Start")
            b = r.get("End_Timestamp") or r.get("EndNs") or r.get("End")
            if name is None or a is None or b is None:
                continue
            rows.append((int(a), int(b), name))
    rows.sort()
    return rows


def short(name):
    n = name.split("(")[0]
    return n.split("<")[0].replace("void ", "").strip()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = -1
    if "--pass" in sys.argv:
        which = int(sys.argv[sys.argv.index("--pass") + 1])
    rows = load(args[0])
    passes = []
    for a, b, name in rows:
        s = short(name)
        if s == "k_gen_camera_rays":
            passes.append([])
        if passes:
            passes[-1].append((a, b, s))
    if not passes:
        sys.exit("no k_gen_camera_rays launch in the trace")
    p = passes[which]
    # (the launches after the pass's film update belong to whatever follows: cut there)
    for i, (a, b, s) in enumerate(p):
        if s.startswith("k_update_film"):
            p = p[:i + 1]
            break
    # groups of launches between closest-hit launches of the whole queue, in order of start ...
    groups, head = [], []
    for a, b, s in p:
        whole = s in ("k_closest_fast", "k_intersect_closest")
        # (the second launch of the two-class scheme follows its first with nothing between them)
        if whole and not (groups and groups[-1][-1][2] == s == "k_closest_fast"):
            groups.append([])
        (groups[-1] if groups else head).append((a, b, s))
    # ... -> depths.  An any-hit launch (and its "Reset shadowRayQueue") that starts before the group's first material kernel is the
    # shadow stage of the depth BEFORE, running beside this one; the last k_reset of a group is the next depth's "Reset queues".
    depths = [[] for _ in groups]
    for d, g in enumerate(groups):
        shaded = False
        for e in g:
            shaded = shaded or e[2].startswith("k_mat_")
            early = not shaded and d > 0 and e[2] in ("k_shadow_fast", "k_intersect_shadow", "k_reset")
            depths[d - 1 if early else d].append(e)
    for d in range(len(depths) - 1):
        resets = [e for e in depths[d] if e[2] == "k_reset"]
        if resets:
            depths[d].remove(resets[-1])
            depths[d + 1].insert(0, resets[-1])
    t0, t1 = p[0][0], max(e[1] for e in p)
    print("pass %d of %d: %d launches, wall span %.3f ms, sum of kernel times %.3f ms" %
          (which if which >= 0 else len(passes) + which, len(passes), len(p), (t1 - t0) / 1e6, sum(b - a for a, b, _ in p) / 1e6))
    print("before depth 0 (camera rays ...): %d launches, %.3f ms" % (len(head), sum(b - a for a, b, _ in head) / 1e6))
    print("%5s %8s %12s %12s %10s %10s  %s" % ("depth", "launches", "kernel sum", "wall span", "closest", "any-hit", "any-hit inside next depth's closest..samples span"))
    for d, L in enumerate(depths):
        ksum = sum(b - a for a, b, _ in L) / 1e6
        span = (max(b for _, b, _ in L) - min(a for a, _, _ in L)) / 1e6
        closest = sum(b - a for a, b, s in L if s in ("k_closest_fast", "k_intersect_closest", "k_closest_retrace")) / 1e6
        sh = [(a, b) for a, b, s in L if s in ("k_shadow_fast", "k_intersect_shadow")]
        inside = ""
        if sh and d + 1 < len(depths):
            nxt = [(a, b) for a, b, s in depths[d + 1] if s in ("k_closest_fast", "k_intersect_closest", "k_closest_retrace", "k_route_hits", "k_resolve_mix", "k_sample_tops",
                                                               "k_gen_ray_samples", "k_gen_ray_samples_shaded", "k_reset")]
            if nxt:
                lo, hi = min(a for a, _ in nxt), max(b for _, b in nxt)
                tot = sum(b - a for a, b in sh)
                ov = sum(max(0, min(b, hi) - max(a, lo)) for a, b in sh)
                inside = "%.2f" % (ov / tot if tot else 0)
        print("%5d %8d %9.3f ms %9.3f ms %7.3f ms %7.3f ms  %s" % (d, len(L), ksum, span, closest, sum(b - a for a, b in sh) / 1e6, inside))


if __name__ == "__main__":
    main()
