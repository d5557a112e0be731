#!/usr/bin/env python3
"""Skinning with per-instance boxes: what one call of fyx_lbs_skin_ex_bounds costs next to the skinning alone
(fyx_lbs_skin_ex) and next to the two-pass way (fyx_lbs_skin_ex, then fyx_skinned_aabb_device).  GPU only.

Configs: C4 (1 M vertices / 256 bones) as plain SoA (position + normal + tangent), position only, and into the mesh's own
68-byte AnimatedVertex layout; C3 (1000 instances x 10 k vertices / 64 bones) as plain SoA in lbs.exact = 1 and 0.
Every config rotates --sets seeded input / output sets (meshes, palettes, outputs, boxes).  Each call is timed by device
events on its launch stream (lbs.streams = 1 and a stream of our own given to the context: the launch stream is that stream,
and the events enclose the whole call -- the fold launch of the bounds form, both launches of the two-pass form).  The three
forms are interleaved round by round; the median per call is reported.  One JSON line (and --out FILE)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=12, help="timed calls per form and round")
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--configs", default="c4_soa,c4_pos,c4_vb68,c3_exact,c3_fused")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.sets >= 6, "at least six rotating input / output sets"
    import torch
    import fyrox_amd
    from fyrox_amd import synth

    L = synth.ANIMATED_VERTEX
    ctx = fyrox_amd.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_option("lbs.streams", 1)
    res = {"sets": args.sets, "rounds": args.rounds, "calls_per_round": args.calls, "configs": {}}

    def setup(name):
        c4 = name.startswith("c4")
        nv, nb, n_inst = (1_000_000, 256, 1) if c4 else (10_000, 64, 1000)
        n = nv * n_inst
        sets = []
        for s in range(args.sets):
            seed = synth.SEED_BASE + 900 + 10 * s + (4 if c4 else 3)
            m = synth.make_mesh(nv, nb, seed)
            mid = 900 + s
            ctx.mesh_upload(mid, m.to_animated_vertex_aos(), nv, L["stride"], off_pos=L["off_pos"], off_normal=L["off_normal"],
                            off_tangent=L["off_tangent"], off_weights=L["off_weights"], off_indices=L["off_indices"])
            st = {"mesh": mid, "pal": ctx.to_device(synth.make_palette(nb, seed, n_instances=n_inst)), "box": ctx.malloc(n_inst * 24 + 64),
                  "bufs": []}
            if name == "c4_vb68":
                b = ctx.to_device(m.to_animated_vertex_aos())
                st["bufs"] = [b]
                st["out"] = dict(d_out_vertices=b.ptr, out_stride=0)
            elif name == "c4_pos":
                b = ctx.malloc(n * 12 + 64)
                st["bufs"] = [b]
                st["out"] = dict(d_out_pos=b.ptr)
            else:
                bs = [ctx.malloc(n * 12 + 64), ctx.malloc(n * 12 + 64), ctx.malloc(n * 16 + 64)]
                st["bufs"] = bs
                st["out"] = dict(d_out_pos=bs[0].ptr, d_out_normal=bs[1].ptr, d_out_tangent=bs[2].ptr)
            sets.append(st)
        return nv, nb, n_inst, sets

    for name in args.configs.split(","):
        ctx.set_option("lbs.exact", 0 if name == "c3_fused" else 1)
        nv, nb, n_inst, sets = setup(name)

        def skin(st):
            ctx.lbs_skin_ex(st["mesh"], st["pal"].ptr, nb, n_inst, **st["out"])

        def two_pass(st):
            skin(st)
            ctx.skinned_aabb_device(st["mesh"], st["pal"].ptr, nb, n_inst, st["box"].ptr)

        def bounds(st):
            ctx.lbs_skin_ex_bounds(st["mesh"], st["pal"].ptr, nb, n_inst, **st["out"], d_out_aabb=st["box"].ptr)

        forms = {"skin_alone": skin, "skin_plus_skinned_aabb_device": two_pass, "skin_ex_bounds": bounds}
        times = {k: [] for k in forms}
        k = 0
        with torch.cuda.stream(stream):
            for f in forms.values():
                for _ in range(args.warmup):
                    f(sets[k % args.sets]); k += 1
            ctx.sync()
            for r in range(args.rounds):
                for fname, f in forms.items():
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
                    for e0, e1 in ev:
                        e0.record(stream)
                        f(sets[k % args.sets]); k += 1
                        e1.record(stream)
                    stream.synchronize()
                    times[fname] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
        ctx.sync()
        med = {f: statistics.median(v) for f, v in times.items()}
        res["configs"][name] = {
            "n_verts": nv, "n_bones": nb, "n_instances": n_inst, "exact": 0 if name == "c3_fused" else 1,
            "us_median": med,
            "us_p10_p90": {f: [float(np.percentile(v, 10)), float(np.percentile(v, 90))] for f, v in times.items()},
            "bounds_over_skin": med["skin_ex_bounds"] / med["skin_alone"],
            "bounds_over_two_pass": med["skin_ex_bounds"] / med["skin_plus_skinned_aabb_device"],
        }
        for st in sets:
            for b in st["bufs"] + [st["pal"], st["box"]]:
                b.free()
            ctx.mesh_free(st["mesh"])
    ctx.close()
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
