#!/usr/bin/env python3
"""Time the fused multi-view field extraction against one extraction per view (needs an MI355X; fails without one).

    python tools/bench_field_fusion.py [--resolution 128] [--views 4] [--repeats 20] [--out profiles/field_fusion.json]

One scene (G = 1) of V views on the same commit, the same seeded model (jacobian_mlp, A = 8, default precision), synthetic
feature maps and cameras around the grid, the same density threshold; four routes alternated inside every repeat:
  (fused_cloud)    extract_field(views_per_scene=V): one cloud for the scene,
  (separate_cloud) V calls of extract_field, one per view (what a caller had before: V clouds that disagree),
  (fused_mesh)     extract_mesh(views_per_scene=V),
  (separate_mesh)  V calls of extract_mesh.
All with in_frustum=True (the frustum decides which views count at a node) and cull=None.  Device events around each route
(the eager forms' host reads of the counts are inside the window: they are part of what a caller waits for); the per-image
projection is warm for all.  The threshold is the quantile of the "mean"-fused density that `--keep` of the valid nodes pass.
Peak extra memory = torch.cuda.max_memory_allocated over a route minus what was allocated before it.  The per-launch split is
one further call per fused route with events around every entry point; `fusion_over_density` = (njf_field_fuse +
njf_field_combine) / the dense per-view density pass of the same call.  No threshold is asserted."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--keep", type=float, default=0.05)
    ap.add_argument("--fuse", default="mean")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_fusion.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_fusion: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import FieldGrid, extract_field, extract_mesh, fuse_views
    from neural_jacobian_field_amd.model import Model

    dev = torch.device("cuda:0")
    v = args.views
    cfg = model_cfg_from_dict({"action_dim": 8, "rendering": {"num_proposal_samples": [16], "num_nerf_samples": 12},
                               "action_decoder": {"name": "jacobian_mlp"}})
    model = Model(cfg)
    model.load_state_dict(synthetic.seeded_state_dict(synthetic.model_shapes("jacobian_mlp", 8), seed=0), strict=True)
    model.to(dev).eval().requires_grad_(False)
    # view 0: the identity camera of the other field benches; the others look from centres spread along x and y with a small
    # seeded rotation, so that every view sees most of the grid and none all of it
    c2w = synthetic.general_pose(7, v, scale=0.04)
    for i in range(v):
        c2w[i, :3, 3] = torch.tensor([0.25 * ((i + 1) // 2) * (1 if i % 2 else -1), 0.1 * (i % 3 - 1), 0.0])
    c2w[0] = torch.eye(4)
    k = synthetic.synthetic_cameras(v)["ctxt_k_norm"]
    enc = PixelEncoding(features=synthetic.synthetic_features(v, 128, 128, seed=1).to(dev), extrinsics=c2w.to(dev),
                        intrinsics=k.to(dev), action=synthetic.synthetic_action(v, 8).to(dev))
    per_view = [PixelEncoding(features=enc.features[i:i + 1].contiguous(), extrinsics=enc.extrinsics[i:i + 1].contiguous(),
                              intrinsics=enc.intrinsics[i:i + 1].contiguous(), action=enc.action[i:i + 1].contiguous())
                for i in range(v)]
    grid = FieldGrid.from_bounds((-0.45, -0.45, 0.8), (0.45, 0.45, 2.0), args.resolution)
    n = grid.num_nodes

    with torch.no_grad():
        pts = grid.points(device=dev)[None]
        dense = torch.cat([model.compute_density(pts, e)[0].density.reshape(1, n) for e in per_view])
        fused, seen, valid = fuse_views(grid, dense, enc, views_per_scene=v, mode=args.fuse)
        thr = float(torch.quantile(fused[valid].double().cpu()[:16_000_000], 1.0 - args.keep))
        seen_count = torch.bincount(sum(((seen >> i) & 1).long() for i in range(v)).reshape(-1), minlength=v + 1).tolist()
        del pts, dense, fused, seen, valid
    kw = dict(views_per_scene=v, fuse=args.fuse)
    routes = {"fused_cloud": lambda: extract_field(model, enc, grid, thr, **kw),
              "separate_cloud": lambda: [extract_field(model, e, grid, thr) for e in per_view],
              "fused_mesh": lambda: extract_mesh(model, enc, grid, thr, **kw),
              "separate_mesh": lambda: [extract_mesh(model, e, grid, thr) for e in per_view]}
    times = {name: [] for name in routes}
    peak = {}
    with torch.no_grad():
        for it in range(args.warmup + args.repeats):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
                peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                del out
        cloud, mesh = routes["fused_cloud"](), routes["fused_mesh"]()
        sizes = {"fused_cloud_points": int(cloud.count.item()), "fused_mesh_vertices": int(mesh.vertex_count.item()),
                 "fused_mesh_triangles": int(mesh.triangle_count.item()),
                 "separate_cloud_points": [int(c.count.item()) for c in routes["separate_cloud"]()]}
        del cloud, mesh
        launches = {}
        for name in ("fused_cloud", "fused_mesh"):
            sink = []
            hip.set_profile_sink(sink)
            routes[name]()
            hip.set_profile_sink(None)
            torch.cuda.synchronize()
            launches[name] = [(nm, round(s.elapsed_time(e), 4)) for nm, s, e in sink]

    def stats(x):
        t = torch.tensor(x, dtype=torch.float64)
        return {"median_ms": round(float(t.median()), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4),
                "repeats": len(x)}

    def split(rows):
        fusion = sum(ms for nm, ms in rows if nm in ("njf_field_fuse", "njf_field_combine"))
        density = next(ms for nm, ms in rows if nm == "njf_field_forward")        # the first one: the dense per-view pass
        return {"fuse_ms": round(sum(ms for nm, ms in rows if nm == "njf_field_fuse"), 4),
                "combine_ms": round(sum(ms for nm, ms in rows if nm == "njf_field_combine"), 4),
                "dense_density_pass_ms": round(density, 4), "fusion_over_density": round(fusion / density, 5) if density > 0 else None}

    result = {
        "what": "fused multi-view extraction vs one extraction per view (tools/bench_field_fusion.py), device events, routes "
                "alternated",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": 8, "precision": model.decoder.precision,
        "grid": list(grid.dims), "nodes": n, "scenes": 1, "views": v, "fuse": args.fuse, "min_views": 1, "in_frustum": True,
        "density_threshold": thr, "nodes_seen_by_k_views": seen_count, **sizes,
        "times": {name: stats(x) for name, x in times.items()},
        "peak_extra_memory_MiB": {name: round(x, 2) for name, x in peak.items()},
        "launch_times_ms": launches,
        "fusion": {name: split(rows) for name, rows in launches.items()},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    print()
    print("| route | median ms | min ms | peak extra MiB |")
    print("|---|---|---|---|")
    for name in routes:
        s = result["times"][name]
        print(f"| {name} | {s['median_ms']} | {s['min_ms']} | {result['peak_extra_memory_MiB'][name]} |")
    for name, s in result["fusion"].items():
        print(f"| {name}: fuse {s['fuse_ms']} ms + combine {s['combine_ms']} ms over the dense pass {s['dense_density_pass_ms']} ms "
              f"= {s['fusion_over_density']} | | | |")


if __name__ == "__main__":
    main()
