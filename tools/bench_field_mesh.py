#!/usr/bin/env python3
"""Time the Jacobian-field surface extraction on a voxel grid (needs an MI355X; fails without one).

    python tools/bench_field_mesh.py [--resolution 128] [--repeats 20] [--out profiles/field_mesh.json]

Two routes on the same commit, the same seeded model (jacobian_mlp, A = 8, default precision), the same synthetic feature map and
the same density threshold, alternated inside every repeat:
  (mesh)  extract_mesh: density pass on every node, six meshing launches, colour + Jacobian on the vertices,
  (cloud) extract_field with cull=None: route (b) of tools/bench_field_volume.py, re-timed here as the yardstick.
Both with in_frustum=False.  Device events around each call (the eager forms' host reads of the counts are inside the window:
they are part of what a caller waits for); the per-image projection is warm for both.  The threshold is the quantile of the
dense density that `--keep` of the nodes pass.  Peak extra memory = torch.cuda.max_memory_allocated over a call minus what was
allocated before it.  The per-launch split is one further call with events around every entry point."""
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
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--keep", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_mesh.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_mesh: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import FieldGrid, extract_field, extract_mesh
    from neural_jacobian_field_amd.model import Model

    dev = torch.device("cuda:0")
    cfg = model_cfg_from_dict({"action_dim": 8, "rendering": {"num_proposal_samples": [16], "num_nerf_samples": 12},
                               "action_decoder": {"name": "jacobian_mlp"}})
    model = Model(cfg)
    model.load_state_dict(synthetic.seeded_state_dict(synthetic.model_shapes("jacobian_mlp", 8), seed=0), strict=True)
    model.to(dev).eval().requires_grad_(False)
    cams = {k: v.to(dev) for k, v in synthetic.synthetic_cameras(1).items()}
    enc = PixelEncoding(features=synthetic.synthetic_features(1, 128, 128, seed=1).to(dev), extrinsics=cams["ctxt_c2w"],
                        intrinsics=cams["ctxt_k_norm"], action=synthetic.synthetic_action(1, 8).to(dev))
    grid = FieldGrid.from_bounds((-0.45, -0.45, 0.8), (0.45, 0.45, 2.0), args.resolution)
    n = grid.num_nodes

    with torch.no_grad():
        head, _ = model.compute_density(grid.points(device=dev)[None], enc)
        thr = float(torch.quantile(head.density.reshape(-1).double().cpu(), 1.0 - args.keep))
        del head
    routes = {"mesh": lambda: extract_mesh(model, enc, grid, thr, in_frustum=False),
              "cloud_b_no_cull": lambda: extract_field(model, enc, grid, thr, cull=None, in_frustum=False)}
    times = {k: [] for k in routes}
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
        mesh = routes["mesh"]()
        launches = {}
        for name in routes:
            sink = []
            hip.set_profile_sink(sink)
            routes[name]()
            hip.set_profile_sink(None)
            torch.cuda.synchronize()
            launches[name] = [(nm, round(s.elapsed_time(e), 4)) for nm, s, e in sink]

    def stats(v):
        t = torch.tensor(v, dtype=torch.float64)
        return {"median_ms": round(float(t.median()), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4),
                "repeats": len(v)}

    meshing = sum(ms for nm, ms in launches["mesh"] if nm.startswith("njf_field_mesh_"))
    density = sum(ms for nm, ms in launches["mesh"] if nm == "njf_field_forward")
    result = {
        "what": "extract_mesh on a voxel grid vs extract_field (tools/bench_field_mesh.py), device events, routes alternated",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": 8, "precision": model.decoder.precision,
        "grid": list(grid.dims), "nodes": n, "batch": 1, "density_threshold": thr, "in_frustum": False,
        "vertices": int(mesh.vertex_count.item()), "triangles": int(mesh.triangle_count.item()),
        "times": {k: stats(v) for k, v in times.items()},
        "peak_extra_memory_MiB": {k: round(v, 2) for k, v in peak.items()},
        "launch_times_ms": launches,
        "meshing_entry_points_ms": round(meshing, 4), "density_pass_ms": round(density, 4),
        "meshing_over_density": round(meshing / density, 4) if density > 0 else None,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
