#!/usr/bin/env python3
"""Time inverse kinematics with a 3 x 3 information per target against the isotropic solver (needs an MI355X; fails without
one).

    python tools/bench_field_metric.py [--resolution 128] [--repeats 20] [--problems 1 16 64] [--out profiles/field_metric.json]

The scene of tools/bench_field_commands.py: the same seeded model, feature map, grid, density threshold, 32 fitted parts, joints
and tree.  The targets are ``cloud_pose`` at random commands; the information is that of the pixel rays of one camera through
those targets (``ray_information`` of the directions from the camera's centre), so that the planted commands are a minimum of
both objectives.  Per M, alternated inside every repeat, in one process:
  (cloud_commands_metric) the three launches of njf_field_commands_metric behind their Python entry: allocations, no host read,
  (cloud_commands)        the untouched isotropic entry on the same rows: THE COMPARATOR.
Device events around each call.  The per-phase split is one further pass with events around each phase, again alternated:
the metric moments in the reduce-scatter form and in the butterfly form, the metric solver, and the isotropic moments and
solver.  Recorded besides: the ratios to the comparator, the accepted steps, the costs, the distance of both routes' commands
from the planted ones.  Nothing is asserted: the numbers are recorded."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keep", type=float, default=0.05)
    ap.add_argument("--min-nodes", type=int, default=64)
    ap.add_argument("--max-parts", type=int, default=32)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--problems", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_metric.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_metric: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import (FieldGrid, cloud_commands, cloud_commands_metric, cloud_components, cloud_joints,
                                                        cloud_pose, cloud_twists, dominant_joint, extract_field, ray_information)
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

    def stats(v):
        t = torch.tensor(v, dtype=torch.float64)
        return {"median_ms": round(float(t.median()), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4),
                "repeats": len(v)}

    with torch.no_grad():
        head, _ = model.compute_density(grid.points(device=dev)[None], enc)
        thr = float(torch.quantile(head.density.reshape(-1).double().cpu(), 1.0 - args.keep))
        del head
        cloud = extract_field(model, enc, grid, thr, cull=None, in_frustum=False)
        n = cloud.index.shape[0]
        labels, sizes, components = cloud_components(cloud, connectivity=6, keys=dominant_joint(cloud.jacobian), batch=1)
        tw = cloud_twists(cloud, labels=labels, sizes=sizes, min_nodes=args.min_nodes, max_parts=args.max_parts)
        joints = cloud_joints(cloud, labels, tw, batch=1)
        tree = joints.tree()
        k = int(tw.count.clamp(max=tw.labels.shape[0]).item())
        if k < 2:
            sys.exit(f"bench_field_metric: fewer than two components of {args.min_nodes} nodes among {n} rows")
        rows = int(cloud.count.item())
        speed = float(torch.linalg.vector_norm(tw.omega, dim=-1).max())
        links = dict(part_a=joints.part_a, part_b=joints.part_b, count=joints.count, anchor=joints.anchor, omega=joints.omega,
                     velocity=joints.velocity, parent=tree[0], joint_of=tree[1])
        kk = tw.labels.shape[0]
        eye = torch.tensor([0.0, 0.0, -1.5], device=dev)                       # a camera in front of the box, looking down +z
        per_m = {}
        for m in args.problems:
            planted = torch.from_numpy((0.5 * np.random.default_rng(m).uniform(-1.0, 1.0, size=(m, 8)) / max(speed, 1e-6))
                                       .astype(np.float32)).to(dev)
            _, targets = cloud_pose(cloud, labels, tw, planted, joints=joints, tree=tree, first_order_elsewhere=False)
            targets[:, rows:] = 0.0                                                   # (rows past the count are not written)
            information = ray_information(targets - eye).contiguous()               # [M, n, 6]
            kw = dict(joints=joints, tree=tree, iterations=args.iterations)
            fit = cloud_commands_metric(cloud, labels, tw, targets, information, **kw)
            iso = cloud_commands(cloud, labels, tw, targets, **kw)
            out = {f: getattr(fit, f) for f in fit.__dataclass_fields__}
            out_iso = {f: getattr(iso, f) for f in iso.__dataclass_fields__}
            workspace = torch.empty(hip.field_commands_metric_workspace(m, kk, 8, n), dtype=torch.float64, device=dev)
            points = dict(xyz=cloud.xyz, labels=labels, count=cloud.count, targets=targets, information=information)

            def metric(phase):
                hip.field_commands_metric(tw.labels, tw.status, tw.centroid, tw.omega, tw.velocity, points, out, parts_count=tw.count,
                                          joints=links, iterations=args.iterations, phase=phase, workspace=workspace)

            def isotropic(phase):
                hip.field_commands(tw.labels, tw.status, tw.centroid, tw.omega, tw.velocity, points, out_iso, parts_count=tw.count,
                                   joints=links, iterations=args.iterations, phase=phase, workspace=workspace)

            routes = {"cloud_commands_metric": lambda: cloud_commands_metric(cloud, labels, tw, targets, information, **kw),
                      "cloud_commands": lambda: cloud_commands(cloud, labels, tw, targets, **kw)}
            times = {name: [] for name in routes}
            for it in range(args.warmup + args.repeats):
                for name, fn in routes.items():
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    result = fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if it >= args.warmup:
                        times[name].append(e0.elapsed_time(e1))
                    del result
            phases = (("metric_moments_reduce_scatter", metric, hip.FIELD_COMMANDS_MOMENTS),
                      ("metric_moments_butterfly", metric, hip.FIELD_COMMANDS_MOMENTS | hip.FIELD_COMMANDS_METRIC_BUTTERFLY),
                      ("isotropic_moments", isotropic, hip.FIELD_COMMANDS_MOMENTS),
                      ("metric_solve", metric, hip.FIELD_COMMANDS_SOLVE),
                      ("isotropic_solve", isotropic, hip.FIELD_COMMANDS_SOLVE))
            per_phase = {name: [] for name, _, _ in phases}
            for it in range(args.warmup + args.repeats):
                sink = []
                hip.set_profile_sink(sink)
                for _, fn, phase in phases:
                    fn(phase)
                hip.set_profile_sink(None)
                torch.cuda.synchronize()
                if it >= args.warmup:
                    for (name, _, _), (_, s, e) in zip(phases, sink):
                        per_phase[name].append(s.elapsed_time(e))
            med = {name: stats(v)["median_ms"] for name, v in list(times.items()) + list(per_phase.items())}
            per_m[str(m)] = {
                "times": {name: stats(v) for name, v in times.items()},
                "phase_split": {name: stats(v) for name, v in per_phase.items()},
                "metric_over_isotropic": {
                    "whole": round(med["cloud_commands_metric"] / med["cloud_commands"], 2),
                    "moments_reduce_scatter": round(med["metric_moments_reduce_scatter"] / med["isotropic_moments"], 2),
                    "moments_butterfly": round(med["metric_moments_butterfly"] / med["isotropic_moments"], 2),
                    "solve": round(med["metric_solve"] / med["isotropic_solve"], 2)},
                "butterfly_over_reduce_scatter": round(med["metric_moments_butterfly"] / med["metric_moments_reduce_scatter"], 2),
                "moments_input_bytes": (12 + 24) * m * rows,                            # targets and information of every row
                "accepted_steps": {"metric": fit.steps.tolist(), "isotropic": iso.steps.tolist()},
                "status": fit.status.tolist(), "cost_max": float(fit.cost.max()), "initial_cost_min": float(fit.initial_cost.min()),
                "largest_distance_to_the_planted_commands": {"cloud_commands_metric": float((fit.commands - planted).abs().max()),
                                                             "cloud_commands": float((iso.commands - planted).abs().max())},
            }
            print(f"M = {m}: " + json.dumps(per_m[str(m)]["times"]) + " " + json.dumps(per_m[str(m)]["phase_split"]), file=sys.stderr,
                  flush=True)
            del targets, information, fit, iso, out, out_iso, workspace

    result = {
        "what": "commands from targets with a 3x3 information on the part tree (tools/bench_field_metric.py), device events, routes "
                "alternated; the isotropic solve_commands on the same rows is the comparator",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": 8, "grid": list(grid.dims),
        "rows": n, "rows_counted": rows, "components": int(components.item()), "parts_true": int(tw.count.item()), "parts_fitted": k,
        "joints": int(joints.count.item()), "iterations": args.iterations, "problems": per_m,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
