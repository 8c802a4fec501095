#!/usr/bin/env python3
"""Time the match of posed rows to a depth frame by projection against the cell-list query (needs an MI355X; fails without one).

    python tools/bench_field_frame.py [--resolution 128] [--repeats 20] [--problems 1 4] [--out profiles/field_frame.json]

The scene of tools/bench_field_visible.py: the rows of the extracted cloud, posed at M planted commands of at most 0.3 rad per
channel, seen by V cameras in 480 x 640 images with footprint 1; the frame is the organised cloud ``depth_points`` makes of the
depth images ``visible_rows`` renders of those rows, the queries are its ``culled`` rows.  Per M and V, alternated inside every
repeat, in one process:
  (lane_r1 / lane_r4 / lane_r8)   njf_field_frame (a lane per row) at reach 1, 4 and 8,
  (nearest_query)                 njf_field_nearest's QUERY phase on the same culled rows against the same points, its cell list
                                  built beforehand; (nearest_build) that build, which the frame route does not need,
  (register_frame) / (register_visible)   one round (3 iterations) from zero of register_commands_frame and of
                                  register_commands_visible against the same frame.
Device events around each call, 2 warm-ups.  Recorded besides: the rows found by every route and the states.  Nothing is asserted:
the numbers are recorded.  (profiles/field_frame.json also holds wave_r1 / wave_r4 / wave_r8, the form with a wave per row that was
measured by this tool and then deleted: DESIGN.md section 26.)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEIGHT, WIDTH, FOOTPRINT, CULL_TOLERANCE, TOLERANCE, MAX_JUMP = 480, 640, 1, 0.01, 0.02, 0.02
REACHES = (1, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keep", type=float, default=0.05)
    ap.add_argument("--min-nodes", type=int, default=64)
    ap.add_argument("--max-parts", type=int, default=32)
    ap.add_argument("--problems", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--views", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_frame.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_frame: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import (FieldGrid, FieldView, cell_grid, cloud_components, cloud_joints, cloud_pose,
                                                        cloud_twists, depth_points, dominant_joint, extract_field,
                                                        register_commands_frame, register_commands_visible, visible_rows)
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

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        result = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), result

    with torch.no_grad():
        head, _ = model.compute_density(grid.points(device=dev)[None], enc)
        thr = float(torch.quantile(head.density.reshape(-1).double().cpu(), 1.0 - args.keep))
        del head
        cloud = extract_field(model, enc, grid, thr, cull=None, in_frustum=False)
        labels, sizes, _ = cloud_components(cloud, connectivity=6, keys=dominant_joint(cloud.jacobian), batch=1)
        tw = cloud_twists(cloud, labels=labels, sizes=sizes, min_nodes=args.min_nodes, max_parts=args.max_parts)
        joints = cloud_joints(cloud, labels, tw, batch=1)
        tree = joints.tree()
        rows = int(cloud.count.item())
        speed = float(torch.linalg.vector_norm(tw.omega, dim=-1).max())
        upper = tuple(o + s * (d - 1) for o, s, d in zip(grid.origin, grid.step, grid.dims))
        cell = 2 * max(grid.step)
        cells, distance = cell_grid(grid.origin, upper, cell), 3.0 * cell
        xyz = cloud.xyz
        n = xyz.shape[0]
        second = cams["ctxt_c2w"][0].clone()
        second[:3, 3] += torch.tensor([0.25, 0.05, 0.0], device=dev)                  # the second camera: a stereo partner
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        per_case = {}
        for m in args.problems:
            planted = torch.from_numpy((0.3 * np.random.default_rng(m).uniform(-1.0, 1.0, size=(m, 8)) / max(speed, 1e-6))
                                       .astype(np.float32)).to(dev)
            _, posed = cloud_pose(cloud, labels, tw, planted, joints=joints, tree=tree, first_order_elsewhere=False)
            posed = posed.contiguous()
            for views in args.views:
                k = cams["ctxt_k_norm"].expand(views, -1, -1).contiguous()
                c2w = torch.stack([cams["ctxt_c2w"][0], second])[:views].contiguous()
                w2c = hip.inverse(c2w)
                view = FieldView(k, c2w, HEIGHT, WIDTH, footprint=FOOTPRINT, tolerance=CULL_TOLERANCE)
                vis = visible_rows(posed, view, labels=labels, count=cloud.count)
                frames = depth_points(vis.depth.reshape(m * views, HEIGHT, WIDTH), k.repeat(m, 1, 1), c2w.repeat(m, 1, 1), kind="z",
                                      max_jump=MAX_JUMP, views_per_scene=views)
                frame, culled = frames.points, vis.culled
                t = frame.shape[1]
                out = {f: torch.empty(s, **(i32 if dt == torch.int32 else f32)) for (f, dt), s in zip(
                    hip.FIELD_FRAME_OUTPUTS, ((m, views, n), (m, views, n), (m, views, n), (m, n), (m, n), (m, n, 3), (m,), (m, 5)))}
                near = dict(index=torch.empty(m, n, **i32), distance2=torch.empty(m, n, **f32), matched=torch.empty(m, n, 3, **f32),
                            found=torch.empty(m, **i32))
                workspace = torch.empty(hip.field_nearest_workspace(m, cells.num_nodes, t), **i32)

                def match(reach):
                    hip.field_frame(culled, frame, k, w2c, HEIGHT, WIDTH, distance, out, m, count=cloud.count, labels=labels, reach=reach,
                                    tolerance=TOLERANCE)

                def nearest(phase):
                    build, query = bool(phase & hip.FIELD_NEAREST_BUILD), bool(phase & hip.FIELD_NEAREST_QUERY)
                    hip.field_nearest(frame if build else (m, t), culled if query else (m, n), cells.c_grid(), distance,
                                      near if query else None, m, count=cloud.count, labels=labels, phase=phase, workspace=workspace)

                kw = dict(joints=joints, tree=tree, count=cloud.count, rounds=1, iterations=3)
                routes = {}
                for reach in REACHES:
                    routes[f"lane_r{reach}"] = lambda reach=reach: match(reach)
                routes["nearest_build"] = lambda: nearest(hip.FIELD_NEAREST_BUILD)
                routes["nearest_query"] = lambda: nearest(hip.FIELD_NEAREST_QUERY)
                routes["register_frame"] = lambda: register_commands_frame(tw, xyz, labels, frame, distance, view, tolerance=TOLERANCE, **kw)
                routes["register_visible"] = lambda: register_commands_visible(tw, xyz, labels, frame, cells, distance, view, **kw)
                times = {name: [] for name in routes}
                for it in range(args.warmup + args.repeats):
                    for name, fn in routes.items():
                        ms, result = timed(fn)
                        if it >= args.warmup:
                            times[name].append(ms)
                        del result
                med = {name: stats(v)["median_ms"] for name, v in times.items()}
                found = {}
                for reach in REACHES:
                    match(reach)
                    found[f"r{reach}"] = out["found"].tolist()
                states, lane = out["states"].tolist(), out
                nearest(hip.FIELD_NEAREST_QUERY)
                name = f"M{m}_V{views}"
                per_case[name] = {
                    "problems": m, "views": views, "times": {r: stats(v) for r, v in times.items()},
                    "visible_rows": vis.visible.tolist(), "frame_points": frames.kept.tolist(), "rows_found_by_reach": found,
                    "rows_found_by_the_cell_list": near["found"].tolist(), "states_at_reach_8": states,
                    "rows_with_the_cell_lists_index_at_reach_8": int((lane["index"] == near["index"]).sum()),
                    "lane_over_nearest_query": {f"r{r}": round(med[f"lane_r{r}"] / med["nearest_query"], 2) for r in REACHES},
                    "register_frame_over_register_visible": round(med["register_frame"] / med["register_visible"], 2),
                }
                print(name + ": " + json.dumps(per_case[name]), file=sys.stderr, flush=True)
                del vis, out, near, frames, workspace
            del posed

    result = {
        "what": "the match of posed rows to a depth frame by projection against the cell-list query (tools/bench_field_frame.py), device "
                "events, routes alternated",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": 8, "grid": list(grid.dims),
        "rows": n, "rows_counted": rows, "frame": [HEIGHT, WIDTH], "footprint": FOOTPRINT, "cull_tolerance": CULL_TOLERANCE,
        "tolerance": TOLERANCE, "max_jump": MAX_JUMP, "registration_cell": cell, "max_distance": distance, "cases": per_case,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
