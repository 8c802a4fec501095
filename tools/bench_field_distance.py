#!/usr/bin/env python3
"""Time the fusion of depth frames into a truncated signed distance, and its sampling, against the same fusion written with torch
ops (needs an MI355X; fails without one).

    python tools/bench_field_distance.py [--resolution 128] [--repeats 20] [--problems 1 4] [--out profiles/field_distance.json]

The scene of tools/bench_field_visible.py: the rows of the extracted cloud, posed at M planted commands of at most 0.3 rad per
channel, seen by V cameras in 480 x 640 images with footprint 1; the depth images are the ones ``visible_rows`` renders of those
rows.  They are fused on the extraction grid itself with a truncation of four grid steps.  Per M and V, alternated inside every
repeat, in one process:
  (fuse_fresh / fuse_into)    njf_field_tsdf without a state, and with its own outputs as the state (in place),
  (torch_fresh / torch_into)  the yardstick: the same rule with torch ops on the same device -- ``grid.points()``, a matmul
                              projection, ``gather``, ``where`` --, out of place,
  (sample)                    njf_field_tsdf_sample of the posed rows in the fused field.
Device events around each call, 2 warm-ups.  Recorded besides: the achieved bytes per second of the fused pass (8 bytes per node
out, 8 more in with a state), the ratio to the yardstick, and on how many nodes the yardstick's weight differs (its projection is
a matmul, not the kernel's fma chain).  Nothing is asserted: the numbers are recorded."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEIGHT, WIDTH, FOOTPRINT, CULL_TOLERANCE, TRUNCATION_STEPS, MAX_WEIGHT = 480, 640, 1, 0.01, 4, 64.0


def torch_fuse(points, depth, k, w2c, near, far, truncation, max_weight, state=None):
    """The rule of njf_field_tsdf with torch ops: (values [M, N], weight [M, N], known [M])."""
    m, views, height, width = depth.shape
    cam = points @ w2c[:, :3, :3].transpose(1, 2) + w2c[:, None, :3, 3]             # [V, N, 3]
    z = cam[..., 2]
    s, t = cam[..., 0] / z, cam[..., 1] / z
    col = torch.floor((k[:, 0, 0, None] * s + k[:, 0, 1, None] * t + k[:, 0, 2, None]) * width)
    row = torch.floor((k[:, 1, 0, None] * s + k[:, 1, 1, None] * t + k[:, 1, 2, None]) * height)
    inside = torch.isfinite(z) & (z > near) & (col >= 0) & (col < width) & (row >= 0) & (row < height)
    pixel = torch.where(inside, row * width + col, 0.0).long()
    d = depth.reshape(m, views, -1).gather(2, pixel[None].expand(m, -1, -1))       # [M, V, N]
    sd = d - z[None]
    ok = inside[None] & torch.isfinite(d) & (d > near) & (d <= far) & (sd >= -truncation)
    total = torch.where(ok, sd.clamp(max=truncation), 0.0).sum(dim=1)
    c = ok.sum(dim=1).to(torch.float32)
    if state is None:
        values = torch.where(c > 0, total / c, float("nan"))
        weight = c.clamp(max=max_weight)
    else:
        d0, w0 = state
        values = torch.where(c == 0, d0, torch.where(w0 > 0, (w0 * d0 + total) / (w0 + c), total / c))
        weight = torch.where(c == 0, w0, torch.where(w0 > 0, w0 + c, c).clamp(max=max_weight))
    return values, weight, (weight > 0).sum(dim=1).to(torch.int32)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_distance.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_distance: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import (FieldGrid, FieldView, cloud_components, cloud_joints, cloud_pose, cloud_twists,
                                                        dominant_joint, extract_field, visible_rows)
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
    nodes = grid.num_nodes
    truncation = float(np.float32(TRUNCATION_STEPS * max(grid.step)))

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
        speed = float(torch.linalg.vector_norm(tw.omega, dim=-1).max())
        n = cloud.xyz.shape[0]
        second = cams["ctxt_c2w"][0].clone()
        second[:3, 3] += torch.tensor([0.25, 0.05, 0.0], device=dev)                  # the second camera: a stereo partner
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        c_grid = grid.c_grid()
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
                depth = vis.depth.contiguous()                                        # [M, V, H, W], 0 = no return
                fresh = dict(values=torch.empty(m, nodes, **f32), weight=torch.empty(m, nodes, **f32), known=torch.empty(m, **i32))
                running = {f: torch.empty_like(t) for f, t in fresh.items()}
                sampled = dict(state=torch.empty(m, n, **i32), distance=torch.empty(m, n, **f32), gradient=torch.empty(m, n, 3, **f32),
                               states=torch.empty(m, hip.FIELD_TSDF_STATES, **i32))

                def fuse(out, state):
                    hip.field_tsdf(c_grid, depth, k, w2c, truncation, out, max_weight=MAX_WEIGHT,
                                   values_in=None if state is None else state["values"], weight_in=None if state is None else state["weight"])

                def yardstick(state):
                    return torch_fuse(grid.points(device=dev), depth, k, w2c, 0.0, float("inf"), truncation, MAX_WEIGHT, state)

                fuse(fresh, None)
                fuse(running, None)
                routes = {
                    "fuse_fresh": lambda: fuse(fresh, None),
                    "fuse_into": lambda: fuse(running, running),
                    "torch_fresh": lambda: yardstick(None),
                    "torch_into": lambda: yardstick((fresh["values"], fresh["weight"])),
                    "sample": lambda: hip.field_tsdf_sample(posed, c_grid, fresh["values"], fresh["weight"], sampled, m, count=cloud.count,
                                                            labels=labels),
                }
                times = {name: [] for name in routes}
                for it in range(args.warmup + args.repeats):
                    for name, fn in routes.items():
                        ms, result = timed(fn)
                        if it >= args.warmup:
                            times[name].append(ms)
                        del result
                med = {name: stats(v)["median_ms"] for name, v in times.items()}
                fuse(fresh, None)
                values, weight, known = yardstick(None)
                both = (weight > 0) & (fresh["weight"] > 0)
                name = f"M{m}_V{views}"
                per_case[name] = {
                    "problems": m, "views": views, "times": {r: stats(v) for r, v in times.items()},
                    "pixels_with_a_depth": (depth > 0).sum(dim=(2, 3)).tolist(), "known_nodes": fresh["known"].tolist(),
                    "known_nodes_of_the_yardstick": known.tolist(),
                    "nodes_whose_weight_differs_from_the_yardsticks": int((weight != fresh["weight"]).sum()),
                    "largest_value_difference_where_both_have_a_weight": float((values - fresh["values"])[both].abs().max()) if both.any() else 0.0,
                    "states_of_the_sampled_rows": sampled["states"].tolist(),
                    "fused_GBps": {"fresh": round(8.0 * m * nodes / med["fuse_fresh"] / 1e6, 1),
                                   "into": round(16.0 * m * nodes / med["fuse_into"] / 1e6, 1)},
                    "kernel_over_yardstick": {"fresh": round(med["fuse_fresh"] / med["torch_fresh"], 4),
                                              "into": round(med["fuse_into"] / med["torch_into"], 4)},
                }
                print(name + ": " + json.dumps(per_case[name]), file=sys.stderr, flush=True)
                del vis, depth, fresh, running, sampled, values, weight
            del posed

    result = {
        "what": "the fusion of depth frames into a truncated signed distance against the same fusion with torch ops "
                "(tools/bench_field_distance.py), device events, routes alternated",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": 8, "grid": list(grid.dims), "nodes": nodes,
        "rows": n, "frame": [HEIGHT, WIDTH], "footprint": FOOTPRINT, "truncation": truncation, "max_weight": MAX_WEIGHT, "cases": per_case,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
