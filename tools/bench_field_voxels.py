#!/usr/bin/env python3
"""Time the back-projection of depth frames and the voxel centroids of the cloud (needs an MI355X; fails without one).

    python tools/bench_field_voxels.py [--resolution 128] [--repeats 20] [--frames 1 4] [--out profiles/field_voxels.json]

The same seeded model, feature map, grid, density threshold, fitted parts, joints and tree as tools/bench_field_nearest.py.  A
frame is a synthetic 480 x 640 depth image of the extracted cloud posed at a planted command of at most 0.3 rad per channel,
seen by the scene's context camera: every posed row is z-buffered into the 3 x 3 pixels around its projection (a row of the
128^3 grid is about 2.6 pixels wide there), empty pixels 0.  B frames are B problems.  Per B and per cell (1, 2 and 4 grid
steps), alternated inside every repeat, in one process:
  (depth_points)        the back-projection behind its Python entry (the 3 x 3 inverse, allocations, one memset, one launch),
  (voxel_reduce)        the whole reduction behind its Python entry,
  (build)               the build phase, which is njf_field_nearest's,
  (reduce_lane)         the reduce phase with a lane per cell,
  (reduce_wave)         the reduce phase with a wave per cell,
  (reduce_compact)      the reduce phase (lane) and the compact phase -- the scan consumes the flags, so the two are timed together,
  (normals_raw / normals_reduced)     point_normals of the cloud itself, radius 1.5 cells, on the lattice of that cell,
  (register_raw / register_reduced)   one round of register_commands (3 iterations) from zero, max_distance 3 cells,
  (torch_route)         what a user writes today: the back-projection in torch from full_frame_rays with the same validity
                        rules, ``torch.unique`` on the cell keys, ``index_add_`` and a division.
Device events around each call; a route whose warm-up call takes more than 250 ms is repeated 3 times instead of --repeats,
which its "repeats" field records.  Recorded besides: the points, the kept cells, the records per occupied cell and the largest
distance between the torch route's centroids and the device's.  Nothing is asserted: the numbers are recorded."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEIGHT, WIDTH, MAX_JUMP = 480, 640, 0.02
SLOW_MS, SLOW_REPEATS = 250.0, 3     # a route whose warm-up call takes longer is repeated 3 times only; "repeats" says so


def depth_frames(posed, intrinsics, cam2world, height, width):
    """[M, H, W] fp32: the smallest camera-space z of the rows of ``posed`` [M, n, 3] over the 3 x 3 pixels around each row's
    projection, 0 where no row falls."""
    m = posed.shape[0]
    w2c = torch.linalg.inv(cam2world.double())
    cam = posed.double() @ w2c[:, :3, :3].transpose(1, 2) + w2c[:, None, :3, 3]
    z = cam[..., 2]
    uv = (cam / z[..., None]) @ intrinsics.double().transpose(1, 2)
    col, row = torch.floor(uv[..., 0] * width).long(), torch.floor(uv[..., 1] * height).long()
    depth = torch.full((m, height * width), float("inf"), dtype=torch.float32, device=posed.device)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            r, c = row + dr, col + dc
            seen = (z > 0) & (c >= 0) & (c < width) & (r >= 0) & (r < height)
            key = torch.where(seen, r * width + c, torch.zeros_like(r))
            depth.scatter_reduce_(1, key, torch.where(seen, z, torch.full_like(z, float("inf"))).float(), "amin")
    return torch.where(torch.isfinite(depth), depth, torch.zeros_like(depth)).reshape(m, height, width)


def torch_route(depth, intrinsics, cam2world, cells, max_jump):
    """``(centroids [n, 3], counts [n], keys [n])`` of all frames together, keys = problem * C + cell index, ascending."""
    from neural_jacobian_field_amd.geometry import full_frame_rays
    b, h, w = depth.shape
    origins, directions, z = full_frame_rays(h, w, intrinsics, cam2world)
    valid = torch.isfinite(depth) & (depth > 0)
    keep = valid.clone()
    for shift, dim in ((1, 1), (-1, 1), (1, 2), (-1, 2)):
        dn, vn = torch.roll(depth, shift, dim), torch.roll(valid, shift, dim)
        edge = torch.ones_like(valid)
        index = [slice(None)] * 3
        index[dim] = 0 if shift == 1 else -1
        edge[tuple(index)] = False                                                  # the rolled-in border is no neighbour
        keep &= ~(vn & edge & valid & ((depth - dn).abs() > max_jump * torch.minimum(depth, dn)))
    points = (origins + directions * (depth.reshape(b, -1, 1) / z))[keep.reshape(b, -1)]
    problem = torch.arange(b, device=depth.device)[:, None].expand(b, h * w)[keep.reshape(b, -1)]
    origin = torch.tensor(cells.origin, device=depth.device)
    dims = torch.tensor(cells.dims, device=depth.device)
    t = (points - origin) * (1.0 / cells.step[0])
    f = torch.floor(t)
    inside = ((f >= 0) & (f < dims)).all(dim=1)
    f, points, problem = f[inside].long(), points[inside], problem[inside]
    key = problem * cells.num_nodes + (f[:, 0] * cells.dims[1] + f[:, 1]) * cells.dims[2] + f[:, 2]
    keys, inverse, counts = torch.unique(key, return_inverse=True, return_counts=True)
    sums = torch.zeros(keys.shape[0], 3, dtype=torch.float64, device=depth.device).index_add_(0, inverse, points.double())
    return (sums / counts[:, None]).float(), counts, keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keep", type=float, default=0.05)
    ap.add_argument("--min-nodes", type=int, default=64)
    ap.add_argument("--max-parts", type=int, default=32)
    ap.add_argument("--cell-steps", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_voxels.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_voxels: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import (FieldGrid, cell_grid, cloud_components, cloud_joints, cloud_pose, cloud_twists,
                                                        depth_points, dominant_joint, extract_field, point_normals,
                                                        register_commands, voxel_reduce)
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
        step = max(grid.step)
        xyz = cloud.xyz
        per_b = {}
        for b in args.frames:
            planted = torch.from_numpy((0.3 * np.random.default_rng(b).uniform(-1.0, 1.0, size=(b, 8)) / max(speed, 1e-6))
                                       .astype(np.float32)).to(dev)
            _, posed = cloud_pose(cloud, labels, tw, planted, joints=joints, tree=tree, first_order_elsewhere=False)
            k, c2w = (cams[key].expand(b, -1, -1).contiguous() for key in ("ctxt_k_norm", "ctxt_c2w"))
            depth = depth_frames(posed[:, :rows], k, c2w, HEIGHT, WIDTH)
            del posed
            raw = depth_points(depth, k, c2w, kind="z", max_jump=MAX_JUMP)
            t = raw.points.shape[1]
            per_cell = {}
            for steps in args.cell_steps:
                cell = steps * step
                cells = cell_grid(grid.origin, upper, cell)
                radius, reach = 1.5 * cell, 3.0 * cell
                c = cells.num_nodes
                capacity = min(t, c)
                workspace = torch.empty(hip.field_voxels_workspace(b, c, t), dtype=torch.int32, device=dev)
                out = dict(points=torch.empty(b, capacity, 3, device=dev), weight=torch.empty(b, capacity, dtype=torch.int32, device=dev),
                           cell=torch.empty(b, capacity, dtype=torch.int32, device=dev),
                           sums=torch.empty(b, capacity, 3, dtype=torch.int64, device=dev),
                           count=torch.empty(b, dtype=torch.int32, device=dev), outside=torch.empty(b, dtype=torch.int32, device=dev))

                def phase(p):
                    hip.field_voxels(raw.points if p & hip.FIELD_VOXELS_BUILD else (b, t), cells.c_grid(), out, phase=p, workspace=workspace)

                vox = voxel_reduce(raw.points, cells)
                kept = int(vox.count.max())
                reduced = vox.points[:, :max(kept, 1)].contiguous()                  # the caller's one host read, outside the timing

                def register(observed, count=None):
                    return register_commands(tw, xyz, labels, observed, cells, reach, joints=joints, tree=tree, count=cloud.count,
                                             observed_count=count, rounds=1, iterations=3)

                routes = {"depth_points": lambda: depth_points(depth, k, c2w, kind="z", max_jump=MAX_JUMP),
                          "voxel_reduce": lambda: voxel_reduce(raw.points, cells),
                          "build": lambda: phase(hip.FIELD_VOXELS_BUILD),
                          "reduce_lane": lambda: phase(hip.FIELD_VOXELS_REDUCE),
                          "reduce_wave": lambda: phase(hip.FIELD_VOXELS_REDUCE | hip.FIELD_VOXELS_WAVE),
                          "reduce_compact": lambda: phase(hip.FIELD_VOXELS_REDUCE | hip.FIELD_VOXELS_COMPACT),
                          "normals_raw": lambda: point_normals(None, raw.points, cells, radius),
                          "normals_reduced": lambda: point_normals(None, reduced, cells, radius, observed_count=vox.count),
                          "register_raw": lambda: register(raw.points),
                          "register_reduced": lambda: register(reduced, vox.count),
                          "torch_route": lambda: torch_route(depth, k, c2w, cells, MAX_JUMP)}
                times = {name: [] for name in routes}
                slow = set()                                                         # above SLOW_MS: SLOW_REPEATS repeats, and said so
                for it in range(args.warmup + args.repeats):
                    for name, fn in routes.items():
                        if name in slow and it >= args.warmup + SLOW_REPEATS:
                            continue
                        ms, result = timed(fn)
                        if it >= args.warmup:
                            times[name].append(ms)
                        elif ms > SLOW_MS:
                            slow.add(name)
                        del result
                med = {name: stats(v)["median_ms"] for name, v in times.items()}
                centroids, counts, keys = torch_route(depth, k, c2w, cells, MAX_JUMP)
                flat = (torch.arange(b, device=dev)[:, None] * c + vox.cell.long())[vox.cell >= 0]
                same_cells = flat.shape[0] == keys.shape[0] and bool((flat == keys).all())
                weight = vox.weight[vox.weight > 0].double()
                per_cell[str(steps)] = {
                    "cell": cell, "cells": list(cells.dims), "times": {name: stats(v) for name, v in times.items()},
                    "points": [int(v) for v in raw.kept.tolist()], "kept_cells": [int(v) for v in vox.count.tolist()],
                    "outside": [int(v) for v in vox.outside.tolist()],
                    "records_per_occupied_cell_mean": float(weight.mean()), "records_per_occupied_cell_max": int(weight.max()),
                    "wave_over_lane_reduce": round(med["reduce_wave"] / med["reduce_lane"], 2),
                    "normals_raw_over_reduced": round(med["normals_raw"] / med["normals_reduced"], 2),
                    "register_raw_over_reduced": round(med["register_raw"] / med["register_reduced"], 2),
                    "torch_route_over_depth_points_and_voxel_reduce": round(med["torch_route"] / (med["depth_points"] + med["voxel_reduce"]), 2),
                    "torch_route_keeps_the_same_cells": same_cells,
                    "torch_route_centroid_distance_max": float(torch.linalg.vector_norm(
                        centroids - vox.points[vox.cell >= 0], dim=1).max()) if same_cells else None,
                }
                print(f"B = {b}, cell {steps} steps: " + json.dumps(per_cell[str(steps)]["times"]), file=sys.stderr, flush=True)
                del workspace, out, vox, reduced
            per_b[str(b)] = {"pixels_with_a_depth": int((depth > 0).sum()), "rows_per_problem": t, "cells_in_steps": per_cell}
            del depth, raw

    result = {
        "what": "depth frames to world points and voxel centroids (tools/bench_field_voxels.py), device events, routes alternated",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": 8, "grid": list(grid.dims),
        "rows_counted": rows, "frame": [HEIGHT, WIDTH], "max_jump": MAX_JUMP, "grid_step": step, "frames": per_b,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
