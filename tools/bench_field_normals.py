#!/usr/bin/env python3
"""Time the normals of an observed cloud from integer moments on the cell list (needs an MI355X; fails without one).

    python tools/bench_field_normals.py [--resolution 128] [--repeats 20] [--problems 1 16 64] [--out profiles/field_normals.json]

The same seeded model, feature map, grid, density threshold, fitted parts, joints and tree as tools/bench_field_nearest.py.  The
observed cloud of a problem is ``cloud_pose`` at a planted command of at most 0.3 rad per channel, its rows in shuffled order;
the cells are ``cell_grid`` over the grid's bounds with the grid's step; the rows whose normals are taken are the observed
points themselves.  Per radius (in cells) and per M, alternated inside every repeat, in one process:
  (point_normals)   the whole call behind its Python entry: allocations, the build, the moments, the finish,
  (build)           the build phase, which is njf_field_nearest's,
  (moments_lane)    the moments phase with a lane per row,
  (moments_wave)    the moments phase with a wave per row,
  (finish)          the finish phase,
  (nearest_query)   the query phase of njf_field_nearest on the same rows with max_distance = radius: one pass over the cell list,
  (torch_route)     what a user writes without it, ONE repeat at the first M only: ``torch.cdist`` in chunks, a masked covariance in
                    double by matrix products, ``torch.linalg.eigh``.
Device events around each call.  Recorded besides: the records a row reads and its neighbours (the numpy restatement, on a
sample of rows), and the |sin| between the torch route's normals and the device's, over all rows that have both and over
those on which the two routes count the same neighbours.  Nothing is asserted: the numbers are
recorded."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_route(observed, radius, min_neighbours=3, chunk_elements=2 ** 26):
    """``(normal [T, 3] float64 with NaN, neighbours [T])`` of one cloud ``observed [T, 3]`` against itself."""
    t = observed.shape[0]
    p = observed.double()
    pp = (p[:, :, None] * p[:, None, :]).reshape(t, 9)
    normal = torch.full((t, 3), float("nan"), dtype=torch.float64, device=observed.device)
    neighbours = torch.zeros(t, dtype=torch.int64, device=observed.device)
    chunk = max(1, chunk_elements // t)
    for lo in range(0, t, chunk):
        w = (torch.cdist(observed[lo:lo + chunk], observed) <= radius).double()
        s0 = w.sum(dim=1)
        mean = (w @ p) / s0[:, None]
        cov = ((w @ pp) / s0[:, None]).reshape(-1, 3, 3) - mean[:, :, None] * mean[:, None, :]
        ok = s0 >= min_neighbours
        _, vec = torch.linalg.eigh(torch.where(ok[:, None, None], cov, torch.eye(3, dtype=torch.float64, device=observed.device)))
        normal[lo:lo + chunk] = torch.where(ok[:, None], vec[:, :, 0], normal[lo:lo + chunk])
        neighbours[lo:lo + chunk] = s0.long()
    return normal, neighbours


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keep", type=float, default=0.05)
    ap.add_argument("--min-nodes", type=int, default=64)
    ap.add_argument("--max-parts", type=int, default=32)
    ap.add_argument("--radius-cells", type=float, nargs="+", default=[1.5, 3.0])
    ap.add_argument("--sample", type=int, default=1000)
    ap.add_argument("--problems", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_normals.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_normals: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    import field_normals_restatement as restatement
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import (FieldGrid, cell_grid, cloud_components, cloud_joints, cloud_pose, cloud_twists,
                                                        dominant_joint, extract_field, point_normals)
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
        cell = max(grid.step)
        cells = cell_grid(grid.origin, upper, cell)
        per_radius = {}
        for radius_cells in args.radius_cells:
            radius = radius_cells * cell
            per_m = {}
            for m in args.problems:
                planted = torch.from_numpy((0.3 * np.random.default_rng(m).uniform(-1.0, 1.0, size=(m, 8)) / max(speed, 1e-6))
                                           .astype(np.float32)).to(dev)
                _, posed = cloud_pose(cloud, labels, tw, planted, joints=joints, tree=tree, first_order_elsewhere=False)
                order = torch.from_numpy(np.random.default_rng(100 + m).permutation(rows)).to(dev)
                observed = posed[:, order].contiguous()                                   # [M, rows, 3]
                del posed
                t = observed.shape[1]
                workspace = torch.empty(hip.field_normals_workspace(m, cells.num_nodes, t), dtype=torch.int32, device=dev)
                out = dict(normal=torch.empty(m, t, 3, device=dev), neighbours=torch.empty(m, t, dtype=torch.int32, device=dev),
                           variation=torch.empty(m, t, device=dev), moments=torch.empty(m, t, 10, dtype=torch.int64, device=dev))
                near = dict(index=torch.empty(m, t, dtype=torch.int32, device=dev), distance2=torch.empty(m, t, device=dev),
                            matched=torch.empty(m, t, 3, device=dev), found=torch.empty(m, dtype=torch.int32, device=dev))

                def phase(p):
                    hip.field_normals(observed if p & hip.FIELD_NORMALS_BUILD else (m, t), observed, cells.c_grid(), radius, out, m, phase=p,
                                      workspace=workspace)

                routes = {"point_normals": lambda: point_normals(None, observed, cells, radius),
                          "build": lambda: phase(hip.FIELD_NORMALS_BUILD),
                          "moments_lane": lambda: phase(hip.FIELD_NORMALS_MOMENTS),
                          "moments_wave": lambda: phase(hip.FIELD_NORMALS_MOMENTS | hip.FIELD_NORMALS_WAVE),
                          "finish": lambda: phase(hip.FIELD_NORMALS_FINISH),
                          "nearest_query": lambda: hip.field_nearest((m, t), observed, cells.c_grid(), radius, near, m,
                                                                     phase=hip.FIELD_NEAREST_QUERY, workspace=workspace)}
                times = {name: [] for name in routes}
                for it in range(args.warmup + args.repeats):
                    for name, fn in routes.items():
                        ms, result = timed(fn)
                        if it >= args.warmup:
                            times[name].append(ms)
                        del result
                med = {name: stats(v)["median_ms"] for name, v in times.items()}
                got = point_normals(None, observed, cells, radius)
                neighbours = got.neighbours.double()
                per_m[str(m)] = {
                    "times": {name: stats(v) for name, v in times.items()},
                    "wave_over_lane_moments": round(med["moments_wave"] / med["moments_lane"], 2),
                    "lane_moments_over_nearest_query": round(med["moments_lane"] / med["nearest_query"], 2),
                    "finish_share_of_the_phases": round(med["finish"] / (med["build"] + med["moments_lane"] + med["finish"]), 3),
                    "neighbours_mean": float(neighbours.mean()), "neighbours_max": int(neighbours.max()),
                    "rows_with_a_normal": int(torch.isfinite(got.variation).sum()), "rows": m * t,
                    "variation_median": float(got.variation[torch.isfinite(got.variation)].median()),
                }
                if m == args.problems[0]:
                    ms, (normal_t, count_t) = timed(lambda: torch_route(observed[0], radius))
                    both = torch.isfinite(normal_t).all(dim=1) & torch.isfinite(got.normal[0]).all(dim=1)
                    a, b = normal_t[both], got.normal[0][both].double()
                    sin = torch.linalg.vector_norm(torch.linalg.cross(a, b), dim=1).clamp(max=1.0)
                    q = torch.tensor([0.5, 0.9, 0.99, 1.0], dtype=torch.float64, device=dev)
                    same = (count_t == got.neighbours[0].long())[both]       # cdist's arithmetic moves points across the sphere
                    per_m[str(m)]["torch_route"] = {
                        "ms_one_repeat": round(ms, 2), "over_point_normals": round(ms / med["point_normals"], 1),
                        "rows_compared": int(both.sum()), "neighbour_counts_differ_on_rows": int((count_t != got.neighbours[0].long()).sum()),
                        "sin_percentiles_50_90_99_100": [float(v) for v in torch.quantile(sin, q)],
                        "rows_compared_of_equal_neighbour_count": int(same.sum()),
                        "sin_percentiles_50_90_99_100_of_equal_neighbour_count": [float(v) for v in torch.quantile(sin[same], q)]}
                    sample = np.random.default_rng(1).permutation(t)[:args.sample]
                    obs = observed[0].cpu().numpy()
                    ref, read = restatement.ring_moments(obs, obs[sample], cells.origin, cells.step[0], cells.dims, radius)
                    per_m[str(m)]["cell_list_of_a_sample"] = {
                        "rows": int(sample.shape[0]), "rings": restatement.ring_count(cells.step[0], radius),
                        "moments_agree_with_the_device": bool((ref[0] == got.moments[0].cpu().numpy()[sample]).all()),
                        "records_read_per_row_mean": float(read.mean()), "records_read_per_row_max": int(read.max()),
                        "neighbours_per_row_mean": float(ref[0, :, 0].mean())}
                print(f"radius {radius_cells} cells, M = {m}: " + json.dumps(per_m[str(m)]["times"]), file=sys.stderr, flush=True)
                del observed, workspace, out, near, got
            per_radius[str(radius_cells)] = {"radius": radius, "problems": per_m}

    result = {
        "what": "normals of an observed cloud from integer moments on the cell list (tools/bench_field_normals.py), device events, "
                "routes alternated",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": 8, "grid": list(grid.dims),
        "rows_counted": rows, "cells": list(cells.dims), "cell": cell, "radius_in_cells": per_radius,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
