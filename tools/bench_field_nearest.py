#!/usr/bin/env python3
"""Time the closest-point query on a cell list and the registration it makes possible (needs an MI355X; fails without one).

    python tools/bench_field_nearest.py [--resolution 128] [--repeats 20] [--problems 1 16 64] [--out profiles/field_nearest.json]

The same seeded model, feature map, grid, density threshold, 32 fitted parts, joints and tree as tools/bench_field_commands.py.
The observed cloud of a problem is ``cloud_pose`` at a planted command of at most 0.3 rad per channel, its rows in shuffled
order; the cells are ``cell_grid`` over the grid's bounds with the grid's step.  Per M, alternated inside every repeat, in one
process:
  (nearest_points)     the query of the un-posed rows behind its Python entry: allocations, the build and the query,
  (nearest_wave)       the same through the C entry with a wave per query instead of a lane,
  (nearest_all_rows)   the same without ``labels``: every row is searched, not only the rows of a component,
  (register_commands)  8 rounds x 3 iterations,
  (torch_route)        what a user writes without it: ``torch.cdist`` + ``argmin`` in fp32 over chunks of the labelled rows sized
                       to fit memory, a gather, ``solve_commands`` -- ONE round of the loop (fewer repeats: it is slow).
Device events around each call.  The split is one further pass with events around the build and the query phases of the entry
point, and around the three pieces of one registration round.  Recorded besides: the ring at which the queries of problem 0
stopped and the records they read (the numpy restatement of the search, on a sample of the labelled rows), and the rows on
which the two routes disagree on ``index`` (ties, and cdist's different arithmetic).  Nothing is asserted: the numbers are
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


def cdist_route(queries, rows, observed, reach, chunk_elements=2 ** 28):
    """``(index [M, n] int64 with -1, matched [M, n, 3] with NaN)``: cdist + argmin over chunks of the rows ``rows`` of
    ``queries [n, 3]`` against ``observed [M, T, 3]``."""
    m, t = observed.shape[:2]
    n = queries.shape[0]
    index = torch.full((m, n), -1, dtype=torch.int64, device=queries.device)
    matched = torch.full((m, n, 3), float("nan"), device=queries.device)
    chunk = max(1, chunk_elements // t)
    for i in range(m):
        for lo in range(0, rows.shape[0], chunk):
            part = rows[lo:lo + chunk]
            d, j = torch.cdist(queries[part], observed[i]).min(dim=1)
            ok = d <= reach
            index[i, part[ok]] = j[ok]
            matched[i, part[ok]] = observed[i, j[ok]]
    return index, matched


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--torch-repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keep", type=float, default=0.05)
    ap.add_argument("--min-nodes", type=int, default=64)
    ap.add_argument("--max-parts", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--reach-cells", type=float, default=3.0)
    ap.add_argument("--sample", type=int, default=1500)
    ap.add_argument("--problems", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_nearest.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_nearest: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    import field_nearest_restatement as restatement
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import (FieldGrid, cell_grid, cloud_components, cloud_joints, cloud_pose, cloud_twists,
                                                        dominant_joint, extract_field, nearest_points, part_poses, register_commands,
                                                        solve_commands)
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
        n = cloud.index.shape[0]
        labels, sizes, components = cloud_components(cloud, connectivity=6, keys=dominant_joint(cloud.jacobian), batch=1)
        tw = cloud_twists(cloud, labels=labels, sizes=sizes, min_nodes=args.min_nodes, max_parts=args.max_parts)
        joints = cloud_joints(cloud, labels, tw, batch=1)
        tree = joints.tree()
        rows = int(cloud.count.item())
        speed = float(torch.linalg.vector_norm(tw.omega, dim=-1).max())
        upper = tuple(o + s * (d - 1) for o, s, d in zip(grid.origin, grid.step, grid.dims))
        cell = max(grid.step)
        cells = cell_grid(grid.origin, upper, cell)
        reach = args.reach_cells * cell
        labelled = torch.nonzero((labels >= 0) & (torch.arange(n, device=dev) < rows)).reshape(-1)
        xyz = cloud.xyz
        q3 = xyz[None].contiguous()
        per_m = {}
        for m in args.problems:
            planted = torch.from_numpy((0.3 * np.random.default_rng(m).uniform(-1.0, 1.0, size=(m, 8)) / max(speed, 1e-6))
                                       .astype(np.float32)).to(dev)
            _, posed = cloud_pose(cloud, labels, tw, planted, joints=joints, tree=tree, first_order_elsewhere=False)
            order = torch.from_numpy(np.random.default_rng(100 + m).permutation(rows)).to(dev)
            observed = posed[:, order].contiguous()                                   # [M, rows, 3]
            del posed
            t = observed.shape[1]
            workspace = torch.empty(hip.field_nearest_workspace(m, cells.num_nodes, t), dtype=torch.int32, device=dev)
            out = dict(index=torch.empty(m, n, dtype=torch.int32, device=dev), distance2=torch.empty(m, n, device=dev),
                       matched=torch.empty(m, n, 3, device=dev), found=torch.empty(m, dtype=torch.int32, device=dev))

            def entry_point(phase, with_labels=True):
                hip.field_nearest(observed if phase & hip.FIELD_NEAREST_BUILD else (m, t), q3 if phase & hip.FIELD_NEAREST_QUERY else (1, n),
                                  cells.c_grid(), reach, out if phase & hip.FIELD_NEAREST_QUERY else None, m, count=cloud.count,
                                  labels=labels if with_labels else None, phase=phase, workspace=workspace)

            def one_round(u):
                posed_u = part_poses(tw, u, joints=joints, tree=tree).apply(xyz, labels, count=cloud.count)
                near = nearest_points(posed_u, observed, cells, reach, count=cloud.count, labels=labels)
                return solve_commands(tw, xyz, labels, near.matched, joints=joints, tree=tree, count=cloud.count, init=u,
                                      iterations=args.iterations)

            def torch_round():
                _, matched = cdist_route(xyz, labelled, observed, reach)
                return solve_commands(tw, xyz, labels, matched, joints=joints, tree=tree, count=cloud.count, iterations=args.iterations)

            routes = {"nearest_points": lambda: nearest_points(xyz, observed, cells, reach, count=cloud.count, labels=labels),
                      "nearest_wave": lambda: entry_point(hip.FIELD_NEAREST_ALL | hip.FIELD_NEAREST_WAVE),
                      "nearest_all_rows": lambda: nearest_points(xyz, observed, cells, reach, count=cloud.count),
                      "register_commands": lambda: register_commands(tw, xyz, labels, observed, cells, reach, joints=joints, tree=tree,
                                                                     count=cloud.count, rounds=args.rounds, iterations=args.iterations)}
            times = {name: [] for name in list(routes) + ["torch_route"]}
            for it in range(args.warmup + args.repeats):
                for name, fn in routes.items():
                    ms, result = timed(fn)
                    if it >= args.warmup:
                        times[name].append(ms)
                    del result
                if it < args.torch_repeats + 1:
                    ms, result = timed(torch_round)
                    if it >= 1:
                        times["torch_route"].append(ms)
                    del result
            names = ("build", "query", "query_wave", "query_all_rows")
            per_phase = {name: [] for name in names}
            pieces = {name: [] for name in ("pose", "query", "solve")}
            zero = torch.zeros(m, 8, device=dev)
            for it in range(args.warmup + args.repeats):
                sink = []
                hip.set_profile_sink(sink)
                entry_point(hip.FIELD_NEAREST_BUILD)
                entry_point(hip.FIELD_NEAREST_QUERY)
                entry_point(hip.FIELD_NEAREST_QUERY | hip.FIELD_NEAREST_WAVE)
                entry_point(hip.FIELD_NEAREST_QUERY, with_labels=False)
                hip.set_profile_sink(None)
                torch.cuda.synchronize()
                a, posed_u = timed(lambda: part_poses(tw, zero, joints=joints, tree=tree).apply(xyz, labels, count=cloud.count))
                p3 = posed_u.contiguous()
                b, _ = timed(lambda: hip.field_nearest((m, t), p3, cells.c_grid(), reach, out, m, count=cloud.count, labels=labels,
                                                       phase=hip.FIELD_NEAREST_QUERY, workspace=workspace))
                c, _ = timed(lambda: solve_commands(tw, xyz, labels, out["matched"], joints=joints, tree=tree, count=cloud.count, init=zero,
                                                    iterations=args.iterations))
                if it >= args.warmup:
                    for name, (_, s, e) in zip(names, sink):
                        per_phase[name].append(s.elapsed_time(e))
                    for name, v in zip(pieces, (a, b, c)):
                        pieces[name].append(v)
            near = nearest_points(xyz, observed, cells, reach, count=cloud.count, labels=labels)
            index_t, _ = cdist_route(xyz, labelled, observed, reach)
            reg = register_commands(tw, xyz, labels, observed, cells, reach, joints=joints, tree=tree, count=cloud.count,
                                    rounds=args.rounds, iterations=args.iterations)
            med = {name: stats(v)["median_ms"] for name, v in times.items()}
            per_m[str(m)] = {
                "times": {name: stats(v) for name, v in times.items()},
                "phase_split": {name: stats(v) for name, v in per_phase.items()},
                "one_registration_round": {name: stats(v) for name, v in pieces.items()},
                "torch_round_over_one_round": round(med["torch_route"] / sum(stats(v)["median_ms"] for v in pieces.values()), 1),
                "wave_over_lane_query": round(stats(per_phase["query_wave"])["median_ms"] / stats(per_phase["query"])["median_ms"], 2),
                "all_rows_over_labelled_query": round(stats(per_phase["query_all_rows"])["median_ms"] / stats(per_phase["query"])["median_ms"], 2),
                "found": near.found.tolist()[:4], "rows_disagreeing_on_index": int((near.index.long() != index_t).sum().item()),
                "registration": {"found_last": reg.found_history[-1].tolist()[:4], "cost_first_round_max": float(reg.cost_history[0].max()),
                                 "cost_last_round_max": float(reg.cost_history[-1].max()),
                                 "largest_distance_to_the_planted_commands": float((reg.fit.commands - planted).abs().max())},
            }
            if m == args.problems[0]:
                sample = labelled[torch.from_numpy(np.random.default_rng(1).permutation(labelled.shape[0])[:args.sample]).to(dev)]
                ref = restatement.rings(observed[0].cpu().numpy(), xyz[sample].cpu().numpy(), cells.origin, cells.step[0], cells.dims, reach)
                agree = bool((ref["index"][0] == near.index[0, sample].cpu().numpy()).all())
                per_m[str(m)]["ring_search_of_a_sample"] = {
                    "queries": int(sample.shape[0]), "agrees_with_the_device": agree,
                    "stopped_after_ring": {str(k): int(v) for k, v in enumerate(np.bincount(ref["rings"][0])) if v},
                    "records_read_per_query_mean": float(ref["records"].mean()), "records_read_per_query_max": int(ref["records"].max())}
            print(f"M = {m}: " + json.dumps(per_m[str(m)]["times"]), file=sys.stderr, flush=True)
            del observed, workspace, out, near, index_t, reg

    result = {
        "what": "closest points on a cell list and registration to an unlabelled cloud (tools/bench_field_nearest.py), device events, "
                "routes alternated",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": 8, "grid": list(grid.dims),
        "rows": n, "rows_counted": rows, "rows_labelled": int(labelled.shape[0]), "components": int(components.item()),
        "parts_true": int(tw.count.item()), "joints": int(joints.count.item()), "cells": list(cells.dims), "cell": cell,
        "max_distance": reach, "rounds": args.rounds, "iterations": args.iterations, "problems": per_m,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
