#!/usr/bin/env python3
"""Time the z-buffer of posed rows and the cull inside the registration (needs an MI355X; fails without one).

    python tools/bench_field_visible.py [--resolution 128] [--repeats 20] [--problems 1 4] [--out profiles/field_visible.json]

The same seeded model, feature map, grid, density threshold, fitted parts, joints and tree as tools/bench_field_nearest.py: the
rows of the extracted cloud, posed at M planted commands of at most 0.3 rad per channel, seen by V cameras -- the scene's
context camera and a second one beside it -- in 480 x 640 images.  Per M, V and footprint (0, 1, 2), alternated inside every
repeat, in one process:
  (visible_rows)        the whole entry behind its Python entry (the 4 x 4 inverses, allocations, three memsets, three launches),
  (splat)               the splat phase in its default form: a plain load of the key before the atomic,
  (splat_direct)        the splat phase with every atomic issued,
  (resolve) / (test)    the other two phases,
  (register) / (register_visible)   one round of register_commands (3 iterations) from zero against the cloud that depth_points
                        makes of the entry's own depth images, and of register_commands_visible against the same cloud,
  (torch_route)         what a user writes today: the projection, ``scatter_reduce_(..., "amin")`` per footprint pixel, a gather
                        and the comparison.
Device events around each call, 2 warm-ups; a route whose warm-up call takes more than 250 ms is repeated 3 times instead of
--repeats, which its "repeats" field records.  Recorded besides: the covered pixels, the visible rows, the rows on which the torch
route decides otherwise, and whether the two forms of the splat give equal bytes.  Nothing is asserted: the numbers are recorded."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEIGHT, WIDTH, TOLERANCE, MAX_JUMP = 480, 640, 0.01, 0.02
SLOW_MS, SLOW_REPEATS = 250.0, 3


def torch_route(points, k, w2c, height, width, footprint, tolerance):
    """``(seen [M, n] bool, depth [M, V, H*W])`` in torch ops: the float z-buffer with ``scatter_reduce_``."""
    m, n = points.shape[:2]
    views = k.shape[0]
    cam = torch.einsum("vab,mnb->mvna", w2c[:, :3, :3], points) + w2c[:, None, :3, 3]
    z = cam[..., 2]
    s, t = cam[..., 0] / z, cam[..., 1] / z
    col = torch.floor((k[:, 0, 0, None] * s + k[:, 0, 1, None] * t + k[:, 0, 2, None]) * width).long()
    row = torch.floor((k[:, 1, 0, None] * s + k[:, 1, 1, None] * t + k[:, 1, 2, None]) * height).long()
    front = torch.isfinite(z) & (z > 0)
    inf = torch.full_like(z, float("inf"))
    depth = torch.full((m * views, height * width), float("inf"), dtype=torch.float32, device=points.device)
    for dr in range(-footprint, footprint + 1):
        for dc in range(-footprint, footprint + 1):
            r, c = row + dr, col + dc
            hit = front & (c >= 0) & (c < width) & (r >= 0) & (r < height)
            key = torch.where(hit, r * width + c, torch.zeros_like(r)).reshape(m * views, n)
            depth.scatter_reduce_(1, key, torch.where(hit, z, inf).reshape(m * views, n), "amin")
    own = front & (col >= 0) & (col < width) & (row >= 0) & (row < height)
    zmin = depth.gather(1, torch.where(own, row * width + col, torch.zeros_like(row)).reshape(m * views, n)).reshape(m, views, n)
    seen = own & (z - zmin <= tolerance * zmin)
    return seen.any(dim=1), depth.reshape(m, views, -1)


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
    ap.add_argument("--footprints", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_visible.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_visible: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import (FieldGrid, FieldView, cell_grid, cloud_components, cloud_joints, cloud_pose,
                                                        cloud_twists, depth_points, dominant_joint, extract_field, register_commands,
                                                        register_commands_visible, visible_rows)
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
        cells, reach = cell_grid(grid.origin, upper, cell), 3.0 * cell
        xyz = cloud.xyz
        n = xyz.shape[0]
        second = cams["ctxt_c2w"][0].clone()
        second[:3, 3] += torch.tensor([0.25, 0.05, 0.0], device=dev)                  # the second camera: a stereo partner
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
                workspace = torch.empty(hip.field_visible_workspace(m, views, HEIGHT, WIDTH), dtype=torch.int32, device=dev)
                for footprint in args.footprints:
                    view = FieldView(k, c2w, HEIGHT, WIDTH, footprint=footprint, tolerance=TOLERANCE)
                    vis = visible_rows(posed, view, labels=labels, count=cloud.count)
                    out = {f: getattr(vis, f) for f in vis.__dataclass_fields__}
                    frames = depth_points(vis.depth.reshape(m * views, HEIGHT, WIDTH), k.repeat(m, 1, 1), c2w.repeat(m, 1, 1), kind="z",
                                          max_jump=MAX_JUMP, views_per_scene=views)

                    def phase(p):
                        hip.field_visible(posed, k, w2c, HEIGHT, WIDTH, out, m, count=cloud.count, labels=labels, footprint=footprint,
                                          tolerance=TOLERANCE, phase=p, workspace=workspace)

                    def register(visible_from=None):
                        kw = dict(joints=joints, tree=tree, count=cloud.count, rounds=1, iterations=3)
                        if visible_from is None:
                            return register_commands(tw, xyz, labels, frames.points, cells, reach, **kw)
                        return register_commands_visible(tw, xyz, labels, frames.points, cells, reach, visible_from, **kw)

                    routes = {"visible_rows": lambda: visible_rows(posed, view, labels=labels, count=cloud.count),
                              "splat": lambda: phase(hip.FIELD_VISIBLE_SPLAT),
                              "splat_direct": lambda: phase(hip.FIELD_VISIBLE_SPLAT | hip.FIELD_VISIBLE_DIRECT),
                              "resolve": lambda: phase(hip.FIELD_VISIBLE_RESOLVE),
                              "test": lambda: phase(hip.FIELD_VISIBLE_TEST),
                              "register": lambda: register(),
                              "register_visible": lambda: register(view),
                              "torch_route": lambda: torch_route(posed, k, w2c, HEIGHT, WIDTH, footprint, TOLERANCE)}
                    times = {name: [] for name in routes}
                    slow = set()
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
                    # the two forms of the splat, resolved: equal bytes
                    phase(hip.FIELD_VISIBLE_SPLAT | hip.FIELD_VISIBLE_DIRECT)
                    phase(hip.FIELD_VISIBLE_RESOLVE)
                    direct = (vis.depth.clone(), vis.index.clone())
                    phase(hip.FIELD_VISIBLE_SPLAT)
                    phase(hip.FIELD_VISIBLE_RESOLVE)
                    same = bool(torch.equal(direct[0], vis.depth) and torch.equal(direct[1], vis.index))
                    seen, _ = torch_route(posed, k, w2c, HEIGHT, WIDTH, footprint, TOLERANCE)
                    seen &= (labels >= 0)[None] & (torch.arange(n, device=dev) < cloud.count)[None]
                    name = f"M{m}_V{views}_f{footprint}"
                    per_case[name] = {
                        "problems": m, "views": views, "footprint": footprint, "times": {r: stats(v) for r, v in times.items()},
                        "covered_pixels": vis.covered.tolist(), "visible_rows": vis.visible.tolist(),
                        "rows_the_torch_route_decides_otherwise": int((seen != (vis.seen != 0)).sum()),
                        "the_two_splat_forms_give_equal_bytes": same,
                        "splat_direct_over_splat": round(med["splat_direct"] / med["splat"], 2),
                        "phases_sum_ms": round(med["splat"] + med["resolve"] + med["test"], 4),
                        "register_visible_over_register": round(med["register_visible"] / med["register"], 2),
                        "torch_route_over_visible_rows": round(med["torch_route"] / med["visible_rows"], 2),
                    }
                    print(name + ": " + json.dumps(per_case[name]), file=sys.stderr, flush=True)
                    del vis, out, frames
                del workspace
            del posed

    result = {
        "what": "the z-buffer of posed rows and the cull inside the registration (tools/bench_field_visible.py), device events, routes "
                "alternated",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": 8, "grid": list(grid.dims),
        "rows": n, "rows_counted": rows, "frame": [HEIGHT, WIDTH], "tolerance": TOLERANCE, "max_jump": MAX_JUMP,
        "registration_cell": cell, "registration_reach": reach, "cases": per_case,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
