#!/usr/bin/env python3
"""Time inverse kinematics on the part tree: M commands from 3-D point targets (needs an MI355X; fails without one).

    python tools/bench_field_commands.py [--resolution 128] [--repeats 20] [--problems 1 16 64] [--out profiles/field_commands.json]

The same seeded model, feature map, grid, density threshold, 32 fitted parts, joints and tree as tools/bench_field_pose.py.  The
targets are ``cloud_pose`` at random commands (rows of no part stay and are not counted).  Per M, alternated inside every repeat,
in one process:
  (cloud_commands) the three launches behind their Python entry: allocations, no host read,
  (torch_route)    what a user writes without it: a Gauss-Newton with the same Levenberg-Marquardt rule and iteration count in
                   torch float64 over the ROWS -- the pose from ``torch.linalg.matrix_exp`` and a loop over the tree depth, its
                   derivative from ``torch.func.jacfwd``, batched over the problems with ``torch.func.vmap``.
Device events around each call.  The per-phase split is one further pass with events around each phase of the entry point
(moments: two launches; solve: one), the solver phase also on the moments of the first 4,096 rows alone -- it never reads a row,
so its time should not depend on n.  Recorded besides: the moments pass against its nominal floor of 12 M n bytes of targets
and against the targets it does read (only rows compacted into a slot's list are read), the
accepted steps, the costs, the distance of the two routes' commands from the planted ones.  Nothing is asserted: the numbers
are recorded."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _hat(w):
    zero = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([zero, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], zero, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], zero], -1)], -2)


def torch_pose(u, omega, velocity, centre, parent, depth):
    """``[K, 4, 4]`` float64: the pose of every slot under ONE command ``u [A]``, from per-slot link twists (already signed, zero
    for a slot that does not move) about ``centre``; good trees only."""
    w, v = torch.einsum("a,kac->kc", u, omega), torch.einsum("a,kac->kc", u, velocity)
    top = torch.cat([_hat(w), (v - torch.linalg.cross(w, centre, dim=-1))[..., None]], dim=-1)
    g = torch.linalg.matrix_exp(torch.cat([top, torch.zeros_like(top[:, :1])], dim=-2))
    t, q = g, parent
    for _ in range(depth):
        has = q >= 0
        qi = q.clamp(min=0)
        t = torch.where(has[:, None, None], g[qi] @ t, t)
        q = torch.where(has, parent[qi], q)
    return t


def torch_route(omega, velocity, centre, parent, depth, slot, weight, xyz, targets, iterations=20, damping=1e-3):
    """``(commands [M, A] fp32, cost [M])``: Levenberg-Marquardt over the rows in torch float64.  ``slot [n]`` (clamped), ``weight [M,
    n]`` float64 (0 = not counted), ``targets [M, n, 3]`` with every uncounted entry finite."""
    m, a_dim = targets.shape[0], omega.shape[1]
    x, y = xyz.double(), targets.double()
    total = weight.sum(dim=1)

    def residual(u, y_m):
        t = torch_pose(u, omega, velocity, centre, parent, depth)
        r = (t[slot, :3, :3] @ x[:, :, None]).squeeze(-1) + t[slot, :3, 3] - y_m
        return r, r

    both = torch.func.vmap(torch.func.jacfwd(residual, has_aux=True))

    def evaluate(u):
        jac, r = both(u, y)                                               # [M, n, 3, A], [M, n, 3]
        return (weight * (r * r).sum(-1)).sum(1) / total, jac, r

    u = torch.zeros(m, a_dim, dtype=torch.float64, device=xyz.device)
    lam = torch.full((m,), damping, dtype=torch.float64, device=xyz.device)
    cost, jac, r = evaluate(u)
    for _ in range(iterations):
        wj = weight[:, :, None, None] * jac
        g = torch.einsum("mnca,mnc->ma", wj, r) / total[:, None]
        h = torch.einsum("mnca,mncb->mab", wj, jac) / total[:, None, None]
        diag = torch.diagonal(h, dim1=1, dim2=2)
        h = h + torch.diag_embed(lam[:, None] * diag.clamp(min=1e-12))
        step = torch.linalg.solve_ex(h, g).result
        cand = (u - step).float().double()
        c2, j2, r2 = evaluate(cand)
        better = c2 < cost
        u, cost = torch.where(better[:, None], cand, u), torch.where(better, c2, cost)
        jac, r = torch.where(better[:, None, None, None], j2, jac), torch.where(better[:, None, None], r2, r)
        lam = torch.where(better, lam / 3.0, lam * 4.0).clamp(1e-9, 1e9)
    return u.float(), cost


def link_twists(tw, joints, parent, joint_of):
    """The signed twist and centre of every slot's link, zero for an unused or empty slot (host read of the part count)."""
    k = int(tw.count.clamp(max=tw.labels.shape[0]).item())
    hung = parent >= 0
    j = joint_of.clamp(min=0).long()
    sign = torch.where(joints.part_a[j] == parent, 1.0, -1.0).double()
    live = ((torch.arange(parent.shape[0], device=parent.device) < k) & ((tw.status & 1) == 0))[:, None, None]
    omega = torch.where(hung[:, None, None], sign[:, None, None] * joints.omega[j], tw.omega) * live
    velocity = torch.where(hung[:, None, None], sign[:, None, None] * joints.velocity[j], tw.velocity) * live
    return omega, velocity, torch.where(hung[:, None], joints.anchor[j], tw.centroid), k


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_commands.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_commands: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import (FieldGrid, cloud_commands, cloud_components, cloud_joints, cloud_pose,
                                                        cloud_twists, dominant_joint, extract_field)
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
        omega, velocity, centre, k = link_twists(tw, joints, tree[0], tree[1])
        if k < 2:
            sys.exit(f"bench_field_commands: fewer than two components of {args.min_nodes} nodes among {n} rows")
        parent_host = tree[0].cpu().numpy()
        tree_depth = 0
        for p in range(len(parent_host)):
            q, d = parent_host[p], 0
            while q >= 0:
                q, d = parent_host[q], d + 1
            tree_depth = max(tree_depth, d)
        rows = int(cloud.count.item())
        speed = float(torch.linalg.vector_norm(tw.omega, dim=-1).max())
        links = dict(part_a=joints.part_a, part_b=joints.part_b, count=joints.count, anchor=joints.anchor, omega=joints.omega,
                     velocity=joints.velocity, parent=tree[0], joint_of=tree[1])
        kk = tw.labels.shape[0]
        part = tw.labels[:k]
        slot = torch.searchsorted(part, labels).clamp(max=k - 1)
        rigid = (part[slot] == labels) & (labels >= 0) & (torch.arange(n, device=dev) < rows)
        per_m = {}
        for m in args.problems:
            planted = torch.from_numpy((0.5 * np.random.default_rng(m).uniform(-1.0, 1.0, size=(m, 8)) / max(speed, 1e-6))
                                       .astype(np.float32)).to(dev)
            pose, targets = cloud_pose(cloud, labels, tw, planted, joints=joints, tree=tree, first_order_elsewhere=False)
            targets[:, rows:] = 0.0                                                   # (rows past the count are not written)
            weight = (rigid & (pose.status[slot] == 0))[None].expand(m, n).double()
            fit = cloud_commands(cloud, labels, tw, targets, joints=joints, tree=tree, iterations=args.iterations)
            out = {f: getattr(fit, f) for f in fit.__dataclass_fields__}
            workspace = torch.empty(hip.field_commands_workspace(m, kk, 8, n), dtype=torch.float64, device=dev)
            short = torch.tensor([min(rows, 4096)], dtype=torch.int32, device=dev)

            def entry_point(phase, count=cloud.count):
                points = dict(xyz=cloud.xyz, labels=labels, count=count, targets=targets)
                hip.field_commands(tw.labels, tw.status, tw.centroid, tw.omega, tw.velocity, points, out, parts_count=tw.count,
                                   joints=links, iterations=args.iterations, phase=phase, workspace=workspace)

            routes = {"cloud_commands": lambda: cloud_commands(cloud, labels, tw, targets, joints=joints, tree=tree,
                                                               iterations=args.iterations),
                      "torch_route": lambda: torch_route(omega, velocity, centre, tree[0].long(), tree_depth, slot, weight, cloud.xyz,
                                                         targets, args.iterations)}
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
            names = ("moments", "solve", "moments_4096_rows", "solve_on_4096_rows")
            per_phase = {name: [] for name in names}
            for it in range(args.warmup + args.repeats):
                sink = []
                hip.set_profile_sink(sink)
                entry_point(hip.FIELD_COMMANDS_MOMENTS)
                entry_point(hip.FIELD_COMMANDS_SOLVE)
                entry_point(hip.FIELD_COMMANDS_MOMENTS, short)
                entry_point(hip.FIELD_COMMANDS_SOLVE, short)
                hip.set_profile_sink(None)
                torch.cuda.synchronize()
                if it >= args.warmup:
                    for name, (_, s, e) in zip(names, sink):
                        per_phase[name].append(s.elapsed_time(e))
            entry_point(hip.FIELD_COMMANDS_ALL)                                       # leave the full problem's outputs in `out`
            tu, tc = torch_route(omega, velocity, centre, tree[0].long(), tree_depth, slot, weight, cloud.xyz, targets, args.iterations)
            med = {name: stats(v)["median_ms"] for name, v in times.items()}
            floor_bytes = 12 * m * rows                                               # the nominal floor: every row's target
            read_bytes = 12 * m * int(rigid.sum().item())                             # what the pass reads: the rows of a slot
            per_m[str(m)] = {
                "times": {name: stats(v) for name, v in times.items()},
                "phase_split": {name: stats(v) for name, v in per_phase.items()},
                "moments_nominal_floor_bytes": floor_bytes,
                "moments_nominal_GBps": round(floor_bytes / (stats(per_phase["moments"])["median_ms"] * 1e-3) / 1e9, 1),
                "moments_target_bytes_read": read_bytes,
                "moments_read_GBps": round(read_bytes / (stats(per_phase["moments"])["median_ms"] * 1e-3) / 1e9, 1),
                "torch_over_cloud_commands": round(med["torch_route"] / med["cloud_commands"], 2),
                "accepted_steps": fit.steps.tolist(), "status": fit.status.tolist(),
                "cost_max": float(fit.cost.max()), "initial_cost_min": float(fit.initial_cost.min()),
                "torch_cost_max": float(tc.max()),
                "largest_distance_to_the_planted_commands": {"cloud_commands": float((fit.commands - planted).abs().max()),
                                                             "torch_route": float((tu - planted).abs().max())},
            }
            print(f"M = {m}: " + json.dumps(per_m[str(m)]["times"]), file=sys.stderr, flush=True)
            del pose, targets, weight, fit, out, workspace, tu, tc

    result = {
        "what": "commands from 3-D point targets on the part tree (tools/bench_field_commands.py), device events, routes alternated",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": 8, "grid": list(grid.dims),
        "rows": n, "rows_counted": rows, "components": int(components.item()), "parts_true": int(tw.count.item()), "parts_fitted": k,
        "joints": int(joints.count.item()), "tree_depth": tree_depth, "rows_of_a_fitted_part": int(rigid.sum().item()),
        "iterations": args.iterations, "problems": per_m,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
