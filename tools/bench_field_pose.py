#!/usr/bin/env python3
"""Time posing the parts of an extracted field under M commands (needs an MI355X; fails without one).

    python tools/bench_field_pose.py [--resolution 128] [--repeats 20] [--commands 1 16 64] [--out profiles/field_pose.json]

The same seeded model (jacobian_mlp, A = 8, default precision), synthetic feature map, grid, density threshold, the same 32
fitted parts and the same joints as tools/bench_field_twists.py and tools/bench_field_joints.py; the tree is
``cloud_joints(...).tree()``.  Per M, alternated inside every repeat, in one process:
  (part_poses)    the links and chain launches behind their Python entry,
  (cloud_pose)    all three launches behind theirs: allocations, no host read,
  (points_*)      the points launch alone on transforms computed once, in its four forms: transforms read per lane from L2 or
                  staged in LDS per command, three dword stores per lane or 16-byte stores through an LDS tile,
  (torch_route)   what a user writes without it: the twist matrices and ``torch.linalg.matrix_exp`` in float64, a Python loop
                  over the tree depth for the chain, a float64 gather of the per-part matrices by slot and a batched multiply,
  (extract_field) the extraction that feeds all of it: the yardstick.
Device events around each call.  The per-launch split is one further pass with events around each launch (the ``phase`` bits of
the entry point).  Recorded besides: the write floor 12 M n bytes of the points launch and the bandwidth each form reaches
against it, the largest ratio of the transforms' difference from the numpy restatement (tests/field_pose_restatement.py) to
its bound, whether the point stage has the restatement's bytes, and the difference between the two routes.  Nothing is
asserted: the numbers are recorded."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _hat(w):
    zero = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([zero, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], zero, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], zero], -1)], -2)


def torch_route(tw, joints, parent, joint_of, depth, commands, xyz, labels, jacobian):
    """(rotation [M, K, 3, 3], translation [M, K, 3], posed [M, n, 3]) with torch ops; ``depth``: the tree's depth, host data
    of ``parents()``.  Good trees only."""
    k = int(tw.count.clamp(max=tw.labels.shape[0]).item())            # the host read that sizes the part list
    u = commands.double()
    hung = parent >= 0
    j = joint_of.clamp(min=0).long()
    sign = torch.where(joints.part_a[j] == parent, 1.0, -1.0).double()
    omega = torch.where(hung[:, None, None], sign[:, None, None] * joints.omega[j], tw.omega)
    velocity = torch.where(hung[:, None, None], sign[:, None, None] * joints.velocity[j], tw.velocity)
    centre = torch.where(hung[:, None], joints.anchor[j], tw.centroid)
    w, v = torch.einsum("ma,kac->mkc", u, omega), torch.einsum("ma,kac->mkc", u, velocity)
    live = ((torch.arange(parent.shape[0], device=parent.device) < k) & ((tw.status & 1) == 0))[None, :, None]
    w, v = torch.where(live, w, torch.zeros_like(w)), torch.where(live, v, torch.zeros_like(v))
    xi = torch.zeros(*w.shape[:2], 4, 4, dtype=torch.float64, device=w.device)
    xi[..., :3, :3] = _hat(w)
    xi[..., :3, 3] = v - torch.linalg.cross(w, centre[None].expand_as(w), dim=-1)
    g = torch.linalg.matrix_exp(xi)
    t, q = g, parent.long()
    for _ in range(depth):                                             # the chain: one batched multiply per level of the tree
        has = q >= 0
        qi = q.clamp(min=0)
        t = torch.where(has[None, :, None, None], g[:, qi] @ t, t)
        q = torch.where(has, parent.long()[qi], q)
    part = tw.labels[:k]
    slot = torch.searchsorted(part, labels).clamp(max=k - 1)
    rigid = (part[slot] == labels) & (labels >= 0) & ((tw.status[slot] & 1) == 0)
    x = xyz.double()
    moved = (t[:, slot, :3, :3] @ x[None, :, :, None]).squeeze(-1) + t[:, slot, :3, 3]      # the gather and the batched multiply
    first = x[None] + torch.einsum("ma,nac->mnc", u, jacobian.double())
    return t[..., :3, :3], t[..., :3, 3], torch.where(rigid[None, :, None], moved, first).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--keep", type=float, default=0.05)
    ap.add_argument("--min-nodes", type=int, default=64)
    ap.add_argument("--max-parts", type=int, default=32)
    ap.add_argument("--commands", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_pose.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_pose: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    import field_pose_restatement as R
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import (FieldGrid, cloud_components, cloud_joints, cloud_pose, cloud_twists,
                                                        dominant_joint, extract_field, part_poses)
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
    forms = {"l2_dword": 0, "lds_dword": hip.FIELD_POSE_STAGED, "l2_wide": hip.FIELD_POSE_WIDE,
             "lds_wide": hip.FIELD_POSE_STAGED | hip.FIELD_POSE_WIDE}
    cpu = lambda t: t.cpu().numpy()   # noqa: E731

    def stats(v):
        t = torch.tensor(v, dtype=torch.float64)
        return {"median_ms": round(float(t.median()), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4),
                "repeats": len(v)}

    with torch.no_grad():
        head, _ = model.compute_density(grid.points(device=dev)[None], enc)
        thr = float(torch.quantile(head.density.reshape(-1).double().cpu(), 1.0 - args.keep))
        del head
        extract = lambda: extract_field(model, enc, grid, thr, cull=None, in_frustum=False)   # noqa: E731
        cloud = extract()
        n = cloud.index.shape[0]
        labels, sizes, components = cloud_components(cloud, connectivity=6, keys=dominant_joint(cloud.jacobian), batch=1)
        tw = cloud_twists(cloud, labels=labels, sizes=sizes, min_nodes=args.min_nodes, max_parts=args.max_parts)
        k = int(tw.count.clamp(max=args.max_parts).item())
        if k < 2:
            sys.exit(f"bench_field_pose: fewer than two components of {args.min_nodes} nodes among {n} rows")
        joints = cloud_joints(cloud, labels, tw, batch=1)
        tree = joints.tree()
        parent_host = tree[0].cpu().numpy()
        depth_host = np.zeros(len(parent_host), dtype=np.int64)
        for p in range(len(parent_host)):
            q = parent_host[p]
            while q >= 0:
                depth_host[p] += 1
                q = parent_host[q]
        tree_depth = int(depth_host.max())
        rows = int(cloud.count.item())
        speed = float(torch.linalg.vector_norm(tw.omega, dim=-1).max())
        twd = dict(status=cpu(tw.status), count=int(tw.count.item()), centroid=cpu(tw.centroid), omega=cpu(tw.omega),
                   velocity=cpu(tw.velocity))
        jd = dict(part_a=cpu(joints.part_a), part_b=cpu(joints.part_b), count=int(joints.count.item()), anchor=cpu(joints.anchor),
                  omega=cpu(joints.omega), velocity=cpu(joints.velocity))
        per_m = {}
        for m in args.commands:
            # commands that turn the fastest twist by up to about a radian per channel
            commands = torch.from_numpy((np.random.default_rng(m).uniform(-1.0, 1.0, size=(m, 8)) / max(speed, 1e-6))
                                        .astype(np.float32)).to(dev)
            pose, posed = cloud_pose(cloud, labels, tw, commands, joints=joints, tree=tree)
            out = dict(rotation=pose.rotation, translation=pose.translation, status=pose.status, depth=pose.depth)
            points = dict(xyz=cloud.xyz, labels=labels, count=cloud.count, jacobian=cloud.jacobian, posed=torch.empty_like(posed))
            links = dict(part_a=joints.part_a, part_b=joints.part_b, count=joints.count, anchor=joints.anchor, omega=joints.omega,
                         velocity=joints.velocity, parent=tree[0], joint_of=tree[1])
            workspace = torch.empty(hip.field_pose_workspace(m, tw.labels.shape[0]), dtype=torch.float64, device=dev)

            def entry_point(phase):
                hip.field_pose(tw.labels, tw.status, tw.centroid, tw.omega, tw.velocity, commands, out, parts_count=tw.count,
                               joints=links, points=points, phase=phase, workspace=workspace)

            routes = {"part_poses": lambda: part_poses(tw, commands, joints=joints, tree=tree),
                      "cloud_pose": lambda: cloud_pose(cloud, labels, tw, commands, joints=joints, tree=tree)}
            for name, form in forms.items():
                routes["points_" + name] = lambda form=form: entry_point(hip.FIELD_POSE_POINTS | form)
            routes["torch_route"] = lambda: torch_route(tw, joints, tree[0], tree[1], tree_depth, commands, cloud.xyz, labels,
                                                        cloud.jacobian)
            routes["extract_field"] = extract
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
            # the three launches one by one
            per_phase = {name: [] for name in hip.FIELD_POSE_PHASE_NAMES}
            for it in range(args.warmup + args.repeats):
                sink = []
                hip.set_profile_sink(sink)
                for p in hip.FIELD_POSE_PHASES:
                    entry_point(p)
                hip.set_profile_sink(None)
                torch.cuda.synchronize()
                if it >= args.warmup:
                    for name, (_, s, e) in zip(hip.FIELD_POSE_PHASE_NAMES, sink):
                        per_phase[name].append(s.elapsed_time(e))
            # every form writes the bytes of the default one; the device against the restatement and against the torch route
            forms_equal = True
            for form in forms.values():
                points["posed"].zero_()
                entry_point(hip.FIELD_POSE_POINTS | form)
                forms_equal = forms_equal and torch.equal(points["posed"][:, :rows], posed[:, :rows])
            ref = R.poses(twd, cpu(commands), jd, (cpu(tree[0]), cpu(tree[1])))
            ratio = R.worst_ratio(cpu(pose.rotation), cpu(pose.translation), ref, R.scale_of(twd, cpu(commands), jd))
            want = R.points(cpu(pose.rotation), cpu(pose.translation), cpu(pose.status), cpu(pose.labels), int(pose.count.item()),
                            cpu(commands), cpu(cloud.xyz), cpu(labels), rows, cpu(cloud.jacobian))
            same_bytes = cpu(posed)[:, :rows].tobytes() == want[:, :rows].tobytes()
            tr, tt, tp = torch_route(tw, joints, tree[0], tree[1], tree_depth, commands, cloud.xyz, labels, cloud.jacobian)
            med = {name: stats(v)["median_ms"] for name, v in times.items()}
            floor_bytes = 12 * m * rows
            per_m[str(m)] = {
                "times": {name: stats(v) for name, v in times.items()},
                "launch_split": {name: stats(v) for name, v in per_phase.items()},
                "points_write_floor_bytes": floor_bytes,
                "points_write_GBps": {name: round(floor_bytes / (med["points_" + name] * 1e-3) / 1e9, 1) for name in forms},
                "torch_over_cloud_pose": round(med["torch_route"] / med["cloud_pose"], 3),
                "cloud_pose_over_extraction": round(med["cloud_pose"] / med["extract_field"], 4),
                "every_form_writes_the_same_bytes": forms_equal,
                "status_and_depth_equal_the_restatement": bool(np.array_equal(cpu(pose.status), ref["status"])
                                                               and np.array_equal(cpu(pose.depth), ref["depth"])),
                "largest_ratio_to_the_transform_bound": round(ratio, 5),
                "points_have_the_restatement_bytes": same_bytes,
                "largest_difference_to_torch": {"rotation": float((tr - pose.rotation).abs().max()),
                                                "translation": float((tt - pose.translation).abs().max()),
                                                "posed": float((tp[:, :rows] - posed[:, :rows]).abs().max())},
            }
            del pose, posed, points, workspace, tp

    result = {
        "what": "posing the parts of an extracted field under M commands (tools/bench_field_pose.py), device events, routes alternated",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": 8, "precision": model.decoder.precision,
        "grid": list(grid.dims), "nodes": grid.num_nodes, "density_threshold": thr, "rows": n, "rows_counted": rows,
        "components": int(components.item()), "min_nodes": args.min_nodes, "max_parts": args.max_parts,
        "parts_true": int(tw.count.item()), "parts_fitted": k, "joints": int(joints.count.item()), "tree_depth": tree_depth,
        "slots_with_a_parent": int((tree[0] >= 0).sum().item()),
        "rows_of_a_fitted_part": int(((labels[:, None] == tw.labels[None, :k]).any(1)).sum().item()),
        "commands": per_m,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
