#!/usr/bin/env python3
"""Time the joints between the parts of an extracted field (needs an MI355X; fails without one).

    python tools/bench_field_joints.py [--resolution 128] [--repeats 20] [--out profiles/field_joints.json]

The same seeded model (jacobian_mlp, A = 8, default precision), synthetic feature map, grid, density threshold and the same 32
fitted parts as tools/bench_field_twists.py: the cloud is extracted once, split by ``cloud_components(cloud,
keys=dominant_joint(cloud.jacobian))`` at connectivity 6, and ``cloud_twists`` fits the first ``--max-parts`` components of at
least ``--min-nodes`` nodes.  Alternated inside every repeat, in one process:
  (cloud_joints)   njf_field_joints behind its Python entry: two memsets and four launches, no host read,
  (joints_combined / joints_per_lane)  the C entry on a workspace allocated once, with the contacts launch in its two forms,
  (torch_route)    what a user writes without it: a dense label volume, shifted compares, ``torch.unique`` on the pair keys (a
                   host read), ``index_add_``, the twist algebra in float64,
  (fit_twists)     the fit that feeds the joints, and (extract_field) the extraction that feeds both: the yardsticks.
Device events around each call.  The per-launch split is one further pass: the memsets and the four launches run one by one
(the ``phase`` bits of the entry point) with events around each, the contacts launch in both forms.  Nothing is asserted: the
numbers are recorded, with the differences between the two routes."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))


def torch_route(grid, batch, index, labels, tw, connectivity, min_contacts):
    """(part_a, part_b, contacts, anchor, omega, velocity) of every joint with torch ops."""
    k = int(tw.count.clamp(max=tw.labels.shape[0]).item())            # the host read that sizes the part list
    part = tw.labels[:k]
    slot = torch.searchsorted(part, labels).clamp(max=k - 1)
    slot = torch.where(part[slot] == labels, slot, torch.full_like(slot, -1))
    nx, ny, nz = grid.dims
    volume = torch.full((batch * grid.num_nodes,), -1, dtype=torch.int64, device=index.device)
    volume[index.long()] = slot
    volume = volume.reshape(batch, nx, ny, nz)
    keys, sums = [], []
    for dx, dy, dz in DIRECTIONS[:connectivity // 2]:
        a, b = volume[:, :nx - dx, :ny - dy, :nz - dz], volume[:, dx:, dy:, dz:]
        hit = (a >= 0) & (b >= 0) & (a != b)
        at = hit.nonzero()                                             # (a host read per direction: the size of the result)
        p, q = a[hit], b[hit]
        keys.append(torch.minimum(p, q) * k + torch.maximum(p, q))
        sums.append(2 * at[:, 1:] + torch.tensor([dx, dy, dz], device=index.device))
    keys, sums = torch.cat(keys), torch.cat(sums)
    pairs, inverse = torch.unique(keys, return_inverse=True)
    contacts = torch.zeros(pairs.shape[0], dtype=torch.int64, device=index.device).index_add_(0, inverse, torch.ones_like(keys))
    sum2 = torch.zeros(pairs.shape[0], 3, dtype=torch.int64, device=index.device).index_add_(0, inverse, sums)
    keep = contacts >= min_contacts
    pairs, contacts, sum2 = pairs[keep], contacts[keep], sum2[keep]
    lo, hi = pairs // k, pairs % k
    f64 = dict(dtype=torch.float64, device=index.device)
    anchor = torch.tensor(grid.origin, **f64) + torch.tensor(grid.step, **f64) * (sum2.double() / (2.0 * contacts.double())[:, None])
    u = []
    for s in (lo, hi):
        r = (anchor - tw.centroid[s])[:, None, :].expand(-1, tw.omega.shape[1], 3)
        u.append(tw.velocity[s] + torch.linalg.cross(tw.omega[s], r, dim=-1))
    return lo, hi, contacts, anchor, tw.omega[hi] - tw.omega[lo], u[1] - u[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--keep", type=float, default=0.05)
    ap.add_argument("--min-nodes", type=int, default=64)
    ap.add_argument("--max-parts", type=int, default=32)
    ap.add_argument("--connectivity", type=int, default=6)
    ap.add_argument("--max-joints", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_joints.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_joints: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import (FieldGrid, cloud_components, cloud_joints, cloud_twists, dominant_joint,
                                                        extract_field, fit_twists)
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

    with torch.no_grad():
        head, _ = model.compute_density(grid.points(device=dev)[None], enc)
        thr = float(torch.quantile(head.density.reshape(-1).double().cpu(), 1.0 - args.keep))
        del head
        extract = lambda: extract_field(model, enc, grid, thr, cull=None, in_frustum=False)   # noqa: E731
        cloud = extract()
        n = cloud.index.shape[0]
        keys = dominant_joint(cloud.jacobian)
        labels, sizes, components = cloud_components(cloud, connectivity=6, keys=keys, batch=1)
        tw = cloud_twists(cloud, labels=labels, sizes=sizes, min_nodes=args.min_nodes, max_parts=args.max_parts)
        k = int(tw.count.clamp(max=args.max_parts).item())
        if k < 2:
            sys.exit(f"bench_field_joints: fewer than two components of {args.min_nodes} nodes among {n} rows")
        a_dim = cloud.jacobian.shape[1]
        options = dict(connectivity=args.connectivity, min_contacts=1)
        joints = cloud_joints(cloud, labels, tw, batch=1, max_joints=args.max_joints, **options)
        out = dict(part_a=joints.part_a, part_b=joints.part_b, contacts=joints.contacts, status=joints.status, count=joints.count,
                   anchor=joints.anchor, omega=joints.omega, velocity=joints.velocity)
        workspace = torch.empty(hip.field_joints_workspace(grid.num_nodes, args.max_parts), dtype=torch.int64, device=dev)
        cg = grid.c_grid()

        def entry_point(phase):
            hip.field_joints(cg, 1, cloud.index, labels, tw.labels, tw.status, tw.centroid, tw.omega, tw.velocity, out,
                             count=cloud.count, parts_count=tw.count, phase=phase, workspace=workspace, **options)

        parts, parts_count = tw.labels.clone(), torch.clamp(tw.count, max=args.max_parts)
        routes = {"cloud_joints": lambda: cloud_joints(cloud, labels, tw, batch=1, max_joints=args.max_joints, **options),
                  "joints_combined": lambda: entry_point(hip.FIELD_JOINTS_ALL),
                  "joints_per_lane": lambda: entry_point(hip.FIELD_JOINTS_ALL | hip.FIELD_JOINTS_PER_LANE),
                  "torch_route": lambda: torch_route(grid, 1, cloud.index, labels, tw, args.connectivity, 1),
                  "fit_twists": lambda: fit_twists(cloud.xyz, cloud.jacobian, labels, parts, parts_count=parts_count,
                                                   count=cloud.count, weights=cloud.density),
                  "extract_field": extract}
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
        # the memsets and the four launches one by one, the contacts launch in both forms
        steps = [(name, p) for name, p in zip(hip.FIELD_JOINTS_PHASE_NAMES, hip.FIELD_JOINTS_PHASES)]
        steps.insert(3, ("contacts_per_lane", hip.FIELD_JOINTS_PHASES[2] | hip.FIELD_JOINTS_PER_LANE))
        order = [steps[i] for i in (0, 1, 3, 0, 1, 2, 4, 5)]            # the per-lane form on a fresh table, then the whole sequence
        per_phase = {name: [] for name, _ in steps}
        for it in range(args.warmup + args.repeats):
            sink = []
            hip.set_profile_sink(sink)
            for _, p in order:
                entry_point(p)
            hip.set_profile_sink(None)
            torch.cuda.synchronize()
            if it >= args.warmup:
                for (name, _), (_, s, e) in list(zip(order, sink))[2:]:
                    per_phase[name].append(s.elapsed_time(e))
        stepwise = {f: out[f].clone() for f in out}
        whole = cloud_joints(cloud, labels, tw, batch=1, max_joints=args.max_joints, **options)
        stepwise_equal = all(torch.equal(stepwise[f], getattr(whole, f)) for f in out)
        lo, hi, contacts, anchor, omega, velocity = torch_route(grid, 1, cloud.index, labels, tw, args.connectivity, 1)
        count = int(whole.count.item())
        stored = min(count, args.max_joints)
        scale = lambda t: float(t.abs().max()) if t.numel() else 0.0   # noqa: E731
        relative = lambda d, t: scale(d) / scale(t) if scale(t) > 0 else scale(d)   # noqa: E731
        same_list = (lo.shape[0] == count and torch.equal(lo[:stored].int(), whole.part_a[:stored])
                     and torch.equal(hi[:stored].int(), whole.part_b[:stored]) and torch.equal(contacts[:stored], whole.contacts[:stored]))
        differences = {"anchor": relative(anchor[:stored] - whole.anchor[:stored], anchor),
                       "omega": relative(omega[:stored] - whole.omega[:stored], omega),
                       "velocity": relative(velocity[:stored] - whole.velocity[:stored], velocity)} if same_list else None

    def stats(v):
        t = torch.tensor(v, dtype=torch.float64)
        return {"median_ms": round(float(t.median()), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4),
                "repeats": len(v)}

    med = {name: stats(v)["median_ms"] for name, v in times.items()}
    result = {
        "what": "joints between the parts of an extracted field (tools/bench_field_joints.py), device events, routes alternated",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": a_dim, "precision": model.decoder.precision,
        "grid": list(grid.dims), "nodes": grid.num_nodes, "density_threshold": thr, "rows": n, "components": int(components.item()),
        "min_nodes": args.min_nodes, "max_parts": args.max_parts, "parts_true": int(tw.count.item()), "parts_fitted": k,
        "connectivity": args.connectivity, "max_joints": args.max_joints, "joints": count,
        "contacts_per_joint": whole.contacts[:stored].tolist(), "contacts_total": int(whole.contacts[:stored].sum().item()),
        "drive": whole.drive()[:stored].tolist(), "workspace_bytes": 8 * workspace.numel(),
        "times": {name: stats(v) for name, v in times.items()},
        "launch_split": {name: stats(v) for name, v in per_phase.items()},
        "torch_over_joints": round(med["torch_route"] / med["cloud_joints"], 3),
        "joints_over_fit_twists": round(med["cloud_joints"] / med["fit_twists"], 4),
        "joints_over_extraction": round(med["cloud_joints"] / med["extract_field"], 4),
        "stepwise_equals_whole": stepwise_equal, "torch_route_lists_the_same_joints": same_list,
        "largest_relative_difference_to_torch": differences,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
