#!/usr/bin/env python3
"""Time the rigid-twist fit of the parts of an extracted field (needs an MI355X; fails without one).

    python tools/bench_field_twists.py [--resolution 128] [--repeats 20] [--out profiles/field_twists.json]

The same seeded model (jacobian_mlp, A = 8, default precision), synthetic feature map, grid and density threshold as
tools/bench_field_volume.py / bench_field_components.py.  The cloud is extracted once and split by
``cloud_components(cloud, keys=dominant_joint(cloud.jacobian))`` at connectivity 6; the parts are the components of at least
``--min-nodes`` nodes, at most ``--max-parts`` of them, weights = the density.  Alternated inside every repeat, in one process:
  (fit_twists)     njf_field_twists on the labels and the part list: one memset and six launches, no host read,
  (cloud_twists)   the same behind the device-side part list (flags, the ordered selection) on labels already computed,
  (torch_route)    what a user writes without it: float64 ``index_add_`` of the same terms per part, ``torch.linalg.solve``, the
                   direct residual, and one host read to size the part list,
  (extract_field)  the extraction that feeds the fit, route (b) of DESIGN.md section 10: the yardstick of "a small fraction".
Device events around each call.  The per-launch split is one further pass: the memset and the six launches run one by one (the
``phase`` bits of the entry point) with events around each.  ``label_scan_bytes`` = 3 passes x K x n x 4: what the three scanning
launches read of the labels.  Nothing is asserted: the numbers are recorded, with the largest difference between the two routes."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_route(xyz, jacobian, labels, parts, parts_count, weights):
    """(omega, velocity, residual, row_residual) of the first ``parts_count`` parts with torch ops in float64."""
    k = int(parts_count.item())                                      # the host read that sizes the part list
    part = parts[:k]
    slot = torch.searchsorted(part, labels).clamp(max=k - 1)
    member = part[slot] == labels
    slot = torch.where(member, slot, torch.full_like(slot, k))       # rows of no part go to a dump slot
    f64 = dict(dtype=torch.float64, device=xyz.device)
    x, jac = xyz.double(), jacobian.double()
    w = torch.where(weights > 0, weights, torch.zeros_like(weights)).double() * member
    big_w = torch.zeros(k + 1, **f64).index_add_(0, slot, w)
    c = torch.zeros(k + 1, 3, **f64).index_add_(0, slot, w[:, None] * x) / big_w[:, None]
    r = torch.where(member[:, None], x - c[slot], torch.zeros_like(x))
    pairs = torch.stack([r[:, 0] * r[:, 0], r[:, 0] * r[:, 1], r[:, 0] * r[:, 2], r[:, 1] * r[:, 1], r[:, 1] * r[:, 2],
                         r[:, 2] * r[:, 2]], dim=1)
    q = torch.zeros(k + 1, 6, **f64).index_add_(0, slot, w[:, None] * pairs)
    a_dim = jac.shape[1]
    ra = r[:, None, :].expand(-1, a_dim, 3)
    big_p = torch.zeros(k + 1, a_dim, 3, **f64).index_add_(0, slot, w[:, None, None] * jac)
    big_l = torch.zeros(k + 1, a_dim, 3, **f64).index_add_(0, slot, w[:, None, None] * torch.linalg.cross(ra, jac, dim=-1))
    tr = q[:, 0] + q[:, 3] + q[:, 5]
    m = torch.stack([torch.stack([tr - q[:, 0], -q[:, 1], -q[:, 2]], dim=1), torch.stack([-q[:, 1], tr - q[:, 3], -q[:, 4]], dim=1),
                     torch.stack([-q[:, 2], -q[:, 4], tr - q[:, 5]], dim=1)], dim=1)
    omega = torch.zeros(k + 1, a_dim, 3, **f64)
    omega[:k] = torch.linalg.solve(m[:k], big_l[:k].transpose(1, 2)).transpose(1, 2)
    velocity = big_p / big_w[:, None, None]
    d = jac - (velocity[slot] + torch.linalg.cross(omega[slot], ra, dim=-1))
    t = torch.where(member[:, None], (d * d).sum(-1), torch.zeros((), **f64))
    residual = torch.zeros(k + 1, a_dim, **f64).index_add_(0, slot, w[:, None] * t)
    return omega[:k], velocity[:k], residual[:k], t.sum(1).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--keep", type=float, default=0.05)
    ap.add_argument("--min-nodes", type=int, default=64)
    ap.add_argument("--max-parts", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_twists.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_twists: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import (FieldGrid, cloud_components, cloud_twists, dominant_joint, extract_field,
                                                        fit_twists)
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
        kw = dict(labels=labels, sizes=sizes, min_nodes=args.min_nodes, max_parts=args.max_parts)
        first = cloud_twists(cloud, **kw)
        parts, parts_count = first.labels.clone(), torch.clamp(first.count, max=args.max_parts)
        k = int(parts_count.item())
        if k < 1:
            sys.exit(f"bench_field_twists: no component of {args.min_nodes} nodes among {n} rows")
        fit = lambda: fit_twists(cloud.xyz, cloud.jacobian, labels, parts, parts_count=parts_count, count=cloud.count,   # noqa: E731
                                 weights=cloud.density)
        routes = {"fit_twists": fit, "cloud_twists": lambda: cloud_twists(cloud, **kw),
                  "torch_route": lambda: torch_route(cloud.xyz, cloud.jacobian, labels, parts, parts_count, cloud.density),
                  "extract_field": extract}
        times = {name: [] for name in routes}
        for it in range(args.warmup + args.repeats):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
                del out
        # the memset and the six launches one by one, median of the repeats
        tw = fit()
        out = dict(labels=tw.labels, count=tw.count, nodes=tw.nodes, status=tw.status, weight=tw.weight, centroid=tw.centroid,
                   omega=tw.omega, velocity=tw.velocity, energy=tw.energy, residual=tw.residual, q=tw.Q, p=tw.P, l=tw.L,
                   row_residual=tw.row_residual)
        a_dim = cloud.jacobian.shape[1]
        workspace = torch.empty(max(hip.field_twists_workspace(n, args.max_parts, a_dim), 1), dtype=torch.float64, device=dev)
        per_phase = {p: [] for p in hip.FIELD_TWISTS_PHASES}
        for it in range(args.warmup + args.repeats):
            sink = []
            hip.set_profile_sink(sink)
            for p in hip.FIELD_TWISTS_PHASES:
                hip.field_twists(cloud.xyz, cloud.jacobian, labels, parts, out, weights=cloud.density, count=cloud.count,
                                 parts_count=parts_count, phase=p, workspace=workspace)
            hip.set_profile_sink(None)
            torch.cuda.synchronize()
            if it >= args.warmup:
                for p, (_, s, e) in zip(hip.FIELD_TWISTS_PHASES, sink):
                    per_phase[p].append(s.elapsed_time(e))
        split = {name: round(float(torch.tensor(per_phase[p], dtype=torch.float64).median()), 4)
                 for p, name in zip(hip.FIELD_TWISTS_PHASES, hip.FIELD_TWISTS_PHASE_NAMES)}
        again = fit()
        stepwise_equal = all(torch.equal(getattr(again, f), getattr(tw, f)) for f in ("omega", "velocity", "residual", "row_residual"))
        omega, velocity, residual, row = torch_route(cloud.xyz, cloud.jacobian, labels, parts, parts_count, cloud.density)
        scale = lambda t: float(t.abs().max())   # noqa: E731
        differences = {"omega": scale(omega - again.omega[:k]) / scale(omega), "velocity": scale(velocity - again.velocity[:k]) / scale(velocity),
                       "residual": scale(residual - again.residual[:k]) / scale(residual),
                       "row_residual": scale(row - again.row_residual) / scale(row)}

    def stats(v):
        t = torch.tensor(v, dtype=torch.float64)
        return {"median_ms": round(float(t.median()), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4),
                "repeats": len(v)}

    med = {name: stats(v)["median_ms"] for name, v in times.items()}
    scans = sum(split[name] for name in ("sums", "moments", "residual"))
    result = {
        "what": "rigid twists of the parts of an extracted field (tools/bench_field_twists.py), device events, routes alternated",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": a_dim, "precision": model.decoder.precision,
        "grid": list(grid.dims), "nodes": grid.num_nodes, "density_threshold": thr, "rows": n, "components": int(components.item()),
        "min_nodes": args.min_nodes, "max_parts": args.max_parts, "parts_true": int(first.count.item()), "parts_fitted": k,
        "part_nodes": again.nodes[:k].tolist(), "part_status": again.status[:k].tolist(),
        "rigidity_median_per_part": [round(float(v), 4) for v in again.rigidity()[:k].median(dim=1).values.tolist()],
        "times": {name: stats(v) for name, v in times.items()},
        "launch_split_ms": split, "scanning_launches_ms": round(scans, 4), "label_scan_bytes": 3 * args.max_parts * n * 4,
        "scan_share_of_fit": round(scans / sum(split.values()), 4),
        "torch_over_fit": round(med["torch_route"] / med["fit_twists"], 3), "fit_over_extraction": round(med["fit_twists"] / med["extract_field"], 4),
        "stepwise_equals_whole": stepwise_equal, "largest_relative_difference_to_torch": differences,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
