#!/usr/bin/env python3
"""Time the connected-component labelling of an extracted field (needs an MI355X; fails without one).

    python tools/bench_field_components.py [--resolution 128] [--repeats 20] [--out profiles/field_components.json]

The same seeded model (jacobian_mlp, A = 8, default precision), synthetic feature map, grid and density threshold as
tools/bench_field_volume.py / bench_field_mesh.py.  Alternated inside every repeat, in one process:
  (cloud_b_no_cull)   extract_field with cull=None, in_frustum=False: route (b) of DESIGN.md section 10, the yardstick,
  (cloud_filtered)    the same with min_component_nodes=K: + labelling of the survivor list, flags, one more selection,
  (label_dense_6/14)  label_components on the dense density (the four launches alone; the host read of the status word is
                      inside the window, as a caller waits for it).
Device events around each call.  The per-launch split is one further pass: the four launches of njf_field_components run one
by one (its `phase` bits) on the dense density with events around each, at both connectivities, and the entry points of the
two cloud routes with events around each.  `components_over_density` = (the four labelling launches at connectivity 6 on the
dense values) / (the density-only pass of njf_field_forward over the same N).  Nothing is asserted: the numbers are recorded."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--keep", type=float, default=0.05)
    ap.add_argument("--min-component-nodes", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_components.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_components: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import FieldGrid, extract_field, label_components
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
    n = grid.num_nodes
    k = args.min_component_nodes

    with torch.no_grad():
        head, _ = model.compute_density(grid.points(device=dev)[None], enc)
        dense = head.density.reshape(1, n).clone()
        thr = float(torch.quantile(dense.reshape(-1).double().cpu(), 1.0 - args.keep))
        del head
    routes = {"cloud_b_no_cull": lambda: extract_field(model, enc, grid, thr, cull=None, in_frustum=False),
              "cloud_filtered": lambda: extract_field(model, enc, grid, thr, cull=None, in_frustum=False, min_component_nodes=k),
              "label_dense_6": lambda: label_components(grid, dense, thr, connectivity=6),
              "label_dense_14": lambda: label_components(grid, dense, thr, connectivity=14)}
    times = {name: [] for name in routes}
    peak = {}
    with torch.no_grad():
        for it in range(args.warmup + args.repeats):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
                peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                del out
        launches = {}
        for name in ("cloud_b_no_cull", "cloud_filtered"):
            sink = []
            hip.set_profile_sink(sink)
            routes[name]()
            hip.set_profile_sink(None)
            torch.cuda.synchronize()
            launches[name] = [(nm, round(s.elapsed_time(e), 4)) for nm, s, e in sink]
        # the four labelling launches one by one, median of the repeats
        i32 = dict(dtype=torch.int32, device=dev)
        labels, sizes = torch.empty(n, **i32), torch.empty(n, **i32)
        count, status, workspace = torch.empty(1, **i32), torch.empty(1, **i32), torch.empty(2 * n, **i32)
        split = {}
        for connectivity in hip.FIELD_COMPONENTS_CONNECTIVITIES:
            per_phase = {p: [] for p in hip.FIELD_COMPONENTS_PHASES}
            for it in range(args.warmup + args.repeats):
                sink = []
                hip.set_profile_sink(sink)
                for p in hip.FIELD_COMPONENTS_PHASES:
                    hip.field_components(grid.c_grid(), 1, connectivity, labels, sizes, count, status, values=dense.reshape(-1),
                                         threshold=thr, phase=p, workspace=workspace)
                hip.set_profile_sink(None)
                torch.cuda.synchronize()
                if it >= args.warmup:
                    for p, (_, s, e) in zip(hip.FIELD_COMPONENTS_PHASES, sink):
                        per_phase[p].append(s.elapsed_time(e))
            names = dict(zip(hip.FIELD_COMPONENTS_PHASES, ("init_local_merge", "global_merge", "label_count", "sizes")))
            split[str(connectivity)] = {names[p]: round(float(torch.tensor(v, dtype=torch.float64).median()), 4)
                                        for p, v in per_phase.items()}
            split[str(connectivity)]["components"] = int(count.item())
            split[str(connectivity)]["status"] = int(status.item())
            split[str(connectivity)]["largest_component_nodes"] = int(sizes.max().item())
        filtered = routes["cloud_filtered"]()
        plain = routes["cloud_b_no_cull"]()

    def stats(v):
        t = torch.tensor(v, dtype=torch.float64)
        return {"median_ms": round(float(t.median()), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4),
                "repeats": len(v)}

    density = [ms for nm, ms in launches["cloud_b_no_cull"] if nm == "njf_field_forward"][0]   # the density-only pass over N
    labelling = sum(v for kk, v in split["6"].items() if kk in ("init_local_merge", "global_merge", "label_count", "sizes"))
    result = {
        "what": "connected components of an extracted field (tools/bench_field_components.py), device events, routes alternated",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": 8, "precision": model.decoder.precision,
        "grid": list(grid.dims), "nodes": n, "batch": 1, "density_threshold": thr, "in_frustum": False,
        "survivors": int(plain.count.item()), "min_component_nodes": k, "survivors_kept": int(filtered.count.item()),
        "times": {name: stats(v) for name, v in times.items()},
        "peak_extra_memory_MiB": {name: round(v, 2) for name, v in peak.items()},
        "launch_times_ms": launches,
        "labelling_launches_ms": split,
        "labelling_ms": round(labelling, 4), "density_pass_ms": round(density, 4),
        "components_over_density": round(labelling / density, 4) if density > 0 else None,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
