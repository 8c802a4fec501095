#!/usr/bin/env python3
"""Time the coarse-to-fine surface extraction against the dense one (needs an MI355X; fails without one).

    python tools/bench_field_band.py [--repeats 20] [--keep 0.05 0.005] [--out profiles/field_band.json]

Two routes on the same commit, the same seeded model (jacobian_mlp, A = 8, default precision), the same synthetic feature map and
the same density threshold, alternated inside every repeat, B = 1, in_frustum=False:
  (dense)   extract_mesh: the density pass on every node, six meshing launches, colour + Jacobian on the vertices,
  (banded)  extract_mesh(coarse=k): the density pass on every k-th node per axis, the four band launches, the density pass on the
            band list, the scatter, the leak count, and the same meshing and vertex launches,
on the grids 129^3 with k = 4 and 257^3 with k = 8, coarse_dilate = 1 and coarse_threshold = density_threshold.  Device events
around each call (the eager forms' host reads of the counts are inside the window: they are part of what a caller waits for); the
per-image projection is warm for both.  The threshold is the quantile of the density on the coarse lattice -- a sample of the
field -- that `--keep` of the nodes pass; every value of `--keep` gives one entry per grid.  Peak extra memory =
torch.cuda.max_memory_allocated over a call minus what was allocated before it.  The per-launch split is one further call with
events around every entry point."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = ((129, 4), (257, 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--keep", type=float, nargs="+", default=[0.05, 0.005])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_band.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_band: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import FieldGrid, coarse_grid, extract_mesh
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

    def stats(v):
        t = torch.tensor(v, dtype=torch.float64)
        return {"median_ms": round(float(t.median()), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4),
                "repeats": len(v)}

    def by_entry_point(launches):
        out = {}
        for name, ms in launches:
            out[name] = round(out.get(name, 0.0) + ms, 4)
        return out

    entries = []
    for resolution, k in GRIDS:
        grid = FieldGrid.from_bounds((-0.45, -0.45, 0.8), (0.45, 0.45, 2.0), resolution)
        with torch.no_grad():
            head, _ = model.compute_density(coarse_grid(grid, k).points(device=dev)[None], enc)
            sample = head.density.reshape(-1).double().cpu()
            del head
        for keep in args.keep:
            thr = float(torch.quantile(sample, 1.0 - keep))
            routes = {"dense": lambda: extract_mesh(model, enc, grid, thr, in_frustum=False),
                      "banded": lambda: extract_mesh(model, enc, grid, thr, in_frustum=False, coarse=k)}
            times = {name: [] for name in routes}
            peak, sizes, launches = {}, {}, {}
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
                for name, fn in routes.items():
                    sink = []
                    hip.set_profile_sink(sink)
                    mesh = fn()
                    hip.set_profile_sink(None)
                    torch.cuda.synchronize()
                    launches[name] = [(nm, round(s.elapsed_time(e), 4)) for nm, s, e in sink]
                    sizes[name] = {"vertices": int(mesh.vertex_count.item()), "triangles": int(mesh.triangle_count.item())}
                    if name == "banded":
                        band_nodes, leaks = int(mesh.band_count.item()), int(mesh.band_leaks.item())
                    del mesh
            t = {name: stats(v) for name, v in times.items()}
            split = {name: by_entry_point(v) for name, v in launches.items()}
            dense_density = split["dense"].get("njf_field_forward", 0.0)
            share = band_nodes / grid.num_nodes
            entries.append({
                "grid": list(grid.dims), "nodes": grid.num_nodes, "coarse": k, "coarse_dilate": 1, "keep": keep,
                "density_threshold": thr, "coarse_threshold": thr,
                "band_nodes": band_nodes, "band_share": round(share, 5), "band_leaks": leaks,
                "mesh": sizes, "times": t,
                "banded_over_dense": round(t["banded"]["median_ms"] / t["dense"]["median_ms"], 4),
                "peak_extra_memory_MiB": {name: round(v, 2) for name, v in peak.items()},
                "entry_points_ms": split,
                "launch_times_ms": launches,
                "dense_density_pass_ms": dense_density,
                "banded_density_passes_ms": split["banded"].get("njf_field_forward", 0.0),
                "expected_banded_density_ms": round((share + 1.0 / k ** 3) * dense_density, 4),
            })
            print(json.dumps({key: entries[-1][key] for key in ("grid", "coarse", "keep", "band_share", "band_leaks", "mesh", "times",
                                                                 "banded_over_dense", "entry_points_ms")}), flush=True)
    result = {
        "what": "extract_mesh(coarse=k) vs extract_mesh (tools/bench_field_band.py), device events, routes alternated",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": 8, "precision": model.decoder.precision,
        "batch": 1, "in_frustum": False, "entries": entries,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
