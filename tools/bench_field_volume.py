#!/usr/bin/env python3
"""Time Model-level field extraction on a voxel grid against the dense route (needs an MI355X; fails without one).

    python tools/bench_field_volume.py [--resolution 128] [--repeats 20] [--out profiles/field_volume.json]

Three routes on the same commit, the same seeded model (jacobian_mlp, A = 8, default precision), the same synthetic feature map and the
same thresholds, alternated inside every repeat:
  (a) extract_field with the proposal cull,
  (b) extract_field with cull=None,
  (c) the dense route: grid.points() -> Model.compute_density (density + colour features + Jacobian head on every node) ->
      threshold / nonzero / gather in torch.
All with in_frustum=False, so that the three return the same set.  Device events around each call (the eager form's host reads
of the stage counts are inside the window: they are part of what a caller waits for); the per-image projection is warm for all
three.  Thresholds are quantiles of the dense values: `--keep` of the nodes pass the decoder threshold, `--cull-keep` the cull.
Peak extra memory = torch.cuda.max_memory_allocated over a call minus what was allocated before it."""
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
    ap.add_argument("--cull-keep", type=float, default=0.15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_volume.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_field_volume: needs a GPU (no CPU path, no fallback)")
    import __graft_entry__ as entry
    entry.build()
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import FieldGrid, extract_field
    from neural_jacobian_field_amd.model import Model

    dev = torch.device("cuda:0")
    cfg = model_cfg_from_dict({"action_dim": 8, "rendering": {"num_proposal_samples": [16], "num_nerf_samples": 12},
                               "action_decoder": {"name": "jacobian_mlp"}})
    model = Model(cfg)
    model.load_state_dict(synthetic.seeded_state_dict(synthetic.model_shapes("jacobian_mlp", 8), seed=0), strict=True)
    model.to(dev).eval().requires_grad_(False)
    cams = {k: v.to(dev) for k, v in synthetic.synthetic_cameras(1).items()}
    # the synthetic scene: seeded weights and an N(0, 1) feature map standing in for the encoder output
    enc = PixelEncoding(features=synthetic.synthetic_features(1, 128, 128, seed=1).to(dev), extrinsics=cams["ctxt_c2w"],
                        intrinsics=cams["ctxt_k_norm"], action=synthetic.synthetic_action(1, 8).to(dev))
    grid = FieldGrid.from_bounds((-0.45, -0.45, 0.8), (0.45, 0.45, 2.0), args.resolution)
    n = grid.num_nodes

    def dense(threshold=None):
        xyz = grid.points(device=dev)[None]
        head, extras = model.compute_density(xyz, enc)
        density = head.density.reshape(-1)
        if threshold is None:
            return density, xyz
        idx = torch.nonzero(density >= threshold).flatten()
        return idx, xyz[0][idx], density[idx], head.density_features[0][idx], extras["jacobian_head_output"][0][idx]

    with torch.no_grad():
        density, xyz = dense()
        proposal = model.proposal_networks[-1].get_density(xyz[:, :, None, :].contiguous(), enc).reshape(-1)
        thr = float(torch.quantile(density.double().cpu(), 1.0 - args.keep))
        cull = float(torch.quantile(proposal.double().cpu(), 1.0 - args.cull_keep))
        del density, xyz, proposal
    routes = {"a_cull": lambda: extract_field(model, enc, grid, thr, cull=cull, in_frustum=False),
              "b_no_cull": lambda: extract_field(model, enc, grid, thr, cull=None, in_frustum=False),
              "c_dense": lambda: dense(thr)}
    times = {k: [] for k in routes}
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
        a, b, c = routes["a_cull"](), routes["b_no_cull"](), routes["c_dense"]()
        # per-launch device times of one call of (a) and (b) (events around every entry point; not part of the timed windows)
        launches = {}
        for name in ("a_cull", "b_no_cull"):
            sink = []
            hip.set_profile_sink(sink)
            routes[name]()
            hip.set_profile_sink(None)
            torch.cuda.synchronize()
            launches[name] = [(nm, round(s.elapsed_time(e), 4)) for nm, s, e in sink]

    def stats(v):
        t = torch.tensor(v, dtype=torch.float64)
        return {"median_ms": round(float(t.median()), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4),
                "repeats": len(v)}

    result = {
        "what": "extract_field on a voxel grid vs the dense route (tools/bench_field_volume.py), device events, routes alternated",
        "device": torch.cuda.get_device_name(0), "decoder": "jacobian_mlp", "action_dim": 8, "precision": model.decoder.precision,
        "proposal_precision": model.proposal_networks[-1].precision, "grid": list(grid.dims), "nodes": n, "batch": 1,
        "density_threshold": thr, "cull": cull, "in_frustum": False,
        "times": {k: stats(v) for k, v in times.items()},
        "peak_extra_memory_MiB": {k: round(v, 2) for k, v in peak.items()},
        "survivor_fractions": {"a_cull": {nm: int(cnt.item()) / n for nm, cnt in zip(a.stage_names, a.stage_counts)},
                               "b_no_cull": {nm: int(cnt.item()) / n for nm, cnt in zip(b.stage_names, b.stage_counts)},
                               "c_dense": {"density": int(c[0].numel()) / n}},
        "same_set_b_vs_dense": bool(torch.equal(b.index.long(), c[0])),
        "launch_times_ms": launches,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
