#!/usr/bin/env python3
"""Headline benchmark: rendered rays/s of the fused hot path (BASELINE.json metric).

A *step* is one eval-mode ``Model.forward`` (reference ``models/model.py:316-396``) over one synthetic 256x256 frame,
config C2 of SURVEY.md 8(d): B=1, 65,536 rays, 64 proposal + 64 final samples per ray, ``jacobian_mlp`` decoder, A=8,
fp32 operands.  The image encoder is excluded as SURVEY 8(d) prescribes (it is per image, not per ray): the model is
built with the ``"precomputed"`` encoder entry, whose forward returns the synthetic 512-channel feature map, so the
timed call IS ``Model.forward`` -- per step and per rank

    per-image lin_z projection of the feature map (ONE launch for all networks; the cache is reset every step)
    -> njf_proposal_forward -> njf_render_forward (frame reductions in its epilogue) -> njf_reduce_frame_partials
    -> [N > 1: ONE all_gather of (pixels | 4 scalars)] -> njf_assemble_frame (global depth clip, rgb + flow loss)

Inputs are resident in HBM when the clock starts.

**Which arithmetic is the headline (VERDICT r03 "next" #2).**  ``value`` / ``dtype`` / ``roofline`` are the run with EXACT fp32
products (``v_mfma_f32_32x32x2_f32``, the reference's arithmetic; roofline against the 157.3 TFLOP/s fp32-MFMA peak).  The
package's default precision (``f16f6``: error-compensated fp16 split with fp6 correction terms) is measured with ``--full`` in
the same process with the same --steps / --warmup, the same barriers and the same max-over-ranks, and reported as
``value_default_precision`` with its own roofline block against the 2.5 PFLOP/s f16 peak -- it is an accelerated mode inside
the parity bounds, not fp32 arithmetic, so it is not in the headline slot.  ``--precision`` moves another mode there.

**Plain run and ``--full``.**  A plain run sets up, warms up, times exactly --steps steps of the headline precision, writes the
outputs of the last timed step when ``--dump-outputs DIR`` is given, and prints the line (``metric``, ``value``, ``unit``,
``ms_per_step``, ``higher_is_better``, ``dtype``, configuration, rank evidence).  ``--full`` adds everything else, as before:
per-launch HIP-event kernel timings in the timed loop and the roofline blocks, the frame digest of one more untimed step, every
other precision, the CPU baseline and the parity check of the timed frame against the CPU oracle.

**Launch (VERDICT r03 "next" #1).**  ``python bench.py --gpus N`` started as a plain process spawns its N ranks itself
(``neural_jacobian_field_amd.launch``: ``python -m torch.distributed.run``, one rank per GPU, rendezvous on 127.0.0.1);
started under a launcher (the driver's ``torch.distributed.run`` line) it checks that WORLD_SIZE == N.  In both cases the
line is refused -- no JSON, non-zero exit -- when its ``n_gpus`` would differ from ``--gpus`` or two ranks share a device, and
it carries ``rccl``: backend, world size, per-rank device identity (PCI bus id / uuid, all-gathered through the process
group) and per-rank step times.

N > 1 -- ``--scaling strong`` (default), SURVEY.md 8(e) literally: the R rays of ONE frame are split into N contiguous
shards (``parallel.shard_bounds``), weights and feature map are replicated, each rank renders its shard through the same
``Model.forward``, ONE collective per step.  value = rays of the frame / max-over-ranks time.  ``--scaling weak``: every
rank renders its own full frame.

Usage:  python bench.py [--gpus N] [--steps K] [--warmup W] [--scaling strong|weak] [--full] [--dump-outputs DIR]
Prints ONE JSON line on rank 0.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

H = W = 256
S_PROP, S_FINAL, ACTION_DIM = 64, 64, 8
PROFILE_ROUNDS = ("r06", "r05", "r04", "r03")   # newest first: where roofline.traffic (PMC passes, never taken in the timed run) is looked up
HEADLINE_PRECISION = "f32"        # the reference's arithmetic; see the module docstring

# Algorithmic work (hoisted-lin_z formulation), MACs per point
MAC_PROPOSAL = 172_032
MAC_DENSITY, MAC_COLOR = 173_952, 6_272


def mac_jacobian(decoder: str, action_dim: int) -> dict:
    """MACs per point of the Jacobian head (SURVEY 8d's table).  `canonical` prices the roofline block.

    jacobian_mlp (action_decoder_jacobian.py:324-337): ResnetFC with d_out = 3A, hoisted lin_z: 8,064 + 163,840 + 128 * 3A
    (A = 8: SURVEY's 174,976).
    jacobian_transformer (action_decoder_jacobian.py:418-446): SURVEY prices the reference formulation at 284,096 (A = 8).  The
    build evaluates an algebraically FOLDED form (decoder.py::ActionDecoderJacobianTransformer.packed: query projection hoisted
    into the feature map like lin_z; to_q, the keys, the LayerNorm affine and the softmax scale folded into one 64 x 8A matrix per
    layer, values and to_out into another): 63 * 64 (encoding part of the query) + 3 * (2 * 64 * 8A + 2 * 64 * 64) + 64 * 3A
    = 28,608 + 3,264 A (A = 8: 54,720).  The canonical figure is the MINIMAL (folded) count, as for the hoisted ResnetFC;
    `reference_formulation` scores the same time against SURVEY's count for comparison."""
    if decoder == "jacobian_mlp":
        return {"canonical": 8_064 + 163_840 + 128 * 3 * action_dim, "reference_formulation": 371_584 - 128 * 3 * (8 - action_dim)}
    folded = 63 * 64 + 3 * (2 * 64 * 8 * action_dim + 2 * 64 * 64) + 64 * 3 * action_dim
    # reference formulation per point: query MLP 575 x 64, per layer to_q 64 x 512 + dots / attn @ V 2 * 512 * A + to_out 512 x 64 +
    # feed-forward 2 * 64 * 64, head 64 x 3A  (= SURVEY's 284,096 at A = 8)
    return {"canonical": folded, "reference_formulation": 284_096 - (8 - action_dim) * (3 * 2 * 512 + 64 * 3)}
# dense MFMA peaks, /opt/skills/guides/MI355X_MICROARCH.md.  "f16f6" issues f16 MFMAs (2.5 PFLOP/s) for the main product and
# fp6 block-scaled MFMAs (10 PFLOP/s) for the correction terms; it is priced against the f16 peak, the slower of the two.
PEAK_TFLOPS = {"f32": 157.3, "f16x2": 2500.0, "f16f6": 2500.0, "f16": 2500.0, "f16+f16x2": 2500.0}
# matrix-pipe time per algorithmic product block, in units of one f16 32x32x16 MFMA: f16x2 evaluates hi*hi + hi*lo + lo*hi;
# f16f6 evaluates hi*hi in f16 and both corrections of FOUR K-steps in two fp6 instructions of the same issue time
ISSUE_FACTOR = {"f32": 1.0, "f16x2": 3.0, "f16f6": 1.5, "f16": 1.0, "f16+f16x2": 1.0}
# modes that are NOT held to the fp32 parity bound: a reduced-precision mode has its own stated tolerance (BASELINE config 5,
# SURVEY 8d "fp16/bf16 MFMA, tolerance stated separately"); never the headline, never the default
# "f16+f16x2" = set_precision("f16", proposal_precision="f16x2"): plain-fp16 FINAL pass (the render kernel of "f16"), error-compensated
# proposal pass, i.e. fp32-class sample placement -- the form whose end-to-end pixels are per-network quantities (VERDICT r05 "next" #2b)
REDUCED_PRECISIONS = ("f16", "f16+f16x2")
MIXED = {"f16+f16x2": ("f16", "f16x2")}    # label -> (decoder precision, proposal precision)
# `dtype` names the ARITHMETIC of the matrix products, not the I/O type (fp32 in, fp32 accumulate, fp32 out in every mode).
DTYPE_TEXT = {
    "f32": "f32 (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate -- the reference's arithmetic)",
    "f16x2": "f16x2 (every fp32 operand split into two fp16, hi*hi + hi*lo + lo*hi as 3 f16 MFMAs per block, fp32 accumulate; "
             "fp32 inputs/outputs; measured error vs fp32 arithmetic ~4e-7 per network)",
    "f16f6": "f16f6 (final pass: hi*hi in f16 MFMAs + both 2^-11-sized correction products in block-scaled fp6 MFMAs, fp32 "
             "accumulate; proposal pass: f16x2; fp32 inputs/outputs; measured error vs fp32 arithmetic ~1.5e-5 per network, "
             "inside north_star's 1e-4 -- see parity_on_bench_frame and profiles/r04_parity_margins.json)",
    "f16": "f16 (PLAIN fp16 products: weights and layer inputs rounded to fp16, one f16 MFMA per block, fp32 accumulate, fp16 "
           "hoisted maps; every network of the frame incl. the proposal pass; fp32 inputs/outputs; a REDUCED-precision mode with "
           "its own stated tolerance, not held to north_star's 1e-4 -- BASELINE config 5's 'fp16 MFMA fused-MLP')",
    "f16+f16x2": "f16 final pass + f16x2 proposal pass (set_precision('f16', proposal_precision='f16x2'): the render kernel evaluates PLAIN "
                 "fp16 products exactly as in 'f16'; the proposal network keeps the error-compensated f16x2 products and its own fp32 "
                 "hoisted map, so SAMPLE PLACEMENT is fp32-class; a REDUCED-precision mode with its own stated tolerance)",
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=60)    # (2 s of timed headline steps: long enough for a 1-s utilisation sampler to see them)
    ap.add_argument("--warmup", type=int, default=5)   # >= 5 warm-ups, >= 20 timed steps
    ap.add_argument("--scaling", choices=["strong", "weak"], default="strong",
                    help="N>1: split ONE frame's rays over the ranks (SURVEY 8e, default) or one full frame per rank")
    ap.add_argument("--simulate-world", type=int, default=0,
                    help="single process: render only rank 0's shard of an N-way strong split (no collectives) -- predicts "
                         "the per-rank step time of --gpus N on one GPU")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample-rays", type=int, default=2048,
                    help="rays per CPU-baseline pass (one patch_render chunk), taken at a constant stride over the frame")
    ap.add_argument("--cpu-passes", type=int, default=3)
    ap.add_argument("--force-dist", action="store_true", help="initialise torch.distributed (RCCL) even with one rank")
    ap.add_argument("--graph", action="store_true",
                    help="strong scaling: replay each rank's compute (Model.forward + partial reduction) as ONE HIP graph; the "
                         "per-kernel HIP-event timings then come from an eager pass after the timed loop.  Default at N > 1 "
                         "(a shard step is 1.4 ms: launch gaps are 8 %% of it); at N = 1 the default is eager")
    ap.add_argument("--no-graph", action="store_true", help="N > 1: keep the rank-local compute eager")
    ap.add_argument("--legacy-step", action="store_true",
                    help="the round-2 step (ATen depth clip / loss sums / concatenation, three collectives) for A/B")
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--samples", type=int, default=S_FINAL, help="proposal and final samples per ray")
    ap.add_argument("--precision", choices=sorted(PEAK_TFLOPS), default=None,
                    help=f"MFMA precision in the headline slot (default {HEADLINE_PRECISION}: the reference's fp32 arithmetic; the "
                         "package default, hip.DEFAULT_PRECISION, is always measured next to it as value_default_precision)")
    ap.add_argument("--no-other-precisions", action="store_true")
    ap.add_argument("--decoder", choices=["jacobian_mlp", "jacobian_transformer"], default="jacobian_mlp",
                    help="Jacobian head of the frame (models/decoder/__init__.py:11-44): the ResnetFC head the headline is quoted on, or "
                         "the attention head configurations/model/model_allegro.yaml:26 selects")
    ap.add_argument("--action-dim", type=int, default=ACTION_DIM,
                    help="A: 8 = Allegro (C2 / C3), 6 = the pneumatic hand of C5 (inference/jacobian_color_map.py:42-49)")
    ap.add_argument("--dry-launch", metavar="STANDINS.py", default=None,
                    help="launcher self-test WITHOUT a GPU (tests/test_host_cpu.py): the same launch / world check / barriers / "
                         "rank evidence / one JSON line, over the gloo backend, with parallel.ShardedFrameStep driven by the "
                         "stand-in kernels the given python file provides.  The line says dry_launch: true and has no value")
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline: the other precisions, per-launch kernel timings and the roofline "
                         "blocks, the frame digest, the CPU baseline and the parity check of the timed frame against the CPU "
                         "oracle (--no-other-precisions / --no-cpu-baseline drop parts of it).  Without it a run sets up, warms "
                         "up, times --steps steps of the headline precision and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (assembled frame, frame scalars, the "
                         "model output of this rank's rays) as DIR/<name>.npy in float32; at most 64 MB in all (a larger output "
                         "is written as a fixed, seeded sample of its rays)")
    return ap.parse_args()


def cpu_model_name() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def timed_loop(step_fn, steps: int, dist, sync):
    """EXACTLY `steps` steps between (barrier + device synchronisation) on both sides.  Returns (seconds until every rank
    has passed the closing barrier, seconds until THIS rank's own device work was done)."""
    if dist is not None:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step_fn()
    sync()
    local = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
    sync()
    return time.perf_counter() - t0, local


def max_over_ranks(dist, seconds: float, device) -> float:
    if dist is None:
        return seconds
    t = torch.tensor([seconds], device=device, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return t.item()


def emit(line: dict, gpus: int) -> None:
    from neural_jacobian_field_amd import launch
    launch.check_line(line, gpus)
    import ctypes
    ctypes.CDLL(None).fflush(None)  # anything native libraries buffered goes out first (to stderr once stdout is reserved)
    sys.stdout.flush()
    launch.print_line(line)         # the process's ORIGINAL stdout: nothing else is ever written there (launch.reserve_stdout)


DUMP_LIMIT_BYTES = 64 * 2**20


def step_arrays(result) -> dict:
    """What one step handed its caller, as {name: tensor}: the step function's (model output, frame scalars / losses, frame)."""
    out, scalars, frame = result
    arrays = {}
    if frame is not None:
        arrays["frame"] = frame                       # [B,R,6] rgb | clipped depth | flow of the whole frame
    if isinstance(scalars, dict):                     # round-2 step: {"loss/rgb": [], "loss/flow_loss": []}
        for k, v in scalars.items():
            arrays[k.replace("/", "_")] = v.reshape(1)
    elif scalars is not None:
        arrays["frame_scalars"] = scalars             # [6] depth-clip min, max, sum sq rgb, sum sq flow, rgb loss, flow loss
    std = getattr(out, "standard_output", out)        # this rank's rays (depth before the frame's clip)
    if std is not None:
        arrays.update(rgb=std.rgb, depth=std.depth, optical_flow=std.optical_flow)
    # copied off the device now: the step's buffers are refilled by every later step
    return {k: v.detach().to("cpu", torch.float64 if v.dtype == torch.float64 else torch.float32, copy=True)
            for k, v in arrays.items()}


def write_outputs(path: str, arrays: dict) -> None:
    """DIR/<name>.npy per array.  Above DUMP_LIMIT_BYTES in all, every array of more than 4,096 rows (rays: all dimensions but
    the last flattened) keeps the same fixed, seeded sample of its rows, so two runs with the same arguments stay comparable."""
    import numpy as np
    total = sum(a.numel() * a.element_size() for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        keep_frac = 0.95 * DUMP_LIMIT_BYTES / total
        sampled = {}
        for k, a in arrays.items():
            rows = a.reshape(-1, a.shape[-1] if a.dim() > 1 else 1)
            n = rows.shape[0]
            if n > 4096:   # (the same permutation for every array of n rows: rgb, depth and flow keep the same rays)
                idx = torch.randperm(n, generator=torch.Generator().manual_seed(0))[: int(n * keep_frac)].sort().values
                a = rows[idx]
                print(f"[bench] --dump-outputs: {k} written as a seeded sample of {a.shape[0]} of its {n} rows", file=sys.stderr)
            sampled[k] = a
        arrays = sampled
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, f"{k}.npy"), a.numpy())


def cpu_baseline(case, ray_index, passes: int):
    # the ONLY place bench.py touches oracle/: the reported CPU baseline and the parity check of the timed frame against it
    # (never the thing measured as `value`)
    """Time the CPU oracle (a port of the reference's PyTorch path) on a bounded sample of the SAME workload: the rays
    `ray_index` of the 256x256 frame (as many as one chunk of Model.patch_render, models/model.py:533), 64+64 samples.
    One warm-up pass, then the median of `passes` timed passes.  Returns (record, oracle outputs of the last pass, the
    oracle's float64 outputs on the same rays = the fp32 floor of every compared quantity, the sub-case)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import parity_harness as ph
    sample_rays = int(ray_index.numel())

    host_cores = os.cpu_count() or 1
    # 32 threads is the fastest setting on the GPU box's 256-core host (tools/cpu_threads_probe.py: 8/16/32/64/128
    # threads -> 760/762/808/707/337 rays/s; all 256 threads oversubscribe these small ops and drop to ~20 rays/s)
    threads = min(host_cores, 32)
    torch.set_num_threads(threads)
    sub = dict(case)
    sub["origins"] = case["origins"][:, ray_index].contiguous()
    sub["directions"] = case["directions"][:, ray_index].contiguous()
    times = []
    ref = None
    for i in range(passes + 1):
        t0 = time.perf_counter()
        ref = ph.oracle_forward(sub, S_PROP, S_FINAL)
        if i:
            times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    ref64 = ph.oracle_forward_fp64(sub, S_PROP, S_FINAL)   # not timed: the yardstick of the parity check below
    rec = {"value": round(sample_rays / med, 1), "unit": "rays/s", "cores": threads, "threads": threads, "host_cores": host_cores,
           "cpu_model": cpu_model_name(), "kind": "port", "passes": passes,
           "pass_seconds": [round(t, 2) for t in times],
           "sample": f"{sample_rays} rays of the same 256x256 frame (every {case['origins'].shape[1] // sample_rays}th ray, 64+64 "
                     f"samples), fp32, torch {torch.__version__} CPU, 1 warm-up + median of {passes} passes of {med:.1f} s, one "
                     "2048-ray chunk like patch_render"}
    return rec, ref, ref64, sub


def parity_on_bench_frame(models, cam, rob, z_near, z_far, origins, directions, ray_index, ref, ref64, sub_case=None):
    """The HIP outputs of the timed frame's rays `ray_index` against the CPU oracle's outputs on the same rays (ray shards
    render bit-identically to the full frame, tests/test_properties_gpu.py, so this IS a full-size check of what was timed),
    for every MFMA precision.  Bound per quantity as in the test-suite: max(1e-4, 2 x floor), floor = the oracle's own
    fp32-vs-float64 difference on these rays; next to it the truth-referenced element-wise columns of
    oracle/parity_harness.py::truth_columns (e_hip = |hip - fp64| against e_ref = |fp32 oracle - fp64|)."""
    import parity_harness as ph
    from neural_jacobian_field_amd.model import RenderingInput

    idx = ray_index.to(origins.device)
    rin = RenderingInput(origins[:, idx].contiguous(), directions[:, idx].contiguous(), z_near, z_far)
    bins_of = lambda r: torch.cat([r.samples_list[1].spacing_starts[..., 0], r.samples_list[1].spacing_ends[..., -1:, 0]], -1)
    ref_bins, ref64_bins = bins_of(ref), bins_of(ref64)
    pairs = {"rgb": (ref.rgb, ref64.rgb), "depth": (ref.depth, ref64.depth), "optical_flow": (ref.optical_flow, ref64.optical_flow),
             "prop_weights": (ref.weights_list[0], ref64.weights_list[0]), "final_bins": (ref_bins, ref64_bins)}
    floors = {k: ph.rel_err(a, b) for k, (a, b) in pairs.items()}
    report = {}
    model16, model16_final = None, None
    for prec, m in models.items():
        with torch.no_grad():
            outs, bins, wl, bl, _ = m._fused_render(cam, rin, rob, m._encode_for_render(None), want_lists=True, want_vis=False,
                                                    want_samples=False)
        torch.cuda.synchronize()
        got = {"rgb": outs["rgb"], "depth": outs["depth"], "optical_flow": outs["flow"], "prop_weights": wl[0], "final_bins": bins}
        rows = {}
        reduced = prec in REDUCED_PRECISIONS
        mixed = prec in MIXED   # reduced final pass, fp32-class placement: the pixels' yardstick is the model's FINAL STAGE at the fp32 bins
        if reduced and not mixed and model16 is None:
            # the yardstick of a reduced-precision mode: the CPU oracle with every matrix operand rounded to fp16
            # (oracle/njf_oracle.py::operand_rounding) on the same rays -- what a correct plain-fp16 evaluation looks like
            me = ph.oracle_forward_f16model(sub_case, S_PROP, S_FINAL)
            model16 = {"rgb": me.rgb, "depth": me.depth, "optical_flow": me.optical_flow, "prop_weights": me.weights_list[0],
                       "final_bins": bins_of(me)}
        if mixed and model16_final is None:
            ms = ph.final_stage_f16model(sub_case, ref_bins)
            model16_final = {"rgb": ms.rgb, "depth": ms.depth, "optical_flow": ms.optical_flow}
        for k, a in got.items():
            b, b64 = pairs[k]
            err, floor = ph.rel_err(a.reshape(b.shape), b), floors[k]
            yard = (model16_final if mixed else model16) if reduced else None
            if reduced and k in yard:
                mfloor = ph.rel_err(yard[k], b)
                small = b.numel() < ph.TRUTH_MIN_ELEMENTS or (k in ("rgb", "depth", "optical_flow") and not mixed)   # (oracle/parity_harness.py)
                limit = max(ph.REDUCED_TOL, (ph.REDUCED_FACTOR_SMALL if small else ph.REDUCED_FACTOR) * mfloor)
                truth = ph.truth_columns(a.reshape(b.shape), yard[k].reshape(b.shape), b64)
                truth["key"] = "truth:" + k
                truth["asserted_ok"] = ph.truth_asserted(truth, "f16", placement_reduced=not mixed)
                rows[k] = {"err": float(f"{err:.3e}"), "floor": float(f"{mfloor:.3e}"), "floor_fp64": float(f"{floor:.3e}"),
                           "limit": float(f"{limit:.3e}"), "ok": bool(err <= limit and truth["asserted_ok"] is not False),
                           "reduced_precision_model_floor": True, "truth": truth}
                continue
            limit = max(1e-4, 2.0 * floor)
            rows[k] = {"err": float(f"{err:.3e}"), "floor": float(f"{floor:.3e}"), "limit": float(f"{limit:.3e}"),
                       "ok": bool(err <= limit), "truth": ph.truth_columns(a.reshape(b.shape), b, b64)}
        report[prec] = rows
    return report


def dry_launch(args, dist, rank: int, world: int) -> None:
    """The launcher path without a GPU: same world check, barriers, max-over-ranks, rank evidence and line gate as a real
    run, with parallel.ShardedFrameStep on CPU tensors and the stand-in kernels of the file named by --dry-launch (the
    tests' self-contained stand-ins: no oracle code runs).  Nothing here is a measurement and the line says so."""
    from neural_jacobian_field_amd import launch, parallel

    standins = os.path.realpath(args.dry_launch)
    if not standins.startswith(os.path.join(ROOT, "tests") + os.sep):   # (this flag executes the file it names)
        raise SystemExit(f"--dry-launch only runs stand-in files under {os.path.join(ROOT, 'tests')}{os.sep}")
    spec = importlib.util.spec_from_file_location("njf_dry_standins", standins)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    step, check = mod.make_frame_step(parallel, world, rank)
    run = lambda: step(None, None, None)
    for _ in range(args.warmup):
        run()
    elapsed, local = timed_loop(run, args.steps, dist, lambda: None)
    elapsed = max_over_ranks(dist, elapsed, "cpu")
    frame, scalars, _ = run()
    ok = torch.tensor([1.0 if check(frame, scalars) else 0.0])
    if dist is not None:
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    evidence = launch.rank_evidence(dist, torch.device("cpu"), 1e3 * local / args.steps)
    if rank == 0:
        emit({"metric": "launcher dry run: stand-in kernels on CPU tensors over gloo -- NOT a measurement", "value": None,
              "unit": "rays/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
              "ms_per_step": round(1e3 * elapsed / args.steps, 3), "dry_launch": True, "frame_ok": bool(ok.item() == 1.0),
              "scaling": "strong", "rccl": evidence}, args.gpus)


def main():
    args = parse()
    from neural_jacobian_field_amd import launch

    dry = args.dry_launch is not None
    # a plain process with --gpus N > 1 spawns its N ranks and exits with their status; under a launcher the world is checked
    launch.ensure_world(args.gpus, os.path.abspath(__file__), sys.argv[1:], need_devices=not dry)
    launch.reserve_stdout()   # from here on only the JSON line reaches this rank's stdout (native libraries print to stderr)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:     # (ensure_world has already refused every such case; kept as the invariant of what follows)
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if dry:
        dist = launch.init_process_group("gloo") if (world > 1 or args.force_dist) else None
        dry_launch(args, dist, rank, world)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    assert torch.cuda.is_available(), "bench.py needs an MI355X; the hot path has no CPU fallback"
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = launch.init_process_group("nccl", device) if (world > 1 or args.force_dist) else None

    import __graft_entry__ as entry

    if rank == 0:
        entry.build()
    if dist is not None:
        dist.barrier()
    from neural_jacobian_field_amd import geometry, hip, parallel, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import CameraInput, Model, RenderingInput, RobotInput

    strong = args.scaling == "strong"
    sim_world = args.simulate_world if (world == 1 and args.simulate_world > 1) else 0
    HH, WW, BB, SS = args.height, args.width, args.batch, args.samples
    DEC, AD = args.decoder, args.action_dim
    macj = mac_jacobian(DEC, AD)
    dev = lambda t: t.to(device)
    # ---- synthetic frame: seeded weights / cameras replicated on every rank; the feature map is the same on
    # every rank under strong scaling (one image) and differs per rank under weak scaling (one image each) ---------------
    params = synthetic.seeded_state_dict(synthetic.model_shapes(DEC, AD, with_encoder=False), seed=0)
    cams = synthetic.synthetic_cameras(BB)
    feats_cpu = synthetic.synthetic_features(BB, HH, WW, seed=1 + (0 if strong else rank))
    action_cpu = synthetic.synthetic_action(BB, AD, seed=2)
    ctxt_c2w, ctxt_k, trgt_c2w = dev(cams["ctxt_c2w"]), dev(cams["ctxt_k_norm"]), dev(cams["trgt_c2w"])
    z_near, z_far, action = dev(cams["z_near"]), dev(cams["z_far"]), dev(action_cpu)
    origins, directions, _ = geometry.full_frame_rays(HH, WW, dev(cams["trgt_k_norm"]), trgt_c2w)  # the HIP ray-generation kernel
    k_pix = geometry.denormalize_intrinsics(dev(cams["trgt_k_norm"]), WW, HH)
    feats = dev(feats_cpu)
    frame_rays = BB * HH * WW
    g = torch.Generator().manual_seed(100 + (0 if strong else rank))
    trgt_rgb = dev(torch.rand(BB, HH * WW, 3, generator=g))
    trgt_flow = dev(torch.randn(BB, HH * WW, 2, generator=g))

    shard_world, shard_rank = (world, rank) if (strong and world > 1) else ((sim_world, 0) if sim_world else (1, 0))
    lo, hi = parallel.shard_bounds(HH * WW, shard_world, shard_rank)
    o_loc, d_loc = origins[:, lo:hi].contiguous(), directions[:, lo:hi].contiguous()
    rgb_loc, flow_loc = trgt_rgb[:, lo:hi].contiguous(), trgt_flow[:, lo:hi].contiguous()
    local_rays = BB * (hi - lo)

    cfg = model_cfg_from_dict({"action_dim": AD, "encoder": {"name": "precomputed"},
                               "rendering": {"num_proposal_samples": [SS], "num_nerf_samples": SS},
                               "action_decoder": {"name": DEC}})
    precision = args.precision or HEADLINE_PRECISION
    default_precision = hip.DEFAULT_PRECISION
    others = args.full and not args.no_other_precisions
    wanted = [precision] + ([p for p in (default_precision, "f16f6", "f16x2", "f32", "f16", "f16+f16x2")] if others else [])
    models = {}
    for prec in dict.fromkeys(wanted):
        m = Model(cfg).to(device).eval().requires_grad_(False)
        m.load_state_dict({k: dev(v) for k, v in params.items()}, strict=True)
        if prec in MIXED:
            m.set_precision(MIXED[prec][0], proposal_precision=MIXED[prec][1])
        else:
            m.set_precision(prec)
        m.bench_label = prec
        m.encoder.set_features(feats)
        if strong and world > 1:
            parallel.enable_ray_sharding(m)
        models[prec] = m
    cam = CameraInput(input_image=None, ctxt_extrinsics=ctxt_c2w, ctxt_intrinsics=ctxt_k, trgt_extrinsics=trgt_c2w,
                      trgt_intrinsics=k_pix)
    rin = RenderingInput(o_loc, d_loc, z_near, z_far)
    rob = RobotInput(action)

    # strong scaling (and N = 1): parallel.ShardedFrameStep -- Model.forward on the shard with the frame-level reductions
    # (depth-clip bounds, loss sums) folded into the render kernel's epilogue, ONE all_gather of [pixels | 4 scalars] per
    # step, one assemble launch (global depth clip + losses).  Weak scaling / --legacy-step: the round-2 step.
    use_frame_step = strong and not args.legacy_step
    frame_steps = {}
    if use_frame_step:
        for prec, m in models.items():
            fs = parallel.ShardedFrameStep(m, BB, HH * WW, device, world_size=shard_world, rank=shard_rank,
                                           collective=not sim_world)
            fs.set_targets(rgb_loc, flow_loc)
            fs.new_image_each_step = True   # the per-image projection stays inside every (eager or captured) step
            frame_steps[prec] = fs

    def step(model):
        if use_frame_step:   # (resets the image cache itself: a new image every step, the projection inside the timed region)
            frame, scalars, out = frame_steps[model.bench_label](cam, rin, rob)
            return out, scalars, frame
        model.reset_image_cache()  # a new image every step: the per-image projection stays inside the timed region
        out = model.forward(cam, rin, rob).standard_output
        # photometric + flow loss (model_wrapper.py:117-163): local sums, ONE all-reduce over the ranks
        losses = parallel.sharded_losses(out.rgb, rgb_loc, out.optical_flow, flow_loc)
        frame = None
        if strong and world > 1:
            frame = parallel.gather_frame(torch.cat([out.rgb, out.depth, out.optical_flow], dim=-1), HH * WW)
        return out, losses, frame

    sync = lambda: torch.cuda.synchronize(device)

    def kernel_ms(records, steps):
        acc = {"project": 0.0, "proposal": 0.0, "render": 0.0}
        for name, e0, e1 in records:
            key = {"njf_project_features_ld": "project", "njf_project_pyramid": "project", "njf_proposal_forward": "proposal",
                   "njf_render_forward": "render"}.get(name)
            if key:
                acc[key] += e0.elapsed_time(e1)
        return {k: v / steps for k, v in acc.items()}

    def measure(prec: str, steps: int, warmup: int, keep_outputs: bool = False) -> dict:
        """`warmup` untimed steps, then EXACTLY `steps` steps between barrier + synchronize on both sides, max over ranks.
        With --full, per-launch HIP events on the launch stream give the kernel durations: inside the timed steps when they run
        eagerly, in an eager pass right after the timed loop when the rank-local compute is replayed as a HIP graph; and one
        more untimed step gives the frame digest.  `keep_outputs`: a host copy of what the last timed step returned."""
        model = models[prec]
        for _ in range(warmup):
            step(model)
        graphed = bool(use_frame_step and not args.no_graph and (args.graph or world > 1))
        if graphed:   # record the rank-local compute once; the graph replays the per-image projection, so no cache reset
            try:
                frame_steps[prec].capture(cam, rin, rob)
            except Exception as exc:   # capture is an optimisation: an eager step is always available
                print(f"[bench] HIP-graph capture failed on rank {rank} ({type(exc).__name__}: {exc}); running eager", file=sys.stderr)
                frame_steps[prec]._graph = None
                graphed = False
            if dist is not None:       # every rank must take the same path through the timed loop's collectives
                flag = torch.tensor([1.0 if graphed else 0.0], device=device)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                if graphed and flag.item() == 0.0:
                    frame_steps[prec]._graph = None
                    graphed = False
        if graphed:
            for _ in range(2):
                step(model)
        launches = []
        if args.full and not graphed:
            hip.set_profile_sink(launches)   # per-launch HIP events on the launch stream (roofline.achieved)
        last = [None]

        def timed_step():
            last[0] = step(model)

        elapsed, local = timed_loop(timed_step, steps, dist, sync)
        hip.set_profile_sink(None)
        outputs = step_arrays(last[0]) if keep_outputs else None
        result = {"elapsed": max_over_ranks(dist, elapsed, device), "local_ms": 1e3 * local / steps, "steps": steps,
                  "warmup": warmup, "graphed": graphed, "outputs": outputs}
        if not args.full:
            return result
        digest_hex = None
        if use_frame_step:   # one more UNTIMED step through the same (possibly graph-replayed) step function, on every rank
            import hashlib
            _, scalars_d, frame_d = step(model)
            sync()
            if frame_d is not None:
                digest_hex = hashlib.sha256(frame_d.detach().float().cpu().numpy().tobytes()
                                            + scalars_d.detach().float().cpu().numpy().tobytes()).hexdigest()
        timing_note = "mean njf_render_forward launch duration over the timed steps, HIP events on the launch stream"
        if graphed:   # events cannot be read back from inside a replayed graph: an eager pass of the same step, not part of `value`
            frame_steps[prec]._graph = None
            hip.set_profile_sink(launches)
            for _ in range(steps):
                step(model)
            sync()
            hip.set_profile_sink(None)
            timing_note = ("mean njf_render_forward launch duration over an EAGER pass of the same steps right after the timed "
                           "(graph-replayed) loop, HIP events on the launch stream")
        result.update(kernel_ms=kernel_ms(launches, steps), launches_per_step=len(launches) / max(steps, 1), timing_note=timing_note,
                      digest=digest_hex)
        return result

    # headline first; with --full the package's default precision with the SAME steps / warm-up / barriers, every other mode likewise
    runs = {precision: measure(precision, args.steps, args.warmup, keep_outputs=args.dump_outputs is not None and rank == 0)}
    for prec in models:
        if prec not in runs:
            # every mode with the SAME --steps / --warmup as the headline (a 60-step run of the slowest extra mode is 0.7 s)
            runs[prec] = measure(prec, args.steps, args.warmup)
    head = runs[precision]
    evidence = launch.rank_evidence(dist, device, head["local_ms"], graph=head["graphed"], kernel_ms=head.get("kernel_ms"))
    # One more UNTIMED step of the headline mode on every rank: the digest of what it produced (assembled frame + the six clip /
    # loss scalars).  The kernels are bit-reproducible, so a one-rank run WITH the collective (--force-dist, eager or --graph)
    # must print the digest of the plain run (tests/test_rccl_gpu.py).
    digest = None
    if head.get("digest") is not None:
        digest = {"sha256": head["digest"],
                  "of": "assembled frame [B,R,6] (rgb | clipped depth | flow) + [depth-clip min, max, sum sq rgb, sum sq flow, rgb loss, "
                        "flow loss] of one extra untimed step in the headline precision, taken right after the timed loop through the "
                        "SAME step function (graph replay included when the step was captured)"}

    total_rays = local_rays if sim_world else (frame_rays if strong else world * frame_rays)
    render_flop = 2.0 * local_rays * SS * (MAC_DENSITY + macj["canonical"] + MAC_COLOR)
    render_flop_reference = 2.0 * local_rays * SS * (370_560 + macj["reference_formulation"] + MAC_COLOR)

    def roofline(prec: str, run: dict) -> dict:
        achieved = render_flop / (run["kernel_ms"]["render"] * 1e-3) / 1e12
        traffic, traffic_source = None, None
        if local_rays == H * W and SS == S_FINAL and (DEC, AD) == ("jacobian_mlp", ACTION_DIM):
            for rnd in PROFILE_ROUNDS:
                pmc = os.path.join(ROOT, "profiles", f"{rnd}_render_kernel_hbm_bytes_{prec}.json")
                if os.path.exists(pmc):
                    with open(pmc) as f:
                        traffic = json.load(f).get("hbm_bytes_per_launch")
                    traffic_source = (f"NOT measured in this run: read from profiles/{os.path.basename(pmc)} (rocprofv3 --pmc passes "
                                      "of this command on an earlier box, tools/profile_rNN.sh + tools/summarize_profile.py)")
                    break
        block = {"kernel": f"render_kernel<{DEC}, {prec}> (density ResnetFC + colour head + Jacobian head + compositing)",
                 "bound": "mfma", "achieved": round(achieved, 2), "peak": PEAK_TFLOPS[prec], "unit": "TFLOP/s",
                 "frac": round(achieved / PEAK_TFLOPS[prec], 4), "traffic": traffic, "traffic_source": traffic_source,
                 "algorithmic_flop_per_launch": render_flop, "mfma_issue_factor": ISSUE_FACTOR[prec],
                 "timing": run["timing_note"]}
        if DEC == "jacobian_transformer":   # the head is evaluated in a folded form: say so, and score SURVEY's count beside it
            block["mac_per_point"] = {"density": MAC_DENSITY, "colour": MAC_COLOR, "jacobian_folded": macj["canonical"],
                                      "jacobian_reference_formulation_SURVEY_8d": macj["reference_formulation"]}
            ach_ref = render_flop_reference / (run["kernel_ms"]["render"] * 1e-3) / 1e12
            block["against_reference_formulation"] = {
                "flop_per_launch": render_flop_reference, "achieved": round(ach_ref, 2), "frac": round(ach_ref / PEAK_TFLOPS[prec], 4),
                "note": "the same launch duration scored against SURVEY 8d's NON-hoisted counts (density 370,560 + colour 6,272 + "
                        "transformer 284,096 MAC/pt): work the folded evaluation does not perform -- context, not the roofline fraction"}
        return block

    if rank == 0:
        ms_step = 1e3 * head["elapsed"] / head["steps"]
        value = total_rays * head["steps"] / head["elapsed"]
        mode = "strong" if strong else "weak"
        workload = ("C2: " if (BB, HH, WW, SS, DEC, AD) == (1, 256, 256, 64, "jacobian_mlp", ACTION_DIM) else "") + (
            f"Allegro single-view PixelNeRF, B={BB}, {HH}x{WW} rays, {SS} proposal + {SS} final samples/ray, {DEC}, A={AD}, "
            "eval-mode Model.forward (encoder excluded: 'precomputed' encoder entry returning the synthetic feature map; the "
            "per-image lin_z projection is inside the timed call) + rgb/flow loss")
        if world > 1:
            workload += (" + RCCL: ONE all_gather of [pixel shard | depth-clip bounds, loss sums] per step (rays of ONE frame split "
                         "over the ranks)" if strong and use_frame_step else
                         (" + RCCL: depth-clip all-reduce, loss all-reduce, all_gather of the pixel shards" if strong else
                          " + RCCL loss all-reduce (one frame per rank)"))
        out = {
            "metric": "rendered rays/s (64 samples/ray, 256^2 image)",
            "value": round(value, 1), "unit": "rays/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_step, 3), "higher_is_better": True, "scaling": mode, "vs_baseline": None,
            "dtype": DTYPE_TEXT[precision], "data": "synthetic",
            "config": {"workload": workload, "precision": precision, "rays_per_gpu": local_rays, "decoder": DEC, "action_dim": AD,
                       "parallelism": f"dp{world} ({'one frame, rays sharded' if strong else 'one frame per rank'}, replicated weights "
                                      "and feature map)"},
            **({"kernel_ms": {k: round(v, 3) for k, v in head["kernel_ms"].items()}} if args.full else {}),
            "step": {"form": ("ShardedFrameStep: Model.forward (one per-image projection for all networks, njf_proposal_forward, njf_render_forward "
                              "with the frame reductions in its epilogue) + njf_reduce_frame_partials + "
                              + ("ONE all_gather of [pixels | 4 scalars] + " if world > 1 else "")
                              + "njf_assemble_frame (global depth clip, rgb / flow loss)") if use_frame_step else
                             "round-2 step: Model.forward + ATen depth clip, loss sums, concatenation (three collectives at N > 1)",
                     **({"c_abi_launches_per_step": round(head["launches_per_step"], 2)} if args.full else {}),
                     "hip_graph": head["graphed"]},
            **({"roofline": roofline(precision, head)} if args.full else {}),
            **({"reduced_precision": True,
                "reduced_precision_note": "--precision put a REDUCED-precision mode in the headline slot: `value` is NOT fp32-parity arithmetic; "
                                          "its tolerance is other_precisions' `tolerance` text (oracle/parity_harness.py: operand-rounding model)"}
               if precision in REDUCED_PRECISIONS else {}),
            "rccl": evidence,
            **({"frame_digest": digest} if args.full else {}),
            "full": bool(args.full),
        }
        if sim_world:
            out["simulated"] = f"rank 0's shard of a {sim_world}-way strong split rendered on ONE GPU, no collectives: value counts only these rays"
        if args.full:   # everything the headline does not need: other precisions, CPU baseline, parity of the timed frame
            out["other_precisions"] = {}
            for prec, run in runs.items():
                if prec == precision:
                    continue
                ms = 1e3 * run["elapsed"] / run["steps"]
                rf = roofline(prec, run)
                out["other_precisions"][prec] = {
                    "ms_per_step": round(ms, 3), "steps": run["steps"], "warmup": run["warmup"],
                    "rays_per_s": round(total_rays / (ms * 1e-3), 1), "kernel_ms": {k: round(v, 3) for k, v in run["kernel_ms"].items()},
                    "roofline_achieved_tflops": rf["achieved"], "roofline_peak_tflops": rf["peak"], "roofline_frac": rf["frac"],
                    "hip_graph": run["graphed"]}
                if prec in REDUCED_PRECISIONS:   # its own roofline block and its own stated tolerance (VERDICT r04 "next" #1)
                    out["other_precisions"][prec].update(
                        dtype=DTYPE_TEXT[prec], roofline=rf, reduced_precision=True,
                        tolerance="norm-wise err <= max(2e-3, f x the operand-rounding model of plain fp16 on the CPU oracle) per quantity, f = 2 for "
                                  "tensors of >= 1,024 elements, 4 for smaller ones and for the placement-dominated pixels rgb / depth / optical_flow "
                                  "of the all-fp16 mode; AND element-wise against float64 on tensors of >= 1,024 elements: rms <= 1.5 x, max <= 2 x "
                                  "the model's error (pixels of the all-fp16 mode: median <= 1.5 x, rms <= 2.5 x, max <= 4 x) -- "
                                  "parity_on_bench_frame; tests/test_hip_parity.py::test_plain_f16_mode_within_stated_tolerance, "
                                  "::test_f16_shading_with_compensated_placement_at_full_size")
                if prec == default_precision:   # the mode a user gets without asking: same protocol as the headline, NOT fp32 arithmetic
                    out["value_default_precision"] = {
                        "value": round(total_rays / (ms * 1e-3), 1), "unit": "rays/s", "ms_per_step": round(ms, 3), "steps": run["steps"],
                        "warmup": run["warmup"], "dtype": DTYPE_TEXT[prec],
                        "timing": "same step function and process as the headline, its own warm-up, barrier + synchronize on both sides "
                                  "of exactly `steps` steps, max over ranks",
                        "kernel_ms": {k: round(v, 3) for k, v in run["kernel_ms"].items()}, "roofline": rf,
                        "note": "an accelerated mode held to the same parity bounds (parity_on_bench_frame, profiles/r04_parity_margins.json); "
                                "its products are not fp32 products, so it is not the headline"}
            out["parity_note"] = ("every PARITY precision (f32, f16x2, f16f6) is held to the SAME bound against the CPU oracle / the reference's goldens "
                                  "(the reduced-precision mode f16 has its own stated rule: other_precisions.f16.tolerance): "
                                  "max(1e-4, 2 x the reference's own fp32-vs-fp64 difference of that quantity), and is reported "
                                  "element-wise against the float64 truth next to the reference's own fp32 error (truth columns).  rgb, "
                                  "depth and the per-sample fields meet north_star's 1e-4; END-TO-END optical_flow is bounded by the "
                                  "reference's own fp32 floor (5e-4 ... 3e-3: sample placement feeds a 2*pi*512-gain encoding), not by "
                                  "1e-4, in EVERY precision including exact fp32 arithmetic")
            if world == 1 and not sim_world and not args.no_cpu_baseline and (BB, HH, WW, SS) == (1, 256, 256, 64):
                case = {"params": params, "feats": feats_cpu, "cams": cams, "origins": origins.cpu(), "directions": directions.cpu(),
                        "k_pix": k_pix.cpu(), "action": action_cpu, "decoder_kind": DEC}
                stride = max(1, (HH * WW) // args.cpu_sample_rays)
                ray_index = torch.arange(0, HH * WW, stride)[: args.cpu_sample_rays]
                out["cpu_baseline"], ref, ref64, sub_case = cpu_baseline(case, ray_index, args.cpu_passes)
                # full-size parity of the frame that was just timed, in every precision
                out["parity_on_bench_frame"] = {
                    "rays": f"{ray_index.numel()} rays of the timed C2 frame (every {stride}th), 128x128x512 feature map, 64+64 samples",
                    "rule": "err <= max(1e-4, 2 x floor); err, floor norm-wise (max|a-b| / max|b|); floor = CPU oracle fp32 vs the same "
                            "oracle in float64 on these rays.  truth: element-wise |hip - fp64| against |fp32 oracle - fp64|, relative "
                            "to max|fp64|; truth_ok = max and 99.9th percentile within 1.5 x the oracle's own (or 4 fp32 ulps of scale) -- "
                            "truth_ok_strict -- OR both within 2.0 x with the rms within 1.5 x (rows then marked tail_outlier)",
                    "rule_reduced_precision": "modes in REDUCED_PRECISIONS ('f16': plain fp16 products; 'f16+f16x2': plain-fp16 final pass, compensated "
                                              "proposal pass -- its pixels are held to the model's FINAL STAGE at the fp32 sample locations with f = 2, "
                                              "its proposal rows to the fp32 rule): err <= max(2e-3, f x model), f = 2 "
                                              "(4 for tensors below 1,024 elements and for rgb / depth / optical_flow, whose error is "
                                              "sample placement through the inverse CDF), model = "
                                              "the CPU oracle with every matrix operand rounded to fp16 (oracle/njf_oracle.py::operand_rounding) "
                                              "against the fp32 oracle on these rays; truth columns then take e_ref = |model - fp64| and are ASSERTED "
                                              "(rms <= 1.5 x, max <= 2 x; all-fp16 pixels: median <= 1.5 x, rms <= 2.5 x, max <= 4 x): `ok` includes them",
                    **parity_on_bench_frame(models, cam, rob, z_near, z_far, origins, directions, ray_index, ref, ref64, sub_case)}
                out["parity_on_bench_frame"]["all_ok"] = all(r["ok"] for k, v in out["parity_on_bench_frame"].items()
                                                             if isinstance(v, dict) for r in v.values())
                out["parity_on_bench_frame"]["headline_truth_ok"] = all(
                    r["truth"]["truth_ok"] for r in out["parity_on_bench_frame"][precision].values())
                out["parity_on_bench_frame"]["headline_truth_ok_strict"] = all(
                    r["truth"]["truth_ok_strict"] for r in out["parity_on_bench_frame"][precision].values())
                out["parity_on_bench_frame"]["headline_tail_outlier_rows"] = sum(
                    bool(r["truth"].get("tail_outlier")) for r in out["parity_on_bench_frame"][precision].values())
        if args.dump_outputs is not None:
            write_outputs(args.dump_outputs, head["outputs"])
            out["outputs_dumped"] = sorted(head["outputs"])
        emit(out, args.gpus)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
