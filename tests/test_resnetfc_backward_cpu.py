"""Pins tests/resnetfc_backward_restatement.py -- the float64 reference of the fused ResnetFC backward chain that
tests/test_resnetfc_backward_gpu.py compares njf_resnetfc_backward with -- without a GPU:

* its chain is the derivative of its forward: deltas, column sums and dW equal ``torch.autograd.grad`` through ``forward`` with
  respect to the layer outputs, the latents, the biases and all weights;
* ``pack_mask`` / ``unpack_mask`` are inverse to each other and follow the bit order dump_vec128 documents, the sign-edge values
  included;
* its fp32 twin (the yardstick of the GPU tests) stays under TWIN_CAP on every input family and shape the GPU tests use, and the
  families are what they claim to be.
"""
import os
import re

import pytest
import torch

import resnetfc_backward_restatement as R

# The GPU tests hold the exact chain to 4 x the twin's error and state that no such limit exceeds 1e-5: the twin alone has to stay
# at or under a quarter of that on every input the GPU tests use (the same cap as tests/test_transformer_backward_cpu.py).
LIMIT_CAP = 1e-5
TWIN_CAP = LIMIT_CAP / 4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "neural-jacobian-field_amd", "csrc", "njf_device.h")) as _f:
    WAVES = int(re.search(r"^#define NJF_WAVES (\d+)", _f.read(), re.M).group(1))
BLOCK = 32 * WAVES
STRESS_POINTS = R.stress_points(BLOCK)


@pytest.mark.parametrize("d_out_dim", [1, 17, 32])
def test_chain_is_autograd_of_the_forward(d_out_dim):
    from neural_jacobian_field_amd import synthetic, training
    pts = 77
    g = torch.Generator().manual_seed(d_out_dim)
    p = {k: v.double().requires_grad_(True)
         for k, v in synthetic.seeded_state_dict(synthetic.resnet_fc_shapes("", 63, 512, d_out_dim), seed=1).items()
         if not k.startswith("lin_z")}
    pe_x = torch.randn(pts, 63, generator=g, dtype=torch.float64)
    latents = torch.randn(3, pts, 128, generator=g, dtype=torch.float64).requires_grad_(True)
    d_out = torch.randn(pts, d_out_dim, generator=g, dtype=torch.float64)
    f = R.forward(p, pe_x, latents)
    assert f["act"].shape == (11, pts, 128) and f["out"].shape == (pts, d_out_dim)
    assert 0.2 < float((f["act"] > 0).double().mean()) < 0.8                              # gates of both kinds
    names = list(p)
    grads = torch.autograd.grad(f["out"], f["pre"] + [latents] + [p[k] for k in names], d_out)
    g_pre, g_lat, g_par = torch.stack(grads[:11]), grads[11], dict(zip(names, grads[12:]))
    res = R.chain({k: v.detach() for k, v in p.items()}, f["act"].detach(), d_out)
    assert res["deltas"].shape == (11, pts, 128) and res["sums"].shape == (11, 128) and res["dW"].shape == (10, 128, 128)
    worst = 0.0
    for l in range(11):
        worst = max(worst, R.rel(res["deltas"][l], g_pre[l]))
    for blk in range(3):                                                               # the latents: slices 0, 2, 4
        worst = max(worst, R.rel(res["deltas"][2 * blk], g_lat[blk]))
    for l, name in enumerate(training._LAYER_NAMES):                                   # the layer whose ReLU'd input is act[l]
        worst = max(worst, R.rel(res["dW"][l], g_par[name + ".weight"]), R.rel(res["sums"][l + 1], g_par[name + ".bias"]))
    worst = max(worst, R.rel(res["sums"][0], g_par["lin_in.bias"]), R.rel(res["deltas"][0].t() @ pe_x, g_par["lin_in.weight"]))
    worst = max(worst, R.rel(d_out.t() @ f["act"][10].detach(), g_par["lin_out.weight"]), R.rel(d_out.sum(0), g_par["lin_out.bias"]))
    print(f"d_out = {d_out_dim}: chain vs autograd {worst:.2e}")
    assert worst <= 1e-12


def test_mask_packing_round_trips_and_follows_the_documented_bit_order():
    for family in ("random", "sign_edges", "gates"):
        act = R.inputs(family, 70, 3)["act"]
        mask = R.pack_mask(act)
        assert mask.shape == (11, 70, 4) and mask.dtype == torch.int32
        assert torch.equal(R.unpack_mask(mask), act.double() > 0)
    # one feature at a time: bit f % 32 of word f // 32, nothing else
    eye = torch.eye(128)
    mask = R.pack_mask(eye).to(torch.int64) & 0xFFFFFFFF
    for f in range(128):
        want = [0, 0, 0, 0]
        want[f // 32] = 1 << (f % 32)
        assert mask[f].tolist() == want, f
    # the kernel-side statement of the same layout (dump_vec128 / the [layer, point, hh, word, m & 1, r] view of
    # tests/test_training_gpu.py::test_backward_chain_f16x2_against_exact)
    act = R.inputs("random", 5, 3)["act"]
    bits = (act > 0).reshape(11, 5, 2, 2, 2, 16).to(torch.int64)
    words = (bits * (1 << torch.arange(32, dtype=torch.int64)).reshape(2, 16)).sum((-1, -2)).reshape(11, 5, 4)
    assert torch.equal(R.pack_mask(act).to(torch.int64) & 0xFFFFFFFF, words)
    # the sign-edge values one by one: zeros of both signs are closed; the denormal, the smallest normal and fp16's zero are open
    row = torch.zeros(128)
    row[:6] = torch.tensor(R.SIGN_EDGE_VALUES)
    assert R.unpack_mask(R.pack_mask(row))[:6].tolist() == [False, False, True, True, True, True]
    assert float(row[4].half()) == 0.0 and float(row[2]) > 0.0 and torch.signbit(row[1])
    assert int(R.pack_mask(torch.ones(128))[3]) == -1                                   # bit 31: a negative int32 word


def _twin_errors(inp):
    ref, tw = R.reference_and_twin(inp)
    named = R.named_rows(ref)
    errs = {k: R.rel(v, named[k]) for k, v in R.named_rows(tw).items()}
    assert all(torch.isfinite(v).all() for v in R.named_rows(tw).values())
    return errs


def _hold_twin(label, cases):
    worst = (0.0, None)
    for args in cases:
        errs = _twin_errors(R.inputs(*args))
        k = max(errs, key=errs.get)
        worst = max(worst, (errs[k], args + (k,)))
        assert errs[k] <= TWIN_CAP, (args, k, errs[k])
    print(f"fp32 twin, {label}: worst {worst[0]:.2e} at {worst[1]} (cap {TWIN_CAP:.1e})")


def test_fp32_twin_stays_under_the_cap_random():
    """Every (points, d_out) of the GPU module's sections a and d, every compared tensor."""
    shapes = set(R.exact_shapes(BLOCK)) | set(R.split_shapes(BLOCK)) | set(R.storage_shapes(BLOCK))
    _hold_twin("random", [("random", p, d) for p, d in sorted(shapes)])


@pytest.mark.parametrize("family", ["decades", "gates", "sign_edges"])
def test_fp32_twin_stays_under_the_cap_stress(family):
    shapes = {(p, 24) for p in STRESS_POINTS}
    if family == "decades":                                                             # section d runs it at every shape
        shapes |= set(R.split_shapes(BLOCK))
    _hold_twin(family, [(family, p, d) for p, d in sorted(shapes)])


def test_fp32_twin_is_exact_on_onehot():
    """d_out = e_d: deltas[10] is a row of lin_out.weight under the mask, in any arithmetic."""
    for d_out_dim in (1, 17, 32):
        for d in range(d_out_dim):
            inp = R.inputs("onehot", 33, d_out_dim, hot=d)
            ref, tw = R.reference_and_twin(inp)
            hot = R.onehot_point(33, d)
            want = torch.where(inp["act"][10, hot] > 0, inp["params"]["lin_out.weight"][d], torch.zeros(()))
            assert torch.equal(tw["deltas"][10, hot], want) and torch.equal(ref["deltas"][10, hot], want.double())
            others = torch.arange(33) != hot
            assert float(ref["deltas"][:, others].abs().max()) == 0.0
    _hold_twin("onehot", [("onehot", 33, 32, 0, d) for d in (0, 15, 16, 31)])


def test_families_are_what_they_claim():
    pts = BLOCK + 1
    rows = R.gate_rows(pts)
    assert {0, 31, pts - 1} <= set(rows["closed"]) and {32, 63, pts - 2} <= set(rows["passing"]) and {1, 33, pts - 3} <= set(rows["open"])
    assert not (set(rows["closed"]) & set(rows["passing"])) and not (set(rows["open"]) & (set(rows["closed"]) | set(rows["passing"])))
    inp = R.inputs("gates", pts, 24)
    gate = R.gates(inp["act"])
    assert not gate[:, rows["closed"]].any() and gate[:, rows["open"]].all()
    assert not gate[:10, rows["passing"]].any() and gate[10, rows["passing"]].all()
    ref, _ = R.reference_and_twin(inp)
    d = ref["deltas"]
    shut = rows["closed"] + rows["passing"]
    for blk in range(5):                                                               # the bit-level statement of the GPU module
        assert torch.equal(d[2 * blk][shut], d[2 * blk + 2][shut]) and float(d[2 * blk + 1][shut].abs().max()) == 0.0
    assert float(d[:, rows["closed"]].abs().max()) == 0.0 and float(d[0][rows["passing"]].abs().min()) > 0.0
    # sign_edges: all six values occur, in every layer
    act = R.inputs("sign_edges", pts, 24)["act"]
    for v in R.SIGN_EDGE_VALUES:
        same = (act.view(torch.int32) == torch.tensor(v, dtype=torch.float32).view(torch.int32))
        assert same.reshape(11, -1).any(1).all(), v
    # decades: per-point magnitudes over 8 decades
    mags = R.inputs("decades", 4096 + 13, 24)["d_out"].abs().amax(1)
    assert float(mags.max() / mags.min()) > 1e8
