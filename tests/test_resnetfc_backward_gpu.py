"""Kernel-level tests of the fused ResnetFC backward chain (njf_resnetfc_backward, csrc/njf_kernels.hip: resnetfc_backward_kernel)
on plain tensors -- no rendered frame, no sample placement -- in all eight forms: product form (f32 | f16x2) x sign source (dumped
activations | dumped bit masks) x storage (fp32 deltas | fp16 deltas16 with compact fp32 latent slices).

Reference: tests/resnetfc_backward_restatement.py in float64 (pinned by tests/test_resnetfc_backward_cpu.py).

Tolerances:
* exact-fp32 chain (sections a, b, e): err = max|kernel - f64| / max|f64| per compared tensor (each deltas slice, each row of the
  column sums, each product dW[l] = deltas[l+1]^T act[l] formed in float64); floor = the same figure for the fp32 twin (the
  restatement in float32 library ops on the same inputs); limit = min(max(4 x floor, 4 x 2^-23), 1e-5): the factor and the cap are
  those of tests/test_transformer_backward_gpu.py, the 4-ulp floor is conftest.py's truth rule (a one-point case, whose twin can
  be exact by luck, must not fail on a single rounding).
* f16x2 chain (section d): against the exact chain's output on the same inputs, limit 2e-5 -- the bound
  tests/test_training_gpu.py::test_backward_chain_f16x2_against_exact states; the ratio of its float64 error to the exact chain's
  is recorded, not asserted.
* fp16 storage through the wrapper (section e): 1e-5 for what the chain makes in fp32, 2e-3 for the fp16-contracted weight gradients
  -- the bounds tests/test_training_gpu.py::test_f16_training_storage_against_fp32_storage states -- and the twin limit for d_feats.
* sections b, c and f and the onehot / gates statements of section a are bit-level and have no tolerance, except the fp16 sub-normal
  range of deltas16 (|deltas x 2^k| < 2^-14), which is held to an absolute 2^-14.
Every compared row with a tolerance is recorded through ``margins.record`` (case, key, err, floor, limit, ok).

Measured on an MI355X (the whole module, 117 cases, runs in ~6.5 s; tests/test_transformer_backward_gpu.py: ~5 s).  NO DEFECT WAS
FOUND: every case passed with the kernel, hip.py and training.py as they were, and nothing in them was changed.  Worst figures:
* section a, 28 shapes x 32 rows: worst err / floor / limit = 2.4e-7 / 1.3e-7 / 5.2e-7 (sums[6], P = 33, d_out = 17: 0.47 of its limit);
  largest err 5.7e-7 (sums[3], P = 33, d_out = 31; floor 3.5e-7); largest err / floor 2.1 (sums[6], P = 129, d_out = 31), i.e. the
  MFMA accumulation order and the DPP column sum cost at most about two twin errors.  Stress families (6 cases x 32 rows): worst
  3.0e-7 / 1.7e-7 / 6.6e-7 (gates, P = 4109, sums[1]); largest err 7.2e-7 (floor 4.3e-7).  The onehot and gates statements hold
  bit for bit, d >= 16 and the first / last lane of a tile and the ragged tile included; two launches give the same bits.
* section b: the mask route gives the act route's bits at all 8 point counts in both product forms, also beside an all-NaN ``act``;
  +0.0, -0.0, 1e-40 (an fp32 denormal: v_cmp_gt_f32 does not flush it), 1.1754944e-38, 1e-8 and 1.0 are decided as float64 decides
  them by a > 0.f, by the mask bit, and by njf_relu_backward (tests/test_properties_gpu.py).
* section c: latent, sums and unscale as stated in all cases; deltas16 equals the host's round-to-nearest-even conversion in every
  normal fp16.  fp16 SUB-NORMALS ARE KEPT by the store (v_cvt_pk_f16_f32), not flushed: all 246 (f32 form; 245 in f16x2) non-zero
  elements with |deltas x 2^k| < 2^-14 at P = 4109 were stored non-zero and equal the host's sub-normal rounding bit for bit
  (largest distance 3.0e-8 = half a sub-normal step against the 2^-14 = 6.1e-5 allowed).  Exactly linear for m = -40, -3, +20 and
  exactly zero for d_out = 0 in all four (product form x storage) combinations.
* section d, 30 cases x 22 rows: f16x2 within 1.3e-6 of the exact chain (deltas[9], decades, P = 33; limit 2e-5); its float64
  error is at most 8.3 x the exact chain's (sums[5], random, P = 129, d_out = 1), typically 3-5 x.
* section e: fp32-made gradients at most 3.3e-7 (lin_in.weight; twin 2.3e-7; limit 1e-5), fp16-contracted ones at most 4.0e-4
  (blocks.1.fc_0.weight; limit 2e-3), d_feats 6.8e-7 / floor 3.2e-7 / limit 1.3e-6 (its scatter uses atomics: 6.7e-7 in another run).
* section f: jac_mask / den_mask equal pack_mask of the activations dumped beside them (B x R x S = 528 points x 11 layers), and are
  the same bits under fp16 storage, whose activations are the fp32 ones rounded once.
* the restatement is what decides: with fc_0 / fc_1 of block 2 swapped, or the residual add of block 1 dropped, all 34 cases of
  section a fail; with pack_mask shifted by one bit 23 cases of sections b, e and f fail; expecting latent[1] from slice 3, or a
  2^-k off by one, fails all 8 cases of test_fp16_storage_is_the_rounded_fp32_storage (scratch copies, not kept).

Run with -m gpu."""
import math
import os
import re

import pytest
import torch

import resnetfc_backward_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "neural-jacobian-field_amd", "csrc", "njf_device.h")) as _f:
    WAVES = int(re.search(r"^#define NJF_WAVES (\d+)", _f.read(), re.M).group(1))     # tiles (of 32 points) per workgroup
BLOCK = 32 * WAVES
POINTS, D_OUT = R.point_counts(BLOCK), R.D_OUT
RAGGED, LARGE = BLOCK + 1, R.LARGE
STRESS_POINTS = R.stress_points(BLOCK)
EXACT_SHAPES, SPLIT_SHAPES, STORAGE_SHAPES = R.exact_shapes(BLOCK), R.split_shapes(BLOCK), R.storage_shapes(BLOCK)
FACTOR, ULP_FLOOR, LIMIT_CAP, SPLIT_LIMIT = 4.0, 4.0 * 2.0 ** -23, 1e-5, 2e-5
PRECISIONS = ("f32", "f16x2")
FORMS = (("f32", "f32"), ("f32", "f16"), ("f16x2", "f32"), ("f16x2", "f16"))      # (product form, storage)
FP16_MIN_NORMAL = 2.0 ** -14


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    assert hip.load_library().njf_rays_per_workgroup() == WAVES
    return torch.device("cuda:0")


_case_cache = {}


def _case(family, points, d_out_dim, **kw):
    """(inputs, float64 chain, fp32 twin), computed once per case and shared by the tests that use it (never modified)."""
    key = (family, points, d_out_dim, tuple(sorted(kw.items())))
    if key not in _case_cache:
        inp = R.inputs(family, points, d_out_dim, **kw)
        _case_cache[key] = (inp,) + R.reference_and_twin(inp)
    return _case_cache[key]


def _pack(dev, params, precision):
    from neural_jacobian_field_amd import hip
    w = torch.empty(hip.RESNET_BACKWARD_W_FLOATS, dtype=torch.float32, device=dev)
    hip.pack_resnetfc_backward({k: v.to(dev) for k, v in params.items() if not k.startswith("lin_z")}, "", w, precision=precision)
    return w


def _launch(dev, inp, route="act", precision="f32", storage="f32", d_out=None, act=None, w=None):
    """One pack + one launch -> the kernel's outputs on the host.  ``route``: "act" (the chain reads the activations' signs) or
    "mask" (it reads pack_mask of the case's activations; ``act`` is then what is handed over beside it).  fp32 storage: deltas
    [11,P,128], sums [11,128].  ``storage`` = "f16" (mask route only): latent [3,P,128], deltas16 [11,P,128] fp16, sums, unscale (a
    float)."""
    from neural_jacobian_field_amd import hip
    w = _pack(dev, inp["params"], precision) if w is None else w
    d_out = (inp["d_out"] if d_out is None else d_out).contiguous().to(dev)
    mask = R.pack_mask(inp["act"]).to(dev) if route == "mask" else None
    if storage == "f16":
        assert route == "mask" and act is None
        latent, deltas16, sums, unscale = hip.resnetfc_backward_f16_storage(d_out, w, mask, precision=precision)
        torch.cuda.synchronize(dev)
        assert latent.dtype == sums.dtype == unscale.dtype == torch.float32 and deltas16.dtype == torch.float16
        assert latent.shape == (3, d_out.shape[0], 128) and deltas16.shape == (11, d_out.shape[0], 128) and sums.shape == (11, 128)
        return {"latent": latent.cpu(), "deltas16": deltas16.cpu(), "sums": sums.cpu(), "unscale": float(unscale.item())}
    act = (inp["act"] if act is None else act).contiguous().to(dev)
    deltas, sums = hip.resnetfc_backward(d_out, act, w, want_colsum=True, mask=mask, precision=precision)
    torch.cuda.synchronize(dev)
    assert deltas.shape == act.shape and sums.shape == (11, 128) and deltas.dtype == sums.dtype == torch.float32
    return {"deltas": deltas.cpu(), "sums": sums.cpu()}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _row(key, err, floor, limit, **more):
    return {"key": key, "err": float(f"{err:.3e}"), "floor": float(f"{floor:.3e}"), "limit": float(f"{limit:.3e}"),
            "needs_floor": False, "ok": bool(err <= limit), **more}


def _twin_limit(floor):
    return min(max(FACTOR * floor, ULP_FLOOR), LIMIT_CAP)


def _compare_exact(margins, case, got, inp, ref, tw):
    """Every deltas slice, every colsum row and the ten dW products of an exact-fp32 launch against float64, each at its twin limit;
    all failures of the case are collected before asserting."""
    rows, bad = [], []
    named_got = R.named_rows({"deltas": got["deltas"], "sums": got["sums"], "dW": R.products64(got["deltas"], inp["act"])})
    named_ref, named_tw = R.named_rows(ref), R.named_rows(tw)
    for key, r in named_ref.items():
        g, t = named_got[key], named_tw[key]
        assert torch.isfinite(g).all(), (case, key)
        err, floor = R.rel(g, r), R.rel(t, r)
        assert math.isfinite(floor) and FACTOR * floor <= LIMIT_CAP, (case, key, floor)     # the inputs keep the twin under a quarter of the cap
        rows.append(_row(key, err, floor, _twin_limit(floor)))
        if not rows[-1]["ok"]:
            bad.append((key, f"err {err:.3e}", f"floor {floor:.3e}", f"limit {_twin_limit(floor):.3e}"))
    worst = max(rows, key=lambda r: r["err"] / r["limit"])
    print(f"[{case}] worst err/limit: {worst['key']} err {worst['err']:.2e} floor {worst['floor']:.2e} limit {worst['limit']:.2e}; "
          f"largest err {max(r['err'] for r in rows):.2e}")
    margins.record(case, rows)
    return bad


def _closed_gate_failures(deltas, gate):
    """The bit-level statement of a closed gate: an exact 0 in slices 10 and 2b+1, an exact pass-through deltas[2b] == deltas[2b+2]
    in the even slices."""
    bad = []
    if bool((deltas[10][~gate[10]] != 0).any()):
        bad.append("deltas[10] != 0 under a closed gate")
    for blk in range(5):
        if bool((deltas[2 * blk + 1][~gate[2 * blk + 1]] != 0).any()):
            bad.append(f"deltas[{2 * blk + 1}] != 0 under a closed gate")
        shut = ~gate[2 * blk]
        if not torch.equal(_bits(deltas[2 * blk])[shut], _bits(deltas[2 * blk + 2])[shut]):
            bad.append(f"deltas[{2 * blk}] is not deltas[{2 * blk + 2}] under a closed gate")
    return bad


# ---- a. the exact chain against float64: every tile edge, every d_out around the lane-half boundary -------------------------------
@pytest.mark.parametrize("points,d_out_dim", EXACT_SHAPES)
def test_exact_chain_equals_float64(dev, margins, points, d_out_dim):
    inp, ref, tw = _case("random", points, d_out_dim)
    got, again = _launch(dev, inp), _launch(dev, inp)
    assert _same_bits(got["deltas"], again["deltas"]) and _same_bits(got["sums"], again["sums"])      # bit-reproducible
    bad = _compare_exact(margins, f"resnetfc_backward exact P={points} D={d_out_dim}", got, inp, ref, tw)
    bad += _closed_gate_failures(got["deltas"], R.gates(inp["act"]))
    assert not bad, (points, d_out_dim, bad)


@pytest.mark.parametrize("points", STRESS_POINTS)
@pytest.mark.parametrize("family", ["decades", "gates", "sign_edges"])
def test_exact_chain_on_stress_inputs(dev, margins, family, points):
    """Per-point gradient magnitudes over 8 decades; points with every gate shut / only the last layer's open / every gate open at
    the first and last lane of a tile and in the ragged last tile; activations at the edges of the sign test."""
    inp, ref, tw = _case(family, points, 24)
    got, again = _launch(dev, inp), _launch(dev, inp)
    assert _same_bits(got["deltas"], again["deltas"]) and _same_bits(got["sums"], again["sums"])
    bad = _compare_exact(margins, f"resnetfc_backward exact stress={family} P={points} D=24", got, inp, ref, tw)
    gate = R.gates(inp["act"])
    bad += _closed_gate_failures(got["deltas"], gate)
    if family == "gates":
        rows = R.gate_rows(points)
        d = got["deltas"]
        assert float(d[:, rows["closed"]].abs().max()) == 0.0
        for blk in range(5):                                # closed and passing points: five blocks leave the stream untouched
            for name in ("closed", "passing"):
                assert _same_bits(d[2 * blk][rows[name]], d[2 * blk + 2][rows[name]]), (blk, name)
                assert float(d[2 * blk + 1][rows[name]].abs().max()) == 0.0, (blk, name)
        assert float(d[0][rows["passing"]].abs().max()) > 0.0 and _same_bits(d[0][rows["passing"]], d[10][rows["passing"]])
        assert bool((d[:, rows["open"]] != 0).all())
    assert not bad, (family, points, bad)


@pytest.mark.parametrize("points,d_out_dim", [(33, d) for d in D_OUT] + [(RAGGED, 17), (RAGGED, 32)])
def test_onehot_d_out_reads_one_row_of_lin_out(dev, points, d_out_dim):
    """d_out = e_d on one point: deltas[10] of that point is row d of lin_out.weight under the mask, bit for bit (1 x w plus zeros is
    exact), every other point is exactly zero in all 11 slices -- the packed layout of lin_out^T for every column, d >= 16 included."""
    w = None
    for d in range(d_out_dim):
        inp = R.inputs("onehot", points, d_out_dim, hot=d)
        w = _pack(dev, inp["params"], "f32") if w is None else w          # (the weights depend on (seed, d_out_dim) only)
        got = _launch(dev, inp, w=w)
        hot = R.onehot_point(points, d)
        want = torch.where(inp["act"][10, hot] > 0, inp["params"]["lin_out.weight"][d], torch.zeros(()))
        assert float(want.abs().max()) > 0.0
        assert _same_bits(got["deltas"][10, hot], want), (d, hot)
        others = torch.arange(points) != hot
        assert float(got["deltas"][:, others].abs().max()) == 0.0, d
        assert _same_bits(got["sums"][10], want), d                        # (a column sum of one non-zero row is that row)


# ---- b. the act route and the mask route are one function -----------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("points", POINTS)
def test_mask_route_is_the_act_route(dev, precision, points):
    inp, _, _ = _case("random", points, 24)
    via_act = _launch(dev, inp, "act", precision)
    via_mask = _launch(dev, inp, "mask", precision)
    assert _same_bits(via_mask["deltas"], via_act["deltas"]) and _same_bits(via_mask["sums"], via_act["sums"])
    blind = _launch(dev, inp, "mask", precision, act=torch.full_like(inp["act"], float("nan")))      # the chain must not read act
    assert _same_bits(blind["deltas"], via_act["deltas"]) and _same_bits(blind["sums"], via_act["sums"])


@pytest.mark.parametrize("route", ["act", "mask"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("points", STRESS_POINTS)
def test_sign_edges_decide_like_float64(dev, precision, route, points):
    """+0.0, -0.0, an fp32 denormal, the smallest normal fp32, a value that is zero as fp16, 1.0: both sign tests (a > 0.f on the value;
    the bit taken from pack_mask, which follows the integer clamp of the forward's dump) decide as float64 does, element for element
    -- a closed gate is an exact 0 / an exact pass-through of the residual, an open gate lets a non-zero gradient through."""
    inp, ref, _ = _case("sign_edges", points, 24)
    gate = R.gates(inp["act"])
    got = _launch(dev, inp, route, precision)
    bad = _closed_gate_failures(got["deltas"], gate)
    for l in (1, 3, 5, 7, 9, 10):
        should = gate[l] & (ref["deltas"][l] != 0)
        if bool((got["deltas"][l][should] == 0).any()):
            bad.append(f"deltas[{l}] == 0 under an open gate")
    for blk in range(5):
        # even slices: an open gate adds a term t to the residual.  Where |t| > 2^-20 |residual| (fp32 cannot absorb it: that takes
        # |t| < 2^-24 |residual|) and |t| > 1e-3 max|t| (either product form has t within 2e-5 max|t|, section d), the sum must move
        term = ref["deltas"][2 * blk] - ref["deltas"][2 * blk + 2]
        should = gate[2 * blk] & (term.abs() > 2.0 ** -20 * ref["deltas"][2 * blk + 2].abs()) & (term.abs() > 1e-3 * term.abs().max())
        assert float(should.double().mean()) > 0.3
        if bool((_bits(got["deltas"][2 * blk])[should] == _bits(got["deltas"][2 * blk + 2])[should]).any()):
            bad.append(f"deltas[{2 * blk}] is deltas[{2 * blk + 2}] under an open gate")
    base =_launch(dev, inp, "act", precision) if route == "mask" else got
    assert _same_bits(got["deltas"], base["deltas"]) and _same_bits(got["sums"], base["sums"])
    assert not bad, bad


# ---- c. fp16 storage, bit level ----------------------------------------------------------------------------------------------------------
def _expected_unscale(d_out):
    """2^-(6 - e), e from math.frexp of the host-side max|d_out| (1 for max|d_out| = 0)."""
    mx = float(d_out.abs().max())
    return 2.0 ** -(6 - math.frexp(mx)[1]) if mx > 0.0 else 1.0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("points,d_out_dim", STORAGE_SHAPES)
def test_fp16_storage_is_the_rounded_fp32_storage(dev, margins, precision, points, d_out_dim):
    """latent = deltas[[0,2,4]] and sums of the fp32-storage mask route in bits; unscale the exact power of two; deltas16 = the
    round-to-nearest-even fp16 of deltas x 2^k in bits wherever that is a normal fp16, and within 2^-14 below.

    Measured on an MI355X: the hardware store KEEPS fp16 sub-normals (it does not flush them) -- every non-zero element below 2^-14
    (246 of 5.8 M at P = 4109) came out non-zero and equal to the host's sub-normal rounding, 3.0e-8 away at most."""
    inp, _, _ = _case("random", points, d_out_dim)
    full, half = _launch(dev, inp, "mask", precision), _launch(dev, inp, "mask", precision, "f16")
    assert _same_bits(half["latent"], full["deltas"][[0, 2, 4]])
    assert _same_bits(half["sums"], full["sums"])
    assert half["unscale"] == _expected_unscale(inp["d_out"]) and half["unscale"] != 1.0       # max|d_out| ~ 4e-3: k > 0
    scaled = full["deltas"] / half["unscale"]                                                  # deltas x 2^k: exact in fp32
    assert _same_bits(scaled * half["unscale"], full["deltas"]) and float(scaled.abs().max()) < 65504.0
    want = scaled.half()                                                                       # host conversion: nearest even
    normal = scaled.abs() >= FP16_MIN_NORMAL
    assert _same_bits(half["deltas16"][normal], want[normal])
    assert bool((half["deltas16"][scaled == 0] == 0).all())
    small = ~normal & (scaled != 0)
    err = float((half["deltas16"][small].double() - scaled[small].double()).abs().max()) if bool(small.any()) else 0.0
    kept = int((half["deltas16"][small] != 0).sum())
    as_host = int((_bits(half["deltas16"][small]) == _bits(want[small])).sum())
    print(f"[fp16 storage {precision} P={points} D={d_out_dim}] unscale 2^{math.frexp(half['unscale'])[1] - 1}; |deltas x 2^k| < 2^-14 "
          f"in {int(small.sum())} non-zero elements: {kept} stored non-zero, {as_host} equal to the host's sub-normal rounding, "
          f"largest distance {err:.3e}")
    margins.record(f"resnetfc_backward fp16 storage {precision} P={points} D={d_out_dim}",
                   [_row("deltas16 below 2^-14 (absolute)", err, 0.0, FP16_MIN_NORMAL)])
    assert err <= FP16_MIN_NORMAL


@pytest.mark.parametrize("precision,storage", FORMS)
def test_chain_is_exactly_linear_in_powers_of_two(dev, precision, storage):
    """d_out x 2^m leaves deltas16 unchanged in bits and multiplies latent, sums and unscale -- and the fp32-storage deltas -- by
    exactly 2^m: the 2^k bookkeeping of all four (product form x storage) combinations."""
    inp, _, _ = _case("random", RAGGED, 24)
    base = _launch(dev, inp, "mask", precision, storage)
    assert float(base["sums"].abs().max()) > 0.0
    for m in (-40, -3, 20):
        f = 2.0 ** m
        got = _launch(dev, inp, "mask", precision, storage, d_out=inp["d_out"] * f)
        assert _same_bits(got["sums"], base["sums"] * f), m
        if storage == "f16":
            assert math.frexp(got["unscale"])[0] == 0.5 and got["unscale"] == base["unscale"] * f, (m, got["unscale"].hex())
            assert _same_bits(got["deltas16"], base["deltas16"]), m
            assert _same_bits(got["latent"], base["latent"] * f), m
        else:
            assert _same_bits(got["deltas"], base["deltas"] * f), m


@pytest.mark.parametrize("precision,storage", FORMS)
def test_zero_d_out_gives_exact_zeros(dev, precision, storage):
    inp, _, _ = _case("random", RAGGED, 24)
    got = _launch(dev, inp, "mask", precision, storage, d_out=torch.zeros_like(inp["d_out"]))
    for k in ("deltas", "latent", "deltas16", "sums"):
        assert k not in got or bool((got[k] == 0).all()), k
    assert storage == "f32" or got["unscale"] == 1.0


# ---- d. the f16x2 chain ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("points,d_out_dim", SPLIT_SHAPES)
@pytest.mark.parametrize("family", ["random", "decades"])
def test_f16x2_chain_against_the_exact_chain(dev, margins, family, points, d_out_dim):
    """Every deltas slice and every colsum row within 2e-5 of the exact chain's on the same inputs; the ratio of its float64 error to
    the exact chain's is recorded."""
    inp, ref, _ = _case(family, points, d_out_dim)
    exact, split = _launch(dev, inp, "act", "f32"), _launch(dev, inp, "act", "f16x2")
    rows, bad = [], []
    pairs = [(f"deltas[{l}]", split["deltas"][l], exact["deltas"][l], ref["deltas"][l]) for l in range(11)]
    pairs += [(f"sums[{l}]", split["sums"][l], exact["sums"][l], ref["sums"][l]) for l in range(11)]
    for key, g, e, r in pairs:
        assert torch.isfinite(g).all(), key
        err, err64, exact64 = R.rel(g, e), R.rel(g, r), R.rel(e, r)
        rows.append(_row(key, err, exact64, SPLIT_LIMIT, err_f64=float(f"{err64:.3e}"),
                         ratio_to_exact_chain_f64_error=float(f"{err64 / exact64:.3e}") if exact64 > 0 else None))
        if not err < SPLIT_LIMIT:
            rows[-1]["ok"] = False
            bad.append((key, f"{err:.3e}"))
    case = f"resnetfc_backward f16x2 {family} P={points} D={d_out_dim}"
    worst = max(rows, key=lambda r: r["err"])
    ratios = [r["ratio_to_exact_chain_f64_error"] for r in rows if r["ratio_to_exact_chain_f64_error"] is not None]
    print(f"[{case}] worst vs exact chain: {worst['key']} {worst['err']:.2e} (limit {SPLIT_LIMIT:.0e}); its f64 error is "
          f"{worst['err_f64']:.2e}; f64 error / exact chain's f64 error: up to {max(ratios, default=0.0):.1f}x")
    margins.record(case, rows)
    assert not bad, (case, bad)


# ---- e. the wrapper with fp16 storage ---------------------------------------------------------------------------------------------------
def test_wrapper_with_fp16_storage_equals_float64_autograd(dev, margins):
    """training.resnetfc_backward with fp16 activations and the masks -- pack, launch, fp16 x fp16 weight-gradient GEMMs, footprint
    scatter, lin_z / lin_in GEMMs, d_feats -- on real float64 forward activations against float64 autograd through the whole net,
    lin_z on bilinear footprints of a feature map included."""
    from neural_jacobian_field_amd import synthetic, training
    points, d_out_dim, texels = 257, 16, 23
    p32 = synthetic.seeded_state_dict(synthetic.resnet_fc_shapes("", 63, 512, d_out_dim), seed=3)
    g = torch.Generator().manual_seed(50)
    pe = torch.randn(points, 64, generator=g)
    pe[:, 63] = 1.0                                                                 # the bias slot of lin_in
    feats = torch.randn(texels, 512, generator=g)
    foot_idx = torch.randint(0, texels, (points, 4), generator=g, dtype=torch.int64)
    foot_w = torch.rand(points, 4, generator=g)
    d_out = torch.randn(points, d_out_dim, generator=g)
    slot = torch.tensor(training._PE_SLOT_TO_CHANNEL)

    def autograd(dtype):
        leaves = {k: v.to(dtype).requires_grad_(True) for k, v in p32.items()}
        f = feats.to(dtype).requires_grad_(True)
        x = torch.zeros(points, 63, dtype=dtype)
        x[:, slot] = pe[:, :63].to(dtype)
        pix = (foot_w.to(dtype)[:, :, None] * f[foot_idx]).sum(1)
        latents = torch.stack([pix @ leaves[f"lin_z.{b}.weight"].t() + leaves[f"lin_z.{b}.bias"] for b in range(3)])
        fw = R.forward(leaves, x, latents)
        grads = torch.autograd.grad(fw["out"], list(leaves.values()) + [f], d_out.to(dtype))
        return fw["act"].detach(), dict(zip(list(leaves) + ["d_feats"], grads))

    act64, ref = autograd(torch.float64)
    _, floor32 = autograd(torch.float32)
    act = act64.float()
    before = training._BACKWARD_PRECISION
    training.set_backward_precision("f32")
    try:
        d_feats = torch.zeros(texels, 512, device=dev)
        grads = training.resnetfc_backward({k: v.to(dev) for k, v in p32.items()}, d_out.to(dev), act.half().to(dev), pe.to(dev),
                                           foot_idx.to(torch.int32).to(dev), foot_w.to(dev), feats.to(dev), d_feats,
                                           mask=R.pack_mask(act).to(dev), forward_precision="f32")
    finally:
        training.set_backward_precision(before)
    grads = dict(grads, d_feats=d_feats)
    assert set(grads) == set(ref)
    rows, bad = [], []
    for name, r in ref.items():
        got = grads[name]
        assert got.shape == r.shape and torch.isfinite(got).all(), name
        err, floor = R.rel(got, r), R.rel(floor32[name], r)
        if name == "d_feats":
            limit = _twin_limit(floor)
        elif name.endswith(".bias") or name.startswith(("lin_z.", "lin_in.")):
            limit = 1e-5                                                            # what the chain makes in fp32
        else:
            limit = 2e-3                                                            # contracted from fp16 operands
        rows.append(_row(name, err, floor, limit))
        if not rows[-1]["ok"]:
            bad.append((name, f"err {err:.3e}", f"floor {floor:.3e}", f"limit {limit:.3e}"))
    case = f"resnetfc_backward wrapper, fp16 storage P={points} D={d_out_dim}"
    for limit in (1e-5, 2e-3):
        worst = max((r for r in rows if r["limit"] == limit), key=lambda r: r["err"])
        print(f"[{case}] limit {limit:.0e}: worst {worst['key']} err {worst['err']:.2e} (twin {worst['floor']:.2e})")
    print(f"[{case}] d_feats: " + str(next(r for r in rows if r["key"] == "d_feats")))
    margins.record(case, rows)
    assert not bad, bad


# ---- f. the forward's dump is consistent -------------------------------------------------------------------------------------------------
def _captured_dumps(dev, monkeypatch, mode, storage):
    """The activation dump and the mask dump a real training forward hands to hip.render_forward (small: B = 1, 16 x 16 features,
    33 rays x 16 samples, un-jittered samplers, 'precomputed' encoder), after the launch."""
    from neural_jacobian_field_amd import hip, synthetic, training
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import CameraInput, Model, RenderingInput, RobotInput
    B, H, W, rays, S, A = 1, 32, 32, 33, 16, 8
    b = synthetic.synthetic_training_batch(B, H, W, rays, A, seed=5, device=dev)
    feats = synthetic.synthetic_features(B, H, W, seed=3).to(dev)
    assert feats.shape[-2:] == (16, 16)
    cam = CameraInput(None, b["ctxt_c2w"], b["ctxt_k_norm"], b["trgt_c2w"], b["trgt_k_pix"])
    rin = RenderingInput(b["origins"], b["directions"], b["z_near"], b["z_far"])
    rob = RobotInput(b["action"])
    seen = []
    real = hip.render_forward

    def recording(*args, **kw):
        outputs = kw["outputs"] if "outputs" in kw else args[12]
        real(*args, **kw)
        seen.append(outputs)

    monkeypatch.setattr(hip, "render_forward", recording)
    before = training._STORAGE_PRECISION
    training.set_storage_precision(storage)
    try:
        model = Model(model_cfg_from_dict({"action_dim": A, "encoder": {"name": "precomputed"},
                                           "rendering": {"num_proposal_samples": [S], "num_nerf_samples": S},
                                           "action_decoder": {"name": "jacobian_mlp"}}))
        model.load_state_dict(synthetic.seeded_state_dict(synthetic.model_shapes("jacobian_mlp", A, with_encoder=False), seed=0))
        model.to(dev).train()
        model.encoder.set_features(feats)
        if mode == "action":
            model.decoder.freeze_non_action_parameters()
            for n, p in model.named_parameters():
                if "decoder" not in n:
                    p.requires_grad = False
        for smp in (model.proposal_sampler.initial_sampler, model.proposal_sampler.pdf_sampler):
            smp.train_stratified = False
        model.step_before_iter(20000)
        model.forward(cam, rin, rob)
        torch.cuda.synchronize(dev)
    finally:
        training.set_storage_precision(before)
        monkeypatch.setattr(hip, "render_forward", real)
    key = "jac" if mode == "action" else "den"
    dumps = [o for o in seen if o.get(key + "_act") is not None]
    assert dumps, [sorted(o) for o in seen]
    # (the first forward after load_state_dict also calibrates its precision on a prefix of the rays: the last call is the forward)
    act, mask = dumps[-1][key + "_act"].cpu(), dumps[-1][key + "_mask"].cpu()
    assert act.shape == (11, B * rays * S, 128) and mask.shape == (11, B * rays * S, 4) and mask.dtype == torch.int32
    assert act.dtype == (torch.float16 if storage == "f16" else torch.float32)
    return act, mask


@pytest.mark.parametrize("mode", ["action", "perception"])
def test_forward_mask_dump_is_the_sign_of_its_activation_dump(dev, monkeypatch, mode):
    """jac_mask / den_mask against the jac_act / den_act dumped beside them: with fp32 storage the mask is pack_mask(act) in bits;
    with fp16 storage the masks are those of the fp32-storage run, the fp16 activations are the fp32 ones rounded once, a positive
    fp16 activation has its bit set and a clear bit has a zero activation."""
    act32, mask32 = _captured_dumps(dev, monkeypatch, mode, "f32")
    assert torch.isfinite(act32).all() and float(act32.min()) >= 0.0
    open32 = R.unpack_mask(mask32)
    share = float(open32.double().mean())
    assert 0.05 < share < 0.95, share
    wrong = int((open32 != (act32 > 0)).sum())
    assert torch.equal(mask32, R.pack_mask(act32)), f"{wrong} of {open32.numel()} mask bits differ from [act > 0]"
    act16, mask16 = _captured_dumps(dev, monkeypatch, mode, "f16")
    assert torch.equal(mask16, mask32)
    open16 = R.unpack_mask(mask16)
    assert bool(open16[act16 > 0].all()) and bool((act16[~open16] == 0).all())
    assert _same_bits(act16, act32.half())
    print(f"[{mode}] {open32.numel()} mask bits, {share:.3f} set; fp16 dump: {int((open16 & (act16 == 0)).sum())} set bits on a zero half")
