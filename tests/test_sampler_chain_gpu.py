"""Kernel-level tests of the sampler chain on plain tensors: njf_alpha_weights (tile_weights / alpha_of, the device functions the fused
proposal and render passes run), njf_pdf_resample (pdf_resample_ray) and njf_composite_backward (the gradient of every
perception-mode level), csrc/njf_kernels.hip.

Reference: tests/sampler_restatement.py in float64 (pinned by tests/test_sampler_chain_cpu.py); its fp32 twin is the yardstick.

Criteria (stated and justified in sampler_restatement.py; the CPU file holds the twin to half of W and C, to no failing element of
P and to a quarter of G's cap on every case used here):
* W, element-wise on the weights: |w - w64| <= (2e-6 + (8 + ceil(S/32)) 2^-24 excl64) w64 + 2^-120, exactly 0 where delta <= 0.
* P, element-wise on the resampled bins, no exceptions: |out - out64| <= 4 x 2^-24 max|bins| OR cdf_residual <= (s_in + 4) 2^-24;
  out non-decreasing along k and inside [bins[0], bins[-1]].
* G, norm-wise per ray on g_sigma: max|g - g64| / max|g64| <= min(max(4 x twin, 4 x 2^-23), 2e-5), exactly 0 where delta <= 0.
* C, element-wise on g_color = w g_rgb: W with one more 2^-24, scaled by |g_rgb|.
Every toleranced comparison is recorded through ``margins.record`` (case, key, err, floor = the twin, limit, ok): the worst element
(W, P, C) or ray (G) of each case.

Measured on an MI355X (the whole module, 36 tests = 2,298 recorded rows, runs in ~4 s).  A DEFECT WAS FOUND in
composite_backward_kernel and fixed there; njf_alpha_weights and njf_pdf_resample passed as they were.  Worst err / floor / limit,
err / limit in brackets:
* W, 240 cases (5 ray counts x 8 sample counts x 6 families): 7.8e-26 / 3.5e-26 / 2.9e-25 (0.27; mixed, R = 9, S = 32, w[3, 17]); by
  family 0.07 (fog) to 0.27 (mixed); the twin's worst is 0.13.  Two launches give the same bits.
* P, 600 cases (10 s_in x 5 s_out x 3 bin families x 4 anneals; weights, u, shared bins and rays cycling): NO failing element;
  worst min(forward, residual) / limit 0.32 (uniform bins, s_in = 2, s_out = 299, half the rays all-zero, anneal 0.5: 1.1e-7 of
  3.6e-7), the same element and figure as the twin's worst; 0.13 - 0.14 for s_in >= 63; the worst element of a case is decided by the
  forward check in 341 cases and by the CDF residual in 259.  Two launches give the same bits.  The 257-sample call is refused with
  "samples per ray must be in [1, 256]" and leaves the output untouched.
* G and C with the kernel AS IT WAS: 302 of 1,458 rows failed.
  - wall: g_sigma failed on 131 of 155 cases, worst err 9.3e-3 against a limit of 4.8e-7 (19,500 x; R = 3, S = 65, all three
    upstream gradients, ray 0: ds = 1e5 at sample 33); g_color on 64 of 80, worst 1.5e-3 of the wall's own weight (4,625 x its
    limit); the backward's weight disagreed with the forward's on 7 of 8 cases, by up to 2,043 x twice criterion W.  Cause: the depth
    in front of a sample formed as `inclusive scan - ds`.
  - mixed 45, gaps 47 (+ 2 of g_color), opaque 6 cases of g_sigma, worst err 4.09 (mixed, R = 4, S = 64, g_rgb only, the ray that
    turns opaque).  Cause, beside the one above (ds up to 50 x the depth in front also occurs there): the suffix sums formed as
    `tile sum - inclusive prefix`, which leaves 2^-24 of the tile's sum in gradients that are exp(-16) small.
  With the shifted scan and a suffix scan from the far end of the tile, still in fp32, 2 rows were left: g_sigma of gaps, R = 1,
  S = 128, g_rgb, 8.4e-7 / 1.6e-7 / 6.6e-7 (1.28) -- a ray on which G_k T_{k+1} - sum cancels 10 x, so that an ulp in each factor
  is 6e-7 of the result with no step at fault (an fp32 emulation of the kernel on the CPU gives 4.8e-7 there, accurate alpha or not).
  The kernel's arithmetic is float64 on the fp32 inputs now, rounded at the store.
* G and C with the kernel as it is: g_sigma, 930 cases: 5.8e-8 / 5.8e-8 / 4.8e-7 (0.12; gaps, R = 4, S = 63, g_rgb, ray 3), every
  family between 5.5e-8 and 5.8e-8 -- the rounding of the store -- where the twin has up to 2.4e-6; wall: 5.6e-8 / 6.9e-8 /
  4.8e-7 (before: 9.3e-3).  g_color, 480 cases: 0.029 of its limit in every family (wall: 4.4e-16 of 1.5e-14; before: 4,625 x).
  The backward's weight against the forward's, 48 cases: 0.14 of twice W (mixed, S = 129), wall 0.08 (before: 2,043 x).  Two launches
  give the same bits; 1,025 samples are refused (code -4).
(For W and C ``floor`` is the err of the twin's own worst element, for G the twin's err on the same ray.)
tests/test_training_gpu.py::test_composite_backward_equals_autograd and the training-gradient tests pass with their bounds unchanged.

Run with -m gpu."""
import os
import re

import pytest
import torch

import sampler_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "neural-jacobian-field_amd", "csrc", "njf_device.h")) as _f:
    WAVES = int(re.search(r"^#define NJF_WAVES (\d+)", _f.read(), re.M).group(1))     # rays per workgroup of the resampler
RESAMPLE_RAYS = R.resample_rays(WAVES)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import hip
    assert hip.load_library().njf_rays_per_workgroup() == WAVES
    return torch.device("cuda:0")


_cache = {}


def _weight_case(family, rays, samples):
    """The inputs of one case, made once and shared by the tests that use it (never modified)."""
    key = (family, rays, samples)
    if key not in _cache:
        _cache[key] = R.weight_inputs(family, rays, samples)
    return _cache[key]


def _gradient_case(family, rays, samples, use):
    """(inputs, float64 gradients, fp32 twin) of one compositing case, computed once."""
    key = (family, rays, samples, use)
    if key not in _cache:
        inp = _weight_case(family, rays, samples)
        kw = R.upstream(inp, use)
        _cache[key] = (inp, R.composite64(inp["deltas"], inp["sigma"], **kw), R.composite32(inp["deltas"], inp["sigma"], **kw))
    return _cache[key]


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _alpha_weights(dev, inp):
    from neural_jacobian_field_amd import hip
    out = torch.full(inp["deltas"].shape, float("nan"), device=dev)
    hip.alpha_weights(inp["deltas"].to(dev), inp["sigma"].to(dev), out)
    torch.cuda.synchronize(dev)
    return out.cpu()


def _resample(dev, inp, s_out, anneal):
    from neural_jacobian_field_amd import hip
    out = torch.full((inp["weights"].shape[0], s_out + 1), float("nan"), device=dev)
    hip.pdf_resample(inp["weights"].to(dev), inp["bins"].to(dev), inp["u"].to(dev), s_out, anneal, out)
    torch.cuda.synchronize(dev)
    return out.cpu()


def _composite_backward(dev, inp, use, color=None, g_rgb=None):
    from neural_jacobian_field_amd import hip
    to = lambda t: t.contiguous().to(dev)
    color = inp["color"] if color is None else color
    g_rgb = inp["g_rgb"] if g_rgb is None else g_rgb
    g_sigma, g_color = hip.composite_backward(to(inp["deltas"]), to(inp["steps"]) if use[2] else None, to(inp["sigma"]),
                                              to(color) if use[1] else None, to(inp["g_w"]) if use[0] else None,
                                              to(g_rgb) if use[1] else None, to(inp["g_depth"]) if use[2] else None)
    torch.cuda.synchronize(dev)
    assert g_sigma.shape == inp["deltas"].shape and (g_color is None) == (not use[1])
    return g_sigma.cpu(), None if g_color is None else g_color.cpu()


def _summary(tag, rows):
    worst = max(rows, key=lambda r: r["err_over_limit"])
    print(f"[{tag}] {len(rows)} cases; worst err / floor / limit = {worst['err']:.2e} / {worst['floor']:.2e} / {worst['limit']:.2e} "
          f"({worst['err_over_limit']:.2f} of its limit; twin {worst['twin_err_over_limit']:.2f}) in {worst['case']}: {worst['key']}")


# ---- njf_alpha_weights ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", R.WEIGHT_SAMPLES)
def test_alpha_weights_meet_criterion_w(dev, margins, samples):
    rows, bad = [], []
    for family in R.WEIGHT_FAMILIES:
        for rays in R.RAYS:
            inp = _weight_case(family, rays, samples)
            d, s = inp["deltas"], inp["sigma"]
            w, again = _alpha_weights(dev, inp), _alpha_weights(dev, inp)
            assert _same_bits(w, again), (family, rays, samples)                         # bit-reproducible
            got, twin = R.check_w(w, d, s), R.check_w(R.weights32(d, s)[0], d, s)
            case = f"sampler chain alpha_weights {family} R={rays} S={samples}"
            rows.append({"case": case, **R.row("w", got, twin)})
            margins.record(case, [R.row("w", got, twin)])
            if not got["ok"]:
                bad.append((family, rays, got))
    _summary(f"alpha_weights S={samples}", rows)
    for family in R.WEIGHT_FAMILIES:
        _summary(f"alpha_weights S={samples} {family}", [r for r in rows if f" {family} " in r["case"]])
    assert not bad, bad


# ---- njf_pdf_resample -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s_in", R.S_IN)
def test_pdf_resample_meets_criterion_p(dev, margins, s_in):
    rows, bad = [], []
    for case_ in R.resample_cases(s_in, RESAMPLE_RAYS):
        family, rays, _, s_out, kind, jitter, shared, anneal = case_
        inp = R.resample_inputs(family, rays, s_in, s_out, kind, jitter, shared)
        w, b, u = inp["weights"], inp["bins"], inp["u"]
        out, again = _resample(dev, inp, s_out, anneal), _resample(dev, inp, s_out, anneal)
        assert _same_bits(out, again), case_
        got, twin = R.check_p(out, w, anneal, b, u), R.check_p(R.resample32(w, anneal, b, u), w, anneal, b, u)
        case = (f"sampler chain pdf_resample {family} R={rays} s_in={s_in} s_out={s_out} weights={kind} "
                f"u={'jittered' if jitter else 'mid-points'} bins={'shared' if shared else 'per-ray'} anneal={anneal:.4g}")
        row = R.p_row(f"bins_out at {got['at']}", got, twin)
        rows.append({"case": case, **row})
        margins.record(case, [row])
        if not got["ok"]:
            bad.append((case_, got))
    _summary(f"pdf_resample s_in={s_in}", rows)
    print(f"[pdf_resample s_in={s_in}] decided by the forward check in {sum(r['check'] == 'forward' for r in rows)} of {len(rows)} worst elements")
    assert not bad, bad


def test_pdf_resample_refuses_257_input_samples(dev):
    from neural_jacobian_field_amd import hip
    w, bins, u = torch.rand(3, 257, device=dev), torch.linspace(0, 1, 258, device=dev), R.midpoint_u(64).to(dev)
    out = torch.full((3, 65), -7.0, device=dev)
    with pytest.raises(ValueError, match=r"samples per ray must be in \[1, 256\]"):
        hip.pdf_resample(w, bins, u, 64, 1.0, out)
    torch.cuda.synchronize(dev)
    assert bool((out == -7.0).all())                                                 # refused before any launch
    hip.pdf_resample(w[:, :256].contiguous(), bins[:257].contiguous(), u, 64, 1.0, out)
    torch.cuda.synchronize(dev)
    assert bool(((out >= 0) & (out <= 1)).all())


# ---- njf_composite_backward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", R.COMPOSITE_SAMPLES)
def test_composite_backward_meets_criteria_g_and_c(dev, margins, samples):
    rows, bad = [], []
    for family in R.WEIGHT_FAMILIES:
        for rays in R.RAYS:
            for use in R.UPSTREAM:
                if samples == 1 and use == (False, False, True):
                    continue   # the depth of a one-sample ray is its t: no gradient above fp32 resolution (test_composite_backward_equals_autograd)
                inp, r64, r32 = _gradient_case(family, rays, samples, use)
                d, s = inp["deltas"], inp["sigma"]
                (g_sigma, g_color), again = _composite_backward(dev, inp, use), _composite_backward(dev, inp, use)
                assert _same_bits(g_sigma, again[0]) and (g_color is None or _same_bits(g_color, again[1])), (family, rays, use)
                name = "+".join(n for n, on in zip(("g_w", "g_rgb", "g_depth"), use) if on)
                case = f"sampler chain composite_backward {family} R={rays} S={samples} upstream={name}"
                g = R.check_g(g_sigma, r64["g_sigma"], r32["g_sigma"], d)
                g_twin = {"ratio": g["floor"] / g["limit"], "err": g["floor"]}
                case_rows = [R.row("g_sigma, ray", g, g_twin)]
                if use[1]:
                    c, c_twin = R.check_c(g_color, d, s, inp["g_rgb"]), R.check_c(r32["g_color"], d, s, inp["g_rgb"])
                    case_rows.append(R.row("g_color", c, c_twin))
                    if not c["ok"]:
                        bad.append((family, rays, use, "C", c))
                if not g["ok"]:
                    bad.append((family, rays, use, "G", g))
                margins.record(case, case_rows)
                rows += [{"case": case, **r} for r in case_rows]
    for family in R.WEIGHT_FAMILIES:
        for crit in ("g_sigma", "g_color"):
            _summary(f"composite_backward S={samples} {family} {crit}", [r for r in rows if f" {family} " in r["case"] and r["key"].startswith(crit)])
    assert not bad, bad


def test_composite_backward_refuses_1025_samples(dev):
    from neural_jacobian_field_amd import hip
    deltas, sigma, g_w = (torch.rand(3, 1025, device=dev) for _ in range(3))
    with pytest.raises(ValueError, match=r"code -4"):
        hip.composite_backward(deltas, None, sigma, None, g_w)
    g_sigma, _ = hip.composite_backward(deltas[:, :1024].contiguous(), None, sigma[:, :1024].contiguous(), None, g_w[:, :1024].contiguous())
    torch.cuda.synchronize(dev)
    assert bool(torch.isfinite(g_sigma).all())


@pytest.mark.parametrize("samples", R.COMPOSITE_SAMPLES)
def test_backward_weights_are_the_forward_weights(dev, margins, samples):
    """g_rgb = (1, 0, 0) with colour (1, 0, 0): g_color[..., 0] is the weight the backward recomputes.  It agrees with njf_alpha_weights
    on the same inputs within twice criterion W (each side is within W of the float64 weight)."""
    rows, bad = [], []
    for family in R.WEIGHT_FAMILIES:
        inp = _weight_case(family, 9, samples)
        d, s = inp["deltas"], inp["sigma"]
        red = torch.zeros(9, samples, 3)
        red[..., 0] = 1.0
        _, g_color = _composite_backward(dev, inp, (False, True, False), color=red, g_rgb=red[:, 0].contiguous())
        forward = _alpha_weights(dev, inp)
        assert bool((g_color[..., 1:] == 0).all())
        w64, excl = R.weights64(d, s)
        err, limit = (g_color[..., 0].double() - forward.double()).abs(), 2.0 * R.w_limit(w64, excl, samples)
        i, ratio = R._worst(err, limit)
        twin_err = (R.weights32(d, s)[0].double() - w64).abs().reshape(-1)[i]
        ok = bool((err <= limit).all())
        case = f"sampler chain backward's weight vs forward's {family} R=9 S={samples}"
        row = {"key": f"w at {divmod(i, samples)}", "err": float(f"{float(err.reshape(-1)[i]):.3e}"), "floor": float(f"{float(twin_err):.3e}"),
               "limit": float(f"{float(limit.reshape(-1)[i]):.3e}"), "needs_floor": False, "ok": ok, "err_over_limit": float(f"{ratio:.3e}"),
               "twin_err_over_limit": float(f"{float(twin_err) / float(limit.reshape(-1)[i]):.3e}")}
        margins.record(case, [row])
        rows.append({"case": case, **row})
        if not ok:
            bad.append((family, row))
    _summary(f"backward's weight vs forward's S={samples}", rows)
    assert not bad, bad
