"""Pins tests/sampler_restatement.py -- the float64 reference, the fp32 twin, the input families and the criteria W, P, G and C that
tests/test_sampler_chain_gpu.py holds njf_alpha_weights, njf_pdf_resample and njf_composite_backward to -- without a GPU:

* ``weights64`` is the oracle's ``alpha_weights`` run in float64; ``resample64`` is the oracle's ``pdf_resample`` run in float64 (and a
  hand-written bisection for per-ray bins and jittered u); ``composite64`` is ``torch.autograd.grad`` through
  ``Model._weights_from_density`` + rgb + the un-clipped depth in float64;
* the fp32 twins stay under their caps on EVERY family and shape the GPU file uses: W and C at most half their limit, P without a
  failing element, the twin of G at most a quarter of G's cap -- so a GPU failure is the kernel's;
* the families are what they claim to be;
* the criteria decide: deliberately wrong variants of each statement fail them.

One variant the criteria cannot fail, because it is not wrong: ``searchsorted(right=False)``.  The 0.01 padding makes the CDF strictly
increasing, so the side only matters where u equals a CDF value, and there the inverse CDF is continuous: both sides give the same
position, on coincident bin edges too (t = 1 in the bin below, t = 0 in the bin above, the same edge).  The test states that.
"""
import bisect
import math
import os
import re

import pytest
import torch

import sampler_restatement as R

TWIN_CAP_W = 0.5                      # of the limit of W and C
TWIN_CAP_G = R.G_CAP / R.G_FACTOR     # the GPU tests hold g_sigma to 4 x the twin's error and state that no such limit exceeds 2e-5
ALL_SAMPLES = sorted(set(R.WEIGHT_SAMPLES + R.COMPOSITE_SAMPLES))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "neural-jacobian-field_amd", "csrc", "njf_device.h")) as _f:
    WAVES = int(re.search(r"^#define NJF_WAVES (\d+)", _f.read(), re.M).group(1))
RESAMPLE_RAYS = R.resample_rays(WAVES)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


# ---- the restatement against the oracle and autograd ----------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.WEIGHT_FAMILIES)
def test_weights64_is_the_oracle_in_float64(family):
    """To 1e-13 relative, element by element -- beside the quantum of the oracle's own alpha: it forms 1 - exp(-ds), which in float64 is a
    multiple of 2^-53 whatever its size (1e-11 of a fog weight of 1e-5; the cancellation alpha_of exists for, 2^29 times smaller)."""
    import njf_oracle as orc
    worst = 0.0
    for rays, samples in ((3, 1), (4, 33), (5, 257)):
        inp = R.weight_inputs(family, rays, samples)
        w64, excl = R.weights64(inp["deltas"], inp["sigma"])
        ref = orc.alpha_weights(inp["deltas"].double()[..., None], inp["sigma"].double()[..., None])[..., 0]
        assert ref.dtype == torch.float64 and w64.dtype == torch.float64 and excl.shape == w64.shape
        over = ((w64 - ref).abs() - 2.0 ** -53 * torch.exp(-excl)).clamp_min(0) / ref.abs().clamp_min(1e-300)
        worst = max(worst, float(over.max()))
        assert torch.equal(excl[:, 0], torch.zeros(rays, dtype=torch.float64))
        assert bool((excl[:, 1:] >= excl[:, :-1]).all())
        assert bool((w64[inp["deltas"] <= 0] == 0).all())
    print(f"{family}: weights64 vs oracle in float64 {worst:.2e}")
    assert worst <= 1e-13


def _oracle_resample64(weights_, anneal, bins, s_out):
    """oracle.pdf_resample with training=False, everything in float64 (its u included) -> (bins_out, the u it used)."""
    import njf_oracle as orc
    rays = weights_.shape[0]
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        o, d = torch.zeros(rays, 3), torch.zeros(rays, 3)
        d[:, 2] = 1
        prev = orc._samples_from_bins(o, d, torch.full((rays, 1), 0.5), torch.full((rays, 1), 10.0), bins.double())
        annealed = torch.pow(weights_.double(), R.as_fp32(anneal))                     # (proposal_sampling: pow before the sampler)
        ref = orc.pdf_resample(prev, annealed[..., None], s_out)
        nb = s_out + 1
        u = torch.linspace(0.0, 1.0 - (1.0 / nb), steps=nb) + 1.0 / (2 * nb)
    finally:
        torch.set_default_dtype(before)
    return torch.cat([ref.spacing_starts[..., 0], ref.spacing_ends[..., -1:, 0]], -1), u


@pytest.mark.parametrize("anneal", R.ANNEALS)
@pytest.mark.parametrize("kind", R.WEIGHT_KINDS)
def test_resample64_is_the_oracle_in_float64(kind, anneal):
    worst = 0.0
    for rays, s_in, s_out in ((3, 1, 5), (4, 65, 64), (5, 256, 299), (9, 128, 1)):
        inp = R.resample_inputs("random", rays, s_in, s_out, kind, False, False)
        ref, u64 = _oracle_resample64(inp["weights"], anneal, inp["bins"], s_out)
        assert ref.dtype == torch.float64 and u64.dtype == torch.float64
        got = R.resample64(inp["weights"], anneal, inp["bins"], u64)
        assert got.shape == ref.shape == (rays, s_out + 1)
        worst = max(worst, float((got - ref).abs().max()))
        # F64(out64) is u, up to the float64 rounding of a position times the slope of the CDF (random bins get as narrow as 1e-6)
        assert float(R.cdf_residual(got, inp["weights"], anneal, inp["bins"], u64).max()) <= 1e-10
    assert worst <= 1e-15, worst


def _by_hand(weights_, anneal, bins, u):
    """PDFSampler one ray and one u at a time, in Python floats (float64) with a bisection."""
    out = []
    for r in range(weights_.shape[0]):
        w = [float(x) ** R.as_fp32(anneal) + 0.01 for x in weights_[r].tolist()]
        total = math.fsum(w)
        pad = max(1e-5 - total, 0.0)
        w, total = [x + pad / len(w) for x in w], total + pad
        c, acc = [0.0], 0.0
        for x in w:
            acc += x / total
            c.append(min(1.0, acc))
        b = (bins if bins.dim() == 1 else bins[r]).tolist()
        row = []
        for uk in (u if u.dim() == 1 else u[r]).tolist():
            i = bisect.bisect_right(c, uk)
            lo, hi = min(max(i - 1, 0), len(w)), min(max(i, 0), len(w))
            t = (uk - c[lo]) / (c[hi] - c[lo]) if c[hi] != c[lo] else 0.0
            row.append(b[lo] + min(max(t, 0.0), 1.0) * (b[hi] - b[lo]))
        out.append(row)
    return torch.tensor(out, dtype=torch.float64)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("family", R.BIN_FAMILIES)
def test_resample64_with_per_ray_jitter_is_the_hand_written_sampler(family, shared):
    for i, (rays, s_in, s_out) in enumerate(((4, 5, 7), (3, 65, 33), (2, 129, 64))):
        inp = R.resample_inputs(family, rays, s_in, s_out, R.WEIGHT_KINDS[i], True, shared)
        assert inp["u"].shape == (rays, s_out + 1) and inp["bins"].dim() == (1 if shared else 2)
        for anneal in R.ANNEALS:
            got, want = R.resample64(inp["weights"], anneal, inp["bins"], inp["u"]), _by_hand(inp["weights"], anneal, inp["bins"], inp["u"])
            # (math.fsum and torch's pairwise sum differ in the last bits of the total: 1e-13 of a position in [0, 1])
            assert float((got - want).abs().max()) <= 1e-13, (family, shared, anneal)


@pytest.mark.parametrize("family", R.WEIGHT_FAMILIES)
def test_composite64_is_autograd_of_the_forward(family):
    """To 1e-12 of each tensor's largest element -- beside the one defect of the float64 autograd itself: torch differentiates
    expm1 as ``result + 1``, so d alpha_k / d ds_k = exp(-ds_k) comes with an absolute error of 2^-53 (it is exactly 0 behind
    ds = 50), which enters dL/dsigma_k as delta_k G_k T_k times that.  Visible only where nothing else is left: one-sample rays."""
    from neural_jacobian_field_amd.model import Model
    worst = 0.0
    for rays, samples in ((3, 1), (5, 65), (4, 200)):
        inp = R.weight_inputs(family, rays, samples)
        for use in R.UPSTREAM:
            s64 = inp["sigma"].double()[..., None].requires_grad_(True)
            c64 = inp["color"].double().requires_grad_(True)
            w = Model._weights_from_density(inp["deltas"].double()[..., None], s64)
            loss = torch.zeros((), dtype=torch.float64) * s64.sum() + 0.0 * c64.sum()
            if use[0]:
                loss = loss + (w[..., 0] * inp["g_w"].double()).sum()
            if use[1]:
                loss = loss + ((w * c64).sum(-2) * inp["g_rgb"].double()).sum()
            if use[2]:
                t = inp["steps"].double()[..., None]
                loss = loss + (((w * t).sum(-2) / (w.sum(-2) + 1e-10))[..., 0] * inp["g_depth"].double()).sum()
            g_s, g_c = torch.autograd.grad(loss, [s64, c64])
            g_s = g_s[..., 0]
            got = R.composite64(inp["deltas"], inp["sigma"], **R.upstream(inp, use))
            assert torch.equal(got["w"], w.detach()[..., 0])
            expm1_backward = 2.0 ** -52 * (inp["deltas"].double() * got["G"]).abs() * torch.exp(-got["excl"])
            over = ((got["g_sigma"] - g_s).abs() - expm1_backward).clamp_min(0)
            worst = max(worst, float(over.max() / g_s.abs().max().clamp_min(1e-300)))
            assert bool((got["g_sigma"][inp["deltas"] <= 0] == 0).all())
            if use[1]:
                worst = max(worst, rel(got["g_color"], g_c))
            else:
                assert got["g_color"] is None and float(g_c.abs().max()) == 0.0
    print(f"{family}: composite64 vs float64 autograd {worst:.2e}")
    assert worst <= 1e-12


# ---- the twins stay under their caps on everything the GPU file uses ---------------------------------------------------------------------
@pytest.mark.parametrize("family", R.WEIGHT_FAMILIES)
def test_weight_and_gradient_twins_stay_under_their_caps(family):
    worst = {"W": 0.0, "C": 0.0, "G": 0.0}
    for samples in ALL_SAMPLES:
        for rays in R.RAYS:
            inp = R.weight_inputs(family, rays, samples)
            d, s = inp["deltas"], inp["sigma"]
            w = R.check_w(R.weights32(d, s)[0], d, s)
            assert w["ok"] and w["ratio"] <= TWIN_CAP_W, (family, rays, samples, w)
            worst["W"] = max(worst["W"], w["ratio"])
            for use in R.UPSTREAM:
                if samples == 1 and use == (False, False, True):
                    continue
                kw = R.upstream(inp, use)
                r64, r32 = R.composite64(d, s, **kw), R.composite32(d, s, **kw)
                floor = float(R.ray_rel(r32["g_sigma"], r64["g_sigma"]).max())
                assert floor <= TWIN_CAP_G, (family, rays, samples, use, floor)
                assert bool((r32["g_sigma"][d <= 0] == 0).all())
                worst["G"] = max(worst["G"], floor)
                if use[1]:
                    c = R.check_c(r32["g_color"], d, s, inp["g_rgb"])
                    assert c["ok"] and c["ratio"] <= TWIN_CAP_W, (family, rays, samples, use, c)
                    worst["C"] = max(worst["C"], c["ratio"])
    print(f"{family}: twin W {worst['W']:.2f} and C {worst['C']:.2f} of their limits; twin of G {worst['G']:.2e} (cap {TWIN_CAP_G:.1e})")


@pytest.mark.parametrize("s_in", R.S_IN)
def test_resampler_twin_fails_no_element(s_in):
    worst, seen = 0.0, set()
    for case in R.resample_cases(s_in, RESAMPLE_RAYS):
        family, rays, _, s_out, kind, jitter, shared, anneal = case
        inp = R.resample_inputs(family, rays, s_in, s_out, kind, jitter, shared)
        p = R.check_p(R.resample32(inp["weights"], anneal, inp["bins"], inp["u"]), inp["weights"], anneal, inp["bins"], inp["u"])
        assert p["ok"] and p["failing"] == 0, (case, p)
        worst = max(worst, p["ratio"])
        seen.add((kind, jitter, shared))
    assert len(seen) == 12                                                          # every weight kind x kind of u x kind of bins
    print(f"s_in = {s_in}: twin's worst min(forward / limit, residual / limit) = {worst:.2f}")


def test_the_resampler_cases_cover_every_choice():
    cases = [c for s_in in R.S_IN for c in R.resample_cases(s_in, RESAMPLE_RAYS)]
    assert len(cases) == len(set(cases)) == len(R.S_IN) * len(R.S_OUT) * len(R.BIN_FAMILIES) * len(R.ANNEALS)
    for a, b, na, nb in ((1, 2, 5, 10), (1, 3, 5, 5), (1, 7, 5, 4), (2, 7, 10, 4), (3, 7, 5, 4), (0, 4, 3, 3), (0, 7, 3, 4), (4, 7, 3, 4),
                         (5, 7, 2, 4), (6, 7, 2, 4), (4, 5, 3, 2), (4, 6, 3, 2), (5, 6, 2, 2), (1, 4, 5, 3), (2, 4, 10, 3), (2, 5, 10, 2),
                         (2, 6, 10, 2)):
        assert len({(c[a], c[b]) for c in cases}) == na * nb, (a, b)                # every pair of choices occurs


# ---- the families are what they claim --------------------------------------------------------------------------------------------------
def test_weight_families_are_what_they_claim():
    vals = R.switch_values()
    assert vals[2] == 0.0625 and vals[1] < 0.0625 < vals[3] and vals[1] == 0.0625 - 2.0 ** -28 and vals[3] == 0.0625 + 2.0 ** -27
    for rays in R.RAYS:
        for samples in ALL_SAMPLES:
            sw = R.weight_inputs("switch", rays, samples)
            ds = sw["deltas"] * sw["sigma"]
            assert set(ds.reshape(-1).tolist()) <= set(vals)
            if rays * samples >= 5:
                assert set(ds.reshape(-1).tolist()) == set(vals)                        # the three values and a neighbour on each side
            fog = R.weight_inputs("fog", rays, samples)
            ds = fog["deltas"].double() * fog["sigma"].double()
            assert 0.9e-8 <= float(ds.min()) and float(ds.max()) <= 1.01e-2 < R.SWITCH
            wall = R.weight_inputs("wall", rays, samples)
            ds = wall["deltas"].double() * wall["sigma"].double()
            for r in range(rays):
                p = R.wall_position(r, samples)
                assert float(ds[r, p]) == R.wall_ds(r, samples) and float(ds[r, :p].sum()) <= 1.0
                behind = ds[r, p + 1:]
                assert behind.numel() > 0 or samples == 1                               # more samples follow the wall
                assert behind.numel() == 0 or float(behind.max()) <= 1.01e-2
            gaps = R.weight_inputs("gaps", rays, samples)
            assert bool((gaps["deltas"][1::3] == 0).all())
            opq = R.weight_inputs("opaque", rays, samples)
            if samples >= 31:
                w64, excl = R.weights64(opq["deltas"], opq["sigma"])
                assert bool((excl[:, -1] > 87).all()) and bool((excl[:, samples // 3] < 87).all())
                assert bool(((w64 < 2.0 ** -120) & (w64 > 0)).any(-1).all())
            for family in ("mixed", "gaps", "opaque"):                                  # (see weight_inputs: the first ds is capped)
                x = R.weight_inputs(family, rays, samples)
                ds = torch.where(x["deltas"] > 0, x["deltas"] * x["sigma"], torch.zeros(()))
                for r in range(rays):
                    nz = torch.nonzero(ds[r] > 0)
                    assert nz.numel() == 0 or float(ds[r, nz[0, 0]]) <= R.FIRST_DS_CAP * (1 + 2.0 ** -22)
    # the wall sits inside a tile on ray 0 and on lanes 31 / 32 / 63 / 64 on rays 1 .. 4, with all three depths
    assert [R.wall_position(r, 1024) for r in range(5)] == [512 + 1, 31, 32, 63, 64] and [R.wall_position(r, 65) for r in range(5)] == [33, 31, 32, 63, 63]
    assert {R.wall_ds(r, 257) for r in range(9)} == set(R.WALL_DS)
    big = R.weight_inputs("gaps", 9, 257)["deltas"]
    assert bool((big == 0).any()) and bool((big < 0).any()) and bool(((big == 0) & torch.signbit(big)).any())
    mixed = R.weights64(*[R.weight_inputs("mixed", 9, 1024)[k] for k in ("deltas", "sigma")])[1]
    assert float(mixed[:, -1].min()) > 87                                              # every long mixed ray ends opaque
    assert all(float(R.weight_inputs(f, 5, 1)["g_depth"].abs().max()) == 0.0 for f in R.WEIGHT_FAMILIES)


def test_resampler_families_are_what_they_claim():
    for s_in in (4, 63, 256):
        for shared in (False, True):
            rep = R.resample_inputs("repeated", 5, s_in, 64, "alpha", True, shared)
            b = rep["bins"] if rep["bins"].dim() == 2 else rep["bins"][None]
            assert bool(((b[:, 1:] - b[:, :-1]) == 0).sum(-1).eq(2).all())              # two zero-width bins per row
            assert bool((b[:, 1:] >= b[:, :-1]).all()) and bool((b[:, 0] == 0).all()) and bool((b[:, -1] == 1).all())
            assert bool((rep["u"][:, 1:] >= rep["u"][:, :-1]).all()) and float(rep["u"].min()) >= 0.0 and float(rep["u"].max()) <= 1.0
            assert not torch.equal(rep["u"][0], rep["u"][1])
    for s_out in R.S_OUT:
        u = R.resample_inputs("random", 9, 65, s_out, "alpha", True, False)["u"]
        assert u.shape == (9, s_out + 1) and bool((u[:, 1:] >= u[:, :-1]).all())         # the jittered u is sorted
        nb = s_out + 1
        assert bool((u >= torch.arange(nb) / nb - 1e-6).all()) and bool((u <= (torch.arange(nb) + 1) / nb + 1e-6).all())
    half = R.resample_inputs("random", 9, 65, 64, "half_zero", False, False)["weights"]
    assert float(half[:5].abs().max()) == 0.0 and float(half[5:].min(-1).values.max()) >= 0.0 and bool((half[5:].sum(-1) > 0).all())
    delta = R.resample_inputs("uniform", 4, 65, 64, "delta", False, True)
    assert bool((delta["weights"].sum(-1) == 1).all()) and bool((delta["weights"].max(-1).values == 1).all()) and delta["bins"].dim() == 1
    assert R.ANNEALS[:3] == (1.0, 0.0, 0.5) and abs(R.ANNEALS[3] - 10 / 11) < 1e-15


# ---- the criteria decide: deliberately wrong variants fail ---------------------------------------------------------------------------------
def test_wrong_weights_fail_criterion_w():
    def literal_alpha(deltas, sigma):
        ds = torch.where(deltas > 0, deltas * sigma, torch.zeros(()))
        return (1.0 - torch.exp(-ds)) * torch.exp(-R._shifted(ds))

    def carry_dropped(deltas, sigma, tile=32):
        """float64 throughout, but the optical depth restarts at sample 32."""
        ds = torch.where(deltas > 0, deltas.double() * sigma.double(), torch.zeros((), dtype=torch.float64))
        excl = R._shifted(ds)
        if ds.shape[-1] > tile:
            excl[:, tile:2 * tile] -= excl[:, tile:tile + 1].clone()
        return -torch.expm1(-ds) * torch.exp(-excl)

    fog = R.weight_inputs("fog", 4, 65)
    bad = R.check_w(literal_alpha(fog["deltas"], fog["sigma"]), fog["deltas"], fog["sigma"])
    assert not bad["ok"] and bad["ratio"] > 1e3, bad
    for family in ("mixed", "fog", "switch", "opaque", "gaps"):
        x = R.weight_inputs(family, 4, 65)
        bad = R.check_w(carry_dropped(x["deltas"], x["sigma"]), x["deltas"], x["sigma"])
        assert not bad["ok"] and bad["at"][1] >= 32, (family, bad)
        assert R.check_w(carry_dropped(x["deltas"], x["sigma"], tile=65), x["deltas"], x["sigma"])["ok"]
    # zeros where delta <= 0 are part of the criterion
    gaps = R.weight_inputs("gaps", 4, 65)
    w = R.weights32(gaps["deltas"], gaps["sigma"])[0]
    assert R.check_w(w, gaps["deltas"], gaps["sigma"])["ok"]
    w[gaps["deltas"] <= 0] = 1e-30
    assert not R.check_w(w, gaps["deltas"], gaps["sigma"])["ok"]


def _composite32_subtracted(deltas, sigma, steps=None, color=None, g_w=None, g_rgb=None, g_depth=None):
    """composite32 with the depth in front of a sample taken as the inclusive sum minus the sample's own ds."""
    ds = torch.where(deltas > 0, deltas * sigma, torch.zeros(()))
    incl = torch.cumsum(ds, -1)
    excl = incl - ds
    w = -torch.expm1(-ds) * torch.exp(-excl)
    G = torch.zeros_like(ds)
    if g_w is not None:
        G = G + g_w
    if g_rgb is not None:
        G = G + (color * g_rgb[:, None, :]).sum(-1)
    if g_depth is not None:
        denom = w.sum(-1, keepdim=True) + 1e-10
        G = G + g_depth[:, None] / denom * (steps - (w * steps).sum(-1, keepdim=True) / denom)
    suffix = R._shifted((G * w).flip(-1)).flip(-1)
    g_sigma = torch.where(deltas > 0, deltas * (G * torch.exp(-incl) - suffix), torch.zeros(()))
    return {"g_sigma": g_sigma, "g_color": w[..., None] * g_rgb[:, None, :] if g_rgb is not None else None}


@pytest.mark.parametrize("samples", [65, 129, 1024])
def test_subtracted_depth_fails_criteria_c_and_g_on_the_wall(samples):
    """... and passes both where nothing large stands behind thin fog: the criteria single out the wall."""
    inp = R.weight_inputs("wall", 9, samples)
    d, s = inp["deltas"], inp["sigma"]
    for use in R.UPSTREAM:
        kw = R.upstream(inp, use)
        r64, r32, bad = R.composite64(d, s, **kw), R.composite32(d, s, **kw), _composite32_subtracted(d, s, **kw)
        g = R.check_g(bad["g_sigma"], r64["g_sigma"], r32["g_sigma"], d)
        assert not g["ok"] and g["ratio"] > 5, (use, g)
        assert R.check_g(r32["g_sigma"], r64["g_sigma"], r32["g_sigma"], d)["ok"]
        if use[1]:
            c = R.check_c(bad["g_color"], d, s, inp["g_rgb"])
            assert not c["ok"] and c["ratio"] > 5 and c["at"][1] == R.wall_position(c["at"][0], samples), (use, c)
            print(f"S = {samples}: subtracted depth on the wall: C {c['ratio']:.1f} x its limit at {c['at']}, G {g['ratio']:.1f} x on ray {g['at']}")
    fog = R.weight_inputs("fog", 9, samples)
    kw = R.upstream(fog, (True, True, True))
    r64, r32, sub = (f(fog["deltas"], fog["sigma"], **kw) for f in (R.composite64, R.composite32, _composite32_subtracted))
    assert R.check_c(sub["g_color"], fog["deltas"], fog["sigma"], fog["g_rgb"])["ok"]
    assert R.check_g(sub["g_sigma"], r64["g_sigma"], r32["g_sigma"], fog["deltas"])["ok"]


def _variant_resample(weights_, anneal, bins, u, padding=0.01, right=True, shift=0):
    rays, s_in = weights_.shape
    c = R.cdf(weights_, anneal, torch.float64, padding=padding)
    bins, u = R._per_ray(bins, rays, torch.float64), R._per_ray(u, rays, torch.float64)
    idx = torch.searchsorted(c, u, right=right)
    lo, hi = torch.clamp(idx - 1, 0, s_in), torch.clamp(idx, 0, s_in)
    c0, c1 = torch.gather(c, -1, lo), torch.gather(c, -1, hi)
    b0, b1 = torch.gather(bins, -1, torch.clamp(lo + shift, 0, s_in)), torch.gather(bins, -1, torch.clamp(hi + shift, 0, s_in))
    return b0 + torch.clip(torch.nan_to_num((u - c0) / (c1 - c0), 0), 0, 1) * (b1 - b0)


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("family", R.BIN_FAMILIES)
def test_wrong_resamplers_fail_criterion_p(family, jitter):
    for rays, s_in, s_out in ((4, 65, 64), (5, 256, 299), (3, 4, 63)):
        inp = R.resample_inputs(family, rays, s_in, s_out, "alpha", jitter, False)
        w, b, u = inp["weights"], inp["bins"], inp["u"]
        for anneal in (1.0, 0.5, R.ANNEALS[3]):
            assert R.check_p(_variant_resample(w, anneal, b, u), w, anneal, b, u)["ok"]
            no_padding = R.check_p(_variant_resample(w, anneal, b, u, padding=0.0), w, anneal, b, u)
            off_by_one = R.check_p(_variant_resample(w, anneal, b, u, shift=1), w, anneal, b, u)
            assert not no_padding["ok"] and no_padding["failing"] > 0, (family, s_in, anneal, no_padding)
            assert not off_by_one["ok"] and off_by_one["failing"] > 0, (family, s_in, anneal, off_by_one)
            if anneal != 1.0:
                ignored = R.check_p(_variant_resample(w, 1.0, b, u), w, anneal, b, u)
                assert not ignored["ok"] and ignored["failing"] > 0, (family, s_in, anneal, ignored)
        # one output moved by 1e-3 (a flat pdf over wide bins forgives 1e-5: there it is (s_in + 4) 2^-24 of the CDF)
        out = R.resample32(w, 1.0, b, u)
        moved = out.clone()
        moved[0, s_out // 2] += 1e-3
        assert R.check_p(out, w, 1.0, b, u)["ok"] and R.check_p(moved, w, 1.0, b, u)["failing"] >= 1


@pytest.mark.parametrize("kind", R.WEIGHT_KINDS)
def test_searchsorted_side_does_not_change_the_resampler(kind):
    """right=False is NOT a wrong variant (module docstring): on ``repeated`` bins, u placed ON CDF values, it gives the positions of
    right=True -- so criterion P passes it, as it must."""
    for s_in in (4, 65, 256):
        inp = R.resample_inputs("repeated", 4, s_in, 64, kind, False, False)
        w, b = inp["weights"], inp["bins"]
        for anneal in R.ANNEALS:
            c = R.cdf64(w, anneal)
            u = c[:, :: max(s_in // 16, 1)].contiguous()                                # every u IS a CDF value (0 and the last included)
            left, right = _variant_resample(w, anneal, b, u, right=False), _variant_resample(w, anneal, b, u, right=True)
            assert torch.equal(right, R.resample64(w, anneal, b, u))
            assert float((left - right).abs().max()) <= 2.0 ** -52, (kind, s_in, anneal)
            assert float(R.cdf_residual(left, w, anneal, b, u).max()) <= 1e-15


def test_cdf_residual_reads_jumps_as_intervals_and_bins_as_lines():
    inp = R.resample_inputs("repeated", 3, 6, 64, "alpha", False, False)
    w, b = inp["weights"], inp["bins"]
    c = R.cdf64(w, 1.0)
    i = 2                                                                               # bins[:, 3] == bins[:, 2]: a jump from c[2] to c[3]
    assert bool((b[:, i + 1] == b[:, i]).all())
    on_edge = b[:, i:i + 1].expand(3, 5).contiguous()
    u = torch.stack([c[:, i] - 1e-3, c[:, i], (c[:, i] + c[:, i + 1]) / 2, c[:, i + 1], c[:, i + 1] + 2e-3], -1)
    res = R.cdf_residual(on_edge, w, 1.0, b, u)
    assert torch.allclose(res, torch.tensor([1e-3, 0.0, 0.0, 0.0, 2e-3], dtype=torch.float64).expand(3, 5), rtol=0, atol=1e-15)
    mid = ((b[:, 0] + b[:, 1]) / 2)[:, None].contiguous()                               # half way through bin 0: F = c[1] / 2
    assert torch.allclose(R.cdf_residual(mid, w, 1.0, b, (c[:, 1] / 2 + 1e-4)[:, None].contiguous()), torch.full((3, 1), 1e-4, dtype=torch.float64), rtol=0, atol=1e-8)
    assert bool(torch.isinf(R.cdf_residual(torch.full((3, 1), 1.5), w, 1.0, b, torch.full((3, 1), 0.5))).all())
