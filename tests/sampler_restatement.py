"""Float64 restatement of the sampler chain -- RaySamples.get_weights (njf_alpha_weights), PDFSampler (njf_pdf_resample) and the
closed-form gradients of alpha compositing (njf_composite_backward) -- in plain tensor code, with the same statements in float32
library ops (the "twin": the yardstick of the GPU tests), the seeded input families and the acceptance criteria W, P, G and C as
functions, so that tests/test_sampler_chain_cpu.py and tests/test_sampler_chain_gpu.py apply the same code.

Every function takes the fp32 inputs the kernels take; ``dtype`` selects float64 (reference) or float32 (twin).  The exclusive
optical depth is a SHIFTED cumulative sum (``cumsum - ds`` cancels: behind thin fog a large ds leaves 2^-53 (excl + ds) in excl,
a factor of 140 in a first twin), alpha is ``-expm1(-ds)``.

No oracle import at module level: the oracle is what tests/test_sampler_chain_cpu.py pins this file against.
"""
import math

import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
EPS = 2.0 ** -24                      # one fp32 rounding, relative
ABS_FLOOR = 2.0 ** -120               # where exp(-excl) underflows in fp32

RAYS = (1, 3, 4, 5, 9)                # one wave per ray, four waves per block
WEIGHT_SAMPLES = (1, 31, 32, 33, 64, 65, 257, 1024)
COMPOSITE_SAMPLES = (1, 63, 64, 65, 128, 129, 1023, 1024)
WEIGHT_FAMILIES = ("mixed", "fog", "switch", "wall", "opaque", "gaps")
UPSTREAM = ((True, False, False), (True, True, True), (False, True, False), (False, False, True))     # (g_w, g_rgb, g_depth)
WALL_DS = (50.0, 2000.0, 1e5)
SWITCH = 0.0625                       # alpha_of: series below, literal form from here on
FIRST_DS_CAP = 16.0                   # (weight_inputs: what is left behind a more opaque first sample is below the fp32 range)

S_IN = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256)
S_OUT = (1, 63, 64, 65, 299)
BIN_FAMILIES = ("random", "uniform", "repeated")
WEIGHT_KINDS = ("alpha", "half_zero", "delta")


def anneal_value(step, max_iters, slope):
    """models/model.py:201-209 (step_before_iter): the mip-NeRF-360 bias schedule."""
    frac = min(max(step / max_iters, 0.0), 1.0)
    return (slope * frac) / ((slope - 1) * frac + 1)


ANNEALS = (1.0, 0.0, 0.5, anneal_value(500, 1000, 10))


# ---- get_weights ------------------------------------------------------------------------------------------------------------------------
def _ds(deltas, sigma, dtype):
    return torch.where(deltas > 0, deltas.to(dtype) * sigma.to(dtype), torch.zeros((), dtype=dtype))


def _shifted(x):
    """Exclusive prefix sum along the last axis from a shifted cumulative sum."""
    return torch.cat([torch.zeros_like(x[..., :1]), torch.cumsum(x[..., :-1], -1)], -1)


def weights(deltas, sigma, dtype=F64):
    """(w, excl) [rays, S]: w_s = (1 - exp(-ds_s)) exp(-excl_s), ds = delta sigma (0 where delta <= 0), excl_s = sum_{j<s} ds_j."""
    ds = _ds(deltas, sigma, dtype)
    excl = _shifted(ds)
    return -torch.expm1(-ds) * torch.exp(-excl), excl


def weights64(deltas, sigma):
    return weights(deltas, sigma, F64)


def weights32(deltas, sigma):
    return weights(deltas, sigma, F32)


# ---- the gradients of compositing -------------------------------------------------------------------------------------------------------
def composite(deltas, sigma, steps=None, color=None, g_w=None, g_rgb=None, g_depth=None, dtype=F64):
    """The closed forms stated above composite_backward_kernel, for any subset of the upstream gradients g_w [rays,S], g_rgb [rays,3]
    (with color [rays,S,3]) and g_depth [rays] (with steps [rays,S]; the gradient of the UN-clipped depth sum w t / (sum w + 1e-10)):
      G_s = g_w[s] + g_rgb . c_s + g_depth (t_s - depth) / (sum w + 1e-10)
      dL/dds_k = G_k T_{k+1} - sum_{s>k} G_s w_s,   dL/dsigma_k = delta_k dL/dds_k (0 where delta <= 0),   dL/dc_k = w_k g_rgb
    -> {"g_sigma", "g_color" (None without g_rgb), "w", "G", "excl"}."""
    ds = _ds(deltas, sigma, dtype)
    excl = _shifted(ds)
    w = -torch.expm1(-ds) * torch.exp(-excl)
    t_next = torch.exp(-(excl + ds))
    G = torch.zeros_like(ds)
    if g_w is not None:
        G = G + g_w.to(dtype)
    if g_rgb is not None:
        G = G + (color.to(dtype) * g_rgb.to(dtype)[:, None, :]).sum(-1)
    if g_depth is not None:
        t = steps.to(dtype)
        denom = w.sum(-1, keepdim=True) + 1e-10
        depth = (w * t).sum(-1, keepdim=True) / denom
        G = G + g_depth.to(dtype)[:, None] / denom * (t - depth)
    suffix = _shifted((G * w).flip(-1)).flip(-1)                                        # sum over s > k, summed back to front
    g_sigma = torch.where(deltas > 0, deltas.to(dtype) * (G * t_next - suffix), torch.zeros((), dtype=dtype))
    g_color = w[..., None] * g_rgb.to(dtype)[:, None, :] if g_rgb is not None else None
    return {"g_sigma": g_sigma, "g_color": g_color, "w": w, "G": G, "excl": excl}


def composite64(deltas, sigma, **kw):
    return composite(deltas, sigma, dtype=F64, **kw)


def composite32(deltas, sigma, **kw):
    return composite(deltas, sigma, dtype=F32, **kw)


# ---- PDFSampler --------------------------------------------------------------------------------------------------------------------------
def as_fp32(x):
    """The value a C float argument carries (the kernel receives ``anneal`` as one)."""
    return float(np.float32(x))


def cdf(weights_, anneal, dtype=F64, padding=0.01, eps=1e-5):
    """[rays, s_in + 1]: pow on the fp32 weights, + 0.01, pad, normalise, clipped cumulative sum, a leading 0."""
    w = torch.pow(weights_.to(dtype), as_fp32(anneal)) + padding
    w_sum = w.sum(-1, keepdim=True)
    pad = torch.relu(eps - w_sum)
    w = w + pad / w.shape[-1]
    w_sum = w_sum + pad
    c = torch.minimum(torch.ones((), dtype=dtype), torch.cumsum(w / w_sum, -1))
    return torch.cat([torch.zeros_like(c[..., :1]), c], -1)


def _per_ray(x, rays, dtype):
    x = x.to(dtype)
    return (x[None].expand(rays, -1) if x.dim() == 1 else x).contiguous()


def resample(weights_, anneal, bins, u, dtype=F64):
    """[rays, len(u)]: the inverse CDF at u (searchsorted right=True, clamp, nan_to_num, clip); bins [s_in+1] or [rays, s_in+1],
    u [s_out+1] or [rays, s_out+1]."""
    rays, s_in = weights_.shape
    c = cdf(weights_, anneal, dtype)
    bins, u = _per_ray(bins, rays, dtype), _per_ray(u, rays, dtype)
    idx = torch.searchsorted(c, u, right=True)
    lo, hi = torch.clamp(idx - 1, 0, s_in), torch.clamp(idx, 0, s_in)
    c0, c1 = torch.gather(c, -1, lo), torch.gather(c, -1, hi)
    b0, b1 = torch.gather(bins, -1, lo), torch.gather(bins, -1, hi)
    t = torch.clip(torch.nan_to_num((u - c0) / (c1 - c0), 0), 0, 1)
    return b0 + t * (b1 - b0)


def cdf64(weights_, anneal):
    return cdf(weights_, anneal, F64)


def resample64(weights_, anneal, bins, u):
    return resample(weights_, anneal, bins, u, F64)


def resample32(weights_, anneal, bins, u):
    return resample(weights_, anneal, bins, u, F32)


def cdf_residual(out, weights_, anneal, bins, u):
    """Distance of u_k from F64(out_k), F64 the float64 piecewise-linear CDF over bin position.  Where out_k sits on one or more
    coincident bin edges F64 is the closed interval of the CDF values at those edges (a zero-width bin is a jump); an out_k outside
    [bins[0], bins[-1]] has an infinite residual."""
    rays, s_in = weights_.shape
    c = cdf64(weights_, anneal)
    bins, u, x = _per_ray(bins, rays, F64), _per_ray(u, rays, F64), out.to(F64)
    first = torch.searchsorted(bins, x, right=False)                                    # first edge >= out
    after = torch.searchsorted(bins, x, right=True)                                     # first edge > out
    on_edge = after > first
    i0, i1 = torch.clamp(first - 1, 0, s_in), torch.clamp(first, 0, s_in)               # the bin around an out strictly inside one
    b0, b1, c0, c1 = torch.gather(bins, -1, i0), torch.gather(bins, -1, i1), torch.gather(c, -1, i0), torch.gather(c, -1, i1)
    inside = c0 + (x - b0) / torch.where(b1 > b0, b1 - b0, torch.ones_like(b0)) * (c1 - c0)
    f_lo = torch.where(on_edge, torch.gather(c, -1, torch.clamp(first, 0, s_in)), inside)
    f_hi = torch.where(on_edge, torch.gather(c, -1, torch.clamp(after - 1, 0, s_in)), inside)
    res = torch.clamp(torch.maximum(f_lo - u, u - f_hi), min=0.0)
    outside = (x < bins[:, :1]) | (x > bins[:, -1:]) | ~torch.isfinite(x)
    return torch.where(outside, torch.full_like(res, math.inf), res)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(_stable_seed(key))


def _stable_seed(key):
    h = 2166136261                                                                      # (FNV-1a: the same seed in every process)
    for ch in "|".join(str(k) for k in key).encode():
        h = ((h ^ ch) * 16777619) % (2 ** 32)
    return h % (2 ** 31 - 1)


def _log_uniform(shape, lo, hi, g):
    return torch.exp(torch.rand(shape, generator=g, dtype=F64) * (math.log(hi) - math.log(lo)) + math.log(lo))


def wall_position(ray, samples):
    """Where the wall of ``ray`` sits: ray % 5 == 0 a position that is no edge of a 32- or 64-sample tile, else lanes 31, 32, 63, 64;
    always with a sample behind it where the ray has one."""
    p = samples // 2
    while p % 32 in (0, 31) and p + 1 < samples:
        p += 1
    p = (p, 31, 32, 63, 64)[ray % 5]
    return max(min(p, samples - 2), 0)


def wall_ds(ray, samples):
    return WALL_DS[(ray + samples) % 3]


def switch_values():
    """0.0625 with its two fp32 neighbours on either side."""
    c = np.float32(SWITCH)
    lo1, hi1 = np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(1))
    return [float(np.nextafter(lo1, np.float32(0))), float(lo1), float(c), float(hi1), float(np.nextafter(hi1, np.float32(1)))]


def weight_inputs(family, rays, samples):
    """{"deltas", "sigma", "steps", "g_w" [rays,S], "color" [rays,S,3], "g_rgb" [rays,3], "g_depth" [rays]} in fp32.

    mixed   the ranges of tests/test_training_gpu.py::test_composite_backward_equals_autograd; the last ray turns opaque
    fog     ds log-uniform in 1e-8 .. 1e-2: the series branch of alpha_of only
    switch  sigma = 1, delta (= ds, exactly) from 0.0625 and its two fp32 neighbours on either side
    wall    fog of total depth <= 0.9, then ONE sample with ds in {50, 2000, 1e5} (wall_position, wall_ds), fog behind it
    opaque  the depth grows as 250 x^2 along the ray: it passes 87 (exp underflows in fp32) at x = 0.59
    gaps    mixed with delta in {0, -0.0, -0.1} on three samples in ten and every third ray all zeros

    Narrowed so that criterion G -- a NORM-WISE figure per ray, with no absolute floor -- is one the fp32 twin can meet at a quarter
    of its cap (each narrowing with the twin figure that forced it; criteria W and C needed none, and with these every family's
    twin is under 2.4e-6):
    * mixed, gaps, opaque: the first sample that has a length has ds <= 16.  Behind a first sample with ds > 87 every gradient of
      the ray lies below the fp32 range (float64 still resolves it to ~1e-170): twin err 1.0; behind ds = 60 the one rounding of
      that ds is 60 x 2^-24 = 3.6e-6 of every gradient: twin err 6.1e-6.
    * mixed, gaps, opaque: a dense ray starts thin (mixed, gaps: the last ray's density x 1, 2, .. 50 instead of x 50 throughout;
      opaque: a linear density ramp).  On a ray whose first sample absorbs everything, every gradient is T_1 (G_0 - the mean of G
      behind): left to the difference of two colours that happen to agree, twin err 1.4e-5.
    * fog, wall: equal intervals (delta = 2^-6, the density carries the six decades).  With delta spread over six decades beside
      ds the depth-only gradient of a ray that one sample dominates is decided by the cancellation in t - depth on that sample:
      twin err 5.4e-6 at S = 33 against the 5e-6 allowed.
    * a one-sample ray has g_depth = 0: its depth is its t, and in fog (w ~ 1e-8) the 1e-10 t / w^2-sized term that the existing
      test skips as below fp32 resolution dominates all three upstream gradients together: twin err 5.6e-3."""
    g = _gen("weights", family, rays, samples)
    shape = (rays, samples)
    if family in ("mixed", "gaps"):
        deltas = torch.rand(shape, generator=g) * 0.3
        sigma = torch.exp(torch.randn(shape, generator=g) * 1.5)
        sigma[-1] *= torch.arange(1, samples + 1).clamp(max=50).float()                 # a ray that turns opaque: x 1, 2, .. 50
        if family == "gaps":
            kind = torch.randint(0, 10, shape, generator=g)
            deltas = torch.where(kind == 0, torch.zeros(()), deltas)
            deltas = torch.where(kind == 1, torch.tensor(-0.0), deltas)
            deltas = torch.where(kind == 2, torch.tensor(-0.1), deltas)
            deltas[1::3] = 0.0                                                          # whole rays of zeros
    elif family in ("fog", "wall"):
        deltas = torch.full(shape, 2.0 ** -6)                                           # equal intervals (docstring); ds stays exact
        ds = _log_uniform(shape, 1e-8, 1e-2, g)
        if family == "wall":
            for r in range(rays):
                p = wall_position(r, samples)
                front = float(ds[r, :p].sum())
                if front > 0.9:
                    ds[r, :p] *= 0.9 / front
        sigma = (ds / deltas.double()).float()
        if family == "wall":
            for r in range(rays):
                p = wall_position(r, samples)
                deltas[r, p], sigma[r, p] = 0.25, wall_ds(r, samples) / 0.25            # both exact in fp32
    elif family == "switch":
        vals = torch.tensor(switch_values(), dtype=F64)
        idx = (torch.arange(rays * samples).reshape(shape) * 2 + rays + samples) % 5
        deltas, sigma = vals[idx].float(), torch.ones(shape)
    elif family == "opaque":
        deltas = torch.rand(shape, generator=g) * 0.3 + 0.01
        ramp = (torch.arange(samples) + 0.5) * (2.0 / samples)                          # thin in front: depth 250 x^2 at fraction x
        sigma = torch.exp(torch.randn(shape, generator=g) * 0.3) * (250.0 / samples / 0.16) * ramp
    else:
        raise ValueError(family)
    if family in ("mixed", "gaps", "opaque"):
        for r in range(rays):
            front = torch.nonzero(deltas[r] > 0)[:1, 0]                                 # the first sample that has a length
            sigma[r, front] = torch.minimum(sigma[r, front], FIRST_DS_CAP / deltas[r, front])
    steps = torch.sort(torch.rand(shape, generator=g) * 9 + 0.5, -1).values
    g_depth = torch.randn(rays, generator=g)
    return {"deltas": deltas.float().contiguous(), "sigma": sigma.float().contiguous(), "steps": steps.contiguous(),
            "color": torch.rand(rays, samples, 3, generator=g), "g_w": torch.randn(shape, generator=g),
            "g_rgb": torch.randn(rays, 3, generator=g), "g_depth": g_depth if samples > 1 else torch.zeros(rays)}


def upstream(inp, use):
    """The keyword arguments of ``composite`` for one combination of upstream gradients."""
    kw = {}
    if use[0]:
        kw["g_w"] = inp["g_w"]
    if use[1]:
        kw.update(color=inp["color"], g_rgb=inp["g_rgb"])
    if use[2]:
        kw.update(steps=inp["steps"], g_depth=inp["g_depth"])
    return kw


def midpoint_u(s_out):
    nb = s_out + 1
    return torch.linspace(0.0, 1.0 - (1.0 / nb), steps=nb) + 1.0 / (2 * nb)


def jittered_u(rays, s_out, g):
    """u = k / nb + rand / nb per ray, as PDFSampler draws it in training; the running maximum keeps it sorted where the fp32 sum of
    two neighbours rounds across each other."""
    nb = s_out + 1
    u = torch.linspace(0.0, 1.0 - (1.0 / nb), steps=nb).expand(rays, nb) + torch.rand(rays, nb, generator=g) / nb
    return torch.cummax(u, -1).values.contiguous()


def resample_inputs(family, rays, s_in, s_out, kind, jitter, shared):
    """{"weights" [rays,s_in], "bins" [s_in+1] (shared) or [rays,s_in+1], "u" [s_out+1] (mid-points) or [rays,s_out+1] (jittered)}."""
    g = _gen("resample", family, rays, s_in, s_out, kind, jitter, shared)
    rows = 1 if shared else rays
    if family == "uniform":
        bins = torch.linspace(0.0, 1.0, s_in + 1).expand(rows, -1).clone()
    else:
        bins = torch.sort(torch.rand(rows, s_in + 1, generator=g), -1).values
        bins[:, 0], bins[:, -1] = 0.0, 1.0
        if family == "repeated":
            for i in {s_in // 3, (2 * s_in) // 3}:                                      # two pairs of coincident edges (one for s_in = 2)
                if i + 1 < s_in:
                    bins[:, i + 1] = bins[:, i]
    deltas = torch.rand(rays, s_in, generator=g) * 0.3
    sigma = torch.exp(torch.randn(rays, s_in, generator=g) * 1.5)
    w = weights64(deltas, sigma)[0].float()
    if kind == "half_zero":
        w[: (rays + 1) // 2] = 0.0                                                      # the padding path
    elif kind == "delta":
        w.zero_()
        w[:, s_in // 2] = 1.0
    u = jittered_u(rays, s_out, g) if jitter else midpoint_u(s_out)
    return {"weights": w.contiguous(), "bins": (bins[0] if shared else bins).contiguous(), "u": u}


def resample_rays(waves):
    """One ray per wave, ``waves`` (NJF_WAVES) per workgroup: a single ray, a ragged / a full / a full and a ragged workgroup, 9."""
    return (1, waves - 1, waves, waves + 1, 9)


def resample_cases(s_in, rays=RAYS):
    """The cases of one s_in: every (s_out, bin family) with all four anneals; rays, the weight kind, the kind of u and shared /
    per-ray bins cycle so that every pair of choices occurs.  -> [(family, rays, s_in, s_out, kind, jitter, shared, anneal)]."""
    cases, c = [], S_IN.index(s_in)
    for s_out in S_OUT:
        for family in BIN_FAMILIES:
            for j, anneal in enumerate(ANNEALS):
                cases.append((family, rays[(c + j) % 5], s_in, s_out, WEIGHT_KINDS[(c + j) % 3], bool((c // 3 + j) % 2),
                              bool((c // 2 + j // 2) % 2), anneal))
            c += 1
    return cases


# ---- criteria ---------------------------------------------------------------------------------------------------------------------------
def w_limit(w64, excl64, samples, extra_roundings=0):
    """Criterion W, element-wise: (2e-6 + (8 + ceil(S/32)) 2^-24 excl) w + 2^-120.  2e-6: alpha_of states <= 1e-6 for itself, plus one
    expf and one product rounding, doubled.  (8 + ceil(S/32)) 2^-24 excl: the roundings of the partial sums <= excl (5 adds of the
    32-wide scan, the shift, the carry, one carry add per tile) -- an absolute error of excl is a relative error of exp(-excl)."""
    return (2e-6 + extra_roundings * EPS + (8 + math.ceil(samples / 32)) * EPS * excl64) * w64.abs() + ABS_FLOOR


def _worst(err, limit):
    ratio = err / limit
    i = int(torch.argmax(ratio.reshape(-1)))
    return i, float(ratio.reshape(-1)[i])


def check_w(w, deltas, sigma, scale=1.0):
    """Criterion W on ``w`` (fp32 or float64) against weights64, both sides x ``scale`` (twice the limit: scale = 2).
    -> {"ok", "ratio" (worst err / limit), "err", "limit", "at" (ray, sample), "zeros_ok"}."""
    w64, excl = weights64(deltas, sigma)
    err, limit = (w.double() - w64).abs(), scale * w_limit(w64, excl, deltas.shape[-1])
    i, ratio = _worst(err, limit)
    zeros_ok = bool((w[deltas <= 0] == 0).all())
    return {"ok": bool((err <= limit).all()) and zeros_ok and bool(torch.isfinite(w).all()), "ratio": ratio,
            "err": float(err.reshape(-1)[i]), "limit": float(limit.reshape(-1)[i]), "at": divmod(i, deltas.shape[-1]), "zeros_ok": zeros_ok}


def check_c(g_color, deltas, sigma, g_rgb):
    """Criterion C: g_color = w g_rgb exposes the backward's recomputed weight -- criterion W with one more 2^-24 for the product,
    scaled by |g_rgb|."""
    w64, excl = weights64(deltas, sigma)
    ref = w64[..., None] * g_rgb.double()[:, None, :]
    limit = w_limit(w64, excl, deltas.shape[-1], extra_roundings=1)[..., None] * g_rgb.double().abs()[:, None, :] + ABS_FLOOR
    err = (g_color.double() - ref).abs()
    i, ratio = _worst(err, limit)
    zeros_ok = bool((g_color[deltas <= 0] == 0).all())
    return {"ok": bool((err <= limit).all()) and zeros_ok and bool(torch.isfinite(g_color).all()), "ratio": ratio,
            "err": float(err.reshape(-1)[i]), "limit": float(limit.reshape(-1)[i]), "at": divmod(i // 3, deltas.shape[-1]),
            "zeros_ok": zeros_ok}


G_FACTOR, G_ULP_FLOOR, G_CAP = 4.0, 4.0 * 2.0 ** -23, 2e-5


def ray_rel(g, g64):
    """max|g - g64| / max|g64| per ray; a ray whose reference is all zero has err 0 if g is all zero there and inf otherwise."""
    num, den = (g.double() - g64).abs().amax(-1), g64.abs().amax(-1)
    return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)),
                       torch.where(num > 0, torch.full_like(num, math.inf), torch.zeros_like(num)))


def g_limit(twin_err):
    """Criterion G: min(max(4 x the twin's err, 4 x 2^-23), 2e-5) per ray."""
    return torch.clamp(torch.clamp(G_FACTOR * twin_err, min=G_ULP_FLOOR), max=G_CAP)


def check_g(g_sigma, g64, g32, deltas):
    """-> {"ok", "ratio", "err", "floor", "limit", "at" (ray), "zeros_ok"}, the worst ray by err / limit."""
    err, floor = ray_rel(g_sigma, g64), ray_rel(g32, g64)
    limit = g_limit(floor)
    i, ratio = _worst(err, limit)
    zeros_ok = bool((g_sigma[deltas <= 0] == 0).all())
    return {"ok": bool((err <= limit).all()) and zeros_ok and bool(torch.isfinite(g_sigma).all()), "ratio": ratio, "err": float(err[i]),
            "floor": float(floor[i]), "limit": float(limit[i]), "at": i, "zeros_ok": zeros_ok}


def check_p(out, weights_, anneal, bins, u):
    """Criterion P, element-wise and without exceptions: |out - out64| <= 4 2^-24 max|bins| (decisive inside narrow bins) OR
    cdf_residual <= (s_in + 4) 2^-24 (decisive where the pdf is flat: s_in adds of partial sums <= 1, the division, the powf, the
    interpolation, the store); out non-decreasing along k and inside [bins[0], bins[-1]].
    -> {"ok", "failing", "ratio" (worst min(fwd / limit, residual / limit)), "fwd", "residual", "fwd_limit", "residual_limit", "at"}."""
    rays, s_in = weights_.shape
    out64 = resample64(weights_, anneal, bins, u)
    fwd, fwd_limit = (out.double() - out64).abs(), 4 * EPS * float(bins.abs().max())
    res, res_limit = cdf_residual(out, weights_, anneal, bins, u), (s_in + 4) * EPS
    ratio = torch.minimum(fwd / fwd_limit, res / res_limit)
    ratio = torch.where(torch.isfinite(out.double()), ratio, torch.full_like(ratio, math.inf))
    i = int(torch.argmax(ratio.reshape(-1)))
    b = _per_ray(bins, rays, F64)
    sorted_ok = bool((out[:, 1:] >= out[:, :-1]).all())
    range_ok = bool(((out.double() >= b[:, :1]) & (out.double() <= b[:, -1:])).all())
    failing = int((~(ratio <= 1.0)).sum())
    return {"ok": failing == 0 and sorted_ok and range_ok, "failing": failing, "ratio": float(ratio.reshape(-1)[i]),
            "fwd": float(fwd.reshape(-1)[i]), "residual": float(res.reshape(-1)[i]), "fwd_limit": fwd_limit, "residual_limit": res_limit,
            "at": divmod(i, out.shape[-1]), "sorted_ok": sorted_ok, "range_ok": range_ok}


def p_row(key, got, twin):
    """The margins row of one resampler case: the worst element's deciding figure (the check it is closer to passing)."""
    by_fwd = got["fwd"] / got["fwd_limit"] <= got["residual"] / got["residual_limit"]
    err, limit = (got["fwd"], got["fwd_limit"]) if by_fwd else (got["residual"], got["residual_limit"])
    return {"key": key, "err": float(f"{err:.3e}"), "floor": float(f"{twin['ratio'] * limit:.3e}"), "limit": float(f"{limit:.3e}"),
            "needs_floor": False, "ok": bool(got["ok"]), "check": "forward" if by_fwd else "cdf residual",
            "err_over_limit": float(f"{got['ratio']:.3e}"), "twin_err_over_limit": float(f"{twin['ratio']:.3e}"), "failing": got["failing"]}


def row(key, got, twin):
    """The margins row of a W / C / G comparison: err and limit of the worst element (W, C) or ray (G) by err / limit; floor = the
    twin's err on that ray (G), the err of the twin's own worst element (W, C)."""
    floor = got.get("floor", twin["err"])
    return {"key": f"{key} at {got['at']}", "err": float(f"{got['err']:.3e}"), "floor": float(f"{floor:.3e}"),
            "limit": float(f"{got['limit']:.3e}"), "needs_floor": False, "ok": bool(got["ok"]),
            "err_over_limit": float(f"{got['ratio']:.3e}"), "twin_err_over_limit": float(f"{twin['ratio']:.3e}")}
