"""Torch restatement of the folded transformer head and of its data-gradient chain (csrc/njf_kernels.hip:
transformer_backward_kernel, njf_transformer_backward), for tests/test_transformer_backward_cpu.py and
tests/test_transformer_backward_gpu.py.

The layer is written once, as the kernel's comment states it, and runs in the dtype of the tensors it is given: float64 is the
reference, float32 (the same code in library ops) is the "twin" whose distance to the float64 result is the yardstick of the GPU
tests.  There is no hand-written derivative here: every gradient comes from ``torch.autograd.grad``.

Per layer (mats[l] = (Mqk, Nov, W1', W2) as [out, in], biases[l] = (bqk, bo, b1', b2)):
    n  = layer_norm(x)                       no affine, eps = 1e-5
    s  = Mqk n + bqk                         64 dots = 8 heads x 8 key slots
    a  = softmax over the first `keys` slots of each head; slots >= keys are exactly 0
    xm = x + (Nov a + bo)
    n2 = layer_norm(xm);  u = W1' n2 + b1';  h = gelu_erf(u)
    x_next = xm + (W2 h) + b2
The pairs a weight gradient contracts over the points are X = (n, a, n2, h) and dY = d/d(s, Nov a + bo, u, W2 h), slot 4 l + i.
"""
from typing import Dict

import torch

EPS = 1e-5
FAMILIES = ("random", "rows", "onehot", "gelu_tails", "all")
# The stress rows (inputs(...)): the offset M of the "large |x|" rows (unit variance around +-M).  An fp32 mean of 64 values near M
# is rounded at M * 2^-24, which is an absolute error of the normalised row in ANY fp32 implementation, and the layers behind
# amplify it: the fp32 twin's worst row measures 1.3e-6 at M = 8, 2.0e-6 at 16, 4.9e-6 at 32, 8.1e-6 at 64, 1.2e-5 at 256 and
# 4.5e-5 at 1e3.  The GPU tests cap the twin at 2.5e-6 (test_transformer_backward_cpu.py), so the family is shrunk to M = 8.
LARGE_X = 8.0
# Softmax saturation, on the first ONEHOT_HEADS heads of every layer: Mqk x 4 and a per-key offset on bqk that separates the dots
# of a head by ~40 or more, so that `a` is 1.0 against < 2^-50 in fp32.  A scale on Mqk alone saturates most rows too, but it
# multiplies the fp32 rounding of n into the dots of the rows it leaves undecided (Mqk x 16: twin 5.1e-6, x 64: 9.5e-6), and with
# EVERY head saturated ds is rounding noise around 1e-20 whose norm-wise error is 1 in any fp32 run: the other heads stay soft.
ONEHOT_STEP = 48.0
ONEHOT_MQK_SCALE = 4.0
ONEHOT_HEADS = 4
GELU_TAIL = 8.0


def layer_norm(x: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.layer_norm(x, x.shape[-1:], eps=EPS)


def layer(mats_l: torch.Tensor, biases_l: torch.Tensor, x: torch.Tensor, keys: int) -> Dict[str, torch.Tensor]:
    """One folded layer with its intermediates kept (all [P, 64])."""
    pts = x.shape[0]
    n = layer_norm(x)
    s = n @ mats_l[0].t() + biases_l[0]
    live = torch.softmax(s.reshape(pts, 8, 8)[:, :, :keys], dim=-1)
    a = torch.nn.functional.pad(live, (0, 8 - keys)).reshape(pts, 64)        # unused key slots: exactly 0
    attn = a @ mats_l[1].t() + biases_l[1]
    xm = x + attn
    n2 = layer_norm(xm)
    u = n2 @ mats_l[2].t() + biases_l[2]
    h = torch.nn.functional.gelu(u)                                          # erf form
    ff = h @ mats_l[3].t()
    return {"n": n, "s": s, "a": a, "attn": attn, "xm": xm, "n2": n2, "u": u, "h": h, "ff": ff, "out": xm + ff + biases_l[3]}


def folded_stream(mats: torch.Tensor, biases4: torch.Tensor, x0: torch.Tensor, keys: int) -> torch.Tensor:
    """x [4, P, 64]: x[l] is the residual stream in front of layer l, x[3] the stream behind layer 2."""
    xs = [x0]
    for l in range(3):
        xs.append(layer(mats[l], biases4[l], xs[-1], keys)["out"])
    return torch.stack(xs)


def chain(mats: torch.Tensor, biases3: torch.Tensor, head_w: torch.Tensor, x: torch.Tensor, d_out: torch.Tensor,
          keys: int) -> Dict[str, torch.Tensor]:
    """What njf_transformer_backward returns -- wg_x [12,P,64], wg_dy [12,P,64], dx0 [P,64], sums [12,64] -- and the gradients of
    the folded parameters themselves, g_mats [3,4,64,64] and g_biases [3,4,64], in the dtype of ``mats``.  ``x`` [4,P,64] is the
    given dump (each layer is rebuilt from x[l] as it stands, as the kernel does), ``biases3`` = (bqk, bo, b1') per layer."""
    dtype = mats.dtype
    x, d_out, head_w = x.to(dtype), d_out.to(dtype), head_w.to(dtype)
    pts = x.shape[1]
    wg_x, wg_dy = [None] * 12, [None] * 12
    g_mats, g_biases = [None] * 3, [None] * 3
    dx = d_out @ head_w
    for l in (2, 1, 0):
        xl = x[l].detach().clone().requires_grad_(True)
        m = mats[l].detach().clone().requires_grad_(True)
        b = torch.cat([biases3[l].detach().to(dtype), torch.zeros(1, 64, dtype=dtype)]).requires_grad_(True)   # (b2 only adds)
        f = layer(m, b, xl, keys)
        d_x, d_s, d_attn, d_u, d_ff, g_m, g_b = torch.autograd.grad(
            f["out"], [xl, f["s"], f["attn"], f["u"], f["ff"], m, b], dx)
        wg_x[4 * l:4 * l + 4] = [f["n"].detach(), f["a"].detach(), f["n2"].detach(), f["h"].detach()]
        wg_dy[4 * l:4 * l + 4] = [d_s, d_attn, d_u, d_ff]
        g_mats[l], g_biases[l] = g_m, g_b
        dx = d_x
    wg_dy = torch.stack(wg_dy)
    assert wg_dy.shape == (12, pts, 64)
    return {"wg_x": torch.stack(wg_x), "wg_dy": wg_dy, "dx0": dx, "sums": wg_dy.sum(1),
            "g_mats": torch.stack(g_mats), "g_biases": torch.stack(g_biases)}


def twin(mats: torch.Tensor, biases3: torch.Tensor, head_w: torch.Tensor, x: torch.Tensor, d_out: torch.Tensor,
         keys: int) -> Dict[str, torch.Tensor]:
    """``chain`` in float32 library ops on the same (fp32-representable) inputs."""
    return chain(mats.float(), biases3.float(), head_w.float(), x.float(), d_out.float(), keys)


def rel(got: torch.Tensor, ref: torch.Tensor) -> float:
    """Norm-wise: max|got - ref| / max|ref| (0 for two all-zero tensors)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    diff = float((got - ref).abs().max())
    return diff / float(ref.abs().max()) if diff > 0.0 else 0.0


def rows26(res: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The 26 compared outputs by name: wg_x[0..11], wg_dy[0..11], dx0, sums."""
    out = {f"wg_x[{k}]": res["wg_x"][k] for k in range(12)}
    out.update({f"wg_dy[{k}]": res["wg_dy"][k] for k in range(12)})
    out["dx0"], out["sums"] = res["dx0"], res["sums"]
    return out


def pair_products(wg_x: torch.Tensor, wg_dy: torch.Tensor) -> torch.Tensor:
    """dY^T X per slot in float64: [3, 4, 64(out), 64(in)]."""
    return torch.einsum("kpo,kpi->koi", wg_dy.double(), wg_x.double()).reshape(3, 4, 64, 64)


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------
def random_head(seed: int, d_out_dim: int, gain: float = 1.0):
    """(mats [3,4,64,64], biases [3,4,64], head_w [d_out_dim,64]) in fp32, all entries random: the Mqk rows, bqk entries and Nov
    columns of unused key slots are NOT zero (a fold would zero them).  Gains chosen so that dots, u and the stream stay O(1)."""
    g = torch.Generator().manual_seed(seed)
    std = torch.tensor([0.125, 0.2, 0.125, 0.125]) * gain
    mats = torch.randn(3, 4, 64, 64, generator=g) * std[None, :, None, None]
    biases = torch.randn(3, 4, 64, generator=g) * 0.1
    head_w = torch.randn(d_out_dim, 64, generator=g) * 0.125 * gain
    return mats, biases, head_w


def stress_rows(points: int) -> Dict[str, list]:
    """Which rows of a batch carry which stress (family "rows" / "all"): spread over the first tile, the half boundary of a tile
    (lanes 31 / 32 hold one point's two channel halves; rows 31 / 32 / 33 sit in two tiles) and the ragged last tile."""
    pick = lambda cand: sorted({i % points for i in cand})
    return {"constant": pick([1, 32, points - 2]), "large": pick([2, 3, 33, points - 1]), "zero_d_out": pick([4, 31, points - 3])}


def inputs(family: str, points: int, keys: int, d_out_dim: int, seed: int = 0, gain: float = 1.0,
           d_out_scale: float = 1e-3) -> Dict[str, torch.Tensor]:
    """Everything one launch needs, fp32 (the float64 reference reads the same values): mats, biases [3,4,64], head_w, d_out [P,D]
    and x [4,P,64] = folded_stream in float64 rounded to fp32 once."""
    assert family in FAMILIES, family
    mats, biases, head_w = random_head(seed, d_out_dim, gain)
    g = torch.Generator().manual_seed(1000 + seed)
    x0 = torch.randn(points, 64, generator=g)
    d_out = torch.randn(points, d_out_dim, generator=g) * d_out_scale
    if family in ("rows", "all"):
        rows = stress_rows(points)
        x0[rows["large"]] += LARGE_X * torch.tensor([1.0, -1.0, 1.0, -1.0])[:len(rows["large"]), None]   # |x| ~ LARGE_X, unit variance
        x0[rows["constant"]] = 2.0 ** -6                                                                # variance 0: rstd = 1 / sqrt(eps)
        d_out[rows["zero_d_out"]] = 0.0
    if family in ("onehot", "all"):
        mats[:, 0, :8 * ONEHOT_HEADS] *= ONEHOT_MQK_SCALE
        order = torch.stack([torch.randperm(8, generator=g) for _ in range(3 * 8)]).reshape(3, 8, 8)
        order[:, ONEHOT_HEADS:] = 0                                                                      # the other heads stay soft
        biases[:, 0] += ONEHOT_STEP * order.reshape(3, 64).float()
    if family in ("gelu_tails", "all"):
        sign = torch.where(torch.arange(64) % 4 == 0, 1.0, torch.where(torch.arange(64) % 4 == 1, -1.0, 0.0))
        biases[:, 2] += GELU_TAIL * sign                                                                 # u ~ +-8 on half the channels
    x = folded_stream(mats.double(), biases.double(), x0.double(), keys).float()
    return {"mats": mats, "biases": biases, "head_w": head_w, "x": x.contiguous(), "d_out": d_out.contiguous()}


def reference_and_twin(inp: Dict[str, torch.Tensor], keys: int):
    """(float64 chain, fp32 twin) on one set of inputs."""
    b3 = inp["biases"][:, :3]
    ref = chain(inp["mats"].double(), b3.double(), inp["head_w"].double(), inp["x"].double(), inp["d_out"].double(), keys)
    return ref, twin(inp["mats"], b3, inp["head_w"], inp["x"], inp["d_out"], keys)
