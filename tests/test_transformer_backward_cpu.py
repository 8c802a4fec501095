"""Pins tests/transformer_backward_restatement.py -- the float64 reference of the fused transformer backward chain that
tests/test_transformer_backward_gpu.py compares njf_transformer_backward with -- without a GPU:

* its forward is the head: ``folded_stream`` on ``training.folded_transformer`` equals ``training.transformer_head``;
* its pair and slot convention: the autograd gradients of the folded parameters equal dY^T X and the column sums of the pairs
  it emits;
* its fp32 twin (the yardstick of the GPU tests) stays under TWIN_CAP on every input family, and the stress families are what
  they claim to be.
"""
import pytest
import torch

import transformer_backward_restatement as R

# The GPU tests hold the exact chain to 4 x the twin's error and state that no such limit exceeds 1e-5: the twin alone has to stay
# at or under a quarter of that on every input the GPU tests use.
LIMIT_CAP = 1e-5
TWIN_CAP = LIMIT_CAP / 4


def _head_parameters(a_dim, seed=3):
    from neural_jacobian_field_amd import synthetic
    shapes = {k: v for k, v in synthetic.model_shapes("jacobian_transformer", a_dim).items() if k.startswith("decoder.jacobian")}
    return {k[len("decoder."):]: v.double() for k, v in synthetic.seeded_state_dict(shapes, seed=seed).items()}


@pytest.mark.parametrize("a_dim", [1, 3, 6, 8])
def test_folded_stream_is_the_transformer_head(a_dim):
    from neural_jacobian_field_amd import training
    p = _head_parameters(a_dim)
    g = torch.Generator().manual_seed(a_dim)
    pts = 45
    xyz = torch.randn(pts, 63, generator=g, dtype=torch.float64)
    feats = torch.randn(pts, 512, generator=g, dtype=torch.float64)
    ref = training.transformer_head(p, xyz, feats)
    folded = training.folded_transformer(p)
    x0 = torch.nn.functional.linear(torch.cat([xyz, feats], -1), p["jacobian_query_mlp.weight"], p["jacobian_query_mlp.bias"])
    x = R.folded_stream(folded["mats"], folded["biases"], x0, a_dim)
    assert x.shape == (4, pts, 64) and torch.equal(x[0], x0)
    out = x[3] @ p["jacobian_head.weight"].t() + p["jacobian_head.bias"]
    err = R.rel(out, ref)
    print(f"A = {a_dim}: folded_stream vs transformer_head {err:.2e}")
    assert err <= 1e-11
    # slots >= keys are exactly 0 whatever Mqk holds there: junk in the unused rows / columns changes nothing
    junk = folded["mats"].clone()
    unused = (torch.arange(64) % 8) >= a_dim
    junk[:, 0, unused, :] = 7.0
    junk_b = folded["biases"].clone()
    junk_b[:, 0, unused] = -3.0
    if a_dim < 8:
        assert torch.equal(R.folded_stream(junk, junk_b, x0, a_dim), x)
        assert float(R.layer(junk[0], junk_b[0], x0, a_dim)["a"][:, unused].abs().max()) == 0.0


@pytest.mark.parametrize("keys,d_out_dim", [(1, 3), (3, 9), (6, 18), (8, 24), (8, 32)])
def test_chain_parameter_gradients_are_the_products_of_its_own_pairs(keys, d_out_dim):
    """g_mats = dY^T X and g_biases = column sums of dY, slot 4 l + (Mqk, Nov, W1', W2): autograd on the folded parameters against
    the pairs ``chain`` emits -- and dx0 / the whole chain against ONE autograd pass through the three layers and the head."""
    inp = R.inputs("all", 77, keys, d_out_dim, seed=keys)
    m64, b64 = inp["mats"].double(), inp["biases"].double()
    res = R.chain(m64, b64[:, :3], inp["head_w"].double(), inp["x"].double(), inp["d_out"].double(), keys)
    assert res["wg_x"].shape == res["wg_dy"].shape == (12, 77, 64) and res["sums"].shape == (12, 64)
    products = R.pair_products(res["wg_x"], res["wg_dy"])
    for l in range(3):
        for i in range(4):
            assert R.rel(products[l, i], res["g_mats"][l, i]) <= 1e-12, (l, i)
            assert R.rel(res["sums"][4 * l + i], res["g_biases"][l, i]) <= 1e-12, (l, i)
    # the layer-by-layer chain on the float64 stream itself is one backward pass through the whole head
    x0 = inp["x"][0].double().requires_grad_(True)
    m, b = m64.clone().requires_grad_(True), b64.clone().requires_grad_(True)
    stream = R.folded_stream(m, b, x0, keys)
    whole = R.chain(m64, b64[:, :3], inp["head_w"].double(), stream.detach(), inp["d_out"].double(), keys)
    g_x0, g_m, g_b = torch.autograd.grad(stream[3] @ inp["head_w"].double().t(), [x0, m, b], inp["d_out"].double())
    assert R.rel(whole["dx0"], g_x0) <= 1e-12 and R.rel(whole["g_mats"], g_m) <= 1e-12 and R.rel(whole["g_biases"], g_b) <= 1e-12
    # unused key slots carry no gradient
    unused = (torch.arange(64) % 8) >= keys
    assert keys == 8 or float(res["wg_dy"][0::4][:, :, unused].abs().max()) == 0.0


def _twin_errors(inp, keys):
    ref, tw = R.reference_and_twin(inp, keys)
    errs = {k: R.rel(v, R.rows26(ref)[k]) for k, v in R.rows26(tw).items()}
    products = R.pair_products(tw["wg_x"], tw["wg_dy"])
    errs.update({f"g_mats[{l},{i}]": R.rel(products[l, i], ref["g_mats"][l, i]) for l in range(3) for i in range(4)})
    return errs


@pytest.mark.parametrize("family", R.FAMILIES)
def test_fp32_twin_stays_under_the_cap(family):
    """Every tensor the GPU tests compare, every (keys, d_out) they use, a one-tile, a ragged and the large point count."""
    worst = (0.0, None)
    for points in (37, 300, 4096 + 13):
        for keys, d_out_dim in ((1, 3), (3, 9), (6, 18), (8, 24), (8, 32)):
            errs = _twin_errors(R.inputs(family, points, keys, d_out_dim), keys)
            k = max(errs, key=errs.get)
            worst = max(worst, (errs[k], (points, keys, d_out_dim, k)))
            assert errs[k] <= TWIN_CAP, (family, points, keys, d_out_dim, k, errs[k])
    print(f"fp32 twin, family {family}: worst {worst[0]:.2e} at {worst[1]} (cap {TWIN_CAP:.1e})")


def test_stress_families_are_what_they_claim():
    keys, pts = 6, 300
    inp = R.inputs("all", pts, keys, 18)
    rows = R.stress_rows(pts)
    x = inp["x"]
    assert float(x[0][rows["constant"]].var(-1, unbiased=False).max()) == 0.0                  # rstd = 1 / sqrt(eps)
    big = x[0][rows["large"]]
    assert float(big.abs().mean(-1).min()) > 0.9 * R.LARGE_X and 0.5 < float(big.var(-1).min()) and float(big.var(-1).max()) < 2.0
    assert float(inp["d_out"][rows["zero_d_out"]].abs().max()) == 0.0 and float(inp["d_out"].abs().sum(-1).min()) == 0.0
    for l in range(3):
        f = R.layer(inp["mats"][l], inp["biases"][l], x[l], keys)                                # in fp32, as the kernel sees it
        a = f["a"].reshape(pts, 8, 8)
        hard, soft = a[:, :R.ONEHOT_HEADS], a[:, R.ONEHOT_HEADS:]
        assert float(hard.max(-1).values.min()) == 1.0 and float(hard.sum(-1).max()) == 1.0     # one-hot to fp32
        assert float(soft.max(-1).values.median()) < 0.9
        assert float(a[:, :, keys:].abs().max()) == 0.0
        u = f["u"]
        assert float(u.max()) > R.GELU_TAIL and float(u.min()) < -R.GELU_TAIL
        d_gelu = torch.autograd.functional.jvp(torch.nn.functional.gelu, u, torch.ones_like(u))[1]
        # gelu' -> 1 / 0: the tail channels are u = +-8 + O(1), exactly 1 / 0 in fp32 for most points
        assert float(d_gelu[:, 0::4].min()) > 1.0 - 1e-3 and float(d_gelu[:, 1::4].abs().max()) < 1e-3
        assert float((d_gelu[:, 0::4] == 1.0).float().mean()) > 0.9 and float((d_gelu[:, 1::4].abs() < 1e-9).float().mean()) > 0.9
