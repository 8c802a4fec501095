"""The ends of the action dimension.  The fused forward is otherwise tested at A = 3, 6 and 8; the ResnetFC head takes A <= 10 (30
of its 32 output rows), the transformer head A <= 8 (its key slots).  Here: A = 1, 2, 7, 9, 10 through render_kernel and
points_kernel with the ResnetFC head, A = 1, 2, 7 with the transformer head, the index mapping of the flow contraction channel
by channel, and action-mode training at A = 10 / A = 7.  (The limits themselves: tests/test_precision_codes_cpu.py.)
Run with -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
MIXES = (("f16f6", "f16x2"), ("f16x2", "f16f6"))
EDGE_SHAPE = dict(batch=2, height=16, width=16, rays=37, s_prop=33, s_final=31)


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


# ---- a. the ResnetFC head at A = 1, 2, 7, 9, 10 -------------------------------------------------------------------------------------
RESNET_EDGES = [(a, p, None) for a in (1, 2, 7, 9, 10) for p in ("f32", "f16x2", "f16f6")] + [(10, d, j) for d, j in MIXES]


@pytest.mark.parametrize("A,precision,jacobian_precision", RESNET_EDGES,
                         ids=[f"A{a}-{p}" + (f"/j:{j}" if j else "") for a, p, j in RESNET_EDGES])
def test_fused_forward_matches_oracle_at_the_ends_of_the_action_dimension(device, margins, A, precision, jacobian_precision):
    """B = 2, 16 x 16, 37 rays, 33 + 31 samples: every row within max(1e-4, 2 x the oracle's own fp32-vs-float64 difference) --
    6e-5 ... 5e-4 on the flow of these cases --, the split modes' element-wise criterion on every tensor of >= 1,024 elements,
    and 3 A channels in the per-sample Jacobian and the composited action features (lin_out packed with d_out = 3 A < 32, the
    `d < 3 A` stores; at A = 10 rows 30 and 31 of the head exist only as padding)."""
    import parity_harness as ph
    from neural_jacobian_field_amd.renderer import RenderRequest
    rep = ph.run_parity_case(device=device, tol=TOL, precision=precision, jacobian_precision=jacobian_precision, action_dim=A,
                             **EDGE_SHAPE)
    tag = f"parity[A={A}:{rep['precision']}]"
    margins.record(tag, rep["rows"])
    margins.record_truth(tag, rep["truth_rows"], asserted=precision != "f32")
    assert rep["ok"], {k: v for k, v in rep.items() if k not in ("rows", "truth_rows")}
    if precision != "f32":
        assert rep["truth_asserted_ok"], [r for r in rep["truth_rows"] if r["asserted_ok"] is False]
        assert rep["truth_asserted_rows"] > 0
    case = ph.make_case(EDGE_SHAPE["batch"], 16, 16, EDGE_SHAPE["rays"], A)
    res, _, _ = ph.hip_forward(case, 33, 31, device, request=RenderRequest(vis=True, sample_weights=True, per_sample=True),
                               precision=precision, jacobian_precision=jacobian_precision)
    assert res.extras["jacobian"].shape == (2, 37, 31, 3 * A) and res.extras["action_features"].shape == (2, 37, 3 * A)
    assert torch.isfinite(res.extras["jacobian"]).all() and torch.isfinite(res.extras["action_features"]).all()


# ---- b. the index mapping of the flow contraction -----------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [10, 7])
def test_flow_contraction_maps_channel_k_to_outputs_3k_to_3k_plus_2(device, A):
    """Logical output d of the head belongs to channel d / 3; channel 5 straddles the two half-waves (d = 15 | 16), channel 9 ends
    at row 29 next to the padding rows.  With the action set to the one-hot e_k the contraction sum_a J[a, s] u[a] has one term
    times 1 and A - 1 terms times 0, so it is exact in any order, fused or not: sample_flow[..., s] == jacobian[..., 3 k + s]
    (compared with ==: a sum of signed zeros may come out as +0 where J holds -0), for every k, in the render kernel (B = 1,
    3 rays, 8 samples at fixed bins, exact-fp32 products) and in the points evaluator (decoder.forward).  The Jacobian itself
    does not depend on the action."""
    import parity_harness as ph
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.renderer import FusedRenderer, RenderRequest
    case = ph.make_case(1, 16, 16, 3, A, seed=2, identity_context=False)
    c = case["cams"]
    to = lambda t: t.to(device)
    fr = FusedRenderer(device, 1, A, precision="f32")
    fr.load_weights({k: to(v) for k, v in case["params"].items()})
    feats = to(case["feats"]).contiguous()
    bins = to(torch.linspace(0.0, 1.0, 9).expand(1, 3, 9).contiguous())
    t = torch.linspace(0.2, 0.9, 5)[None, None, :, None] * (c["z_far"] - c["z_near"])[:, None, None, None] + c["z_near"][:, None, None, None]
    pos = to((case["origins"][:, :, None, :] + case["directions"][:, :, None, :] * t).contiguous())
    dirs = to(case["directions"][:, :, None, :].expand(pos.shape).contiguous())
    first = None
    for k in range(A):
        e_k = torch.zeros(1, A)
        e_k[0, k] = 1.0
        res = fr.render(feats, to(case["origins"]), to(case["directions"]), to(c["ctxt_c2w"]), to(c["ctxt_k_norm"]), to(c["z_near"]),
                        to(c["z_far"]), [8], 8, trgt_c2w=to(c["trgt_c2w"]), trgt_k_pix=to(case["k_pix"]), action=to(e_k),
                        request=RenderRequest(vis=True, sample_weights=True, per_sample=True), final_bins=bins)
        jac, flow = res.extras["jacobian"].clone(), res.extras["sample_flow"].clone()
        assert jac.shape == (1, 3, 8, 3 * A) and flow.shape == (1, 3, 8, 3)
        assert bool((flow == jac[..., 3 * k:3 * k + 3]).all()), (k, float((flow - jac[..., 3 * k:3 * k + 3]).abs().max()))
        dec = fr.model.decoder.forward(pos, dirs, PixelEncoding(feats, to(c["ctxt_c2w"]), to(c["ctxt_k_norm"]), to(e_k)))
        pj, pf = dec.action_features.clone(), dec.flow.clone()
        assert pj.shape == (1, 3, 5, 3 * A) and pf.shape == (1, 3, 5, 3)
        assert bool((pf == pj[..., 3 * k:3 * k + 3]).all()), (k, float((pf - pj[..., 3 * k:3 * k + 3]).abs().max()))
        if first is None:
            first = (jac, pj)
            # the channels are distinguishable: no two of them hold the same values
            assert all(not torch.equal(jac[..., 3 * a:3 * a + 3], jac[..., 3 * b:3 * b + 3]) for a in range(A) for b in range(a))
            assert float(jac.abs().min(dim=-1).values.max()) > 0    # every one of the 3 A outputs is live somewhere
        else:
            assert torch.equal(jac, first[0]) and torch.equal(pj, first[1]), k


# ---- c. the transformer head at A = 1, 2, 7 -----------------------------------------------------------------------------------------
_TRANSFORMER_REFERENCES = {}


def _transformer_references(A):
    """The oracle on the seeded ``jacobian_transformer`` case of ``A`` keys, in fp32 and in float64: Model.forward end to end, and
    the decoder at the fp32 run's sample positions."""
    import njf_oracle as orc
    import parity_harness as ph
    if A not in _TRANSFORMER_REFERENCES:
        case = ph.make_case(2, 16, 16, 37, A, seed=5, identity_context=False, decoder="jacobian_transformer")
        assert case["decoder_kind"] == "jacobian_transformer"
        ref32, ref64 = ph.oracle_forward(case, 33, 31), ph.oracle_forward_fp64(case, 33, 31)
        pos = ref32.positions
        dirs = case["directions"][..., None, :].expand(pos.shape).contiguous()
        c = case["cams"]

        def decoder(cv):
            enc = orc.PixelEncoding(cv(case["feats"]), cv(c["ctxt_c2w"]), cv(c["ctxt_k_norm"]), cv(case["action"]))
            params = {k[len("decoder."):]: cv(v) for k, v in case["params"].items() if k.startswith("decoder.")}
            return orc.decoder_forward(params, cv(pos), cv(dirs), enc, "jacobian_transformer", A)

        prev = torch.get_default_dtype()
        dec32 = decoder(lambda v: v)
        torch.set_default_dtype(torch.float64)
        try:
            dec64 = decoder(lambda v: v.double())
        finally:
            torch.set_default_dtype(prev)
        _TRANSFORMER_REFERENCES[A] = (case, ref32, ref64, pos, dirs, dec32, dec64)
    return _TRANSFORMER_REFERENCES[A]


@pytest.mark.parametrize("precision", ["default", "f32"])
@pytest.mark.parametrize("A", [1, 2, 7])
def test_transformer_head_at_the_ends_of_its_key_range(device, margins, A, precision):
    """The key mask `a < keys` of transformer_tile with one, two and seven live keys (the fixtures have six and eight): the fused
    forward and decoder.forward on a seeded state dict against the oracle in fp32, bound max(1e-4, 2 x |oracle fp32 - oracle
    float64|) per output.  At A = 1 the softmax has a single key, but the head's output still depends on the query through the
    residual connections (the oracle's Jacobian moves by 0.5 of its scale when jacobian_query_mlp's weights are scaled by 1.5),
    so there is no independence of the query to assert."""
    import parity_harness as ph
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.renderer import RenderRequest
    case, ref32, ref64, pos, dirs, dec32, dec64 = _transformer_references(A)
    p = None if precision == "default" else precision
    res, fr, gmap = ph.hip_forward(case, 33, 31, device, request=RenderRequest(vis=True, sample_weights=True, per_sample=True), precision=p)
    assert fr.model.decoder.JACOBIAN_KIND == 2 and res.extras["jacobian"].shape == (2, 37, 31, 3 * A)
    tag = f"transformer[A={A}:{precision}]"
    margins(tag + ".forward", "rgb", res.rgb, ref32.rgb, ref64.rgb)
    margins(tag + ".forward", "depth", res.depth, ref32.depth, ref64.depth)
    margins(tag + ".forward", "optical_flow", res.optical_flow, ref32.optical_flow, ref64.optical_flow)
    margins(tag + ".forward", "action_features", res.extras["action_features"], ref32.action_features, ref64.action_features)
    c = case["cams"]
    to = lambda t: t.to(device)
    dec = fr.model.decoder.forward(to(pos), to(dirs), PixelEncoding(gmap, to(c["ctxt_c2w"]), to(c["ctxt_k_norm"]), to(case["action"])))
    for key, got, i in (("density", dec.density, 0), ("color", dec.color, 1), ("flow", dec.flow, 2), ("action_features", dec.action_features, 3)):
        margins(tag + ".decoder@oracle-positions", key, got, dec32[i], dec64[i])
    assert dec.action_features.shape == (2, 37, 31, 3 * A)


# ---- d. action-mode training at the limits ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup10():
    import test_training_gpu as T
    return T.build_setup(action_dim=10)


def test_action_mode_gradients_at_ten_channels(setup10, margins):
    """tests/test_training_gpu.py::test_action_mode_gradients_match_oracle_autograd with A = 10: lin_out of the backward chain at
    d_out = 30, the flow contraction's adjoint over ten channels."""
    import test_training_gpu as T
    assert setup10["model"].decoder.jacobian_head.lin_out.weight.shape == (30, 128)
    T.check_action_mode_gradients(setup10, margins, tag="train.action[jacobian_mlp:A=10]")


def test_transformer_action_mode_gradients_at_seven_keys(setup10, margins):
    """tests/test_training_gpu.py::test_transformer_action_mode_gradients_match_oracle_autograd with A = 7 (the rays, cameras and
    target of the set-up above; the transformer model is the test's own)."""
    import test_training_gpu as T
    T.check_transformer_action_mode_gradients(setup10, margins, A=7, tag="train.action[jacobian_transformer:A=7]")
