"""The Jacobian head in another split precision than the density and colour networks: Model.set_precision(d,
jacobian_precision=j), NJF_PRECISION_MIXED(d, j) -- render_kernel<JKIND, P, DUMP, AF, PJ> and points_kernel<SRC, 3 | 4, P, PJ[, FEAT]>
with PJ != P.  Parity against the oracle and the reference's fixtures under the rules of the pure modes, and -- what a swapped
pair, a blob packed for the wrong precision or a map in the wrong channel order would break -- WHICH network ran in WHICH
precision: every output of one network alone equals, bit for bit, the pure run of that network's precision (the stages are the
same device functions with the same template arguments on the same inputs; the library is built with -ffp-contract=off).
The training forwards under the mixes: tests/test_training_gpu.py.  Run with -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
MIXES = (("f16f6", "f16x2"), ("f16x2", "f16f6"))
name_of = "/j:".join
# outputs that only the density + colour networks (and the samples) decide / that only the head decides
DENSITY_SIDE = ("density", "color", "weights", "rgb", "depth", "pos")
HEAD_SIDE = ("jacobian", "sample_flow")


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- a. parity of the fused forward, ResnetFC head --------------------------------------------------------------------------------
def _parity_cases():
    import parity_harness as ph
    from test_hip_parity import RAGGED
    return [("parity[1", 1, ph.PARITY_CASES[1]), ("parity[4", 4, ph.PARITY_CASES[4]), ("parity[ragged0", None, RAGGED[0])]


# the tensors of a parity case that have a sample axis ([B, R, S, *]): at least 1,024 elements in each of the three cases
PER_SAMPLE_ROWS = ("truth:s_weights", "truth:s_density", "truth:s_color", "truth:s_sample_flow", "truth:s_jacobian")


@pytest.mark.parametrize("which", range(3))
@pytest.mark.parametrize("precisions", MIXES, ids=name_of)
def test_fused_forward_matches_oracle_under_the_mixes(device, margins, precisions, which):
    """What tests/test_hip_parity.py::test_fused_forward_matches_oracle asserts of an accelerated mode, under both mixes, on
    PARITY_CASES[1] (B = 2, ragged ray count, 64 + 64 samples), PARITY_CASES[4] (general context pose) and RAGGED[0]: every
    norm-wise row within max(1e-4, 2 x floor) with the floor from the reference's fixture where the case has one, and the
    accelerated modes' element-wise criterion on every tensor of >= 1,024 elements.  Every per-sample tensor ([B, R, S, *]) of
    these shapes has that many, so none of them is left out; the per-ray composites at the oracle's bins (s_rgb, s_depth,
    s_optical_flow, s_pos, s_pos_warped: [B, R, 2 | 3], 120 ... 333 elements here) are asserted exactly where
    parity_harness.TRUTH_MIN_ELEMENTS says so, like in every other parity test."""
    import parity_harness as ph
    tag, case_id, cfg = _parity_cases()[which]
    d, j = precisions
    rep = ph.run_parity_case(device=device, tol=TOL, precision=d, jacobian_precision=j, case_id=case_id, **cfg)
    tag = f"{tag}:{name_of(precisions)}]"
    margins.record(tag, rep["rows"])
    margins.record_truth(tag, rep["truth_rows"], asserted=True)
    assert rep["precision"] == name_of(precisions)
    if case_id is not None:
        assert rep["floor_source"].startswith("reference"), rep["floor_source"]
    assert rep["ok"], {k: v for k, v in rep.items() if k not in ("rows", "truth_rows")}
    assert rep["truth_asserted_ok"], [r for r in rep["truth_rows"] if r["asserted_ok"] is False]
    rows = {r["key"]: r for r in rep["truth_rows"]}
    assert all(rows[k]["asserted_ok"] is not None for k in PER_SAMPLE_ROWS), {k: rows[k]["elements"] for k in PER_SAMPLE_ROWS}
    for k, r in rows.items():
        if k.startswith("truth:s_"):
            assert (r["asserted_ok"] is not None) == (r["elements"] >= ph.TRUTH_MIN_ELEMENTS), (k, r["elements"])


# ---- b. which head ran in which precision ------------------------------------------------------------------------------------------
def _render(fr, case, bins, device, s_final):
    """One render of ``case`` at the given final bins through the renderer ``fr`` (parity_harness.hip_forward's call)."""
    from neural_jacobian_field_amd.renderer import RenderRequest
    c = case["cams"]
    to = lambda t: t.to(device)
    fr.load_weights({k: to(v) for k, v in case["params"].items()})
    res = fr.render(to(case["feats"]).contiguous(), to(case["origins"]), to(case["directions"]), to(c["ctxt_c2w"]), to(c["ctxt_k_norm"]),
                    to(c["z_near"]), to(c["z_far"]), [s_final], s_final, trgt_c2w=to(c["trgt_c2w"]), trgt_k_pix=to(case["k_pix"]),
                    action=to(case["action"]), request=RenderRequest(vis=True, sample_weights=True, per_sample=True),
                    ctxt_w2c=to(torch.inverse(c["ctxt_c2w"])), trgt_w2c=to(torch.inverse(c["trgt_c2w"])), final_bins=to(bins))
    torch.cuda.synchronize(device)
    out = {k: v.clone() for k, v in res.extras.items()}
    out.update(rgb=res.rgb.clone(), depth=res.depth.clone(), optical_flow=res.optical_flow.clone())
    return out


@pytest.fixture(scope="module")
def selection_case(device):
    """B = 2, 16 x 16, 70 rays, 64 samples, general context pose, at the oracle's final bins; the pure runs X and F."""
    import parity_harness as ph
    from neural_jacobian_field_amd.renderer import FusedRenderer
    case = ph.make_case(2, 16, 16, 70, 8, seed=3, identity_context=False)
    ref = ph.oracle_forward(case, 64, 64)
    bins = torch.cat([ref.samples_list[1].spacing_starts[..., 0], ref.samples_list[1].spacing_ends[..., -1:, 0]], -1)
    pure = {p: _render(FusedRenderer(device, 1, 8, precision=p), case, bins, device, 64) for p in ("f16x2", "f16f6")}
    return case, bins, pure


def test_the_pure_runs_differ_so_that_equal_bits_say_something(selection_case):
    _, _, pure = selection_case
    x, f = pure["f16x2"], pure["f16f6"]
    assert not bits_equal(x["density"], f["density"]) and not bits_equal(x["jacobian"], f["jacobian"])
    assert not bits_equal(x["optical_flow"], f["optical_flow"])
    assert x["jacobian"].shape[-1] == 24 and x["density"].shape == (2, 70, 64, 1)


@pytest.mark.parametrize("precisions", MIXES, ids=name_of)
def test_each_network_of_a_mixed_render_equals_its_pure_run_bit_for_bit(device, selection_case, precisions):
    """render_kernel<1, P, 0, true, PJ>: density, colour, weights, rgb, depth and the composited position equal the pure run of
    the DENSITY precision bit for bit, the per-sample Jacobian and scene flow the pure run of the HEAD's precision.
    action_features, optical_flow and pos_warped depend on both networks: held to parity only (test above)."""
    from neural_jacobian_field_amd.renderer import FusedRenderer
    case, bins, pure = selection_case
    d, j = precisions
    fr = FusedRenderer(device, 1, 8, precision=d, jacobian_precision=j)
    assert fr.model.decoder.precision == d and fr.model.decoder.j_precision == j
    got = _render(fr, case, bins, device, 64)
    wrong = [k for k in DENSITY_SIDE if not bits_equal(got[k], pure[d][k])] + [k for k in HEAD_SIDE if not bits_equal(got[k], pure[j][k])]
    assert not wrong, {k: float((got[k] - pure[d if k in DENSITY_SIDE else j][k]).abs().max()) for k in wrong}
    # ... and not the other pure run's (the two pure runs differ, see above)
    assert not bits_equal(got["density"], pure[j]["density"]) and not bits_equal(got["jacobian"], pure[d]["jacobian"])
    for k in ("action_features", "optical_flow", "pos_warped"):
        assert torch.isfinite(got[k]).all(), k


# ---- f. the repack when only the head's precision changes --------------------------------------------------------------------------
def test_changing_the_heads_precision_alone_repacks_the_head(device, selection_case):
    """One model: "f16f6", then set_precision("f16f6", jacobian_precision="f16x2"), then "f16f6" again.  The third output is the
    first bit for bit, the second that of a freshly built mixed model bit for bit, and the second's flow differs from the first's
    (decoder._packed_version["jacobian"] carries the head's precision; the head's block of the hoisted map changes its channel
    order with it)."""
    from neural_jacobian_field_amd.renderer import FusedRenderer
    case, bins, pure = selection_case
    fr = FusedRenderer(device, 1, 8, precision="f16f6")
    first = _render(fr, case, bins, device, 64)
    fr.model.set_precision("f16f6", jacobian_precision="f16x2")
    second = _render(fr, case, bins, device, 64)
    fr.model.set_precision("f16f6")
    third = _render(fr, case, bins, device, 64)
    fresh = _render(FusedRenderer(device, 1, 8, precision="f16f6", jacobian_precision="f16x2"), case, bins, device, 64)
    assert set(first) == set(second) == set(third) == set(fresh)
    assert [k for k in first if not bits_equal(first[k], third[k])] == []
    assert [k for k in second if not bits_equal(second[k], fresh[k])] == []
    assert [k for k in first if not bits_equal(first[k], pure["f16f6"][k])] == []
    assert not bits_equal(second["optical_flow"], first["optical_flow"]) and not bits_equal(second["jacobian"], first["jacobian"])


# ---- c. the transformer head under both mixes ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def transformer_model_and_golden(device, golden):
    import test_model_api_gpu as api
    return api.make_transformer_model_and_golden(device, golden)


def _decoder_at_fixture_positions(model, g, d, j):
    """decoder.forward at the fixture's positions with the density / colour networks on ``d`` and the head on ``j``."""
    from neural_jacobian_field_amd import hip
    from neural_jacobian_field_amd.decoder import PixelEncoding
    enc = PixelEncoding(g["features"], g["ctxt_c2w"], g["ctxt_k_norm"], g["action"])
    pos = g["final_positions"]
    dirs = g["directions"][..., None, :].expand(pos.shape).contiguous()
    model.set_precision(d, jacobian_precision=j)
    try:
        dec = model.decoder.forward(pos, dirs, enc)
        return {k: getattr(dec, k).clone() for k in ("density", "color", "flow", "action_features")}
    finally:
        model.set_precision(hip.DEFAULT_PRECISION)


def _check_selection_at_points(model, g, head_differs=True):
    """``head_differs``: the head's own outputs differ between the two pure runs (they do for the ResnetFC head)."""
    pure = {p: _decoder_at_fixture_positions(model, g, p, p) for p in ("f16x2", "f16f6")}
    for k in ("density", "color") + (("action_features", "flow") if head_differs else ()):
        assert not bits_equal(pure["f16x2"][k], pure["f16f6"][k]), k
    for d, j in MIXES:
        got = _decoder_at_fixture_positions(model, g, d, j)
        wrong = [k for k in ("density", "color") if not bits_equal(got[k], pure[d][k])]
        wrong += [k for k in ("action_features", "flow") if not bits_equal(got[k], pure[j][k])]
        assert not wrong, (d, j, wrong)
        assert not bits_equal(got["density"], pure[j]["density"])
        if head_differs:
            assert not bits_equal(got["flow"], pure[d]["flow"])


@pytest.mark.parametrize("precisions", MIXES, ids=name_of)
def test_transformer_decoder_at_reference_sample_locations_under_the_mixes(transformer_model_and_golden, margins, precisions):
    import test_model_api_gpu as api
    from neural_jacobian_field_amd import hip
    model, g = transformer_model_and_golden
    model.set_precision(precisions[0], jacobian_precision=precisions[1])
    try:
        api.check_transformer_decoder_at_reference_positions(model, g, margins, f"model_transformer[{name_of(precisions)}].decoder@ref-positions")
    finally:
        model.set_precision(hip.DEFAULT_PRECISION)


@pytest.mark.parametrize("precisions", MIXES, ids=name_of)
def test_transformer_model_forward_vs_reference_golden_under_the_mixes(transformer_model_and_golden, margins, precisions):
    import test_model_api_gpu as api
    from neural_jacobian_field_amd import hip
    model, g = transformer_model_and_golden
    model.set_precision(precisions[0], jacobian_precision=precisions[1])
    try:
        api.check_transformer_model_forward(model, g, margins, f"model_transformer[{name_of(precisions)}].forward")
    finally:
        model.set_precision(hip.DEFAULT_PRECISION)


@pytest.mark.parametrize("precisions", MIXES, ids=name_of)
def test_transformer_head_with_eight_keys_under_the_mixes(device, golden, margins, precisions):
    import test_model_api_gpu as api
    api.check_transformer_head_with_eight_keys(device, golden, margins, f"model_transformer8[{name_of(precisions)}]", precisions=precisions)


def test_transformer_decoder_at_points_selects_each_networks_precision(transformer_model_and_golden):
    """points_kernel<SRC, 4, P, PJ>: density and colour from the pure run of the density precision, action features and flow
    from the pure run of the head's precision, bit for bit.  The two pure runs of THIS head give the same bits (measured: its
    64-wide layers have one split form, launch_pack keeps narrow layers in the f16x2 chunk form under "f16f6"; what "f16f6"
    changes for it is the channel order of its block of the hoisted map and the gather that reads it, which sum the same four
    terms), so the head's equalities here say: the right blob behind the density blob, and a map in the order the gather of
    PJ reads -- either mistake gives other numbers than both pure runs -- not which of two arithmetics ran."""
    _check_selection_at_points(*transformer_model_and_golden, head_differs=False)


# ---- d. the points evaluator and the field extraction, ResnetFC and flow heads -------------------------------------------------------
@pytest.fixture(scope="module")
def model_and_golden(device, golden):
    import test_model_api_gpu as api
    return api.make_model_and_golden(device, golden)


@pytest.fixture(scope="module")
def flow_model_and_golden(device, golden):
    import test_model_api_gpu as api
    return api.make_flow_model_and_golden(device, golden)


@pytest.mark.parametrize("precisions", MIXES, ids=name_of)
def test_decoder_forward_at_reference_sample_locations_under_the_mixes(model_and_golden, margins, precisions):
    """points_kernel<SRC, 3, P, PJ> behind decoder.forward, encode_image and compute_density of the jacobian_mlp fixture: the
    margins of tests/test_model_api_gpu.py::test_decoder_forward_at_reference_sample_locations."""
    import test_model_api_gpu as api
    from neural_jacobian_field_amd import hip
    model, g = model_and_golden
    model.set_precision(precisions[0], jacobian_precision=precisions[1])
    try:
        api.check_mlp_decoder_at_reference_positions(model, g, margins, f"model_mlp[{name_of(precisions)}].decoder@ref-positions")
    finally:
        model.set_precision(hip.DEFAULT_PRECISION)


def test_mlp_decoder_at_points_selects_each_networks_precision(model_and_golden):
    _check_selection_at_points(*model_and_golden)


@pytest.mark.parametrize("precisions", MIXES, ids=name_of)
def test_flow_mlp_decoder_at_reference_sample_locations_under_the_mixes(flow_model_and_golden, margins, precisions):
    """The flow head's 640 hidden features come out of the FEAT instantiation, points_kernel<SRC, 3, P, PJ, true>: the margins of
    tests/test_model_api_gpu.py::test_flow_mlp_decoder_at_reference_sample_locations, and the features themselves equal the pure
    run of the head's precision bit for bit."""
    import test_model_api_gpu as api
    from neural_jacobian_field_amd import hip
    model, g = flow_model_and_golden
    d, j = precisions
    pure = _decoder_at_fixture_positions(model, g, j, j)
    other = _decoder_at_fixture_positions(model, g, d, d)
    model.set_precision(d, jacobian_precision=j)
    try:
        dec = api.check_flow_mlp_decoder_at_reference_positions(model, g, margins, f"model_flow[{name_of(precisions)}].decoder@ref-positions")
    finally:
        model.set_precision(hip.DEFAULT_PRECISION)
    assert bits_equal(dec.action_features, pure["action_features"]) and bits_equal(dec.flow, pure["flow"])
    assert bits_equal(dec.density, other["density"]) and bits_equal(dec.color, other["color"])
    assert not bits_equal(pure["action_features"], other["action_features"]) and not bits_equal(pure["density"], other["density"])


def test_field_extraction_selects_each_networks_precision(device):
    """extract_field(..., want_jacobian=True) on a 13 x 11 x 9 grid under both mixes: the same nodes survive as in the pure run
    of the DENSITY precision, with the same densities and colours bit for bit, and the Jacobians of the nodes that also survive in
    the pure run of the HEAD's precision (the two pure runs select by densities that differ in the last bits) equal that run's
    bit for bit."""
    from neural_jacobian_field_amd import hip, synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.field_volume import FieldGrid, extract_field
    from neural_jacobian_field_amd.model import Model
    model = Model(model_cfg_from_dict({"action_dim": 8, "rendering": {"num_proposal_samples": [16], "num_nerf_samples": 12},
                                       "action_decoder": {"name": "jacobian_mlp"}}))
    model.load_state_dict(synthetic.seeded_state_dict(synthetic.model_shapes("jacobian_mlp", 8), seed=0), strict=True)
    model.to(device).eval().requires_grad_(False)
    c2w = synthetic.general_pose(7, 2, scale=0.04)
    c2w[0] = torch.eye(4)
    enc = PixelEncoding(features=synthetic.synthetic_features(2, 16, 16, seed=1).to(device), extrinsics=c2w.to(device),
                        intrinsics=synthetic.synthetic_cameras(2)["ctxt_k_norm"].to(device),
                        action=synthetic.synthetic_action(2, 8).to(device))
    grid = FieldGrid.from_bounds((-0.97, -0.91, 0.83), (1.03, 0.87, 2.05), (13, 11, 9))
    head, _ = model.compute_density(grid.points(device=device)[None].expand(2, -1, 3).contiguous(), enc)
    threshold = float(torch.quantile(head.density.reshape(-1).double().cpu(), 0.6))

    def extract(d, j):
        model.set_precision(d, jacobian_precision=j)
        try:
            return extract_field(model, enc, grid, threshold, want_jacobian=True)
        finally:
            model.set_precision(hip.DEFAULT_PRECISION)

    pure = {p: extract(p, p) for p in ("f16x2", "f16f6")}
    assert all(cloud.index.shape[0] > 100 for cloud in pure.values())
    both = torch.isin(pure["f16x2"].index, pure["f16f6"].index)
    assert not bits_equal(pure["f16x2"].jacobian[both], pure["f16f6"].jacobian[torch.isin(pure["f16f6"].index, pure["f16x2"].index)])
    for d, j in MIXES:
        got = extract(d, j)
        assert torch.equal(got.index, pure[d].index), (d, j)
        assert bits_equal(got.density, pure[d].density) and bits_equal(got.color, pure[d].color) and bits_equal(got.xyz, pure[d].xyz)
        mine, theirs = torch.isin(got.index, pure[j].index), torch.isin(pure[j].index, got.index)
        assert int(mine.sum()) > 100 and torch.equal(got.index[mine], pure[j].index[theirs])
        assert got.jacobian.shape[1:] == (8, 3) and bits_equal(got.jacobian[mine], pure[j].jacobian[theirs]), (d, j)
        assert not bits_equal(got.jacobian[mine], pure[d].jacobian[mine])
