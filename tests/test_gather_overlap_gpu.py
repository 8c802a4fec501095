"""GPU tests of the exact-fp32 inference passes with the lin_z gathers folded under the preceding layer
(njf_device.h::mma_chunk_gather_f32).  Everything runs in "f32".  Run with -m gpu.

Cases: R = 1, 3 and 5 rays per image x 64 proposal + 64 final samples on a 16 x 16 x 512 feature map with B = 2 -- 2, 6 and 10
rays for workgroups of 4: at R = 1 the only workgroup is half empty, at R = 3 and R = 5 the last one is ragged.  The context
camera is moved sideways so that the near part of every ray projects outside the context view and the far part inside it:
the border-clamped footprint and the in-view path both run (asserted on the case itself).  Jacobian head: jacobian_mlp, A = 8.

Checked: (1) proposal weights, final bins, per-sample density and Jacobian, rgb, depth and flow against the CPU oracle under
tests/test_hip_parity.py's rule max(1e-4, 2 x the oracle's fp32-vs-fp64 floor); (2) the inference route against the dump route
(training forwards: the serial gather between the layers) bit for bit -- both run the same products and the same folds in the
same order; (3) two consecutive calls return identical bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
RAYS = [1, 3, 5]
SHAPE = dict(batch=2, height=32, width=32, s_prop=64, s_final=64, action_dim=8)   # the encoder map is H/2 x W/2 = 16 x 16
SEED = 23            # (a seed no other test uses: the harness caches oracle runs by case key)
CTXT_SHIFT_X = 1.5   # context camera at x = 1.5: x_c / z < -0.625 (outside the view) for the near samples of every ray


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need an MI355X")
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


import parity_harness as _ph

_harness_make_case = _ph.make_case   # (the parity test below replaces the harness's own with _make_case)


def _make_case(rays):
    case = _harness_make_case(SHAPE["batch"], SHAPE["height"], SHAPE["width"], rays, SHAPE["action_dim"], seed=SEED)
    case["cams"]["ctxt_c2w"][:, 0, 3] = CTXT_SHIFT_X
    return case


def _out_of_view_fraction(case, samples=64):
    """Share of uniformly spaced sample points whose projection into the context camera leaves [0, 1]^2."""
    c = case["cams"]
    t = torch.linspace(0.0, 1.0, samples)[None, None, :, None]
    z = c["z_near"][:, None, None, None] * (1 - t) + c["z_far"][:, None, None, None] * t
    pts = case["origins"][:, :, None, :] + case["directions"][:, :, None, :] * z
    w2c = torch.inverse(c["ctxt_c2w"])
    cam = torch.einsum("bij,brsj->brsi", w2c[:, :3, :3], pts) + w2c[:, None, None, :3, 3]
    uv = torch.einsum("bij,brsj->brsi", c["ctxt_k_norm"], cam)
    uv = uv[..., :2] / uv[..., 2:]
    outside = ((uv < 0) | (uv > 1)).any(-1)
    return float(outside.float().mean())


@pytest.fixture(scope="module")
def cases():
    return {r: _make_case(r) for r in RAYS}


@pytest.mark.parametrize("rays", RAYS)
def test_rays_leave_and_enter_the_context_view(cases, rays):
    """(no GPU work) the camera placement does what the cases are for: some samples outside the view, some inside"""
    frac = _out_of_view_fraction(cases[rays])
    assert 0.05 < frac < 0.95, frac


@pytest.mark.parametrize("rays", RAYS)
def test_fused_gather_matches_oracle(device, rays, margins, monkeypatch):
    import parity_harness as ph
    monkeypatch.setattr(ph, "make_case", lambda *a, **k: _make_case(rays))
    rep = ph.run_parity_case(device=device, tol=TOL, precision="f32", rays=rays, seed=SEED, **SHAPE)
    margins.record(f"gather-overlap[R={rays}:f32]", rep["rows"])
    margins.record_truth(f"gather-overlap[R={rays}:f32]", rep["truth_rows"], asserted=False)
    rows = {r["key"]: r for r in rep["rows"]}
    for key in ("prop_weights", "final_bins", "s_density", "s_jacobian", "rgb", "depth", "optical_flow"):
        print(key, rows[key])
        assert rows[key]["ok"], rows[key]
    assert rep["floor_source"] == "oracle fp32 vs fp64", rep["floor_source"]
    assert rep["ok"], {k: v for k, v in rep.items() if k not in ("rows", "truth_rows")}


def _routes(case, device):
    """Model._fused_render on one case: inference, Jacobian-dump and perception-dump forwards (and inference again)."""
    import parity_harness as ph
    from neural_jacobian_field_amd.model import CameraInput, RenderingInput, RobotInput
    from neural_jacobian_field_amd.renderer import FusedRenderer
    c = case["cams"]
    dev = lambda t: t.to(device)
    fr = FusedRenderer(device, 1, SHAPE["action_dim"], precision="f32")
    fr.load_weights({k: dev(v) for k, v in case["params"].items()})
    m = fr.model
    m.cfg.rendering.num_proposal_samples = (SHAPE["s_prop"],)
    m.cfg.rendering.num_nerf_samples = SHAPE["s_final"]
    m.proposal_sampler.num_proposal_samples_per_ray = (SHAPE["s_prop"],)
    m.proposal_sampler.num_nerf_samples_per_ray = SHAPE["s_final"]
    m.encoder.set_features(dev(case["feats"]).contiguous())
    cam = CameraInput(input_image=None, ctxt_extrinsics=dev(c["ctxt_c2w"]), ctxt_intrinsics=dev(c["ctxt_k_norm"]),
                      trgt_extrinsics=dev(c["trgt_c2w"]), trgt_intrinsics=dev(case["k_pix"]))
    rin = RenderingInput(dev(case["origins"]), dev(case["directions"]), dev(c["z_near"]), dev(c["z_far"]))
    robot = RobotInput(dev(case["action"]))

    def run(**kw):
        with torch.no_grad():
            outs, bins, weights_list, _, _ = m._fused_render(
                cam, rin, robot, m._encode_for_render(None), want_lists=True, want_vis=False, want_samples=True,
                ctxt_w2c=dev(torch.inverse(c["ctxt_c2w"])), trgt_w2c=dev(torch.inverse(c["trgt_c2w"])), **kw)
        torch.cuda.synchronize(device)
        keep = {k: outs[k].clone() for k in ("rgb", "depth", "flow", "density", "jacobian", "weights")}
        keep["bins"] = bins.clone()
        keep["prop_weights"] = weights_list[0].clone()
        return keep

    return {"inference": run(), "jacobian_dump": run(dump_jacobian=True), "perception_dump": run(dump_perception=True),
            "inference_again": run()}


@pytest.fixture(scope="module")
def routes(device, cases):
    return {r: _routes(cases[r], device) for r in RAYS}


@pytest.mark.parametrize("rays", RAYS)
def test_inference_route_equals_serial_dump_route(routes, rays):
    """The dump instantiations keep the serial gather (they write h out between gather and layer): the proposal network and
    the density network under the perception dump, the Jacobian head under the Jacobian dump.  Same products, same order."""
    r = routes[rays]
    inf = r["inference"]
    for route in ("jacobian_dump", "perception_dump"):
        for key in ("prop_weights", "bins", "density", "jacobian", "weights", "rgb", "depth", "flow"):
            assert torch.isfinite(inf[key]).all(), key
            assert torch.equal(inf[key], r[route][key]), (route, key, float((inf[key] - r[route][key]).abs().max()))


@pytest.mark.parametrize("rays", RAYS)
def test_two_calls_return_identical_bits(routes, rays):
    a, b = routes[rays]["inference"], routes[rays]["inference_again"]
    for key in a:
        assert torch.equal(a[key], b[key]), key
