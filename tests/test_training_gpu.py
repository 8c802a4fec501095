"""Action-mode training: gradients of the flow loss w.r.t. the Jacobian head (HIP forward + dumped activations +
library-GEMM backward) against autograd of the CPU oracle.  Run with -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def ulp_nudged(t, seed):
    """Every element moved by one unit in the last place, up or down at random (seeded): the smallest input change any fp32
    implementation of the ray generation may produce -- the perturbation tests/golden/make_golden_r02.py applies to the
    reference for its floor_ulp figures."""
    g = torch.Generator().manual_seed(seed)
    up = torch.rand(t.shape, generator=g) < 0.5
    return torch.where(up, torch.nextafter(t, torch.full_like(t, float("inf"))), torch.nextafter(t, torch.full_like(t, float("-inf"))))


def noisy(t, scale=2e-7, seed=1234):
    """t + scale * max|t| * n, n ~ N(0,1) seeded: the size of the difference between two fp32 encoders.  MIOpen's convolutions
    against ATen's CPU ones measure 6.6e-7 of max|features| on the reference's fixture (row model_mlp.encoder / features of
    the margins table); additive noise of sigma = 2e-7 max|t| has its largest element near 1e-6 max|t|.  Round 2 assumed a
    relative 1e-5 on every element."""
    g = torch.Generator().manual_seed(seed)
    return t + (scale * t.detach().abs().max() * torch.randn(t.shape, generator=g)).to(t.dtype)


RAY_SEEDS = (1, 2, 3, 4)
FEATURE_SEEDS = (11, 12, 13)
FLOOR_MODES = ("fp64",) + tuple(f"rays{s}" for s in RAY_SEEDS) + tuple(f"features{s}" for s in FEATURE_SEEDS)
# Round 4: there is no fixed gradient ceiling any more.  Rounds 2-3 passed ~90 perception-mode gradient rows on a 5e-3 bound
# because every proposal-net gradient sat 2.3-2.9e-3 from the oracle; the cause was `1 - exp(-ds)` quantising tiny weights to
# multiples of 2^-24 (device expf and torch's Sleef rounding to different neighbours) under the ds-nerf loss's 1 / (w + 1e-7)
# -- fixed in the kernels (csrc: alpha_of).  Every gradient row is now held to max(1e-4, 2 x its own floors) like any other.


def feature_seed(mode):
    """Seed of a "features<seed>" floor mode (None for every other mode): the ENCODER OUTPUT moved by the measured size of the
    MIOpen-vs-ATen difference.  This is the dominant real discrepancy between the HIP path and the oracle in the gradient
    tests (tools/diag/diag_perception.py: it moves the proposal weights by 1.4e-5 and, through the ds-nerf loss's
    1 / (w + 1e-7), their upstream gradient by 4.6 %), so the floor models it where it arises -- at the feature level, also
    when the encoder trains."""
    return int(mode[8:]) if mode is not None and mode.startswith("features") else None


def moved_rays(origins, directions, mode):
    """(origins, directions) of an oracle run: both moved by one ulp at random for the "rays<seed>" floors."""
    if mode is not None and mode.startswith("rays"):
        seed = int(mode[4:])
        return ulp_nudged(origins, seed), ulp_nudged(directions, 100 + seed)
    return origins, directions


def gradient_floor(run_oracle_backward, names):
    """What fp32 arithmetic itself costs the ORACLE's gradients: its fp32 run against its own float64 run ("fp64": the
    ds-nerf depth loss differentiates log(w + eps) of tiny weights, ~2e-3 on its own), and how far its fp32 gradients move
    under input changes no fp32 implementation can avoid -- ray origins and directions moved by one ulp at random, four seeds
    ("rays1".."rays4": the samplers' inverse-CDF placement and the 2*pi*512-gain encoding amplify it) and the encoder's
    output / input moved by 1e-6 of its largest element ("features").  `run_oracle_backward(mode)` returns {name: gradient}.  Returns, PER PARAMETER, the fp64 floor and
    the largest of all floors (the `margins` rule consults the latter only where twice the former fails), and the base run."""
    base = run_oracle_backward(None)
    moved = {mode: run_oracle_backward(mode) for mode in FLOOR_MODES}
    floor64 = {n: rel(moved["fp64"][n], base[n]) for n in names}
    floor_all = {n: max(rel(m[n], base[n]) for m in moved.values()) for n in names}
    return floor64, floor_all, base


def as_dtype(mode):
    """Tensor converter of an oracle run: float64 for the "fp64" floor, identity otherwise."""
    if mode == "fp64":
        return lambda t: t.double() if torch.is_tensor(t) and t.is_floating_point() else t
    return lambda t: t


# the two mixed forms of Model.set_precision(d, jacobian_precision=j): the Jacobian head in the OTHER split precision
HEAD_MIXES = (("f16f6", "f16x2"), ("f16x2", "f16f6"))
# Oracle gradients and their floors, per test body and action dimension: they depend on the case alone, not on the MFMA precision
# under test, so the runs of one body under several precisions share them (each is nine CPU evaluations of the oracle)
_ORACLE_RUNS = {}


def build_setup(action_dim=8):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    import parity_harness as ph
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import CameraInput, Model, RenderingInput, RobotInput
    dev = torch.device("cuda:0")
    B, H, W, R, S = 2, 16, 16, 40, 32
    case = ph.make_case(B, H, W, R, action_dim, seed=4)
    full = synthetic.seeded_state_dict(synthetic.model_shapes("jacobian_mlp", action_dim), seed=4)
    full.update(case["params"])  # decoder / proposal weights of the case + a seeded encoder
    model = Model(model_cfg_from_dict({"action_dim": action_dim, "rendering": {"num_proposal_samples": [S], "num_nerf_samples": S},
                                       "action_decoder": {"name": "jacobian_mlp"}}))
    model.load_state_dict(full, strict=True)
    model.to(dev).eval()
    # reference action mode: only the Jacobian head trains (models/model_wrapper.py:75-85)
    model.decoder.freeze_non_action_parameters()
    for n, p in model.named_parameters():
        if "decoder" not in n:
            p.requires_grad = False
    g2 = torch.Generator().manual_seed(9)
    image = torch.rand(B, 3, H, W, generator=g2)
    target = torch.randn(B, R, 2, generator=g2) * 3
    c = case["cams"]
    d = lambda t: t.to(dev)
    cam = CameraInput(d(image), d(c["ctxt_c2w"]), d(c["ctxt_k_norm"]), d(c["trgt_c2w"]), d(case["k_pix"]))
    rin = RenderingInput(d(case["origins"]), d(case["directions"]), d(c["z_near"]), d(c["z_far"]))
    rob = RobotInput(d(case["action"]))
    return dict(model=model, case=case, full=full, image=image, target=target, cam=cam, rin=rin, rob=rob, dev=dev, S=S)


@pytest.fixture(scope="module")
def setup():
    return build_setup()


def fused_render_outputs(model):
    """Context manager: the output dictionaries of every Model._fused_render call made inside it (the activation dumps of a
    training forward among them), in call order."""
    import contextlib

    @contextlib.contextmanager
    def scope():
        seen, real = [], model._fused_render

        def spy(*args, **kwargs):
            res = real(*args, **kwargs)
            seen.append(res[0])
            return res

        model._fused_render = spy
        try:
            yield seen
        finally:
            del model._fused_render
    return scope()


def head_precisions(model, precisions):
    """Context manager: ``Model.set_precision(d, jacobian_precision=j)`` for ``precisions = (d, j)`` (None: nothing changes), the
    package's default precision afterwards."""
    import contextlib
    from neural_jacobian_field_amd import hip

    @contextlib.contextmanager
    def scope():
        if precisions is not None:
            model.set_precision(precisions[0], jacobian_precision=precisions[1])
            assert model.decoder.precision == precisions[0] and model.decoder.j_precision == precisions[1]
        try:
            yield
        finally:
            if precisions is not None:
                model.set_precision(hip.DEFAULT_PRECISION)
    return scope()


def check_action_mode_gradients(s, margins, tag="train.action[jacobian_mlp]", precisions=None):
    """The body of test_action_mode_gradients_match_oracle_autograd on a ``build_setup`` dictionary (any action dimension);
    ``precisions = (d, j)``: with the density / colour networks on ``d`` and the Jacobian head on ``j``."""
    import njf_oracle as orc
    from neural_jacobian_field_amd import training
    from neural_jacobian_field_amd.training import JACOBIAN_PARAM_ORDER
    model, case, dev = s["model"], s["case"], s["dev"]
    model.zero_grad(set_to_none=True)
    with head_precisions(model, precisions), fused_render_outputs(model) as rendered:
        out = model.forward(s["cam"], s["rin"], s["rob"])
        assert out.standard_output.optical_flow.requires_grad and not out.standard_output.rgb.requires_grad
        loss = 0.01 * torch.nn.functional.mse_loss(out.standard_output.optical_flow, s["target"].to(dev))
        loss.backward()
        # the head's activation dump is stored as the training storage setting says for the HEAD's forward precision
        # (the last one: the range check of a model's first forward pass renders with dumps of its own before it)
        dumps = [o["jac_act"] for o in rendered if "jac_act" in o]
        assert dumps and dumps[-1].dtype == training.activation_dump_dtype(model.decoder.j_precision)
        assert dumps[-1].shape == (11, case["origins"].shape[0] * case["origins"].shape[1] * s["S"], 128)
    # oracle: same weights, encoder features from the oracle's own encoder, autograd through everything
    c = case["cams"]
    key = ("action[jacobian_mlp]", case["action"].shape[-1])
    if key not in _ORACLE_RUNS:
        losses = {}

        with torch.no_grad():
            feats = orc.encoder_features({k[len("encoder."):]: v for k, v in s["full"].items() if k.startswith("encoder.")}, s["image"])

        def oracle_backward(mode):
            cv = as_dtype(mode)
            params = {k: cv(v.clone()) for k, v in s["full"].items()}
            for k in params:
                if k.startswith("decoder.jacobian_head."):
                    params[k].requires_grad_(True)
            origins, directions = moved_rays(case["origins"], case["directions"], mode)
            ref = orc.model_forward(params, features=cv(feats if feature_seed(mode) is None else noisy(feats, seed=feature_seed(mode))),
                                    ctxt_c2w=cv(c["ctxt_c2w"]), ctxt_k_norm=cv(c["ctxt_k_norm"]),
                                    trgt_c2w=cv(c["trgt_c2w"]), trgt_k_pix=cv(case["k_pix"]), origins=cv(origins),
                                    directions=cv(directions), z_near=cv(c["z_near"]), z_far=cv(c["z_far"]),
                                    action=cv(case["action"]),
                                    num_proposal_samples=[s["S"]], num_nerf_samples=s["S"], decoder_kind="jacobian_mlp")
            ref_loss = orc.flow_loss(ref.optical_flow, cv(s["target"]))
            ref_loss.backward()
            losses[mode] = ref_loss.detach().reshape(1)
            return {n: params["decoder.jacobian_head." + n].grad for n in JACOBIAN_PARAM_ORDER}

        _ORACLE_RUNS[key] = gradient_floor(oracle_backward, JACOBIAN_PARAM_ORDER) + (losses,)
    floor64, floor, g_ref, losses = _ORACLE_RUNS[key]
    margins(tag, "loss", loss.reshape(1), losses[None],
            floor=max(rel(losses[m], losses[None]) for m in FLOOR_MODES), floor_fp64=rel(losses["fp64"], losses[None]))
    head = dict(model.decoder.jacobian_head.named_parameters())
    for name in JACOBIAN_PARAM_ORDER:
        assert head[name].grad is not None and torch.isfinite(head[name].grad).all(), name
        # bound: twice the oracle's own movement under one-ulp rays (sample locations feed a 2*pi*512-gain encoding)
        margins(tag, "grad " + name, head[name].grad, g_ref[name], floor=floor[name],
                floor_fp64=floor64[name])
    # frozen parameters received no gradient
    assert all(p.grad is None for n, p in model.named_parameters() if "jacobian_head" not in n)


def test_action_mode_gradients_match_oracle_autograd(setup, margins):
    check_action_mode_gradients(setup, margins)


@pytest.mark.parametrize("precisions", HEAD_MIXES, ids="/j:".join)
def test_action_mode_gradients_with_the_head_in_the_other_split_precision(setup, margins, precisions):
    """render_kernel<1, P, 1, AF, PJ> with PJ != P: the action-mode training forward under Model.set_precision(d,
    jacobian_precision=j), same rule as above (gradient_floor); the activation dump follows the HEAD's precision."""
    check_action_mode_gradients(setup, margins, tag=f"train.action[jacobian_mlp:{'/j:'.join(precisions)}]", precisions=precisions)


def test_one_adam_step_reduces_the_flow_loss_and_repacks_weights(setup):
    s = setup
    model, dev = s["model"], s["dev"]
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        out = model.forward(s["cam"], s["rin"], s["rob"])
        loss = 0.01 * torch.nn.functional.mse_loss(out.standard_output.optical_flow, s["target"].to(dev))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses        # packed weights are refreshed after every optimiser step


def test_flow_backward_outside_action_mode_is_refused_loudly(setup):
    """With any trainable set other than the reference's action mode, optical_flow is a value only."""
    model = setup["model"]
    p = model.decoder.density_head.lin_out.weight
    p.requires_grad = True
    try:
        out = model.forward(setup["cam"], setup["rin"], setup["rob"])
        assert torch.isfinite(out.standard_output.optical_flow).all()
        with pytest.raises(NotImplementedError, match="action mode"):
            out.standard_output.optical_flow.sum().backward()
    finally:
        p.requires_grad = False
        model.zero_grad(set_to_none=True)


@pytest.mark.parametrize("precision", ["f32", "default"] + ["/j:".join(mix) for mix in HEAD_MIXES])
def test_perception_mode_gradients_match_oracle_autograd(setup, margins, precision):
    """Reference perception mode (model_wrapper.py:117-146): every parameter trains; the losses read rgb, depth and
    the per-level weights.  HIP forward with activation dumps + GEMM backward, against autograd through the CPU oracle
    (encoder included).  Deterministic (un-jittered) samples so both sides place the same points.  Run with exact fp32
    products, in the package's default precision (f16f6 final pass, f16x2 proposal pass), and with the Jacobian head in the other
    split precision than the density and colour networks ("d/j:j": render_kernel<1, P, 2, AF, PJ> with PJ != P -- the flow it
    computes is a value only here, the dumped networks are the density net and the colour head in ``d``)."""
    import njf_oracle as orc
    from neural_jacobian_field_amd import hip
    s = setup
    model, case, dev = s["model"], s["case"], s["dev"]
    if "/j:" in precision:
        model.set_precision(precision.split("/j:")[0], jacobian_precision=precision.split("/j:")[1])
        assert model.decoder.j_precision == precision.split("/j:")[1] != model.decoder.precision
    else:
        model.set_precision("f32" if precision == "f32" else hip.DEFAULT_PRECISION)
    tag = f"train.perception[{precision}]"
    req = {n: p.requires_grad for n, p in model.named_parameters()}
    for p in model.parameters():
        p.requires_grad = True
    model.zero_grad(set_to_none=True)
    model.train()
    model.encoder.eval()  # BatchNorm on running statistics, as the oracle's encoder restatement
    samplers = (model.proposal_sampler.initial_sampler, model.proposal_sampler.pdf_sampler)
    for smp in samplers:
        smp.train_stratified = False
    g2 = torch.Generator().manual_seed(21)
    B, R = case["origins"].shape[:2]
    t_rgb = torch.rand(B, R, 3, generator=g2)
    t_depth = torch.rand(B, R, 1, generator=g2) * 0.5 + 0.6
    sigma = torch.tensor([0.05])

    def loss_fn(rgb, depth, weights_list, starts_ends, to):
        loss = torch.nn.functional.mse_loss(rgb, to(t_rgb)) + 0.1 * (depth - to(t_depth)).abs().mean()
        for w, (st, en) in zip(weights_list, starts_ends):
            loss = loss + 0.08 * orc.ds_nerf_depth_loss(w, to(t_depth), (st + en) / 2, en - st, to(sigma)) / len(weights_list)
        return loss

    try:
        out = model.forward(s["cam"], s["rin"], s["rob"])
        tr = out.training_output
        assert len(tr.weights_list) == 2 and all(w.requires_grad for w in tr.weights_list)
        loss = loss_fn(out.standard_output.rgb, out.standard_output.depth, tr.weights_list,
                       [(x.starts, x.ends) for x in tr.ray_samples_list], lambda t: t.to(dev))
        loss.backward()
        # the in-kernel compositing of the inference path gives the same values, up to the noise two runs of the SAME
        # path show here: MIOpen's convolutions are not bit-reproducible, the ulps move the resampled bins by ~3e-6 and
        # the 2*pi*512-gain encoding amplifies that (measured run-to-run: 5e-5 on the final weights)
        with torch.no_grad():
            inf = model.forward(s["cam"], s["rin"], s["rob"])
        assert rel(out.standard_output.rgb, inf.standard_output.rgb) < 1e-3
        assert rel(out.standard_output.depth, inf.standard_output.depth) < 1e-3
        for w_g, w_i in zip(tr.weights_list, inf.training_output.weights_list):
            assert rel(w_g, w_i) < 2e-3

        c = case["cams"]
        losses = {}
        names = [n for n, _ in model.named_parameters()]

        def oracle_backward(mode):
            cv = as_dtype(mode)
            params = {k: cv(v.clone()) for k, v in s["full"].items()}
            for k, v in params.items():
                if v.is_floating_point() and "running_" not in k:
                    v.requires_grad_(True)
            origins, directions = moved_rays(case["origins"], case["directions"], mode)
            source = dict(input_image=cv(s["image"]))
            if feature_seed(mode) is not None:   # the encoder trains, and its OUTPUT carries the arithmetic noise of another fp32 conv
                enc = {k[len("encoder."):]: v for k, v in params.items() if k.startswith("encoder.")}
                source = dict(features=noisy(orc.encoder_features(enc, cv(s["image"])), seed=feature_seed(mode)))
            ref = orc.model_forward(params, **source, ctxt_c2w=cv(c["ctxt_c2w"]), ctxt_k_norm=cv(c["ctxt_k_norm"]),
                                    trgt_c2w=cv(c["trgt_c2w"]), trgt_k_pix=cv(case["k_pix"]), origins=cv(origins),
                                    directions=cv(directions), z_near=cv(c["z_near"]), z_far=cv(c["z_far"]),
                                    action=cv(case["action"]),
                                    num_proposal_samples=[s["S"]], num_nerf_samples=s["S"], decoder_kind="jacobian_mlp")
            ref_loss = loss_fn(ref.rgb, ref.depth, ref.weights_list, [(x.starts, x.ends) for x in ref.samples_list], cv)
            ref_loss.backward()
            losses[mode] = ref_loss.detach().reshape(1)
            return {n: params[n].grad for n in names}

        if "perception" not in _ORACLE_RUNS:   # (the oracle's runs do not depend on the precision under test)
            _ORACLE_RUNS["perception"] = (oracle_backward(None), {mode: oracle_backward(mode) for mode in FLOOR_MODES}, losses)
        base, moved, losses = _ORACLE_RUNS["perception"]
        margins(tag, "loss", loss.reshape(1), losses[None],
                floor=max(rel(losses[m], losses[None]) for m in FLOOR_MODES), floor_fp64=rel(losses["fp64"], losses[None]))
        # EVERY parameter is held to ITS OWN floors (a group's largest floor used to excuse the group's worst
        # parameter): twice the oracle's fp32-vs-fp64 difference of that gradient, and only where that fails twice its
        # largest movement under one-ulp rays / the 1e-6 image perturbation (row marked; limit capped by `margins`)
        failures = []
        for name, p in model.named_parameters():
            g_ref = base[name]
            if g_ref is None or name.startswith("decoder.jacobian_head."):
                # not on the differentiated path: the Jacobian head (optical_flow is not in a perception loss), and
                # ResNet-34's layer4 / fc, which EncoderResnet (num_layers=4) never evaluates
                assert p.grad is None and (g_ref is None or g_ref.abs().max() == 0), name
                continue
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
            f64 = rel(moved["fp64"][name], g_ref)
            f_all = max(rel(m[name], g_ref) for m in moved.values())
            try:
                # (ref64: the float64 oracle gradient -- adds the truth-referenced element-wise row of this parameter)
                margins(tag, "grad " + name, p.grad, g_ref, ref64=moved["fp64"][name],
                        floor=f_all, floor_fp64=f64)
            except AssertionError as e:
                d = e.args[0] if e.args and isinstance(e.args[0], dict) else {}
                failures.append((round(d.get("err", 0.0) / max(d.get("limit", 1.0), 1e-30), 2), name))
        assert not failures, (len(failures), sorted(failures, reverse=True)[:6])
    finally:
        for n, p in model.named_parameters():
            p.requires_grad = req[n]
        for smp in samplers:
            smp.train_stratified = True
        model.zero_grad(set_to_none=True)
        model.eval()
        model.set_precision(hip.DEFAULT_PRECISION)


def test_perception_step_trains_all_parts(setup):
    """A few Adam steps on the rgb loss with every parameter trainable lower the loss (packed weights and the hoisted
    feature map are refreshed after each optimiser step)."""
    s = setup
    model, dev = s["model"], s["dev"]
    state = {k: v.clone() for k, v in model.state_dict().items()}
    req = {n: p.requires_grad for n, p in model.named_parameters()}
    for p in model.parameters():
        p.requires_grad = True
    g2 = torch.Generator().manual_seed(22)
    target = torch.rand(s["case"]["origins"].shape[0], s["case"]["origins"].shape[1], 3, generator=g2).to(dev)
    try:
        opt = torch.optim.Adam(model.parameters(), lr=2e-4)
        losses = []
        for _ in range(5):
            opt.zero_grad()
            out = model.forward(s["cam"], s["rin"], s["rob"])
            loss = torch.nn.functional.mse_loss(out.standard_output.rgb, target)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        assert losses[-1] < losses[0], losses
    finally:
        model.load_state_dict(state)
        for n, p in model.named_parameters():
            p.requires_grad = req[n]
        model.zero_grad(set_to_none=True)


def test_wrapper_training_step_perception_and_action(setup):
    """ModelWrapper.training_step (model_wrapper.py:107-163) end to end on a dataset-schema batch: the perception loss
    reaches encoder, density/colour heads and proposal net; the action loss reaches only the Jacobian head."""
    from neural_jacobian_field_amd.geometry import get_pixel_coordinates
    from neural_jacobian_field_amd.model_wrapper import ModelWrapper
    s = setup
    model, dev, case = s["model"], s["dev"], s["case"]
    state = {k: v.clone() for k, v in model.state_dict().items()}
    req = {n: p.requires_grad for n, p in model.named_parameters()}
    B, H, W = 2, 16, 16
    c = case["cams"]
    g2 = torch.Generator().manual_seed(31)
    coords, _ = get_pixel_coordinates(H, W, dev)

    def batch():
        return {"context": {"rgb": s["image"].to(dev), "extrinsics": c["ctxt_c2w"].to(dev), "intrinsics": c["ctxt_k_norm"].to(dev),
                            "robot_action": case["action"].to(dev)},
                "target": {"rgb": torch.rand(B, 3, H, W, generator=g2).to(dev), "depth": (torch.rand(B, 1, H, W, generator=g2) + 0.5).to(dev),
                           "flow": torch.randn(B, 2, H, W, generator=g2).to(dev), "extrinsics": c["trgt_c2w"].to(dev),
                           "intrinsics": c["ctxt_k_norm"].to(dev)},
                "scene": {"near": c["z_near"].to(dev), "far": c["z_far"].to(dev), "coordinates": coords[None].expand(B, -1, -1, -1)}}

    try:
        for p in model.parameters():
            p.requires_grad = True
        wrapper = ModelWrapper("perception", 48, model).train()
        loss = wrapper.training_step(batch())
        assert torch.isfinite(loss)
        loss.backward()
        got = {n.split(".")[1] + "." + n.split(".")[2] for n, p in wrapper.named_parameters() if p.grad is not None}
        assert {"encoder.model", "decoder.density_head", "decoder.color_head", "proposal_networks.0"} <= got, got
        assert all(p.grad is None for n, p in wrapper.named_parameters() if "jacobian_head" in n)
        wrapper.zero_grad(set_to_none=True)

        wrapper = ModelWrapper("action", 48, model).train()     # freezes everything but the Jacobian head
        loss = wrapper.training_step(batch())
        loss.backward()
        assert all((p.grad is not None) == ("jacobian_head" in n) for n, p in wrapper.named_parameters())
    finally:
        model.load_state_dict(state)
        for n, p in model.named_parameters():
            p.requires_grad = req[n]
        model.zero_grad(set_to_none=True)
        model.eval()


def check_transformer_action_mode_gradients(s, margins, A=6, tag="train.action[jacobian_transformer]", precisions=None):
    """The body of test_transformer_action_mode_gradients_match_oracle_autograd for a head of ``A`` keys; ``precisions = (d, j)``:
    with the density / colour networks on ``d`` and the transformer head on ``j``."""
    import njf_oracle as orc
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import Model, RobotInput
    case, dev = s["case"], s["dev"]
    full = synthetic.seeded_state_dict(synthetic.model_shapes("jacobian_transformer", A), seed=6)
    model = Model(model_cfg_from_dict({"action_dim": A, "rendering": {"num_proposal_samples": [s["S"]], "num_nerf_samples": s["S"]},
                                       "action_decoder": {"name": "jacobian_transformer"}}))
    model.load_state_dict(full, strict=True)
    model.to(dev).eval()
    frozen = model.decoder.freeze_non_action_parameters()
    assert frozen > 0
    for n, p in model.named_parameters():
        if "decoder" not in n:
            p.requires_grad = False
    trainable = [n for n, p in model.named_parameters() if p.requires_grad]
    assert trainable and all(n.startswith("decoder.jacobian") for n in trainable)
    action = torch.randn(case["action"].shape[0], A, generator=torch.Generator().manual_seed(8)) * 0.3
    with head_precisions(model, precisions):
        out = model.forward(s["cam"], s["rin"], RobotInput(action.to(dev)))
        loss = 0.01 * torch.nn.functional.mse_loss(out.standard_output.optical_flow, s["target"].to(dev))
        loss.backward()

    c = case["cams"]
    key = ("action[jacobian_transformer]", A)
    if key not in _ORACLE_RUNS:
        losses = {}

        with torch.no_grad():
            feats = orc.encoder_features({k[len("encoder."):]: v for k, v in full.items() if k.startswith("encoder.")}, s["image"])

        def oracle_backward(mode):
            cv = as_dtype(mode)
            params = {k: cv(v.clone()) for k, v in full.items()}
            for k in trainable:
                params[k].requires_grad_(True)
            origins, directions = moved_rays(case["origins"], case["directions"], mode)
            ref = orc.model_forward(params, features=cv(feats if feature_seed(mode) is None else noisy(feats, seed=feature_seed(mode))),
                                    ctxt_c2w=cv(c["ctxt_c2w"]), ctxt_k_norm=cv(c["ctxt_k_norm"]),
                                    trgt_c2w=cv(c["trgt_c2w"]), trgt_k_pix=cv(case["k_pix"]), origins=cv(origins),
                                    directions=cv(directions), z_near=cv(c["z_near"]), z_far=cv(c["z_far"]), action=cv(action),
                                    num_proposal_samples=[s["S"]], num_nerf_samples=s["S"], decoder_kind="jacobian_transformer")
            ref_loss = orc.flow_loss(ref.optical_flow, cv(s["target"]))
            ref_loss.backward()
            losses[mode] = ref_loss.detach().reshape(1)
            return {k: params[k].grad for k in trainable}

        _ORACLE_RUNS[key] = gradient_floor(oracle_backward, trainable) + (losses,)
    floor64, floor, g_ref, losses = _ORACLE_RUNS[key]
    margins(tag, "loss", loss.reshape(1), losses[None],
            floor=max(rel(losses[m], losses[None]) for m in FLOOR_MODES), floor_fp64=rel(losses["fp64"], losses[None]))
    named = dict(model.named_parameters())
    for k in trainable:
        margins(tag, "grad " + k, named[k].grad, g_ref[k], floor=floor[k], floor_fp64=floor64[k])
    assert all(p.grad is None for n, p in named.items() if n not in trainable)


def test_transformer_action_mode_gradients_match_oracle_autograd(setup, margins):
    """jacobian_transformer (the shipped Allegro decoder, model_allegro.yaml:26) in action mode: the kernel evaluates
    the folded head, the backward pass recomputes the un-folded head on the dumped encoding + footprint; gradients of
    every "jacobian*" parameter against autograd through the CPU oracle."""
    check_transformer_action_mode_gradients(setup, margins)


@pytest.mark.parametrize("precisions", HEAD_MIXES, ids="/j:".join)
def test_transformer_action_mode_gradients_with_the_head_in_the_other_split_precision(setup, margins, precisions):
    """render_kernel<2, P, 1, AF, PJ> with PJ != P, same rule as above."""
    check_transformer_action_mode_gradients(setup, margins, tag=f"train.action[jacobian_transformer:{'/j:'.join(precisions)}]",
                                            precisions=precisions)


@pytest.mark.parametrize("rays,samples", [(37, 64), (5, 20), (9, 200), (1, 1)])
def test_composite_backward_equals_autograd(rays, samples):
    """njf_composite_backward (one launch) against autograd through the tensor-op form of RaySamples.get_weights +
    render_rgb + the un-clipped render_depth (ray_samplers.py:77-101, model.py:257-279) in float64: gradients w.r.t. the
    densities and the colours for any combination of upstream gradients (weights only = a proposal level; all three = the
    final level), several 64-sample tiles, zero-length intervals, opaque rays."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g_
    g_.build()
    from neural_jacobian_field_amd import training
    from neural_jacobian_field_amd.model import Model
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(rays * 1000 + samples)
    deltas = (torch.rand(2, rays, samples, 1, generator=g) * 0.3)
    deltas[0, 0, samples // 2:] = 0.0                                        # zero-length intervals: no density there
    sigma = torch.exp(torch.randn(2, rays, samples, 1, generator=g) * 1.5)
    sigma[1, -1] *= 50.0                                                     # an opaque ray: weights vanish behind the surface
    color = torch.rand(2, rays, samples, 3, generator=g)
    steps = torch.sort(torch.rand(2, rays, samples, 1, generator=g) * 9 + 0.5, dim=-2).values
    gw, grgb, gdep = (torch.randn(2, rays, samples, 1, generator=g), torch.randn(2, rays, 3, generator=g), torch.randn(2, rays, 1, generator=g))

    def reference(use):
        s64, c64 = sigma.double().requires_grad_(True), color.double().requires_grad_(True)
        w = Model._weights_from_density(deltas.double(), s64)
        loss = (w * gw.double()).sum() if use[0] else 0.0
        if use[1]:
            loss = loss + ((w * c64).sum(-2) * grgb.double()).sum()
        if use[2]:
            loss = loss + (((w * steps.double()).sum(-2) / (w.sum(-2) + 1e-10)) * gdep.double()).sum()
        loss.backward()
        return s64.grad, c64.grad, w.detach()

    to = lambda t: t.to(dev).contiguous()
    for use in ((True, False, False), (True, True, True), (False, True, False), (False, False, True)):
        if samples == 1 and use == (False, False, True):
            continue   # the depth of a one-sample ray is its t: the gradient (-1e-10 t / w^2-sized) is below fp32 resolution
        ref_s, ref_c, w64 = reference(use)
        sg, cl = to(sigma).requires_grad_(True), to(color).requires_grad_(True)
        values = {"weights": to(w64.float()[..., 0]), "rgb": to((w64 * color.double()).sum(-2).float()),
                  "depth": to(((w64 * steps.double()).sum(-2) / (w64.sum(-2) + 1e-10)).float())}
        if use == (True, False, False):                                      # the proposal-level form: weights only
            w = training.CompositeFunction.apply(to(deltas), None, sg, None, values)
            (w * to(gw)).sum().backward()
        else:
            w, rgb, dep = training.CompositeFunction.apply(to(deltas), to(steps), sg, cl, values)
            loss = (w * to(gw)).sum() * float(use[0]) + (rgb * to(grgb)).sum() * float(use[1]) + (dep * to(gdep)).sum() * float(use[2])
            loss.backward()
        assert rel(sg.grad, ref_s) < 2e-5, (use, rel(sg.grad, ref_s))
        if use[1]:
            assert rel(cl.grad, ref_c) < 2e-6, (use, rel(cl.grad, ref_c))
        assert (sg.grad[0, 0, samples // 2:] == 0).all()                     # no gradient through zero-length intervals


def test_fused_backward_chain_equals_the_gemm_chain(setup):
    """njf_resnetfc_backward (one launch: 11 transposed-weight MFMA products, ReLU masks, residual adds, gradient resident
    in registers) against the layer-by-layer form -- library GEMMs + njf_relu_backward -- on random activations with
    ragged point counts and every d_out the model uses; and the parameter gradients built from it against autograd."""
    from neural_jacobian_field_amd import synthetic, training
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(5)
    for points, d_out in ((1, 1), (37, 16), (4096 + 13, 24), (300, 3)):
        shapes = synthetic.resnet_fc_shapes("", 63, 512, d_out)
        p = {k: v.to(dev) for k, v in synthetic.seeded_state_dict(shapes, seed=2).items()}
        act = torch.randn(11, points, 128, generator=gen).clamp_min(0).to(dev)       # ReLU'd layer inputs: ~half zeros
        g = torch.randn(points, d_out, generator=gen).to(dev) * 1e-3
        got = training.resnetfc_backward_chain(p, g, act)
        ref = training.resnetfc_backward_reference_chain(p, g, act)
        assert got.shape == ref.shape == (11, points, 128)
        for l in range(11):
            scale = ref[l].abs().max().item() + 1e-30
            assert ((got[l] - ref[l]).abs().max().item() / scale) < 2e-6, (points, d_out, l)
        again, sums = training.resnetfc_backward_chain(p, g, act, want_colsum=True)
        assert torch.equal(got, again)                                            # bit-reproducible
        ref_sums = got.double().sum(1)                                            # the in-kernel per-tile column sums
        assert sums.shape == (11, 128)
        assert ((sums.double() - ref_sums).abs().max() / (ref_sums.abs().max() + 1e-30)).item() < 2e-6, (points, d_out)
    # parameter gradients of a whole ResnetFC against autograd of the same net in torch (fp64)
    points, d_out = 257, 16
    shapes = synthetic.resnet_fc_shapes("", 63, 512, d_out)
    p = {k: v.to(dev) for k, v in synthetic.seeded_state_dict(shapes, seed=3).items()}
    pe = torch.randn(points, 64, generator=gen).to(dev)
    pe[:, 63] = 1.0                                                                # the bias slot of lin_in
    z = [torch.randn(points, 128, generator=gen).to(dev) for _ in range(3)]       # the three hoisted latents
    slot = torch.tensor(training._PE_SLOT_TO_CHANNEL, device=dev)
    leaves = {k: v.double().requires_grad_(True) for k, v in p.items() if not k.startswith("lin_z")}
    x = pe.double().new_zeros(points, 63)
    x[:, slot] = pe[:, :63].double()
    h = x @ leaves["lin_in.weight"].t() + leaves["lin_in.bias"]
    acts = []
    for blk in range(5):
        if blk < 3:
            h = h + z[blk].double()
        acts.append(torch.relu(h))
        net = acts[-1] @ leaves[f"blocks.{blk}.fc_0.weight"].t() + leaves[f"blocks.{blk}.fc_0.bias"]
        acts.append(torch.relu(net))
        h = h + acts[-1] @ leaves[f"blocks.{blk}.fc_1.weight"].t() + leaves[f"blocks.{blk}.fc_1.bias"]
    acts.append(torch.relu(h))
    out = acts[-1] @ leaves["lin_out.weight"].t() + leaves["lin_out.bias"]
    g = torch.randn(points, d_out, generator=gen).to(dev)
    ref_grads = dict(zip(leaves, torch.autograd.grad(out, list(leaves.values()), g.double())))
    act = torch.stack([a.detach().float() for a in acts])
    feats = torch.zeros(4, 512, device=dev)
    grads = training.resnetfc_backward(p, g, act, pe, torch.zeros(points, 4, dtype=torch.int32, device=dev),
                                       torch.zeros(points, 4, device=dev), feats)
    for k, r in ref_grads.items():
        err = (grads[k].double() - r).abs().max().item() / (r.abs().max().item() + 1e-30)
        assert err < 5e-6, (k, err)


def test_backward_chain_f16x2_against_exact():
    """The opt-in product form of the fused backward chain (training.set_backward_precision("f16x2"): hi*hi + hi*lo + lo*hi of fp16
    halves on gradients scaled by a power of two taken from max|d_out|) against the exact-fp32 chain on the SAME dumped activations,
    masks and upstream gradient, for upstream gradients of three very different magnitudes (a loss-scale independence check: the
    scaling is by powers of two and must cancel exactly).  Stated tolerance: every deltas slice and every bias column sum within
    2e-5 of the exact chain's, norm-wise -- the reference's own training arithmetic is TF32 (train.py:64-65: 2^-11 per operand)."""
    from neural_jacobian_field_amd import hip, synthetic
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    P = 4096 + 17                                        # ragged last tile
    params = synthetic.seeded_state_dict(synthetic.model_shapes("jacobian_mlp", 8, with_encoder=False), seed=0)
    net = {k[len("decoder.jacobian_head."):]: v.to(dev) for k, v in params.items() if k.startswith("decoder.jacobian_head.")}
    act = torch.relu(torch.randn(11, P, 128, generator=g)).to(dev).contiguous()
    bits = (act > 0).reshape(11, P, 2, 2, 2, 16)         # [layer, point, hh, word, m & 1, r]: feature = 64 hh + 32 word + 16 (m & 1) + r
    weights = (1 << torch.arange(32, dtype=torch.int64, device=dev)).reshape(2, 16)
    mask = (bits.to(torch.int64) * weights).sum((-1, -2))                      # [11, P, 2, 2] -> word index 2 hh + word
    mask = mask.reshape(11, P, 4)
    mask = torch.where(mask >= 2 ** 31, mask - 2 ** 32, mask).to(torch.int32).contiguous()
    w32 = torch.empty(hip.RESNET_BACKWARD_W_FLOATS, device=dev)
    w16 = torch.empty_like(w32)
    hip.pack_resnetfc_backward(net, "", w32, precision="f32")
    hip.pack_resnetfc_backward(net, "", w16, precision="f16x2")
    base = torch.randn(P, 24, generator=g).to(dev) * torch.rand(P, 1, generator=g).to(dev) ** 8     # per-point magnitudes over 8 decades
    for scale in (1.0, 3.7e-9, 5.0e6):
        d_out = (base * scale).contiguous()
        ref, ref_sums = hip.resnetfc_backward(d_out, act, w32, want_colsum=True, mask=mask, precision="f32")
        via_act, _ = hip.resnetfc_backward(d_out, act, w32, want_colsum=True, precision="f32")
        assert torch.equal(ref, via_act)                 # the mask route IS the activation route, bit for bit
        got, got_sums = hip.resnetfc_backward(d_out, act, w16, want_colsum=True, mask=mask, precision="f16x2")
        assert torch.isfinite(got).all()
        for l in range(11):
            assert rel(got[l], ref[l]) < 2e-5, (scale, l, rel(got[l], ref[l]))
            assert rel(got_sums[l], ref_sums[l]) < 2e-5, (scale, l)


@pytest.mark.parametrize("mode", ["action", "perception"])
def test_f16_training_storage_against_fp32_storage(mode):
    """The opt-in 16-bit training storage (training.set_storage_precision("f16"): fp16 activation dumps, fp16 deltas x 2^k, weight-
    gradient GEMMs with fp32 accumulation) against the default fp32 storage on the SAME batch and weights, with a 'precomputed'
    encoder and un-jittered sampling so that the two forwards are the same bits (MIOpen's convolutions are not run-to-run
    reproducible, and the flow's conditioning turns that into per-cent differences between ANY two runs).  Then

        * loss and pixels identical (the dumps' format does not enter the forward arithmetic);
        * every weight gradient contracted from 16-bit operands within  max |g16 - g32| <= 2e-3 x max |g32|  (operands rounded to
          11 significant bits; the reference's own training arithmetic, TF32, rounds to the same 11 bits: train.py:64-65);
        * what the chain itself produces in fp32 -- bias gradients (column sums of deltas), lin_z and lin_in weights -- within 1e-5."""
    from neural_jacobian_field_amd import model_wrapper as mw, synthetic, training
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import CameraInput, Model, ModelTarget, RenderingInput, RobotInput
    dev = torch.device("cuda:0")
    B, H, W, R, S, A = 2, 64, 64, 256, 64, 8
    b = synthetic.synthetic_training_batch(B, H, W, R, A, seed=5, device=dev)
    feats = synthetic.synthetic_features(B, H, W, seed=3).to(dev)
    cam = CameraInput(None, b["ctxt_c2w"], b["ctxt_k_norm"], b["trgt_c2w"], b["trgt_k_pix"])
    rin = RenderingInput(b["origins"], b["directions"], b["z_near"], b["z_far"])
    rob = RobotInput(b["action"])
    ptarget = ModelTarget(rgb=b["target_rgb"], depth=b["target_depth"], optical_flow=None, visible_mask=None)
    grads, losses, pixels = {}, {}, {}
    try:
        for storage in ("f32", "f16"):
            training.set_storage_precision(storage)
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
            out = model.forward(cam, rin, rob)
            if mode == "action":
                loss = 0.01 * torch.nn.functional.mse_loss(out.standard_output.optical_flow, b["target_flow"])
            else:
                tr = out.training_output
                loss = (mw.rgb_loss(out, ptarget) + mw.depth_loss(out, ptarget) + mw.interlevel_loss(tr.weights_list, tr.ray_samples_list)
                        + 0.01 * mw.distortion_loss(tr.weights_list, tr.ray_samples_list))
            loss.backward()
            torch.cuda.synchronize()
            losses[storage] = float(loss.detach())
            pixels[storage] = out.standard_output.optical_flow.detach().clone()
            grads[storage] = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    finally:
        training.set_storage_precision("auto")
    assert losses["f16"] == losses["f32"] and torch.equal(pixels["f16"], pixels["f32"]), losses
    assert set(grads["f16"]) == set(grads["f32"]) and len(grads["f32"]) > 0
    worst = {n: rel(grads["f16"][n], g32) for n, g32 in grads["f32"].items()}
    bad = {n: v for n, v in worst.items() if not v <= 2e-3}
    assert not bad, bad
    fp32_made = {n: v for n, v in worst.items() if ("density_head" in n or "jacobian_head" in n) and
                 (n.endswith(".bias") or ".lin_z." in n or ".lin_in." in n)}
    assert fp32_made and all(v <= 1e-5 for v in fp32_made.values()), fp32_made


@pytest.mark.parametrize("mode", ["regular", "arm"])
def test_flow_mlp_arm_head_and_action_mode_training_vs_reference_golden(golden, margins, mode):
    """``flow_mlp`` beyond inference (tests/golden/model_flow_train.npz, produced by the reference itself): the decoder built with
    ``use_arm_model`` in both modes -- decoder at the reference's sample positions and Model.forward end to end, fp64 floors from
    the reference's float64 run -- and the reference's ACTION-MODE gradient (parameters frozen like ModelWrapper.freeze_parameters,
    0.01 * mse(optical_flow, target), autograd through the whole reference model) of the ACTIVE flow head, which the HIP path
    produces with the ResnetFC backward chain + the action columns of ``lin_z`` (training.resnetfc_backward: latent_constants).
    Gradient floors per parameter: the reference's own fp32-vs-float64 distance (fixture); where twice that fails, the oracle's
    movement under one-ulp rays (the same rule as every other gradient row)."""
    import njf_oracle as orc
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.decoder import PixelEncoding
    from neural_jacobian_field_amd.model import CameraInput, Model, RenderingInput, RobotInput
    from neural_jacobian_field_amd.training import JACOBIAN_PARAM_ORDER
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    dev = torch.device("cuda:0")
    raw = golden("model_flow_train")
    g = {k[len(mode) + 1:]: v for k, v in raw.items() if k.startswith(mode + ".")}
    g.update({k: v for k, v in raw.items() if "." not in k})
    d = lambda t: t.to(dev)
    A = 5
    cfg = model_cfg_from_dict({"action_dim": A, "rendering": {"num_proposal_samples": [16], "num_nerf_samples": 12},
                               "action_decoder": {"name": "flow_mlp", "use_arm_model": True, "arm_action_dim": A}})
    model = Model(cfg)
    full = synthetic.seeded_state_dict(synthetic.model_shapes("flow_mlp", A, arm_action_dim=A), seed=0)
    model.load_state_dict(full, strict=True)
    model.to(dev).eval().requires_grad_(False)
    model.set_precision("f32")
    model.decoder.switch_mode(mode)
    features = d(g["features"])
    model._encode_for_render = lambda image: features       # the reference's encoder output: the rendering path alone
    cam = CameraInput(d(g["image"]), d(g["ctxt_c2w"]), d(g["ctxt_k_norm"]), d(g["trgt_c2w"]), d(g["trgt_k_pix"]))
    rin = RenderingInput(d(g["origins"]), d(g["directions"]), d(g["z_near"]), d(g["z_far"]))
    rob = RobotInput(d(g["action"]))
    # ---- forward: decoder at the reference's positions, Model.forward end to end ---------------------------------------------
    enc = PixelEncoding(features, cam.ctxt_extrinsics, cam.ctxt_intrinsics, rob.robot_action)
    pos = d(g["final_positions"])
    dec = model.decoder.forward(pos, rin.directions[..., None, :].expand(pos.shape).contiguous(), enc)
    c = f"model_flow_train[{mode}].decoder@ref-positions"
    margins(c, "flow", dec.flow, g["dec_flow"], g["dec_flow_f64"])
    margins(c, "density", dec.density, g["dec_density"], g["dec_density_f64"])
    margins(c, "color", dec.color, g["dec_color"], g["dec_color_f64"])
    # the flow head's 640 hidden features (ResnetFC.forward(compute_features=True)), stored by the point-query kernel (ABI v18)
    rays = g["dec_action_features"].shape[1]
    assert dec.action_features.shape == (*pos.shape[:3], 640)
    margins(c, "action_features", dec.action_features[:, :rays], g["dec_action_features"], g["dec_action_features_f64"])
    out = model.forward(cam, rin, rob, compute_vis_features=True)
    c = f"model_flow_train[{mode}].forward"
    so = out.standard_output
    # the fixture holds no self-noise figures; the oracle's movement under one-ulp rays supplies them (consulted only on failure)
    common = dict(ctxt_c2w=g["ctxt_c2w"], ctxt_k_norm=g["ctxt_k_norm"], trgt_c2w=g["trgt_c2w"], trgt_k_pix=g["trgt_k_pix"],
                  z_near=g["z_near"], z_far=g["z_far"], num_proposal_samples=[16], num_nerf_samples=12, decoder_kind="flow_mlp")

    def as_regular(params):   # the oracle evaluates flow_head.*: arm mode = the same arithmetic on flow_head_arm.*
        if mode == "regular":
            return params
        keep = {k: v for k, v in params.items() if not k.startswith("decoder.flow_head.")}
        keep.update({"decoder.flow_head." + k[len("decoder.flow_head_arm."):]: v for k, v in params.items()
                     if k.startswith("decoder.flow_head_arm.")})
        return keep

    losses = {}

    def oracle_backward(fmode):
        cv = as_dtype(fmode)
        params = as_regular({k: cv(v.clone()) for k, v in full.items()})
        for k in params:
            if k.startswith("decoder.flow_head."):
                params[k].requires_grad_(True)
        origins, directions = moved_rays(g["origins"], g["directions"], fmode)
        feats = g["features"] if feature_seed(fmode) is None else noisy(g["features"], seed=feature_seed(fmode))
        ref = orc.model_forward(params, features=cv(feats), origins=cv(origins), directions=cv(directions), action=cv(g["action"]),
                                **{k: (cv(v) if torch.is_tensor(v) else v) for k, v in common.items()})
        loss = orc.flow_loss(ref.optical_flow, cv(g["target"]))
        loss.backward()
        losses[fmode] = (loss.detach().reshape(1), ref.rgb.detach(), ref.depth.detach(), ref.optical_flow.detach(),
                         ref.action_features.detach(), ref.weights.detach(), ref.ray_positions_warped.detach())
        return {n: params["decoder.flow_head." + n].grad for n in JACOBIAN_PARAM_ORDER}

    _, floor, _ = gradient_floor(oracle_backward, JACOBIAN_PARAM_ORDER)
    ray_modes = [m for m in FLOOR_MODES if m.startswith("rays")]
    for i, (key, got) in enumerate((("rgb", so.rgb), ("depth", so.depth), ("optical_flow", so.optical_flow)), start=1):
        margins(c, key, got, g[key], g[key + "_f64"], self_noise=[rel(losses[m][i], losses[None][i]) for m in ray_modes])
    # ModelVisOutput.action_features = sum_s w_s f_s over the 640 hidden features (model.py:381-390)
    vis = out.vis_output
    assert vis.action_features.shape == (*so.rgb.shape[:2], 640)
    margins(c, "vis.action_features", vis.action_features, g["vis_action_features"], g["vis_action_features_f64"],
            self_noise=[rel(losses[m][4], losses[None][4]) for m in ray_modes])
    margins(c, "vis.weights", vis.weights, g["vis_weights"], g["vis_weights_f64"],
            self_noise=[rel(losses[m][5], losses[None][5]) for m in ray_modes])
    margins(c, "vis.ray_positions_warped", vis.ray_positions_warped, g["vis_ray_positions_warped"], g["vis_ray_positions_warped_f64"],
            self_noise=[rel(losses[m][6], losses[None][6]) for m in ray_modes])
    # ---- the action-mode step ---------------------------------------------------------------------------------------------------
    model.requires_grad_(True)
    model.decoder.freeze_non_action_parameters()           # action_decoder_flow.py:281-288
    for n, p in model.named_parameters():
        if "decoder" not in n:
            p.requires_grad = False                          # model_wrapper.py:79-82
    from neural_jacobian_field_amd import training
    assert training.is_action_mode(model) and training.action_kind(model) == "flow_mlp"
    out = model.forward(cam, rin, rob)
    assert out.standard_output.optical_flow.requires_grad and not out.standard_output.rgb.requires_grad
    loss = 0.01 * torch.nn.functional.mse_loss(out.standard_output.optical_flow, d(g["target"]))
    loss.backward()
    c = f"train.action[flow_mlp,{mode}]"
    margins(c, "loss", loss.reshape(1), g["loss"], floor=max(rel(losses[m][0], losses[None][0]) for m in FLOOR_MODES),
            floor_fp64=rel(g["loss_f64"], g["loss"]))
    active = "flow_head_arm." if mode == "arm" else "flow_head."
    idle = "flow_head." if mode == "arm" else "flow_head_arm."
    named = dict(model.decoder.named_parameters())
    for name in JACOBIAN_PARAM_ORDER:
        grad = named[active + name].grad
        assert grad is not None and torch.isfinite(grad).all() and grad.shape == named[active + name].shape, name
        margins(c, "grad " + name, grad, g["grad." + name], floor=max(floor[name], float(g["floor64." + name])),
                floor_fp64=float(g["floor64." + name]))
    assert all(named[idle + n].grad is None for n in JACOBIAN_PARAM_ORDER)              # the inactive head: no gradient
    assert all(p.grad is None for n, p in model.named_parameters() if "flow_head" not in n)
    # one optimiser step moves the loss (the hoisted map's action bias and the packed head are refreshed)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=2e-4)
    opt.step()
    with torch.no_grad():
        after = 0.01 * torch.nn.functional.mse_loss(model.forward(cam, rin, rob).standard_output.optical_flow, d(g["target"]))
    assert float(after) < float(loss.detach()), (float(after), float(loss.detach()))


def test_reference_matmul_precision_selects_the_tf32_class_backward():
    """``torch.set_float32_matmul_precision("high")`` is how the reference trains (train.py:64-65: TF32 products in every GEMM of the
    step).  With the package's "auto" settings the same switch selects the TF32-class forms of THIS backward pass -- the f16x2 chain
    and the 16-bit training storage, each with its own stated tolerance (the two tests above) -- for networks whose forward runs in
    a split precision; torch's default ("highest") and a network forced to exact fp32 products keep the exact backward."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from neural_jacobian_field_amd import synthetic, training
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import CameraInput, Model, RenderingInput, RobotInput
    dev = torch.device("cuda:0")
    B, H, W, R, S, A = 2, 64, 64, 128, 32, 8
    b = synthetic.synthetic_training_batch(B, H, W, R, A, seed=7, device=dev)
    feats = synthetic.synthetic_features(B, H, W, seed=4).to(dev)
    cam = CameraInput(None, b["ctxt_c2w"], b["ctxt_k_norm"], b["trgt_c2w"], b["trgt_k_pix"])
    rin = RenderingInput(b["origins"], b["directions"], b["z_near"], b["z_far"])
    rob = RobotInput(b["action"])
    seen = {}

    def step(forward_precision=None):
        model = Model(model_cfg_from_dict({"action_dim": A, "encoder": {"name": "precomputed"},
                                           "rendering": {"num_proposal_samples": [S], "num_nerf_samples": S},
                                           "action_decoder": {"name": "jacobian_mlp"}}))
        model.load_state_dict(synthetic.seeded_state_dict(synthetic.model_shapes("jacobian_mlp", A, with_encoder=False), seed=0))
        model.to(dev).eval()
        model.encoder.set_features(feats)
        if forward_precision is not None:
            model.set_precision(forward_precision)
        model.decoder.freeze_non_action_parameters()
        for n, p in model.named_parameters():
            if "decoder" not in n:
                p.requires_grad = False
        original = training.resnetfc_backward

        def spy(p, d_out, act, *args, **kw):
            seen["act_dtype"], seen["chain"] = act.dtype, training.backward_precision(kw.get("forward_precision"))
            return original(p, d_out, act, *args, **kw)

        training.resnetfc_backward = spy
        try:
            out = model.forward(cam, rin, rob)
            (0.01 * torch.nn.functional.mse_loss(out.standard_output.optical_flow, b["target_flow"])).backward()
        finally:
            training.resnetfc_backward = original
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

    assert torch.get_float32_matmul_precision() == "highest" and training.backward_precision("f16f6") == "f32"
    try:
        exact = step()
        assert (seen["act_dtype"], seen["chain"]) == (torch.float32, "f32")
        training.set_backward_precision("f16x2"); training.set_storage_precision("f16")
        explicit = step()
        assert (seen["act_dtype"], seen["chain"]) == (torch.float16, "f16x2")
        training.set_backward_precision("auto"); training.set_storage_precision("auto")
        torch.set_float32_matmul_precision("high")
        auto_high = step()
        assert (seen["act_dtype"], seen["chain"]) == (torch.float16, "f16x2")
        forced_exact = step("f32")          # exact fp32 forward products (by hand, or by the range guard): exact backward
        assert (seen["act_dtype"], seen["chain"]) == (torch.float32, "f32")
    finally:
        torch.set_float32_matmul_precision("highest")
        training.set_backward_precision("auto"); training.set_storage_precision("auto")
    assert set(auto_high) == set(explicit) == set(exact) and len(exact) > 0
    worst = {n: (rel(auto_high[n], explicit[n]), rel(auto_high[n], exact[n]), rel(forced_exact[n], exact[n])) for n in exact}
    print("[matmul-precision high] worst rel: vs explicit opt-ins %.2e, vs exact %.2e; forced-f32 forward vs exact %.2e"
          % tuple(max(v[i] for v in worst.values()) for i in range(3)))
    for n, (vs_explicit, vs_exact, forced) in worst.items():
        # the same forms of OUR kernels; under "high" torch's own GEMMs (lin_z / lin_in / lin_out gradients) may run reduced products
        # too -- the caller's switch -- so the comparison is held to the stated tolerance of the TF32-class forms, not to bit equality
        assert vs_explicit <= 2e-3, (n, vs_explicit)
        assert vs_exact <= 2e-3, (n, vs_exact)                     # the stated tolerance of the 16-bit storage
        # (exact HIP chain behind an exact-fp32 FORWARD: against the default-precision forward's gradient this is the 1e-3-class
        # difference of the two forward precisions -- ReLU-mask flips, sample placement -- plus torch's GEMMs as switched: sanity only)
        assert forced <= 5e-3 and torch.isfinite(forced_exact[n]).all(), (n, forced)


def test_reduced_backward_reports_an_exceeded_fp16_range():
    """The safety net of the TF32-class backward forms (training._note_reduced_results / reduced_backward_overflowed): a network whose
    transposed weights amplify the gradient beyond the scaled chain's head room (max|d_out| = 64 of fp16's 65504) yields non-finite
    gradients where the exact backward does not; every reduced call folds that into one device scalar, read (and reset) by the
    model's periodic range check.  Ordinary weights leave it clear."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import __graft_entry__ as g
    g.build()
    from neural_jacobian_field_amd import training
    from neural_jacobian_field_amd.training import JACOBIAN_PARAM_ORDER
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(3)
    P, T = 512, 64
    shapes = {"lin_in.weight": (128, 63), "lin_in.bias": (128,), "lin_out.weight": (8, 128), "lin_out.bias": (8,)}
    for b in range(5):
        for fc in ("fc_0", "fc_1"):
            shapes[f"blocks.{b}.{fc}.weight"], shapes[f"blocks.{b}.{fc}.bias"] = (128, 128), (128,)
    for i in range(3):
        shapes[f"lin_z.{i}.weight"], shapes[f"lin_z.{i}.bias"] = (128, 512), (128,)
    assert set(shapes) == set(JACOBIAN_PARAM_ORDER)
    act = torch.rand(11, P, 128, generator=gen).half().to(dev)
    mask = torch.randint(-2 ** 31, 2 ** 31 - 1, (11, P, 4), generator=gen, dtype=torch.int64).to(torch.int32).to(dev)
    pe = torch.randn(P, 64, generator=gen).to(dev)
    foot_idx = torch.randint(0, T, (P, 4), generator=gen, dtype=torch.int64).to(torch.int32).to(dev)
    foot_w = torch.rand(P, 4, generator=gen).to(dev)
    feats = torch.randn(T, 512, generator=gen).to(dev)
    d_out = torch.randn(P, 8, generator=gen).to(dev)

    def run(weight_scale):
        p = {k: (torch.randn(*v, generator=gen) * (weight_scale if k.endswith("weight") else 0.0)).to(dev) for k, v in shapes.items()}
        return training.resnetfc_backward(p, d_out, act, pe, foot_idx, foot_w, feats, mask=mask)

    training.reduced_backward_overflowed(dev)                      # (clear whatever earlier tests left)
    try:
        training.set_backward_precision("f16x2")
        grads = run(0.08)                                          # kaiming-sized weights: gain ~1 per layer
        assert all(torch.isfinite(v).all() for v in grads.values())
        assert not training.reduced_backward_overflowed(dev)
        grads = run(8.0)                                           # gain ~1e2 per layer: far beyond 2^9 over eleven layers
        assert not all(torch.isfinite(v).all() for v in grads.values())
        assert training.reduced_backward_overflowed(dev)           # reported ...
        assert not training.reduced_backward_overflowed(dev)       # ... and reset by the query
    finally:
        training.set_backward_precision("auto")


def test_transformer_backward_chain_equals_the_library_recomputation(setup):
    """The fused backward of the folded transformer head (njf_transformer_backward: one launch for the data-gradient chain of its three
    layers on the residual stream the training forward dumped, one batched GEMM for the K = points weight gradients, the fold's own
    autograd graph back to the reference's parameters) against the route it replaces -- the head recomputed in its ORIGINAL
    parameterisation (transformer.py:38-135) in library ops from the dumped encoding + footprint, differentiated by autograd
    (NJF_TRANSFORMER_BACKWARD=torch) -- on the same forward: every "jacobian*" parameter, A = 6 (two unused key slots) and A = 8.
    This is the end-to-end check: both sides differentiate a default-precision forward with its own sample placement, hence 2e-4.
    The kernel-level check of the chain -- float64 autograd on plain tensors, every tile shape, key count and storage / product
    form, at a few fp32 roundings -- is tests/test_transformer_backward_gpu.py."""
    import os
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import CameraInput, Model, RenderingInput, RobotInput
    s = setup
    case, dev = s["case"], s["dev"]
    for A in (6, 8):
        model = Model(model_cfg_from_dict({"action_dim": A, "rendering": {"num_proposal_samples": [s["S"]], "num_nerf_samples": s["S"]},
                                           "action_decoder": {"name": "jacobian_transformer"}}))
        model.load_state_dict(synthetic.seeded_state_dict(synthetic.model_shapes("jacobian_transformer", A), seed=6), strict=True)
        model.to(dev).eval()
        model.decoder.freeze_non_action_parameters()
        for n, p in model.named_parameters():
            if "decoder" not in n:
                p.requires_grad = False
        # the frozen trunk's library convolutions (MIOpen) are not bit-reproducible from one call to the next, and at A = 8 the
        # samples they place move the comparisons below by as much as their 1e-4 bound: the trunk runs ONCE and every route
        # differentiates the forward pass on those same latents
        latents = [t.detach() for t in model.encoder._latents(s["cam"].input_image)]
        model.encoder._latents = lambda rgb, kept=latents: [t.clone() for t in kept]
        action = torch.randn(case["action"].shape[0], A, generator=torch.Generator().manual_seed(8)) * 0.3
        grads = {}
        for route in ("torch", "hip"):
            os.environ["NJF_TRANSFORMER_BACKWARD"] = route
            try:
                model.zero_grad(set_to_none=True)
                out = model.forward(s["cam"], s["rin"], RobotInput(action.to(dev)))
                (0.01 * torch.nn.functional.mse_loss(out.standard_output.optical_flow, s["target"].to(dev))).backward()
            finally:
                os.environ.pop("NJF_TRANSFORMER_BACKWARD", None)
            grads[route] = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        assert set(grads["hip"]) == set(grads["torch"]) and len(grads["hip"]) >= 40
        worst = {n: rel(grads["hip"][n], g) for n, g in grads["torch"].items()}
        # both are fp32 evaluations of the same derivative on the same samples: the library route recomputes the head from the
        # encoding in exact fp32, the fused chain reads the forward's (default-precision, fp32-class) residual stream
        bad = {n: v for n, v in worst.items() if not v <= 2e-4}
        assert not bad, (A, bad)
        print(f"[transformer backward, A = {A}] worst rel vs the library recomputation: {max(worst.values()):.2e} over {len(worst)} tensors")
        # the 16-bit training storage of the (X, dY) pairs (fp16 operands, fp32 accumulation: the 11 bits per operand TF32 keeps)
        from neural_jacobian_field_amd import training
        try:
            training.set_storage_precision("f16")
            model.zero_grad(set_to_none=True)
            out = model.forward(s["cam"], s["rin"], RobotInput(action.to(dev)))
            (0.01 * torch.nn.functional.mse_loss(out.standard_output.optical_flow, s["target"].to(dev))).backward()
        finally:
            training.set_storage_precision("auto")
        half = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        worst16 = {n: rel(half[n], g) for n, g in grads["hip"].items()}
        assert max(worst16.values()) <= 2e-3 and all(torch.isfinite(v).all() for v in half.values()), worst16
        assert not training.reduced_backward_overflowed(dev)
        print(f"[transformer backward, A = {A}] 16-bit storage vs fp32 storage: {max(worst16.values()):.2e}")
        # the chain itself on split fp16 products (njf_transformer_backward with NJF_PRECISION_F16X2, ABI v19: the layer's re-evaluation
        # and the chain on d_out x 2^k; fp32-class, the TF32-class opt-in of the ResnetFC chain) against the exact chain, fp32 pairs;
        # then both opt-ins together -- what matmul precision "high" selects
        for storage, limit in (("f32", 1e-4), ("f16", 2e-3)):
            try:
                training.set_backward_precision("f16x2")
                training.set_storage_precision(storage)
                model.zero_grad(set_to_none=True)
                out = model.forward(s["cam"], s["rin"], RobotInput(action.to(dev)))
                (0.01 * torch.nn.functional.mse_loss(out.standard_output.optical_flow, s["target"].to(dev))).backward()
            finally:
                training.set_backward_precision("auto")
                training.set_storage_precision("auto")
            split = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
            worst_split = {n: rel(split[n], g) for n, g in grads["hip"].items()}
            assert max(worst_split.values()) <= limit and all(torch.isfinite(v).all() for v in split.values()), (storage, worst_split)
            assert not training.reduced_backward_overflowed(dev)
            print(f"[transformer backward, A = {A}] f16x2 chain ({storage} pairs) vs the exact chain: {max(worst_split.values()):.2e}")


def test_wrapper_action_steps_with_the_shipped_allegro_head(setup):
    """ModelWrapper("action").training_step with the decoder the reference ships for Allegro (jacobian_transformer, model_allegro.yaml:26)
    in TRAINING mode (jittered samplers, annealed proposal weights): every "jacobian*" parameter and nothing else receives a finite
    gradient through the fused chain (njf_transformer_backward), and a few Adam steps on one batch lower the flow loss -- the head is
    re-folded and re-packed after every optimiser step."""
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.geometry import get_pixel_coordinates
    from neural_jacobian_field_amd.model import Model
    from neural_jacobian_field_amd.model_wrapper import ModelWrapper
    s = setup
    dev, case, A = s["dev"], s["case"], 8
    model = Model(model_cfg_from_dict({"action_dim": A, "rendering": {"num_proposal_samples": [s["S"]], "num_nerf_samples": s["S"]},
                                       "action_decoder": {"name": "jacobian_transformer"}}))
    model.load_state_dict(synthetic.seeded_state_dict(synthetic.model_shapes("jacobian_transformer", A), seed=6), strict=True)
    model.to(dev)
    B, H, W = 2, 16, 16
    c = case["cams"]
    g2 = torch.Generator().manual_seed(33)
    coords, _ = get_pixel_coordinates(H, W, dev)
    action = (torch.randn(B, A, generator=g2) * 0.3).to(dev)
    t_rgb, t_depth = torch.rand(B, 3, H, W, generator=g2).to(dev), (torch.rand(B, 1, H, W, generator=g2) + 0.5).to(dev)
    t_flow = torch.randn(B, 2, H, W, generator=g2).to(dev)

    def batch():   # (a fresh dict per step, as a data loader hands it over: the wrapper reshapes target entries)
        return {"context": {"rgb": s["image"].to(dev), "extrinsics": c["ctxt_c2w"].to(dev), "intrinsics": c["ctxt_k_norm"].to(dev),
                            "robot_action": action},
                "target": {"rgb": t_rgb.clone(), "depth": t_depth.clone(), "flow": t_flow.clone(), "extrinsics": c["trgt_c2w"].to(dev),
                           "intrinsics": c["ctxt_k_norm"].to(dev)},
                "scene": {"near": c["z_near"].to(dev), "far": c["z_far"].to(dev), "coordinates": coords[None].expand(B, -1, -1, -1)}}

    wrapper = ModelWrapper("action", 64, model).train()
    trainable = [p for p in wrapper.parameters() if p.requires_grad]
    opt = torch.optim.Adam(trainable, lr=1e-3)
    losses = []
    for it in range(6):
        torch.manual_seed(100)                       # the same ray subset and jitter every step: the loss is comparable across steps
        opt.zero_grad(set_to_none=True)
        loss = wrapper.training_step(batch())
        loss.backward()
        if it == 0:
            for n, p in wrapper.named_parameters():
                has = p.grad is not None
                assert has == (".jacobian" in n), n
                assert not has or torch.isfinite(p.grad).all(), n
        opt.step()
        losses.append(float(loss.detach()))
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
