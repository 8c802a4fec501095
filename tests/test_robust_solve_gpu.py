"""njf_solve_action_robust on the device: the kernel against its float64 restatement (tests/robust_solve_reference.py),
outlier tracks, several views per command, the unchanged default route, the model end to end against the notebook's
Adam loop, and the graphed controller."""

import pytest
import torch
import torch.nn.functional as F

import robust_solve_reference as rsr
from neural_jacobian_field_amd import hip
from neural_jacobian_field_amd.inverse_dynamics import (FlowLinearization, GraphedInverseDynamics, _projection_matrix,
                                                        action_objective, linearize_flow, solve_action)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _on(lin, device):
    return FlowLinearization(*(t.to(device) for t in (lin.mean_position, lin.jacobian, lin.trgt_extrinsics,
                                                      lin.trgt_intrinsics)))


def _score(lin, target, act, mask, **kw):
    return action_objective(rsr.as_float64(lin), target.double(), act.double(),
                            None if mask is None else mask.double(), **kw)


@pytest.mark.parametrize("views", [1, 4])
@pytest.mark.parametrize("a", [1, 8, 16])
def test_robust_kernel_matches_the_restatement(a, views):
    """Rays 1 / 200 / 257 / 1000 per view, both losses, masks, reg > 0, an active box and starts outside it: the kernel's
    command scores within max(1e-7, 1e-5 L) of the restatement's optimum, matches its command where the problem is
    well conditioned, stays inside the box exactly, and two launches are bit-identical."""
    gen = torch.Generator().manual_seed(100 * a + views)
    g = 2
    for r in (1, 200, 257, 1000):
        lin_cpu = rsr.synthetic_linearization(gen, g * views, r, a)
        lin = _on(lin_cpu, DEV)
        truth = (torch.randn(g, a, generator=gen) * 0.5).to(DEV)
        target = lin.optical_flow(truth.repeat_interleave(views, 0))
        target = target + (torch.randn(target.shape, generator=gen) * 0.3).to(DEV)
        target[:, ::10] += 20.0
        mask = (torch.rand(g * views, r, generator=gen) > 0.2).float().to(DEV)
        lower, upper = truth - 0.3, truth + 0.3
        lower[:, 0] = truth[:, 0] + 0.1                  # binds: the optimum lies below the box
        if a > 1:
            upper[:, -1] = truth[:, -1] - 0.1            # binds from above
        init = (truth + torch.randn(g, a, generator=gen).to(DEV)).clamp(-3, 3)
        init[:, 0] = upper[:, 0] + 0.5                   # starts outside the box
        for loss in ("mse", "smooth_l1"):
            kw = dict(loss=loss, beta=1.0, reg=1e-3, views_per_command=views)
            got = solve_action(lin, target, init, 150, visible_mask=mask, bounds=(lower, upper), **kw)
            assert torch.equal(got, solve_action(lin, target, init, 150, visible_mask=mask, bounds=(lower, upper), **kw))
            assert got.shape == (g, a) and torch.all(got >= lower) and torch.all(got <= upper)
            ref = rsr.robust_solve_action(lin_cpu, target.cpu(), init.cpu(), 200, visible_mask=mask.cpu(),
                                          lower=lower.cpu(), upper=upper.cpu(), **kw)
            l_got = _score(lin_cpu, target.cpu(), got.cpu(), mask.cpu(), **kw)
            l_ref = _score(lin_cpu, target.cpu(), ref, mask.cpu(), **kw)
            assert torch.all(l_got - l_ref <= torch.clamp(1e-5 * l_ref, min=1e-7)), (r, loss, l_got, l_ref)
            if 2 * r * views >= 8 * a:
                diff = (got.cpu().double() - ref).abs().max()
                assert torch.allclose(got.cpu().double(), ref, atol=2e-4, rtol=1e-3), (r, loss, diff)


def _outlier_problem(seed):
    gen = torch.Generator().manual_seed(seed)
    r, a = 400, 6
    lin = rsr.synthetic_linearization(gen, 1, r, a, DEV)
    truth = (torch.randn(1, a, generator=gen) * 0.5).to(DEV)
    target = lin.optical_flow(truth)
    bad = torch.randperm(r, generator=gen)[: r // 10]
    angle = torch.rand(bad.numel(), generator=gen) * 2 * torch.pi
    size = 30.0 + 20.0 * torch.rand(bad.numel(), generator=gen)
    target[0, bad.to(DEV)] += (torch.stack([angle.cos(), angle.sin()], -1) * size[:, None]).to(DEV)
    return lin, target, truth


def test_robust_kernel_shrugs_off_outlier_tracks():
    lin, target, truth = _outlier_problem(3)
    err = {}
    for loss in ("smooth_l1", "mse"):
        got = solve_action(lin, target, iterations=40, loss=loss, beta=0.01, reg=0.0, bounds=(-10.0, 10.0))
        err[loss] = ((got - truth).norm() / truth.norm()).item()
    assert err["smooth_l1"] <= 1e-3, err
    assert err["mse"] >= 1e-2, err


def test_two_views_observe_what_one_cannot():
    """Joint 2 moves nothing in view 0 (its Jacobian column is zero there) but is seen by view 1: view 0 alone leaves
    it at its start, the two views together recover the command, and V = 1 groups equal separate solves."""
    gen = torch.Generator().manual_seed(21)
    r, a = 150, 5
    lin = rsr.synthetic_linearization(gen, 2, r, a, DEV)
    lin.jacobian[0, :, :, 2] = 0.0
    truth = (torch.randn(1, a, generator=gen) * 0.5).to(DEV)
    target = lin.optical_flow(truth.repeat(2, 1))
    init = torch.full((1, a), 0.3, device=DEV)
    one = FlowLinearization(*(t[:1] for t in (lin.mean_position, lin.jacobian, lin.trgt_extrinsics, lin.trgt_intrinsics)))
    single = solve_action(one, target[:1], init, 20, loss="smooth_l1", beta=0.1)
    assert single[0, 2] == init[0, 2] and (single[0, 2] - truth[0, 2]).abs() > 0.01
    joint = solve_action(lin, target, init, 20, loss="smooth_l1", beta=0.1, views_per_command=2)
    assert torch.allclose(joint, truth, atol=1e-4, rtol=1e-4), (joint - truth).abs().max()
    both = solve_action(lin, target, init.repeat(2, 1), 20, loss="smooth_l1", beta=0.1)
    other = FlowLinearization(*(t[1:] for t in (lin.mean_position, lin.jacobian, lin.trgt_extrinsics, lin.trgt_intrinsics)))
    assert torch.equal(both[:1], single)
    assert torch.equal(both[1:], solve_action(other, target[1:], init, 20, loss="smooth_l1", beta=0.1))


def test_defaults_keep_the_least_squares_solve_and_mse_agrees_with_it():
    gen = torch.Generator().manual_seed(8)
    for b, r, a in ((2, 40, 6), (1, 700, 8), (3, 256, 16)):
        lin = rsr.synthetic_linearization(gen, b, r, a, DEV)
        target = lin.optical_flow((torch.randn(b, a, generator=gen) * 0.5).to(DEV))
        target = target + (torch.randn(target.shape, generator=gen) * 0.2).to(DEV)
        mask = (torch.rand(b, r, generator=gen) > 0.2).float().to(DEV)
        args = [lin.mean_position, lin.jacobian, _projection_matrix(lin).contiguous(), target, mask, None]
        plain = torch.empty(b, a, device=DEV)
        hip.solve_action(*args, 20, 1e-3, plain)
        assert torch.equal(solve_action(lin, target, iterations=20, visible_mask=mask), plain)
        robust = torch.empty(b, a, device=DEV)
        hip.solve_action_robust(*args, None, None, 1, "mse", 1.0, 0.0, 20, 1e-3, robust)
        assert torch.allclose(robust, plain, atol=2e-4, rtol=1e-3), (robust - plain).abs().max()


def _control_model(h=64, w=64, r=128, a=8, s=32):
    """The control-loop setup of tools/bench_control.py at a smaller image."""
    from neural_jacobian_field_amd import synthetic
    from neural_jacobian_field_amd.config import model_cfg_from_dict
    from neural_jacobian_field_amd.model import CameraInput, Model, RenderingInput
    torch.manual_seed(0)
    case = synthetic.synthetic_case(1, h, w, r, a, seed=0, device=DEV)
    model = Model(model_cfg_from_dict({"action_dim": a, "rendering": {"num_proposal_samples": [s], "num_nerf_samples": s},
                                       "action_decoder": {"name": "jacobian_mlp"}}))
    sd = synthetic.seeded_state_dict(synthetic.model_shapes("jacobian_mlp", a), seed=0)
    for k in sd:
        if k.startswith("decoder.jacobian_head.lin_out"):
            sd[k] = sd[k] * 0.01
    model.load_state_dict(sd)
    model.to(DEV).eval().requires_grad_(False)
    c = case["cams"]
    d = lambda t: t.to(DEV)
    cam = CameraInput(d(torch.rand(1, 3, h, w)), d(c["ctxt_c2w"]), d(c["ctxt_k_norm"]), d(c["trgt_c2w"]),
                      d(case["k_pix"]))
    rin = RenderingInput(d(case["origins"]), d(case["directions"]), d(c["z_near"]), d(c["z_far"]))
    return model, cam, rin


def test_solve_reaches_the_notebooks_adam_loss_end_to_end():
    """linearize_flow + solve_action(loss="smooth_l1", reg=1e-4), scored through Model.infer_optical_flow with torch's
    smooth_l1_loss + reg, is no worse than the notebook's route: encode_image, then 100 Adam steps at lr 0.1."""
    from neural_jacobian_field_amd.model import RobotInput
    model, cam, rin = _control_model()
    a, reg = 8, 1e-4
    lin = linearize_flow(model, cam, rin)
    gen = torch.Generator().manual_seed(2)
    target = lin.optical_flow((torch.randn(1, a, generator=gen) * 0.1).to(DEV))
    target[:, ::10] += 5.0
    enc = model.encode_image(cam, rin, RobotInput(torch.zeros(1, a, device=DEV)))

    def loss_of(act):
        return F.smooth_l1_loss(model.infer_optical_flow(enc, cam, RobotInput(act)), target) + reg * act.pow(2).mean()

    act = torch.zeros(1, a, device=DEV, requires_grad=True)
    opt = torch.optim.Adam([act], lr=0.1)
    for _ in range(100):
        opt.zero_grad()
        loss_of(act).backward()
        opt.step()
    with torch.no_grad():
        adam = loss_of(act).item()
        got = solve_action(lin, target, iterations=20, loss="smooth_l1", reg=reg)
        ours = loss_of(got).item()
    assert ours <= adam * (1 + 1e-4) + 1e-6, (ours, adam)


def test_graphed_robust_controller_replays_the_eager_solve():
    """GraphedInverseDynamics with smooth-L1, a box and two views per command: each replay equals, bit for bit, the eager
    solve on the graph's own linearisation, and tracks an eager linearize_flow + solve_action (two encoder runs: MIOpen
    ulps), across two changes of image and target."""
    from neural_jacobian_field_amd.model import CameraInput, RenderingInput
    model, cam1, rin1 = _control_model()
    two = lambda t: torch.cat([t, t], 0)
    cam = CameraInput(two(cam1.input_image), two(cam1.ctxt_extrinsics), two(cam1.ctxt_intrinsics),
                      two(cam1.trgt_extrinsics), two(cam1.trgt_intrinsics))
    rin = RenderingInput(two(rin1.origins), two(rin1.directions), two(rin1.z_near), two(rin1.z_far))
    a = 8
    opts = dict(loss="smooth_l1", beta=0.5, reg=1e-4, bounds=(-0.15, torch.full((a,), 0.15)), views_per_command=2)
    ctrl = GraphedInverseDynamics(model, cam, rin, iterations=6, **opts)
    gen = torch.Generator().manual_seed(4)
    for _ in range(2):
        image = torch.rand(cam.input_image.shape, generator=gen).to(DEV)
        cam_t = CameraInput(image, cam.ctxt_extrinsics, cam.ctxt_intrinsics, cam.trgt_extrinsics, cam.trgt_intrinsics)
        lin = linearize_flow(model, cam_t, rin)
        target = lin.optical_flow((torch.randn(1, a, generator=gen) * 0.1).to(DEV).repeat(2, 1))
        got = ctrl(image, target).clone()
        assert got.shape == (1, a) and torch.all(got.abs() <= 0.15)
        assert torch.equal(got, solve_action(ctrl.linearization, target, None, 6, **opts))
        eager = solve_action(lin, target, None, 6, **opts)
        flow = lambda act: lin.optical_flow(act.repeat(2, 1))
        assert ((flow(got) - flow(eager)).abs().max() / flow(eager).abs().max()).item() < 1e-2
