"""The robust inverse-dynamics objective (smooth-L1 / mse + regulariser, joint bounds, several views per command) on
the CPU: the float64 restatement of njf_solve_action_robust (tests/robust_solve_reference.py) against an independent
minimiser, its robustness to outlier tracks, the objective helper against the notebook's loss, and the API's checks."""

import pytest
import torch
import torch.nn.functional as F

import robust_solve_reference as rsr
from neural_jacobian_field_amd.inverse_dynamics import action_objective, solve_action


def _objective_and_grad(lin64, target, act, **kw):
    x = act.detach().clone().requires_grad_(True)
    val = action_objective(lin64, target, x, **kw)
    val.sum().backward()
    return val.detach(), x.grad


@pytest.mark.parametrize("views", [1, 3])
@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("reg", [0.0, 1e-2])
@pytest.mark.parametrize("loss", ["mse", "smooth_l1"])
def test_restatement_reaches_the_bounded_minimiser(loss, reg, bounded, views):
    """The restatement's command scores within 1e-9 (relative) of what L-BFGS-B reaches on the same objective (the
    product's action_objective, float64), and satisfies the box's first-order conditions to 1e-8."""
    scipy_opt = pytest.importorskip("scipy.optimize")
    import numpy as np
    gen = torch.Generator().manual_seed(7 + views + 2 * bounded)
    g, r, a = 2, 60, 5
    lin = rsr.as_float64(rsr.synthetic_linearization(gen, g * views, r, a))
    truth = torch.randn(g, a, generator=gen, dtype=torch.float64) * 0.5
    target = lin.optical_flow(truth.repeat_interleave(views, 0))
    target = target + torch.randn(target.shape, generator=gen, dtype=torch.float64) * 0.5
    target[:, ::9] += 30.0                                       # a few bad tracks: both smooth-L1 zones in use
    mask = (torch.rand(g * views, r, generator=gen) > 0.2).double()
    if bounded:   # a box that cuts through the unconstrained optimum
        lower, upper = truth - 0.1, truth + 0.05
        lower[:, 0], upper[:, 0] = truth[:, 0] + 0.2, truth[:, 0] + 0.5
        lower[:, 1], upper[:, 1] = truth[:, 1] - 0.5, truth[:, 1] - 0.2
    else:
        lower, upper = torch.full_like(truth, -10.0), torch.full_like(truth, 10.0)
    kw = dict(loss=loss, beta=1.0, reg=reg, views_per_command=views)
    init = torch.randn(g, a, generator=gen, dtype=torch.float64) * 0.1
    got = rsr.robust_solve_action(lin, target, init, iterations=200, visible_mask=mask, lower=lower, upper=upper, **kw)

    def fun(x):
        val, grad = _objective_and_grad(lin, target, torch.from_numpy(x).reshape(g, a), visible_mask=mask, **kw)
        return val.sum().item(), grad.reshape(-1).numpy()

    box = list(zip(lower.reshape(-1).tolist(), upper.reshape(-1).tolist()))
    x0 = torch.minimum(torch.maximum(init, lower), upper).reshape(-1).numpy()
    res = scipy_opt.minimize(fun, x0, jac=True, method="L-BFGS-B", bounds=box,
                             options=dict(maxiter=20000, maxfun=40000, ftol=1e-16, gtol=1e-13, maxcor=30))
    ref = torch.from_numpy(np.asarray(res.x)).reshape(g, a)
    l_got, grad = _objective_and_grad(lin, target, got, visible_mask=mask, **kw)
    l_ref, _ = _objective_and_grad(lin, target, ref, visible_mask=mask, **kw)
    assert torch.all((l_got - l_ref).abs() <= 1e-9 * l_ref.abs()), (l_got, l_ref)
    kkt = (got - torch.minimum(torch.maximum(got - grad, lower), upper)).abs().max().item()
    assert kkt <= 1e-8, kkt
    assert torch.all(got >= lower) and torch.all(got <= upper)
    if bounded:
        assert torch.any(got == lower) and torch.any(got == upper)   # the box is active on both sides


def test_smooth_l1_shrugs_off_outlier_tracks():
    """Exact target flow with 10 % of the tracks moved by 30-50 px: smooth-L1 still lands on the generating command
    (1e-3 relative), least squares is pulled at least ten times further off."""
    gen = torch.Generator().manual_seed(3)
    r, a = 400, 6
    lin = rsr.as_float64(rsr.synthetic_linearization(gen, 1, r, a))
    truth = torch.randn(1, a, generator=gen, dtype=torch.float64) * 0.5
    target = lin.optical_flow(truth)
    bad = torch.randperm(r, generator=gen)[: r // 10]
    angle = torch.rand(bad.numel(), generator=gen, dtype=torch.float64) * 2 * torch.pi
    size = 30.0 + 20.0 * torch.rand(bad.numel(), generator=gen, dtype=torch.float64)
    target[0, bad] += torch.stack([angle.cos(), angle.sin()], -1) * size[:, None]
    err = {}
    for loss in ("smooth_l1", "mse"):
        got = rsr.robust_solve_action(lin, target, iterations=100, loss=loss, beta=0.01)
        err[loss] = ((got - truth).norm() / truth.norm()).item()
    assert err["smooth_l1"] <= 1e-3, err
    assert err["mse"] >= 1e-2, err


def test_action_objective_is_the_notebooks_loss():
    """Binary mask, one view: action_objective is F.smooth_l1_loss(pred[m], target[m], beta) + reg * a.pow(2).mean()
    (and the same with mse_loss) -- the loss of notebooks/real_world/2_inverse_dynamics.ipynb."""
    gen = torch.Generator().manual_seed(5)
    lin = rsr.as_float64(rsr.synthetic_linearization(gen, 1, 50, 4))
    act = torch.randn(1, 4, generator=gen, dtype=torch.float64) * 0.3
    target = lin.optical_flow(torch.randn(1, 4, generator=gen, dtype=torch.float64) * 0.3)
    target[:, ::7] += 5.0
    m = torch.rand(1, 50, generator=gen) > 0.3
    pred = lin.optical_flow(act)
    for loss, fn in (("smooth_l1", lambda p, t: F.smooth_l1_loss(p, t, beta=0.5)), ("mse", F.mse_loss)):
        want = fn(pred[m], target[m]) + 1e-2 * act.pow(2).mean()
        got = action_objective(lin, target, act, m.double(), loss=loss, beta=0.5, reg=1e-2)
        assert torch.allclose(got, want.reshape(1), rtol=1e-12, atol=0), (loss, got, want)


def test_solve_action_rejects_bad_options():
    gen = torch.Generator().manual_seed(1)
    lin = rsr.synthetic_linearization(gen, 4, 20, 3)
    target = lin.optical_flow(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="loss"):
        solve_action(lin, target, loss="huber")
    with pytest.raises(ValueError, match="lower"):
        solve_action(lin, target, loss="smooth_l1", bounds=(torch.tensor([0.0, 1.0, 0.0]), torch.zeros(3)))
    with pytest.raises(ValueError, match="views_per_command"):
        solve_action(lin, target, views_per_command=3)
    with pytest.raises(ValueError, match="beta"):
        solve_action(lin, target, loss="smooth_l1", beta=0.0)
    with pytest.raises(ValueError, match="reg"):
        solve_action(lin, target, reg=-1.0)
    with pytest.raises(ValueError, match="GPU"):   # the solve is HIP-only: no CPU path
        solve_action(lin, target, loss="smooth_l1", reg=1e-3, bounds=(-1.0, 1.0), views_per_command=2)
