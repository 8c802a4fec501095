"""Float64 tensor restatement of the robust inverse-dynamics solve (njf_solve_action_robust) -- TEST INFRASTRUCTURE:
only tests import it.  Same algorithm as the kernel (projected IRLS Levenberg-Marquardt on the notebook's objective,
several views per command, a box on the command), in batched float64 torch ops on any device, with a dense solve of
the damped system; a step is kept where the objective drops, judged from the per-residual differences (see
``decrease``) so that the float64 iteration reaches the first-order conditions.  Also builds the synthetic
linearisations the robust-solve tests share."""

from typing import Optional

import torch

from neural_jacobian_field_amd.inverse_dynamics import FlowLinearization


def synthetic_linearization(gen: torch.Generator, b: int, r: int, a: int, device="cpu") -> FlowLinearization:
    """Rays 1.5-2 units in front of b cameras that differ by small translations, composited Jacobians of ~7 px per unit
    command (the layout of tests/test_model_api_gpu.py::test_solve_action_kernel_matches_the_tensor_restatement)."""
    pos = torch.rand(b, r, 3, generator=gen) * torch.tensor([1.0, 1.0, 0.5]) + torch.tensor([-0.5, -0.5, 1.5])
    jac = torch.randn(b, r, 3, a, generator=gen) * 0.05
    ext = torch.eye(4).repeat(b, 1, 1)
    ext[:, :3, 3] = torch.randn(b, 3, generator=gen) * 0.05
    k = torch.tensor([[200.0, 0, 128], [0, 210.0, 120], [0, 0, 1]]).repeat(b, 1, 1)
    return FlowLinearization(pos.to(device), jac.to(device), ext.to(device), k.to(device))


def as_float64(lin: FlowLinearization) -> FlowLinearization:
    return FlowLinearization(*(t.double() for t in (lin.mean_position, lin.jacobian, lin.trgt_extrinsics,
                                                   lin.trgt_intrinsics)))


def _rho(e: torch.Tensor, loss: str, beta: float):
    """Loss of each residual component and its IRLS weight omega (rho'(e) = omega * e)."""
    if loss == "mse":
        return e.square(), torch.full_like(e, 2.0)
    small = e.abs() < beta
    return (torch.where(small, 0.5 * e.square() / beta, e.abs() - 0.5 * beta),
            torch.where(small, torch.full_like(e, 1.0 / beta), 1.0 / e.abs()))


@torch.no_grad()
def robust_solve_action(lin, target_flow: torch.Tensor, init_action: Optional[torch.Tensor] = None,
                        iterations: int = 100, damping: float = 1e-3, visible_mask: Optional[torch.Tensor] = None, *,
                        loss: str = "mse", beta: float = 1.0, reg: float = 0.0, lower: Optional[torch.Tensor] = None,
                        upper: Optional[torch.Tensor] = None, views_per_command: int = 1) -> torch.Tensor:
    """Minimise (1/N) sum_i m_i rho(r_i(a)) + (reg/A) |a|^2 per command over lower <= a <= upper ([G,A] or None).
    Returns the float64 command [G,A]."""
    f64 = torch.float64
    b, r = target_flow.shape[:2]
    a_dim = lin.jacobian.shape[-1]
    v = views_per_command
    g = b // v
    dev = target_flow.device
    pos, jac, tgt = lin.mean_position.to(f64), lin.jacobian.to(f64), target_flow.to(f64)
    m = torch.ones(b, r, dtype=f64, device=dev) if visible_mask is None else visible_mask.to(f64)
    lo = torch.full((g, a_dim), -torch.inf, dtype=f64, device=dev) if lower is None else lower.to(f64)
    hi = torch.full((g, a_dim), torch.inf, dtype=f64, device=dev) if upper is None else upper.to(f64)
    act = torch.zeros(g, a_dim, dtype=f64, device=dev) if init_action is None else init_action.to(f64)
    act = torch.minimum(torch.maximum(act, lo), hi)
    proj = lin.trgt_intrinsics.to(f64) @ torch.linalg.inv(lin.trgt_extrinsics.to(f64))[:, :3, :]   # [B,3,4]
    n = 2 * m.reshape(g, -1).sum(1)                                                                  # [G]
    observed = n > 0
    n_b = n.clamp_min(1e-300).repeat_interleave(v)[:, None, None]                                    # [B,1,1]
    seen = (m != 0)[..., None]                                                                       # [B,R,1]
    eye = torch.eye(a_dim, dtype=f64, device=dev)

    def project(x):
        xyw = torch.einsum("bij,brj->bri", proj[..., :3], x) + proj[:, None, :, 3]
        d = xyw[..., 2:] + 1e-9
        return xyw[..., :2] / d, d

    uv0, _ = project(pos)

    def evaluate(cmd):
        x = pos + torch.einsum("brca,ba->brc", jac, cmd.repeat_interleave(v, dim=0))
        uv, d = project(x)
        e = (uv - uv0) - tgt
        rho, omega = _rho(e, loss, beta)
        data = torch.where(seen, m[..., None] * rho, torch.zeros_like(rho)).reshape(g, -1).sum(1) / n.clamp_min(1e-300)
        return torch.where(observed, data, torch.zeros_like(data)) + reg / a_dim * cmd.square().sum(1), uv, d, e, omega

    def decrease(cmd_c, cmd, e, uv, d):
        """L(cmd_c) - L(cmd) from the change of every residual, de = (dh - uv dd) / (d + dd) with (dh, dd) the change of
        the homogeneous pixel: unlike the difference of two sums it stays accurate to a few ulps of itself near the
        minimum, so the float64 iteration is not stopped short of the first-order conditions by rounding of L."""
        dxyw = torch.einsum("bij,brj->bri", proj[..., :3],
                            torch.einsum("brca,ba->brc", jac, (cmd_c - cmd).repeat_interleave(v, dim=0)))
        de = (dxyw[..., :2] - uv * dxyw[..., 2:]) / (d + dxyw[..., 2:])
        e_c = e + de
        if loss == "mse":
            diff = de * (2 * e + de)
        else:
            small_c, small = e_c.abs() < beta, e.abs() < beta
            diff = torch.where(small_c & small, 0.5 * de * (2 * e + de) / beta,
                               torch.where(~small_c & ~small & (e_c.sign() == e.sign()), de * e.sign(),
                                           _rho(e_c, loss, beta)[0] - _rho(e, loss, beta)[0]))
        data = torch.where(seen, m[..., None] * diff, torch.zeros_like(diff)).reshape(g, -1).sum(1) / n.clamp_min(1e-300)
        return data + reg / a_dim * ((cmd_c - cmd) * (cmd_c + cmd)).sum(1)

    lam = torch.full((g, 1), damping, dtype=f64, device=dev)
    for _ in range(iterations):
        _, uv, d, e, omega = evaluate(act)
        duv_dx = (proj[:, None, :2, :3] - uv[..., None] * proj[:, None, 2:3, :3]) / d[..., None]   # [B,R,2,3]
        j = torch.where(seen[..., None], duv_dx @ jac, torch.zeros(1, dtype=f64, device=dev))        # [B,R,2,A]
        w = torch.where(seen, m[..., None] * omega / n_b, torch.zeros_like(omega))                   # [B,R,2]
        h = torch.einsum("brca,brc,brcd->bad", j, w, j).reshape(g, v, a_dim, a_dim).sum(1) + 2 * reg / a_dim * eye
        we = torch.where(seen, w * e, torch.zeros_like(e))
        grad = torch.einsum("brca,brc->ba", j, we).reshape(g, v, a_dim).sum(1) + 2 * reg / a_dim * act
        active = ((act <= lo) & (grad > 0)) | ((act >= hi) & (grad < 0))
        free = (~active).to(f64)
        h = h * free[:, :, None] * free[:, None, :] + torch.diag_embed(active.to(f64))
        grad = grad * free
        h = h + lam[..., None] * torch.diag_embed(torch.diagonal(h, dim1=1, dim2=2).clamp_min(1e-12))
        step = torch.linalg.solve(h, grad)
        cand = torch.minimum(torch.maximum(act - step, lo), hi)
        better = (decrease(cand, act, e, uv, d) < 0) & observed   # NaN (behind the camera): rejected
        act = torch.where(better[:, None], cand, act)
        lam = torch.where(better[:, None], lam / 3.0, lam * 4.0).clamp(1e-9, 1e9)
    return act
