"""Inverse dynamics on a rendered Jacobian field: find the robot command that produces a desired optical flow.

Reference: notebooks/real_world/2_inverse_dynamics.ipynb (cells 26-29) encodes the image once
(``Model.encode_image``) and then runs 100 Adam steps through ``Model.infer_optical_flow``; the authors note the
loop becomes real-time "if a least square solver is used" (1_visualize_jacobian_fields.ipynb:448).  Because the scene
flow is linear in the command (``flow_s = J_s a``), the composited warped point is ``x_bar + M a`` with
``M = sum_s w_s J_s`` -- exactly the ``action_features`` the fused render kernel already composites -- so one fused
render of the tracked rays yields everything a Gauss-Newton / least-squares solve needs; the per-iteration work is a
[2R x A] least-squares problem.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from .model import CameraInput, Model, RenderingInput, RobotInput


@dataclass
class FlowLinearization:
    """Per-ray composited quantities of one fused render: optical_flow(a) = proj(x_bar + M a) - proj(x_bar)."""
    mean_position: torch.Tensor  # [B,R,3]  sum_s w_s x_s
    jacobian: torch.Tensor       # [B,R,3,A] sum_s w_s J_s, spatial-major (J viewed (action, spatial) in the reference)
    trgt_extrinsics: torch.Tensor
    trgt_intrinsics: torch.Tensor

    def optical_flow(self, action: torch.Tensor) -> torch.Tensor:
        warped = self.mean_position + torch.einsum("brca,ba->brc", self.jacobian, action)
        return (Model._project(warped, self.trgt_extrinsics, self.trgt_intrinsics)
                - Model._project(self.mean_position, self.trgt_extrinsics, self.trgt_intrinsics))


@torch.no_grad()
def linearize_flow(model: Model, camera_input: CameraInput, rendering_input: RenderingInput,
                   action_dim: Optional[int] = None) -> FlowLinearization:
    """One fused render (any command: the composited Jacobian does not depend on it)."""
    a = action_dim or model.cfg.action_dim
    b = rendering_input.origins.shape[0]
    zero = torch.zeros(b, a, dtype=torch.float32, device=rendering_input.origins.device)
    was_training = model.training
    model.eval()
    try:
        out = model._forward_inference(camera_input, rendering_input, RobotInput(zero), compute_vis_features=True)
    finally:
        model.train(was_training)
    feat = out.vis_output.action_features  # [B,R,3A], (action, spatial) order
    jac = feat.reshape(*feat.shape[:2], a, 3).transpose(-1, -2).contiguous()
    return FlowLinearization(out.vis_output.ray_positions, jac, camera_input.trgt_extrinsics, camera_input.trgt_intrinsics)


def _projection_matrix(lin: FlowLinearization) -> torch.Tensor:
    """[B,3,4] world -> homogeneous pixel matrix K . inv(E)[:3]."""
    from . import hip
    return lin.trgt_intrinsics @ hip.inverse(lin.trgt_extrinsics)[:, :3, :]


LOSSES = ("mse", "smooth_l1")


def _check_options(loss: str, beta: float, reg: float, views_per_command: int, batch: int) -> None:
    if loss not in LOSSES:
        raise ValueError(f"solve_action: unknown loss {loss!r}; choose from {LOSSES}")
    if not beta > 0:
        raise ValueError(f"solve_action: beta must be > 0 (got {beta})")
    if not reg >= 0:
        raise ValueError(f"solve_action: reg must be >= 0 (got {reg})")
    if views_per_command < 1 or batch % views_per_command:
        raise ValueError(f"solve_action: views_per_command={views_per_command} must be >= 1 and divide the batch of "
                         f"{batch} linearisations")


def _box(bounds, groups: int, action_dim: int, device) -> tuple:
    """(lower, upper), each None, a number, [A] or [G,A] -> contiguous fp32 [G,A] tensors (or None) on `device`."""
    if bounds is None:
        return None, None
    if len(bounds) != 2:
        raise ValueError("solve_action: bounds must be a pair (lower, upper)")
    out = []
    for name, b in zip(("lower", "upper"), bounds):
        if b is None:
            out.append(None)
            continue
        t = torch.as_tensor(b, dtype=torch.float32, device=device)
        if t.dim() > 2 or (t.dim() == 2 and t.shape[0] not in (1, groups)) or (t.dim() >= 1 and t.shape[-1] not in (1, action_dim)):
            raise ValueError(f"solve_action: {name} bound must be [A] or [G,A] = [{groups},{action_dim}] (got {list(t.shape)})")
        out.append(t.expand(groups, action_dim).contiguous())
    lo, hi = out
    # lower <= upper lives on the device: checked here, in eager calls (a capture cannot synchronise; the graphed
    # controller runs this check in its eager warm-up)
    if lo is not None and hi is not None and not (lo.is_cuda and torch.cuda.is_current_stream_capturing()):
        if bool((lo > hi).any()):
            raise ValueError("solve_action: lower bound exceeds upper bound")
    return lo, hi


@torch.no_grad()
def solve_action(lin: FlowLinearization, target_flow: torch.Tensor, init_action: Optional[torch.Tensor] = None,
                 iterations: int = 20, damping: float = 1e-3, visible_mask: Optional[torch.Tensor] = None, *,
                 loss: str = "mse", beta: float = 1.0, reg: float = 0.0, bounds=None,
                 views_per_command: int = 1) -> torch.Tensor:
    """Levenberg-Marquardt on ``|| optical_flow(a) - target_flow ||^2`` (pixels): all iterations in ONE HIP launch
    (``njf_solve_action``: one workgroup per batch element, deterministic reductions, no host synchronisation).

    target_flow [B,R,2], visible_mask [B,R] (the notebook masks the loss with the tracker's visibility) -> [B,A].
    The only non-linearity is the perspective divide, so for the few-pixel flows of a control step a handful of
    iterations reach the minimum; a step is kept only where it lowers the cost, which keeps large-flow problems
    stable.  GPU tensors only (no CPU path); the tensor-op restatement used by the tests lives in oracle/.

    The keyword options select the notebook's own objective (``njf_solve_action_robust``, see ``action_objective``):
    ``loss`` "mse" | "smooth_l1" (torch's, with ``beta``) on the masked mean of the flow residuals, plus
    ``reg * a.pow(2).mean()``; ``bounds = (lower, upper)``, each a number, [A] or [G,A] (either may be None), a box on
    the command; ``views_per_command = V``: each run of V consecutive linearisations (cameras) constrains one command,
    so init_action is [G,A] and the result [G,A] with G = B / V.  With every option at its default the call is the
    plain least-squares solve above, unchanged."""
    from . import hip
    b = target_flow.shape[0]
    a = lin.jacobian.shape[-1]
    _check_options(loss, beta, reg, views_per_command, b)
    f = lambda t: None if t is None else t.float().contiguous()
    if loss == "mse" and reg == 0 and bounds is None and views_per_command == 1:
        out = torch.empty(b, a, dtype=torch.float32, device=target_flow.device)
        hip.solve_action(f(lin.mean_position), f(lin.jacobian), f(_projection_matrix(lin)), f(target_flow),
                         f(visible_mask), f(init_action), iterations, damping, out)
        return out
    g = b // views_per_command
    lower, upper = _box(bounds, g, a, target_flow.device)
    out = torch.empty(g, a, dtype=torch.float32, device=target_flow.device)
    hip.solve_action_robust(f(lin.mean_position), f(lin.jacobian), f(_projection_matrix(lin)), f(target_flow),
                            f(visible_mask), f(init_action), lower, upper, views_per_command, loss, beta, reg,
                            iterations, damping, out)
    return out


def action_objective(lin: FlowLinearization, target_flow: torch.Tensor, action: torch.Tensor,
                     visible_mask: Optional[torch.Tensor] = None, *, loss: str = "mse", beta: float = 1.0,
                     reg: float = 0.0, views_per_command: int = 1) -> torch.Tensor:
    """The objective ``solve_action``'s options select, per command, in torch ops (any device, differentiable):
    ``L(a) = (1/N) sum_i m_i rho(r_i(a)) + (reg/A) |a|^2`` over the two flow components r_i of every ray of the
    command's views, N = 2 sum_r m_r, rho = r^2 ("mse") or torch's smooth-L1 with ``beta``.  With a binary mask and
    one view this is the notebook's ``F.smooth_l1_loss(pred[m], target[m], beta=beta) + reg * a.pow(2).mean()`` (or
    ``mse_loss``).  action [G,A] -> [G]; a command without observed rays scores its regulariser alone."""
    _check_options(loss, beta, reg, views_per_command, target_flow.shape[0])
    g = action.shape[0]
    res = lin.optical_flow(action.repeat_interleave(views_per_command, dim=0)) - target_flow
    if loss == "mse":
        rho = res.square()
    else:
        rho = torch.where(res.abs() < beta, 0.5 * res.square() / beta, res.abs() - 0.5 * beta)
    m = torch.ones_like(res[..., 0]) if visible_mask is None else visible_mask.to(res.dtype)
    rho = torch.where(m[..., None] != 0, rho * m[..., None], torch.zeros_like(rho))   # unobserved rays: no term at all
    n = 2 * m.reshape(g, -1).sum(1)
    data = torch.where(n > 0, rho.reshape(g, -1).sum(1) / n.clamp_min(1e-30), torch.zeros_like(n))
    return data + reg * action.square().mean(-1)


class GraphedLinearizer:
    """``linearize_flow`` for a fixed camera rig and ray set, captured once into a HIP graph and replayed per frame:
    at control-loop sizes (a few hundred tracked rays) the fused render is launch-bound, so replaying one graph
    (encoder + lin_z hoist + proposal pass + final pass) removes the per-launch host cost.  ``__call__(image)`` copies
    the new context image into the captured input buffer and replays; the returned tensors are the graph's static
    outputs (overwritten by the next call)."""

    def __init__(self, model: Model, camera_input: CameraInput, rendering_input: RenderingInput,
                 action_dim: Optional[int] = None, warmup: int = 2):
        self._image = camera_input.input_image.clone()
        cam = CameraInput(self._image, camera_input.ctxt_extrinsics, camera_input.ctxt_intrinsics,
                          camera_input.trgt_extrinsics, camera_input.trgt_intrinsics)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):      # warm-up off the default stream: packs weights, loads MIOpen kernels
            for _ in range(warmup):
                linearize_flow(model, cam, rendering_input, action_dim)
        torch.cuda.current_stream().wait_stream(side)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self._out = linearize_flow(model, cam, rendering_input, action_dim)

    def __call__(self, image: torch.Tensor) -> FlowLinearization:
        self._image.copy_(image)
        self._graph.replay()
        return self._out


class GraphedInverseDynamics:
    """The whole control step -- encoder, lin_z hoist, proposal pass, final pass, ``iterations`` Levenberg-Marquardt
    steps -- as ONE replayed HIP graph: ``action = controller(image, target_flow[, init_action, visible_mask])``.
    Camera rig, tracked rays and iteration count are fixed at capture time; nothing in the step synchronises with the
    host, so the per-frame host cost is three small copies and one graph launch.

    ``loss``, ``beta``, ``reg``, ``bounds`` and ``views_per_command`` are ``solve_action``'s options, fixed at capture
    time as well.  With ``views_per_command = V`` the rig's B = G * V cameras constrain G commands: one call takes the B
    images [B,3,H,W] and target flows [B,R,2] (init_action [G,A]) and returns [G,A].  ``linearization`` holds the
    graph's static linearisation of the last call."""

    def __init__(self, model: Model, camera_input: CameraInput, rendering_input: RenderingInput, iterations: int = 8,
                 damping: float = 1e-3, action_dim: Optional[int] = None, warmup: int = 2, *, loss: str = "mse",
                 beta: float = 1.0, reg: float = 0.0, bounds=None, views_per_command: int = 1):
        a = action_dim or model.cfg.action_dim
        b, r = rendering_input.origins.shape[:2]
        dev = rendering_input.origins.device
        _check_options(loss, beta, reg, views_per_command, b)
        g = b if views_per_command == 1 else b // views_per_command
        self._image = camera_input.input_image.clone()
        self._target = torch.zeros(b, r, 2, device=dev)
        self._init = torch.zeros(g, a, device=dev)
        self._mask = torch.ones(b, r, device=dev)
        if bounds is not None:   # static copies, kept alive with the graph: the captured launch reads these buffers
            bounds = self._bounds = tuple(None if t is None else t.clone() for t in _box(bounds, g, a, dev))
        options = dict(loss=loss, beta=beta, reg=reg, bounds=bounds, views_per_command=views_per_command)
        cam = CameraInput(self._image, camera_input.ctxt_extrinsics, camera_input.ctxt_intrinsics,
                          camera_input.trgt_extrinsics, camera_input.trgt_intrinsics)

        def step():
            self.linearization = linearize_flow(model, cam, rendering_input, a)
            return solve_action(self.linearization, self._target, self._init, iterations, damping, self._mask, **options)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                step()
        torch.cuda.current_stream().wait_stream(side)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self._action = step()

    def __call__(self, image: torch.Tensor, target_flow: torch.Tensor, init_action: Optional[torch.Tensor] = None,
                 visible_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._image.copy_(image)
        self._target.copy_(target_flow)
        if init_action is None:
            self._init.zero_()
        else:
            self._init.copy_(init_action)
        if visible_mask is None:
            self._mask.fill_(1.0)
        else:
            self._mask.copy_(visible_mask)
        self._graph.replay()
        return self._action
