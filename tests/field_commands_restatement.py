"""Numpy restatement of inverse kinematics on the part tree (field_volume.solve_commands / cloud_commands; njf_field_commands
in include/njf_hip.h), written from the stated semantics:

* counted rows of problem m: ``i < min(count, n)``, the label has a slot p by the rule of the pose, the slot's pose status is 0,
  the weight is finite and > 0 (1 without weights), the three target coordinates are finite;
* objective ``L_m(u) = (1/W_m) sum_i w_i |R_p(u) x_i + t_p(u) - y_mi|^2 + (reg/A) |u|^2`` with section 17's pose, in double;
* moments per (m, p), centred on ``c_p``: ``s0, s1 [3], S2 [6: xx xy xz yy yz zz], t1 [3], C [9, row-major: target row, point
  column], e`` -- the terms ``w``, ``w x_r``, ``(w x_r) x_c``, ``w y_r``, ``(w y_r) x_c``, ``w ((y0 y0 + y1 y1) + y2 y2)`` in double;
* the link derivative twist ``(W, U)`` per slot and channel, carried up the chain by the adjoint, ``d x'/d u_a = W_a x x' + U_a``;
* cost, half-gradient g and Gauss-Newton matrix H per part from the moments, or row by row (``evaluate_rows``);
* the Levenberg-Marquardt iteration of the robust solve, in double, on the fp32 lattice.

``moments`` gives the exactly rounded sums (math.fsum) with the worst-case bound of any summation order beside them."""
import math

import numpy as np

import field_joints_restatement as J
import field_pose_restatement as R

MOMENTS = 23
SERIES = 1e-2
NO_ROWS, NOT_FINITE = 1, 2


def derivative_coefficients(th2, a, b, g, series=None):
    """``(b2, g2) = (db/dth2, dg/dth2)``: the series up to ``th2 <= 1e-2``, the closed forms above."""
    if (th2 <= SERIES) if series is None else series:
        return (((1.0 / 907200.0) * th2 - 1.0 / 13440.0) * th2 + 1.0 / 360.0) * th2 - 1.0 / 24.0, \
               (((1.0 / 9979200.0) * th2 - 1.0 / 120960.0) * th2 + 1.0 / 2520.0) * th2 - 1.0 / 120.0
    return (a - 2.0 * b) / (2.0 * th2), (b - 3.0 * g) / (2.0 * th2)


def _link_source(twists, joints, tree, p, sign):
    if sign:
        j = int(tree[1][p])
        return joints["omega"][j], joints["velocity"][j], joints["anchor"][j], sign
    return twists["omega"][p], twists["velocity"][p], twists["centroid"][p], 1.0


def link_twists(twists, u, joints=None, tree=None):
    """``(G [K] of (R, t), S [K, A, 6], bits [K])`` of one command ``u`` (fp32 values): the link motions of section 17 and the
    spatial derivative twist ``(W, U)`` of every link and channel; a slot with a link bit has the identity and zero twists."""
    bits, sign = R.link_bits(twists["status"], twists["count"], joints, tree)
    u = np.asarray(u, dtype=np.float32).astype(np.float64)
    k, a_dim = len(bits), u.shape[0]
    g_all, s_all = [], np.zeros((k, a_dim, 6))
    for p in range(k):
        if bits[p]:
            g_all.append(R.IDENTITY)
            continue
        ws, vs, c, s = _link_source(twists, joints, tree, p, sign[p])
        ws, vs, c = (np.asarray(t, dtype=np.float64) for t in (ws, vs, c))
        w, v = np.zeros(3), np.zeros(3)
        for a in range(a_dim):
            w = w + u[a] * ws[a]
            v = v + u[a] * vs[a]
        w, v = s * w, s * v
        g_all.append(R.motion(w, v, c))
        th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
        ca, cb, cg = R.coefficients(th2)
        b2, g2 = derivative_coefficients(th2, ca, cb, cg)
        wx, eye = R.hat(w), np.eye(3)
        wx2 = np.outer(w, w) - eye * th2
        vm = (eye + cb * wx) + cg * wx2
        base = c + vm @ v
        for a in range(a_dim):
            wd, vd = s * ws[a], s * vs[a]
            big_w = vm @ wd
            wdx = R.hat(wd)
            dv = 2.0 * (w @ wd) * (b2 * wx + g2 * wx2) + cb * wdx + cg * (wdx @ wx + wx @ wdx)
            s_all[p, a, :3] = big_w
            s_all[p, a, 3:] = -np.cross(big_w, base) + vm @ vd + dv @ v
    return g_all, s_all, bits


def chain(twists, u, joints=None, tree=None):
    """dict of rotation [K, 3, 3], translation [K, 3], twist [K, A, 6], status, depth [K] of one command: the pose of section 17
    and the derivative twists carried up the chain, ``S <- Ad_G(S) + S_q`` before ``T <- G_q o T``."""
    g, s_link, bits = link_twists(twists, u, joints, tree)
    k = len(bits)
    rotation, translation, twist = np.zeros((k, 3, 3)), np.zeros((k, 3)), np.zeros_like(s_link)
    status, depth = bits.copy(), np.zeros(k, np.int32)
    for p in range(k):
        ok, steps = not bits[p] & 2, 0
        t, s = g[p], s_link[p].copy()
        q = -1 if tree is None else int(tree[0][p])
        while ok and q != -1:
            if q < -1 or q >= k or steps >= k or bits[q] & 2:
                ok = False
                break
            rq, tq = g[q]
            w = s[:, :3] @ rq.T
            s = np.concatenate([w, s[:, 3:] @ rq.T - np.cross(w, tq)], axis=1) + s_link[q]
            t = R.compose(g[q], t)
            steps += 1
            q = int(tree[0][q])
        depth[p] = steps
        if not ok:
            status[p] |= 2
            t, s = R.IDENTITY, np.zeros_like(s)
        rotation[p], translation[p], twist[p] = t[0], t[1], s
    return dict(rotation=rotation, translation=translation, twist=twist, status=status, depth=depth)


def pose_status(twists, joints=None, tree=None):
    a_dim = np.asarray(twists["omega"]).shape[1]
    ref = R.poses(twists, np.zeros((1, a_dim), np.float32), joints, tree)
    return ref["status"], ref["depth"]


def counted(xyz, labels, targets, parts, parts_count, status, weights=None, count=None):
    """``(slot [n], w [M, n])``: the slot of every row (-1: none) and the weight of every (problem, row), 0.0 where it is not
    counted."""
    targets = np.asarray(targets, dtype=np.float32)
    m, n = targets.shape[:2]
    slot = J.slots(labels, parts, parts_count, count)
    ok = slot >= 0
    ok[ok] = np.asarray(status)[slot[ok]] == 0
    w = np.ones((m, n)) if weights is None else np.broadcast_to(np.asarray(weights, dtype=np.float32).astype(np.float64), (m, n)).copy()
    w[~(np.isfinite(w) & (w > 0.0))] = 0.0
    w[:, ~ok] = 0.0
    w[~np.isfinite(targets).all(axis=2)] = 0.0
    return slot, w


def moment_terms(xyz, y, w, c):
    """[rows, 23] float64: the terms of the moments of rows ``xyz`` with targets ``y`` (fp32) and weights ``w`` about ``c``."""
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64) - c
    t = np.asarray(y, dtype=np.float32).astype(np.float64) - c
    out = np.zeros((x.shape[0], MOMENTS))
    out[:, 0] = w
    wx, wy = w[:, None] * x, w[:, None] * t
    out[:, 1:4] = wx
    for e, (r, col) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        out[:, 4 + e] = wx[:, r] * x[:, col]
    out[:, 10:13] = wy
    for r in range(3):
        for col in range(3):
            out[:, 13 + 3 * r + col] = wy[:, r] * x[:, col]
    out[:, 22] = w * ((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
    return out


def moments(xyz, labels, targets, parts, parts_count, status, centroid, weights=None, count=None, exact=True):
    """``(moments [M, K, 23], bound [M, K, 23])``: the exactly rounded sums (``exact``; numpy's pairwise sums otherwise) and
    ``(n_p + 3) 2^-53 sum |terms|``, the worst-case error of any summation order."""
    slot, w = counted(xyz, labels, targets, parts, parts_count, status, weights, count)
    m, k = w.shape[0], len(parts)
    out, bound = np.zeros((m, k, MOMENTS)), np.zeros((m, k, MOMENTS))
    targets = np.asarray(targets, dtype=np.float32)
    for i in range(m):
        for p in range(k):
            rows = (slot == p) & (w[i] > 0.0)
            if not rows.any():
                continue
            terms = moment_terms(np.asarray(xyz)[rows], targets[i][rows], w[i][rows], np.asarray(centroid[p], dtype=np.float64))
            out[i, p] = [math.fsum(col) for col in terms.T] if exact else terms.sum(axis=0)
            bound[i, p] = (terms.shape[0] + 3) * 2.0 ** -53 * np.abs(terms).sum(axis=0)
    return out, bound


def energy(mom):
    """``(E [M], W [M])``: ``E_m = sum w (|x~|^2 + |y~|^2)`` and ``W_m`` from the moments."""
    mom = np.asarray(mom)
    return (mom[..., 4] + mom[..., 7] + mom[..., 9] + mom[..., 22]).sum(axis=-1), mom[..., 0].sum(axis=-1)


def _sym(s2):
    return np.array([[s2[0], s2[1], s2[2]], [s2[1], s2[3], s2[4]], [s2[2], s2[4], s2[5]]])


def evaluate_moments(mom, pose, centroid):
    """``(cost, g [A], H [A, A], W)`` of one problem from its moments ``mom [K, 23]`` and the ``chain`` result ``pose``; cost, g
    and H are divided by W (all zero when W is 0)."""
    a_dim = pose["twist"].shape[1]
    cost, g, h, weight = 0.0, np.zeros(a_dim), np.zeros((a_dim, a_dim)), 0.0
    for p in range(mom.shape[0]):
        if pose["status"][p] != 0:
            continue
        mp = mom[p]
        s0, s1, s2, t1, c_m, e = mp[0], mp[1:4], _sym(mp[4:10]), mp[10:13], mp[13:22].reshape(3, 3), mp[22]
        r, t = pose["rotation"][p], pose["translation"][p]
        c = np.asarray(centroid[p], dtype=np.float64)
        d = r @ c + t
        dt = d - c
        rs1 = r @ s1
        cost += np.trace(s2) + 2.0 * (dt @ rs1) + s0 * (dt @ dt) - 2.0 * np.sum(r * c_m) - 2.0 * (dt @ t1) + e
        big_a, beta = [], []
        for a in range(a_dim):
            w, u = pose["twist"][p, a, :3], pose["twist"][p, a, 3:]
            big_a.append(R.hat(w) @ r)
            beta.append(np.cross(w, d) + u)
        for a in range(a_dim):
            g[a] += np.trace(big_a[a] @ s2 @ r.T) + (big_a[a] @ s1) @ dt - np.sum(big_a[a] * c_m) + beta[a] @ rs1 \
                + s0 * (beta[a] @ dt) - beta[a] @ t1
            for b in range(a_dim):
                h[a, b] += np.trace(big_a[a] @ s2 @ big_a[b].T) + beta[a] @ (big_a[b] @ s1) + beta[b] @ (big_a[a] @ s1) \
                    + s0 * (beta[a] @ beta[b])
        weight += s0
    if weight > 0.0:
        return cost / weight, g / weight, h / weight, weight
    return 0.0, np.zeros(a_dim), np.zeros((a_dim, a_dim)), 0.0


def evaluate_rows(xyz, slot, w, y, pose):
    """The same by float64 sums over the rows: ``slot [n]``, ``w [n]`` (0.0 = not counted), ``y [n, 3]`` of one problem."""
    a_dim = pose["twist"].shape[1]
    rows = w > 0.0
    weight = w[rows].sum()
    if not weight > 0.0:
        return 0.0, np.zeros(a_dim), np.zeros((a_dim, a_dim)), 0.0
    p = slot[rows]
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64)[rows]
    moved = np.einsum("nij,nj->ni", pose["rotation"][p], x) + pose["translation"][p]
    res = moved - np.asarray(y, dtype=np.float32).astype(np.float64)[rows]
    tw = pose["twist"][p]                                                     # [rows, A, 6]
    vel = np.cross(tw[:, :, :3], moved[:, None, :]) + tw[:, :, 3:]            # [rows, A, 3]
    ww = w[rows]
    cost = (ww * (res * res).sum(axis=1)).sum() / weight
    g = np.einsum("n,nac,nc->a", ww, vel, res) / weight
    h = np.einsum("n,nac,nbc->ab", ww, vel, vel) / weight
    return cost, g, h, weight


def _clamp32(u, lo, hi):
    return np.minimum(np.maximum(u, lo), hi).astype(np.float32)


def solve(twists, xyz, labels, targets, parts, joints=None, tree=None, weights=None, count=None, init=None, lower=None, upper=None,
          reg=0.0, iterations=20, damping=1e-3, given_moments=None, by_rows=False):
    """dict of commands [M, A] fp32, cost, initial_cost, weight [M], steps, status [M], gradient [M, A], part_status, depth [K],
    moments [M, K, 23].  ``given_moments``: solve on these instead of the exactly rounded ones; ``by_rows``: evaluate row by
    row instead of from the moments."""
    targets = np.asarray(targets, dtype=np.float32)
    m, a_dim = targets.shape[0], np.asarray(twists["omega"]).shape[1]
    part_status, depth = pose_status(twists, joints, tree)
    slot, w = counted(xyz, labels, targets, parts, twists["count"], part_status, weights, count)
    mom = given_moments
    if mom is None:
        mom, _ = moments(xyz, labels, targets, parts, twists["count"], part_status, twists["centroid"], weights, count)
    rows = lambda v, dtype: np.broadcast_to(np.asarray(v, dtype=dtype), (m, a_dim))   # noqa: E731
    lo = rows(-np.inf if lower is None else lower, np.float32).astype(np.float64)
    hi = rows(np.inf if upper is None else upper, np.float32).astype(np.float64)
    start = rows(0.0 if init is None else init, np.float32).astype(np.float64)
    out = dict(commands=np.zeros((m, a_dim), np.float32), cost=np.zeros(m), initial_cost=np.zeros(m), weight=np.zeros(m),
               steps=np.zeros(m, np.int32), status=np.zeros(m, np.int32), gradient=np.zeros((m, a_dim)), part_status=part_status,
               depth=depth, moments=np.asarray(mom))
    reg_a = reg / a_dim

    def evaluate(i, u):
        pose = chain(twists, u, joints, tree)
        if by_rows:
            c, g, h, wt = evaluate_rows(xyz, slot, w[i], targets[i], pose)
        else:
            c, g, h, wt = evaluate_moments(np.asarray(mom)[i], pose, twists["centroid"])
        c = max(c, 0.0) if c == c else c
        u64 = u.astype(np.float64)
        return c, g, h, wt, c + reg_a * (u64 @ u64)

    for i in range(m):
        u = _clamp32(start[i], lo[i], hi[i])
        c, g, h, wt, obj = evaluate(i, u)
        out["weight"][i], out["initial_cost"][i] = wt, c
        lam, steps = damping, 0
        if not wt > 0.0:
            out["status"][i] |= NO_ROWS
        elif not np.isfinite(obj):
            out["status"][i] |= NOT_FINITE
        else:
            for _ in range(iterations):
                u64 = u.astype(np.float64)
                gb, hb = g + reg_a * u64, h + reg_a * np.eye(a_dim)
                frozen = ((u64 <= lo[i]) & (gb > 0.0)) | ((u64 >= hi[i]) & (gb < 0.0))
                rhs = np.where(frozen, 0.0, gb)
                for a in range(a_dim):
                    if frozen[a]:
                        hb[a, :], hb[:, a] = 0.0, 0.0
                        hb[a, a] = 1.0
                for a in range(a_dim):
                    hb[a, a] += lam * max(hb[a, a], 1e-12)
                step = gauss_jordan(hb, rhs)
                cand = _clamp32(u64 - step, lo[i], hi[i])
                cc, cg, ch, _, cobj = evaluate(i, cand)
                better = cobj < obj
                if better:
                    u, c, g, h, obj, steps = cand, cc, cg, ch, cobj, steps + 1
                lam = min(max(lam / 3.0 if better else lam * 4.0, 1e-9), 1e9)
        out["commands"][i], out["cost"][i], out["steps"][i] = u, c, steps
        out["gradient"][i] = g + reg_a * u.astype(np.float64)
    return out


def gauss_jordan(h, rhs):
    """The solution of ``h x = rhs`` by un-pivoted Gauss-Jordan."""
    a_dim = rhs.shape[0]
    mat = np.concatenate([h, rhs[:, None]], axis=1)
    for p in range(a_dim):
        row = mat[p] * (1.0 / mat[p, p])
        mat = mat - mat[:, p:p + 1] * row[None, :]
        mat[p] = row
    return mat[:, a_dim]


def posed_targets(twists, commands, xyz, labels, parts, joints=None, tree=None, count=None):
    """fp32 [M, n, 3]: the rows under the planted ``commands`` (``R.poses`` + ``R.points``; rows of no part stay)."""
    ref = R.poses(twists, commands, joints, tree)
    return R.points(ref["rotation"], ref["translation"], ref["status"], parts, twists["count"], commands, xyz, labels, count)
