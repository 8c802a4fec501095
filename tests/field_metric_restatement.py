"""Numpy restatement of inverse kinematics with a 3 x 3 information per target (field_volume.solve_commands_metric /
register_commands_metric; njf_field_commands_metric in include/njf_hip.h), written from the stated
semantics on top of field_commands_restatement (``chain``, ``counted``, ``gauss_jordan``, the Levenberg-Marquardt rule):

* counted rows: those of section 18 with six finite information entries;
* objective ``L_m(u) = (1/W_m) sum_i w_i z_mi^T Q_mi z_mi + (reg/A) |u|^2``, ``z = R_p(u) x + t_p(u) - y``, in double;
* the 74 moments per (m, p) about ``c_p``: ``s0``, ``P[e][f] = sum (w Q_e) (x^_i x^_j)``, ``B[a][j] = sum (w b_a) x^_j``, ``e = sum w
  ((y~0 b0 + y~1 b1) + y~2 b2)`` with ``x^ = (x~, 1)`` and ``b_a = (Q_a0 y~0 + Q_a1 y~1) + Q_a2 y~2``;
* the shares of a slot from ``G = (R | d - c)`` and ``D_k = ([W_k]x R | W_k x d + U_k)``: cost ``<G, G> - 2 G.B + e``, half-gradient
  ``<D_k, G> - D_k.B``, Gauss-Newton matrix ``<D_k, D_l>``, ``<X, Y> = sum X_ai Y_bj P[ab][ij]`` -- or row by row;
* the helpers that turn pixels and normals into (targets, information), and the registration loop with its gather.

``moments`` gives the exactly rounded sums (math.fsum) with the worst-case bound of any summation order beside them."""
import math

import numpy as np

import field_commands_restatement as F
import field_nearest_restatement as N
import field_pose_restatement as R

MOMENTS = 74
P_AT, B_AT, E_AT = 1, 61, 73
SIX = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))                                      # xx xy xz yy yz zz
TEN = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))
IDENTITY6 = np.float32([1, 0, 0, 1, 0, 1])


def symmetric(q6):
    """``[..., 3, 3]`` float64 from the packed ``[..., 6]`` (fp32 values)."""
    q = np.asarray(q6, dtype=np.float32).astype(np.float64)
    return np.stack([np.stack([q[..., 0], q[..., 1], q[..., 2]], -1), np.stack([q[..., 1], q[..., 3], q[..., 4]], -1),
                     np.stack([q[..., 2], q[..., 4], q[..., 5]], -1)], -2)


def pack(matrix):
    """fp32 ``[..., 6]`` from symmetric ``[..., 3, 3]``."""
    matrix = np.asarray(matrix)
    return np.stack([matrix[..., r, c] for r, c in SIX], -1).astype(np.float32)


def per_problem(information, m):
    """fp32 ``[M, n, 6]`` from ``[n, 6]`` or ``[M, n, 6]``."""
    information = np.asarray(information, dtype=np.float32)
    return np.broadcast_to(information, (m,) + information.shape[-2:])


def counted(xyz, labels, targets, information, parts, parts_count, status, weights=None, count=None):
    """``(slot [n], w [M, n])`` of section 18, with 0.0 also where an information entry is not finite."""
    slot, w = F.counted(xyz, labels, targets, parts, parts_count, status, weights, count)
    w[~np.isfinite(per_problem(information, w.shape[0])).all(axis=2)] = 0.0
    return slot, w


def moment_terms(xyz, y, q6, w, c):
    """[rows, 74] float64: the terms of the moments in the header's parenthesisation."""
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64) - c
    t = np.asarray(y, dtype=np.float32).astype(np.float64) - c
    q = np.asarray(q6, dtype=np.float32).astype(np.float64)
    xh = np.concatenate([x, np.ones((x.shape[0], 1))], axis=1)
    out = np.zeros((x.shape[0], MOMENTS))
    out[:, 0] = w
    for e in range(6):
        wq = w * q[:, e]
        for f, (i, j) in enumerate(TEN):
            out[:, P_AT + 10 * e + f] = wq * (xh[:, i] * xh[:, j])
    rows = ((0, 1, 2), (1, 3, 4), (2, 4, 5))
    b = [(q[:, r[0]] * t[:, 0] + q[:, r[1]] * t[:, 1]) + q[:, r[2]] * t[:, 2] for r in rows]
    for a in range(3):
        wb = w * b[a]
        for j in range(4):
            out[:, B_AT + 4 * a + j] = wb * xh[:, j]
    out[:, E_AT] = w * ((t[:, 0] * b[0] + t[:, 1] * b[1]) + t[:, 2] * b[2])
    return out


def moments(xyz, labels, targets, information, parts, parts_count, status, centroid, weights=None, count=None, exact=True):
    """``(moments [M, K, 74], bound [M, K, 74])``: the exactly rounded sums and ``(n_p + 3) 2^-53 sum |terms|``."""
    slot, w = counted(xyz, labels, targets, information, parts, parts_count, status, weights, count)
    m, k = w.shape[0], len(parts)
    out, bound = np.zeros((m, k, MOMENTS)), np.zeros((m, k, MOMENTS))
    targets, information = np.asarray(targets, dtype=np.float32), per_problem(information, m)
    for i in range(m):
        for p in range(k):
            rows = (slot == p) & (w[i] > 0.0)
            if not rows.any():
                continue
            terms = moment_terms(np.asarray(xyz)[rows], targets[i][rows], information[i][rows], w[i][rows],
                                 np.asarray(centroid[p], dtype=np.float64))
            out[i, p] = [math.fsum(col) for col in terms.T] if exact else terms.sum(axis=0)
            bound[i, p] = (terms.shape[0] + 3) * 2.0 ** -53 * np.abs(terms).sum(axis=0)
    return out, bound


def energy(xyz, labels, targets, information, parts, parts_count, status, centroid, weights=None, count=None):
    """``(E [M], W [M])``: ``E_m = sum w tr(Q) (|x~|^2 + |y~|^2)`` over the counted rows, about each row's own centroid."""
    slot, w = counted(xyz, labels, targets, information, parts, parts_count, status, weights, count)
    m = w.shape[0]
    targets, information = np.asarray(targets, dtype=np.float32).astype(np.float64), per_problem(information, m).astype(np.float64)
    c = np.asarray(centroid, dtype=np.float64)[np.maximum(slot, 0)]
    x2 = ((np.asarray(xyz, dtype=np.float32).astype(np.float64) - c) ** 2).sum(axis=1)
    out = np.zeros(m)
    for i in range(m):
        rows = w[i] > 0.0
        trace = information[i][rows][:, [0, 3, 5]].sum(axis=1)
        out[i] = (w[i][rows] * trace * (x2[rows] + ((targets[i][rows] - c[rows]) ** 2).sum(axis=1))).sum()
    return out, w.sum(axis=1)


def _p_tensor(mp):
    """``P[a, b, i, j]`` [3, 3, 4, 4] of one slot's moments."""
    p = np.zeros((3, 3, 4, 4))
    for e, (a, b) in enumerate(SIX):
        for f, (i, j) in enumerate(TEN):
            v = mp[P_AT + 10 * e + f]
            p[a, b, i, j] = p[a, b, j, i] = p[b, a, i, j] = p[b, a, j, i] = v
    return p


def evaluate_moments(mom, pose, centroid):
    """``(cost, g [A], H [A, A], W)`` of one problem from its moments ``mom [K, 74]`` and the ``chain`` result ``pose``, divided
    by W (all zero when W is 0)."""
    a_dim = pose["twist"].shape[1]
    cost, g, h, weight = 0.0, np.zeros(a_dim), np.zeros((a_dim, a_dim)), 0.0
    for p in range(mom.shape[0]):
        if pose["status"][p] != 0:
            continue
        mp = mom[p]
        pt, b, e = _p_tensor(mp), mp[B_AT:B_AT + 12].reshape(3, 4), mp[E_AT]
        r, t = pose["rotation"][p], pose["translation"][p]
        c = np.asarray(centroid[p], dtype=np.float64)
        d = r @ c + t
        big_g = np.concatenate([r, (d - c)[:, None]], axis=1)
        big_d = []
        for a in range(a_dim):
            w, u = pose["twist"][p, a, :3], pose["twist"][p, a, 3:]
            big_d.append(np.concatenate([R.hat(w) @ r, (np.cross(w, d) + u)[:, None]], axis=1))
        pg = np.einsum("abij,bj->ai", pt, big_g)
        cost += np.sum(big_g * pg) - 2.0 * np.sum(big_g * b) + e
        for a in range(a_dim):
            g[a] += np.sum(big_d[a] * pg) - np.sum(big_d[a] * b)
            pd = np.einsum("abij,bj->ai", pt, big_d[a])
            for k in range(a_dim):
                h[k, a] += np.sum(big_d[k] * pd)
        weight += mp[0]
    if weight > 0.0:
        return cost / weight, g / weight, h / weight, weight
    return 0.0, np.zeros(a_dim), np.zeros((a_dim, a_dim)), 0.0


def evaluate_rows(xyz, slot, w, y, q6, pose):
    """The same by float64 sums over the rows: ``slot [n]``, ``w [n]`` (0.0 = not counted), ``y [n, 3]``, ``q6 [n, 6]``."""
    a_dim = pose["twist"].shape[1]
    rows = w > 0.0
    weight = w[rows].sum()
    if not weight > 0.0:
        return 0.0, np.zeros(a_dim), np.zeros((a_dim, a_dim)), 0.0
    p = slot[rows]
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64)[rows]
    q = symmetric(np.asarray(q6)[rows])
    moved = np.einsum("nij,nj->ni", pose["rotation"][p], x) + pose["translation"][p]
    res = moved - np.asarray(y, dtype=np.float32).astype(np.float64)[rows]
    tw = pose["twist"][p]
    vel = np.cross(tw[:, :, :3], moved[:, None, :]) + tw[:, :, 3:]            # [rows, A, 3]
    ww = w[rows]
    qres = np.einsum("ncd,nd->nc", q, res)
    cost = (ww * (res * qres).sum(axis=1)).sum() / weight
    g = np.einsum("n,nac,nc->a", ww, vel, qres) / weight
    h = np.einsum("n,nac,ncd,nbd->ab", ww, vel, q, vel) / weight
    return cost, g, h, weight


def solve(twists, xyz, labels, targets, information, parts, joints=None, tree=None, weights=None, count=None, init=None, lower=None,
          upper=None, reg=0.0, iterations=20, damping=1e-3, given_moments=None, by_rows=False):
    """``F.solve`` on the anisotropic objective: the same dict, moments [M, K, 74]."""
    targets = np.asarray(targets, dtype=np.float32)
    m, a_dim = targets.shape[0], np.asarray(twists["omega"]).shape[1]
    information = per_problem(information, m)
    part_status, depth = F.pose_status(twists, joints, tree)
    slot, w = counted(xyz, labels, targets, information, parts, twists["count"], part_status, weights, count)
    mom = given_moments
    if mom is None:
        mom, _ = moments(xyz, labels, targets, information, parts, twists["count"], part_status, twists["centroid"], weights, count)
    rows = lambda v, dtype: np.broadcast_to(np.asarray(v, dtype=dtype), (m, a_dim))   # noqa: E731
    lo = rows(-np.inf if lower is None else lower, np.float32).astype(np.float64)
    hi = rows(np.inf if upper is None else upper, np.float32).astype(np.float64)
    start = rows(0.0 if init is None else init, np.float32).astype(np.float64)
    out = dict(commands=np.zeros((m, a_dim), np.float32), cost=np.zeros(m), initial_cost=np.zeros(m), weight=np.zeros(m),
               steps=np.zeros(m, np.int32), status=np.zeros(m, np.int32), gradient=np.zeros((m, a_dim)), part_status=part_status,
               depth=depth, moments=np.asarray(mom))
    reg_a = reg / a_dim

    def evaluate(i, u):
        pose = F.chain(twists, u, joints, tree)
        if by_rows:
            c, g, h, wt = evaluate_rows(xyz, slot, w[i], targets[i], information[i], pose)
        else:
            c, g, h, wt = evaluate_moments(np.asarray(mom)[i], pose, twists["centroid"])
        c = max(c, 0.0) if c == c else c
        u64 = u.astype(np.float64)
        return c, g, h, wt, c + reg_a * (u64 @ u64)

    for i in range(m):
        u = F._clamp32(start[i], lo[i], hi[i])
        c, g, h, wt, obj = evaluate(i, u)
        out["weight"][i], out["initial_cost"][i] = wt, c
        lam, steps = damping, 0
        if not wt > 0.0:
            out["status"][i] |= F.NO_ROWS
        elif not np.isfinite(obj):
            out["status"][i] |= F.NOT_FINITE
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
                cand = F._clamp32(u64 - F.gauss_jordan(hb, rhs), lo[i], hi[i])
                cc, cg, ch, _, cobj = evaluate(i, cand)
                better = cobj < obj
                if better:
                    u, c, g, h, obj, steps = cand, cc, cg, ch, cobj, steps + 1
                lam = min(max(lam / 3.0 if better else lam * 4.0, 1e-9), 1e9)
        out["commands"][i], out["cost"][i], out["steps"][i] = u, c, steps
        out["gradient"][i] = g + reg_a * u.astype(np.float64)
    return out


# ---- pixels and normals into (targets, information) ---------------------------------------------------------------------------------
def world_rays(coordinates_xy, intrinsics, cam2world):
    """``(origins, directions)`` [M, n, 3] float64 of normalised pixels: the unit vector along ``K^-1 (x, y, 1)`` turned into the
    world, from the camera's centre."""
    xy = np.asarray(coordinates_xy, dtype=np.float64)
    hom = np.concatenate([xy, np.ones(xy.shape[:-1] + (1,))], axis=-1)
    cam = np.einsum("mij,mnj->mni", np.linalg.inv(np.asarray(intrinsics, dtype=np.float64)), hom)
    cam = cam / np.linalg.norm(cam, axis=-1, keepdims=True)
    c2w = np.asarray(cam2world, dtype=np.float64)
    return np.broadcast_to(c2w[:, None, :3, 3], cam.shape), np.einsum("mij,mnj->mni", c2w[:, :3, :3], cam)


def plane_information(normals):
    """``(1 - 2^-21) n n^T + 2^-21 I`` of the normalised normals, packed fp32."""
    n = np.asarray(normals, dtype=np.float64)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    return pack((1.0 - 2.0 ** -21) * n[..., :, None] * n[..., None, :] + 2.0 ** -21 * np.eye(3))


INFORMATION_FLOOR = 2.0 ** -21


def ray_information(directions, along=0.0):
    """``I - (1 - max(along, 2^-21)) d d^T`` of the normalised directions, packed fp32."""
    d = np.asarray(directions, dtype=np.float64)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return pack(np.eye(3) - (1.0 - max(along, INFORMATION_FLOOR)) * d[..., :, None] * d[..., None, :])


def ray_targets(xyz, coordinates_xy, intrinsics, cam2world):
    """fp32 ``(targets [M, n, 3], information [M, n, 6])``: the foot of every row on the ray of its pixel, ``ray_information(d)``; NaN
    targets where a coordinate is not finite."""
    xy = np.asarray(coordinates_xy, dtype=np.float64)
    seen = np.isfinite(xy).all(axis=-1)
    o, d = world_rays(np.where(seen[..., None], xy, 0.5), intrinsics, cam2world)
    x = np.asarray(xyz, dtype=np.float64)[None]
    foot = o + d * ((x - o) * d).sum(axis=-1, keepdims=True)
    foot[~seen] = np.nan
    return foot.astype(np.float32), ray_information(d)


def project(points, intrinsics, cam2world):
    """Normalised pixels [M, n, 2] float64 of world ``points`` [M, n, 3]: the inverse of ``world_rays``."""
    c2w = np.asarray(cam2world, dtype=np.float64)
    cam = np.einsum("mji,mnj->mni", c2w[:, :3, :3], np.asarray(points, dtype=np.float64) - c2w[:, None, :3, 3])
    pix = np.einsum("mij,mnj->mni", np.asarray(intrinsics, dtype=np.float64), cam)
    return pix[..., :2] / pix[..., 2:]


def look_at(eye, centre):
    """A cam2world [4, 4] float64 at ``eye`` whose +z looks at ``centre``."""
    eye, centre = np.asarray(eye, dtype=np.float64), np.asarray(centre, dtype=np.float64)
    z = (centre - eye) / np.linalg.norm(centre - eye)
    helper = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(helper, z)
    x /= np.linalg.norm(x)
    out = np.eye(4)
    out[:3, 0], out[:3, 1], out[:3, 2], out[:3, 3] = x, np.cross(z, x), z, eye
    return out


# ---- registration ------------------------------------------------------------------------------------------------------------------
def register(twists, xyz, labels, observed, observed_information, max_distance, parts, joints=None, tree=None, observed_count=None,
             count=None, weights=None, init=None, lower=None, upper=None, reg=0.0, rounds=8, iterations=3, damping=1e-3,
             search=N.brute):
    """``N.register`` with the gather ``information[m, i] = observed_information[mo, max(index[m, i], 0)]`` and ``solve``."""
    observed = N._three(observed)
    mo, t = observed.shape[:2]
    source = np.broadcast_to(np.asarray(observed_information, dtype=np.float32), (mo, t, 6))
    a_dim = np.asarray(twists["omega"]).shape[1]
    m = max(mo, 1 if init is None else np.asarray(init).shape[0])
    box = lambda v, fill: np.broadcast_to(np.asarray(fill if v is None else v, dtype=np.float32), (m, a_dim))   # noqa: E731
    u = np.minimum(np.maximum(box(init, 0.0), box(lower, -np.inf)), box(upper, np.inf)).astype(np.float32)
    out = dict(commands_history=np.zeros((rounds, m, a_dim), np.float32), cost_history=np.zeros((rounds, m)),
               found_history=np.zeros((rounds, m), np.int32))
    for r in range(rounds):
        posed = F.posed_targets(twists, u, xyz, labels, parts, joints, tree, count=count)
        near = search(observed, posed, max_distance, observed_count, count, labels)
        information = np.stack([source[0 if mo == 1 else i][np.maximum(near["index"][i], 0)] for i in range(m)])
        fit = solve(twists, xyz, labels, near["matched"], information, parts, joints, tree, weights=weights, count=count, init=u,
                    lower=lower, upper=upper, reg=reg, iterations=iterations, damping=damping)
        out["commands_history"][r], out["cost_history"][r], out["found_history"][r] = fit["commands"], fit["cost"], near["found"]
        out["fit"], out["matches"], u = fit, near, fit["commands"]
    return out
