"""Numpy restatement of posing the parts of an extracted field under a command (field_volume.part_poses / cloud_pose /
FieldPose.apply; njf_field_pose in include/njf_hip.h), written from the stated semantics:

* link motion ``G[m, p] = (R, t)``: with ``u = commands[m]`` (fp32, exactly double), ``w = sum_a u_a omega_a`` and ``v = sum_a u_a
  v_a`` in ascending a from 0.0 -- of the slot's own twist about its centroid (no tree, or ``parent[p] < 0``) or of the relative
  twist of joint ``j = joint_of[p]`` about its anchor, times +1 when ``part_a[j] == parent[p]`` and -1 when ``part_b[j] ==
  parent[p]`` --; ``th2 = (wx wx + wy wy) + wz wz``; the coefficients a, b, g by their series up to ``th2 <= 1e-6`` and by
  ``sin(th)/th``, ``2 sin(th/2)^2 / th2``, ``(th - sin th) / (th2 th)`` above; ``R = I + a [w]x + b [w]x^2``, ``V = I + b [w]x + g
  [w]x^2``, ``t = (c - R c) + V v``;
* link bits: 1 = unused slot or twist status bit 1; 2 = ``parent[p] >= 0`` and (``q >= Ku``, ``q == p``, ``j`` outside ``[0, Ju)``
  or the joint does not join p and q); a slot with a bit has ``G = I``;
* pose: ``T = G[m, p]``, then ``T <- G[m, q] o T`` up the parents; the identity and status bit 2 when p or a slot on the walk
  is a bad link, when the walk would take more than K steps or meets a q outside ``[-1, K)``; ``depth`` = the steps taken;
* points: a row below ``min(count, n)`` whose label is a part of status 0 gets ``(float)(((R_c0 x + R_c1 y) + R_c2 z) + t_c)``;
  any other such row ``(float)(x_c + u_0 J_0c + u_1 J_1c + ...)`` in double, one add per term, with a Jacobian, and ``x``
  without; rows past the count are not written.

The transforms hold to a tolerance (two libm calls per link); the point stage has no transcendental and no sum over rows, so
numpy's element-wise IEEE arithmetic in the stated order gives the device's bytes."""
import numpy as np

import field_joints_restatement as J

SMALL = 1e-6
IDENTITY = (np.eye(3), np.zeros(3))


def coefficients(th2):
    if th2 <= SMALL:
        th4 = th2 * th2
        return (1.0 - th2 / 6.0) + th4 / 120.0, (0.5 - th2 / 24.0) + th4 / 720.0, (1.0 / 6.0 - th2 / 120.0) + th4 / 5040.0
    th = np.sqrt(th2)
    s, sh = np.sin(th), np.sin(0.5 * th)
    return s / th, 2.0 * (sh * sh) / th2, (th - s) / (th2 * th)


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def motion(w, v, c):
    """``(R [3, 3], t [3])`` of the twist ``(w, v)`` about the point ``c``."""
    w, v, c = (np.asarray(x, dtype=np.float64) for x in (w, v, c))
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    a, b, g = coefficients(th2)
    wx, eye = hat(w), np.eye(3)
    wx2 = np.outer(w, w) - eye * th2
    r = (eye + a * wx) + b * wx2
    vm = (eye + b * wx) + g * wx2
    rc = (r[:, 0] * c[0] + r[:, 1] * c[1]) + r[:, 2] * c[2]
    vv = (vm[:, 0] * v[0] + vm[:, 1] * v[1]) + vm[:, 2] * v[2]
    return r, (c - rc) + vv


def compose(outer, inner):
    """``outer o inner``: first ``inner``, then ``outer``."""
    (rq, tq), (r, t) = outer, inner
    rn = (rq[:, 0:1] * r[0:1, :] + rq[:, 1:2] * r[1:2, :]) + rq[:, 2:3] * r[2:3, :]
    tn = ((rq[:, 0] * t[0] + rq[:, 1] * t[1]) + rq[:, 2] * t[2]) + tq
    return rn, tn


def _active(count, capacity):
    return capacity if count is None else min(max(int(count), 0), capacity)


def link_bits(status, parts_count, joints=None, tree=None):
    """``(bits [K], sign [K])``: the link bits of every slot and the sign of its joint's twist (0 where it has none)."""
    k = len(status)
    ku = _active(parts_count, k)
    bits, sign = np.zeros(k, np.int32), np.zeros(k)
    for p in range(k):
        if p >= ku or int(status[p]) & 1:
            bits[p] |= 1
        q = -1 if tree is None else int(tree[0][p])
        if q < 0:
            continue
        j, ju = int(tree[1][p]), _active(joints["count"], len(joints["part_a"]))
        if q >= ku or q == p or not 0 <= j < ju:
            bits[p] |= 2
        elif (int(joints["part_a"][j]), int(joints["part_b"][j])) == (q, p):
            sign[p] = 1.0
        elif (int(joints["part_a"][j]), int(joints["part_b"][j])) == (p, q):
            sign[p] = -1.0
        else:
            bits[p] |= 2
    return bits, sign


def links(twists, commands, joints=None, tree=None):
    """``(G, bits)``: ``G[m][p] = (R, t)``.  ``twists``: a dict of status, count, centroid, omega, velocity; ``joints``: a dict of
    part_a, part_b, count, anchor, omega, velocity; ``tree``: (parent, joint_of)."""
    bits, sign = link_bits(twists["status"], twists["count"], joints, tree)
    commands = np.asarray(commands, dtype=np.float32).astype(np.float64)
    out = []
    for u in commands:
        row = []
        for p in range(len(bits)):
            if bits[p]:
                row.append(IDENTITY)
                continue
            if sign[p]:
                j = int(tree[1][p])
                ws, vs, c = joints["omega"][j], joints["velocity"][j], joints["anchor"][j]
            else:
                ws, vs, c = twists["omega"][p], twists["velocity"][p], twists["centroid"][p]
            w, v = np.zeros(3), np.zeros(3)
            for a in range(len(u)):
                w = w + u[a] * np.asarray(ws[a], dtype=np.float64)
                v = v + u[a] * np.asarray(vs[a], dtype=np.float64)
            s = sign[p] if sign[p] else 1.0
            row.append(motion(s * w, s * v, c))
        out.append(row)
    return out, bits


def poses(twists, commands, joints=None, tree=None):
    """dict of rotation [M, K, 3, 3], translation [M, K, 3] float64, status, depth [K] int32; every walk is bounded by K."""
    g, bits = links(twists, commands, joints, tree)
    m, k = len(g), len(bits)
    rotation, translation = np.zeros((m, k, 3, 3)), np.zeros((m, k, 3))
    status, depth = bits.copy(), np.zeros(k, np.int32)
    for p in range(k):
        ok, steps, chain = not bits[p] & 2, 0, []
        q = -1 if tree is None else int(tree[0][p])
        while ok and q != -1:
            if q < -1 or q >= k or steps >= k or bits[q] & 2:
                ok = False
                break
            chain.append(q)
            steps += 1
            q = int(tree[0][q])
        assert steps <= k
        depth[p] = steps
        if not ok:
            status[p] |= 2
        for i in range(m):
            t = g[i][p]
            for q in chain:
                t = compose(g[i][q], t)
            rotation[i, p], translation[i, p] = t if ok else IDENTITY
    return dict(rotation=rotation, translation=translation, status=status, depth=depth)


def points(rotation, translation, status, parts, parts_count, commands, xyz, labels, count=None, jacobian=None, out=None):
    """``posed [M, n, 3]`` fp32 from GIVEN transforms; ``out`` (a pre-filled buffer) keeps its rows past the count."""
    xyz = np.asarray(xyz, dtype=np.float32)
    n, m = xyz.shape[0], rotation.shape[0]
    rows = _active(count, n)
    slot = J.slots(labels, parts, parts_count, count)
    rigid = slot >= 0
    rigid[rigid] = np.asarray(status)[slot[rigid]] == 0
    rigid[rows:] = False
    other = ~rigid
    other[rows:] = False
    posed = np.zeros((m, n, 3), np.float32) if out is None else out
    x = xyz.astype(np.float64)
    u = np.asarray(commands, dtype=np.float32).astype(np.float64)
    for i in range(m):
        r, t = rotation[i][slot[rigid]], translation[i][slot[rigid]]
        xr = x[rigid]
        moved = ((r[:, :, 0] * xr[:, 0:1] + r[:, :, 1] * xr[:, 1:2]) + r[:, :, 2] * xr[:, 2:3]) + t
        posed[i][rigid] = moved.astype(np.float32)
        acc = x[other].copy()
        if jacobian is not None:
            jac = np.asarray(jacobian, dtype=np.float32)[other].astype(np.float64)
            for a in range(u.shape[1]):
                acc = acc + u[i, a] * jac[:, a, :]
        posed[i][other] = acc.astype(np.float32)
    return posed


def twists_of(scene, **override):
    """The twists dict of a scene of field_joints_restatement."""
    s = dict(scene)
    s.update(override)
    return dict(status=s["status"], count=s["parts_count"], centroid=s["centroid"], omega=s["omega"], velocity=s["velocity"])


def joints_of(ref):
    """The joints dict of a result of field_joints_restatement.run."""
    return dict(part_a=ref["part_a"], part_b=ref["part_b"], count=int(ref["count"][0]), anchor=ref["anchor"], omega=ref["omega"],
                velocity=ref["velocity"])


def line(k=256, a_dim=3, seed=5, scale=0.02):
    """K one-node parts in a row, each hinged on the previous one (depth K - 1), with small random twists: a scene dict in the
    form of field_joints_restatement's, its joints (K - 1 rows) and its tree."""
    rng = np.random.default_rng(seed)
    parts = np.arange(k, dtype=np.int32)
    centroid = np.stack([0.05 * np.arange(k), np.zeros(k), np.ones(k)], axis=-1)
    scene = dict(parts=parts, parts_count=None, status=np.zeros(k, np.int32), centroid=centroid,
                 omega=scale * rng.normal(size=(k, a_dim, 3)), velocity=scale * rng.normal(size=(k, a_dim, 3)))
    lo = np.arange(k - 1, dtype=np.int32)
    joints = dict(part_a=lo, part_b=lo + 1, count=k - 1, anchor=0.5 * (centroid[:-1] + centroid[1:]),
                  omega=scale * rng.normal(size=(k - 1, a_dim, 3)), velocity=scale * rng.normal(size=(k - 1, a_dim, 3)))
    tree = (np.arange(-1, k - 1, dtype=np.int32), np.arange(-1, k - 1, dtype=np.int32))
    return scene, joints, tree


TRANSFORM_TOLERANCE = 1e-13


def scale_of(twists, commands, joints=None):
    """L of the transform tolerance: the largest magnitude among the centroid and anchor coordinates and the speeds ``|sum_a u_a
    v_a|`` of every twist that can enter a link."""
    u = np.asarray(commands, dtype=np.float64)
    big = [np.abs(np.asarray(twists["centroid"])).max(), np.linalg.norm(np.einsum("ma,kac->mkc", u, twists["velocity"]), axis=-1).max()]
    if joints is not None:
        big += [np.abs(np.asarray(joints["anchor"])).max(), np.linalg.norm(np.einsum("ma,kac->mkc", u, joints["velocity"]), axis=-1).max()]
    return float(max(big))


def worst_ratio(rotation, translation, ref, scale):
    """The largest ``|R - R_ref| / (1e-13 (depth + 1))`` and ``|t - t_ref| / (1e-13 (depth + 1) max(1, L))``: at most 1 within the
    tolerance (a link is about 100 double operations and two libm calls of 1-2 ulp on either side, under 1e-14; the bound
    leaves an order of magnitude, and an fp32 evaluation misses it by four)."""
    bound = TRANSFORM_TOLERANCE * (ref["depth"].astype(np.float64) + 1.0)
    dr = np.abs(np.asarray(rotation) - ref["rotation"]).max(axis=(2, 3)) / bound[None]
    dt = np.abs(np.asarray(translation) - ref["translation"]).max(axis=2) / (bound[None] * max(1.0, scale))
    return float(max(dr.max(), dt.max()))
