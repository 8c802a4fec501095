"""Numpy restatement of the joints between the parts of an extracted field (field_volume.part_joints / cloud_joints;
njf_field_joints in include/njf_hip.h), written from the stated semantics:

* the list of a cloud on a grid x batch: ``index [n]`` ascending global indices with a row count (rows from ``min(count, n)`` on
  are never read, an index outside ``[0, B*N)`` is dropped), ``labels [n]`` per row (negative: no part); the part list ``parts
  [K]`` with its true ``parts_count``; row i has slot p iff ``i < count``, ``p < min(parts_count, K)`` and ``labels[i] ==
  parts[p]``;
* contacts: for every row with slot p at node g and every direction d among the first ``connectivity / 2`` of the table, the
  neighbour ``g + d`` inside the grid (no wrap, same batch element) that is a list row with slot ``q != p`` adds 1 to
  ``contacts[lo][hi]`` and ``i_c + i'_c`` to ``sum2[lo][hi][c]``, ``lo = min(p, q)``, ``hi = max(p, q)``, in int64;
* the pairs with ``contacts >= min_contacts`` in ascending ``(lo, hi)``, the first J stored, ``count`` their true number,
  ``status = status[lo] | status[hi]``, unused rows -1 / 0;
* anchor: ``m = (double)sum2_c / (2.0 * (double)contacts)``, ``x_c = (double)origin_c + (double)step_c * m``;
* relative twist per joint and channel, in double in this order: ``r_s = x - c_s``, ``u_s = v_s + cross(omega_s, r_s)``, ``omega =
  omega_hi - omega_lo``, ``velocity = u_hi - u_lo``.

No floating-point sum runs over rows, so numpy's element-wise IEEE arithmetic gives the device's bytes.  ``tables`` is the
vectorised form of the contact table, ``tables_loop`` the same written as a node-pair loop in Python integers, against which
the vectorised form is itself checked.  The scenes the CPU and GPU tests share are built here, once."""
import numpy as np

DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
EMPTY, TRANSLATION = 1, 2
OUTPUTS = ("part_a", "part_b", "contacts", "status", "count", "anchor", "omega", "velocity")


def slots(labels, parts, parts_count=None, count=None):
    """[n] int64: the slot of every row, -1 without one."""
    labels, parts = np.asarray(labels), np.asarray(parts)
    n, k = labels.shape[0], parts.shape[0]
    rows = n if count is None else min(max(int(count), 0), n)
    active = min(k if parts_count is None else max(int(parts_count), 0), k)
    slot = np.full(n, -1, dtype=np.int64)
    for p in range(active):
        if parts[p] >= 0:
            slot[:rows][labels[:rows] == parts[p]] = p
    return slot


def _unravel(dims, g):
    nodes = dims[0] * dims[1] * dims[2]
    node = g % nodes
    yz = dims[1] * dims[2]
    return g // nodes, node // yz, (node % yz) // dims[2], node % dims[2]


def tables(dims, batch, index, slot, connectivity, k):
    """(contacts [K, K], sum2 [K, K, 3]) int64 of the rows ``index`` with slots ``slot`` (-1: none)."""
    total = batch * dims[0] * dims[1] * dims[2]
    index, slot = np.asarray(index, dtype=np.int64), np.asarray(slot, dtype=np.int64)
    keep = (index >= 0) & (index < total) & (slot >= 0)
    g, p = index[keep], slot[keep]
    volume = np.full(total, -1, dtype=np.int64)
    volume[g] = p
    _, ix, iy, iz = _unravel(dims, g)
    contacts, sum2 = np.zeros((k, k), dtype=np.int64), np.zeros((k, k, 3), dtype=np.int64)
    for dx, dy, dz in DIRECTIONS[:connectivity // 2]:
        inside = (ix + dx < dims[0]) & (iy + dy < dims[1]) & (iz + dz < dims[2])
        off = (dx * dims[1] + dy) * dims[2] + dz
        q = np.full(g.shape[0], -1, dtype=np.int64)
        q[inside] = volume[g[inside] + off]
        hit = (q >= 0) & (q != p)
        lo, hi = np.minimum(p, q)[hit], np.maximum(p, q)[hit]
        np.add.at(contacts, (lo, hi), 1)
        for c, (i, d) in enumerate(((ix, dx), (iy, dy), (iz, dz))):
            np.add.at(sum2[:, :, c], (lo, hi), (2 * i + d)[hit])
    return contacts, sum2


def tables_loop(dims, batch, index, slot, connectivity, k):
    """The same table, node pair by node pair in Python integers."""
    nodes = dims[0] * dims[1] * dims[2]
    slot_of = {}
    for g, p in zip(index, slot):
        if 0 <= int(g) < batch * nodes and int(p) >= 0:
            slot_of[int(g)] = int(p)
    contacts = [[0] * k for _ in range(k)]
    sum2 = [[[0, 0, 0] for _ in range(k)] for _ in range(k)]
    for g, p in slot_of.items():
        b, node = divmod(g, nodes)
        ix, rest = divmod(node, dims[1] * dims[2])
        iy, iz = divmod(rest, dims[2])
        for dx, dy, dz in DIRECTIONS[:connectivity // 2]:
            jx, jy, jz = ix + dx, iy + dy, iz + dz
            if jx >= dims[0] or jy >= dims[1] or jz >= dims[2]:
                continue
            q = slot_of.get(b * nodes + (jx * dims[1] + jy) * dims[2] + jz, -1)
            if q < 0 or q == p:
                continue
            lo, hi = min(p, q), max(p, q)
            contacts[lo][hi] += 1
            for c, v in enumerate((ix + jx, iy + jy, iz + jz)):
                sum2[lo][hi][c] += v
    return np.array(contacts, dtype=np.int64), np.array(sum2, dtype=np.int64)


def _cross(w, r):
    return np.stack([w[..., 1] * r[..., 2] - w[..., 2] * r[..., 1],
                     w[..., 2] * r[..., 0] - w[..., 0] * r[..., 2],
                     w[..., 0] * r[..., 1] - w[..., 1] * r[..., 0]], axis=-1)


def joints(dims, origin, step, batch, index, labels, parts, status, centroid, omega, velocity, parts_count=None, count=None,
           connectivity=6, min_contacts=1, max_joints=256, table=tables):
    """The joint list as a dict of numpy arrays named like FieldJoints' fields, plus the raw ``table`` (contacts, sum2)."""
    k, a_dim, j_max = len(parts), omega.shape[1], max_joints
    slot = slots(labels, parts, parts_count, count)
    contacts, sum2 = table(dims, batch, index, slot, connectivity, k)
    pairs = [(lo, hi) for lo in range(k) for hi in range(k) if contacts[lo, hi] >= min_contacts]
    out = dict(part_a=np.full(j_max, -1, np.int32), part_b=np.full(j_max, -1, np.int32), contacts=np.zeros(j_max, np.int64),
               status=np.zeros(j_max, np.int32), count=np.array([len(pairs)], np.int32), anchor=np.zeros((j_max, 3)),
               omega=np.zeros((j_max, a_dim, 3)), velocity=np.zeros((j_max, a_dim, 3)), table=(contacts, sum2))
    origin64 = np.asarray(origin, dtype=np.float32).astype(np.float64)
    step64 = np.asarray(step, dtype=np.float32).astype(np.float64)
    centroid, omega, velocity = (np.asarray(t, dtype=np.float64) for t in (centroid, omega, velocity))
    for j, (lo, hi) in enumerate(pairs[:j_max]):
        out["part_a"][j], out["part_b"][j], out["contacts"][j] = lo, hi, contacts[lo, hi]
        out["status"][j] = int(status[lo]) | int(status[hi])
        m = sum2[lo, hi].astype(np.float64) / (2.0 * np.float64(contacts[lo, hi]))
        x = origin64 + step64 * m
        out["anchor"][j] = x
        u = [velocity[s] + _cross(omega[s], np.broadcast_to(x - centroid[s], (a_dim, 3))) for s in (lo, hi)]
        out["omega"][j] = omega[hi] - omega[lo]
        out["velocity"][j] = u[1] - u[0]
    return out


def run(scene, table=tables, **kw):
    """``joints`` on a scene dict; ``kw`` overrides the scene's entries (parts, parts_count, count, ...) and the options."""
    keys = ("dims", "origin", "step", "batch", "index", "labels", "parts", "status", "centroid", "omega", "velocity", "parts_count",
            "count")
    args = {key: scene[key] for key in keys}
    args.update(kw)
    return joints(table=table, **args)


# ---- the shared scenes ---------------------------------------------------------------------------------------------------------
ORIGIN, STEP = (-0.55, -0.45, 0.9), (0.1, 0.09, 0.125)


def _box_nodes(dims, element, box):
    x0, nx, y0, ny, z0, nz = box
    nodes = dims[0] * dims[1] * dims[2]
    return sorted(element * nodes + (x * dims[1] + y) * dims[2] + z for x in range(x0, x0 + nx) for y in range(y0, y0 + ny)
                  for z in range(z0, z0 + nz))


def node_coordinates(dims, index, origin=ORIGIN, step=STEP):
    """float64 [n, 3]: the node coordinates ``origin + step * i`` (float64 of the fp32 grid constants; test geometry only)."""
    _, ix, iy, iz = _unravel(dims, np.asarray(index, dtype=np.int64))
    o, s = np.asarray(origin, np.float32).astype(np.float64), np.asarray(step, np.float32).astype(np.float64)
    return o + s * np.stack([ix, iy, iz], axis=-1)


def _finish(dims, batch, label_of, a_dim, seed, twists=None, origin=ORIGIN, step=STEP):
    """A scene from a node -> label map: rows in ascending index, parts = the ascending labels >= 0, random twists in double
    (or the given ones), centroid = the mean node coordinate, weight = the node count, energy = sum over the nodes of |J|^2."""
    rng = np.random.default_rng(seed)
    index = np.array(sorted(label_of), dtype=np.int64)
    labels = np.array([label_of[int(g)] for g in index], dtype=np.int32)
    parts = np.unique(labels[labels >= 0]).astype(np.int32)
    k = parts.shape[0]
    xyz = node_coordinates(dims, index, origin, step)
    centroid = np.stack([xyz[labels == p].mean(axis=0) for p in parts])
    if twists is None:
        omega, velocity = rng.normal(size=(k, a_dim, 3)), rng.normal(size=(k, a_dim, 3))
    else:
        omega, velocity = twists(parts, centroid)
    weight = np.array([(labels == p).sum() for p in parts], dtype=np.float64)
    energy = np.zeros((k, a_dim))
    for s, p in enumerate(parts):
        r = xyz[labels == p] - centroid[s]
        for a in range(a_dim):
            jac = velocity[s, a] + _cross(np.broadcast_to(omega[s, a], r.shape), r)
            energy[s, a] = (jac * jac).sum()
    return dict(dims=tuple(dims), origin=origin, step=step, batch=batch, index=index.astype(np.int32), labels=labels, count=None,
                parts=parts, parts_count=None, status=np.zeros(k, np.int32), centroid=centroid, omega=omega, velocity=velocity,
                weight=weight, energy=energy)


CHAIN_DIMS = (12, 10, 9)
CHAIN_BOXES = ((0, 4, 2, 6, 1, 6), (4, 4, 3, 4, 2, 4), (8, 4, 3, 4, 2, 4))     # base, link 1, link 2: x0 nx y0 ny z0 nz
CHAIN_FACE_PAIRS = 16                                                           # the 4 x 4 nodes of a link's end face
CHAIN_FACE_CENTRES = ((3.5, 4.5, 3.5), (7.5, 4.5, 3.5))                         # in node units


def chain(element=0):
    """The planted 3-link chain on a 2 x (12, 10, 9) grid: a base box with zero Jacobian, link 1 hinged on its face with the base
    under channel 0 (axis z through the face centre), link 2 hinged on link 1 under channel 1 (axis y through their face's
    centre) and carried by channel 0; channel 2 moves nothing."""
    label_of = {}
    for box in CHAIN_BOXES:
        g = _box_nodes(CHAIN_DIMS, element, box)
        for i in g:
            label_of[i] = g[0]
    o, s = np.asarray(ORIGIN, np.float32).astype(np.float64), np.asarray(STEP, np.float32).astype(np.float64)
    hinge = [o + s * np.array(c) for c in CHAIN_FACE_CENTRES]
    w0, w1 = np.array([0.0, 0.0, 0.7]), np.array([0.0, -1.3, 0.0])

    def twists(parts, centroid):
        omega, velocity = np.zeros((3, 3, 3)), np.zeros((3, 3, 3))
        for link in (1, 2):                                  # channel 0 turns both links about the first hinge
            omega[link, 0], velocity[link, 0] = w0, np.cross(w0, centroid[link] - hinge[0])
        omega[2, 1], velocity[2, 1] = w1, np.cross(w1, centroid[2] - hinge[1])
        return omega, velocity

    return _finish(CHAIN_DIMS, 2, label_of, 3, 1, twists)


BLOCK_DIMS = (7, 6, 5)


def blocks(seed=2):
    """2 x (7, 6, 5) nodes cut into blocks of 3 x 2 x 2 nodes, one part each, so that parts touch every grid face, linear index
    + 1 lands in the next row or plane between parts, and the part that ends on the last node of element 0 is followed by the
    part that starts on node 0 of element 1.  Then: a single-row part (one node with a label of its own), nodes missing from
    the list, unlabelled rows (-1), one block whose label is taken out of the part list (a label outside it, between parts), a
    negative index and an index past B*N inside the count (dropped), a part of status TRANSLATION, and PAD rows past ``count``
    that repeat listed nodes' neighbours with fitted labels (they must never be read)."""
    rng = np.random.default_rng(seed)
    dims, batch = BLOCK_DIMS, 2
    nodes = dims[0] * dims[1] * dims[2]
    g = np.arange(batch * nodes, dtype=np.int64)
    b, ix, iy, iz = _unravel(dims, g)
    block = ((b * 3 + ix // 3) * 3 + iy // 2) * 3 + iz // 2
    first = {int(k): int(g[block == k].min()) for k in np.unique(block)}
    label_of = {int(i): first[int(k)] for i, k in zip(g, block)}
    single = int(nodes + (4 * dims[1] + 3) * dims[2] + 2)            # an inner node of element 1 becomes a part of its own
    label_of[single] = single
    interior = [int(i) for i in g if int(i) not in (0, nodes - 1, nodes, single)]
    gone = rng.choice(interior, size=60, replace=False)
    for i in gone[:30]:
        del label_of[int(i)]
    for i in gone[30:]:
        label_of[int(i)] = -1
    scene = _finish(dims, batch, label_of, 4, seed)
    outside = 7                                                       # this block's label leaves the part list
    keep = np.arange(scene["parts"].shape[0]) != outside
    scene["single"], scene["outside_label"] = single, int(scene["parts"][outside])
    for key in ("parts", "status", "centroid", "omega", "velocity", "weight", "energy"):
        scene[key] = scene[key][keep]
    scene["status"][3] = TRANSLATION
    scene["omega"][3] = 0.0
    # rows that are dropped, and rows past the count
    index = np.concatenate([[-3], scene["index"], [batch * nodes + 5]]).astype(np.int32)
    labels = np.concatenate([[scene["parts"][0]], scene["labels"], [scene["parts"][1]]]).astype(np.int32)
    scene["count"] = index.shape[0]
    pad = np.array([int(i) for i in gone[:30]], dtype=np.int32)       # nodes missing from the list: reading them adds contacts
    scene["index"] = np.concatenate([index, pad])
    scene["labels"] = np.concatenate([labels, np.full(pad.shape[0], scene["parts"][2], dtype=np.int32)])
    return scene


FACE = 40


def face(seed=3):
    """Two slabs of 40 x 40 nodes facing each other: 1,600 contacts in ONE pair at connectivity 6, from 1,600 rows in seven
    workgroups whose waves hold one key each -- the in-wave combination and several workgroups adding to one table entry.  A
    third part, one row of 40 nodes, lies on the second slab."""
    dims = (3, FACE, FACE)
    label_of = {}
    for x in (0, 1):
        g = _box_nodes(dims, 0, (x, 1, 0, FACE, 0, FACE))
        for i in g:
            label_of[i] = g[0]
    g = _box_nodes(dims, 0, (2, 1, 17, 1, 0, FACE))
    for i in g:
        label_of[i] = g[0]
    return _finish(dims, 1, label_of, 10, seed)


def field_twists(scene, device="cpu", **override):
    """A ``FieldTwists`` holding the scene's part list and twists (the fields the joints read; the rest zeros)."""
    import torch
    from neural_jacobian_field_amd.field_volume import FieldTwists
    s = dict(scene)
    s.update(override)
    k, a = s["parts"].shape[0], s["omega"].shape[1]
    count = k if s["parts_count"] is None else s["parts_count"]
    t = lambda v, dtype: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).to(device)   # noqa: E731
    f64, i32 = torch.float64, torch.int32
    return FieldTwists(labels=t(s["parts"], i32), count=torch.tensor([count], dtype=i32, device=device),
                       nodes=t(s["weight"], i32), status=t(s["status"], i32), weight=t(s["weight"], f64),
                       centroid=t(s["centroid"], f64), omega=t(s["omega"], f64), velocity=t(s["velocity"], f64),
                       energy=t(s["energy"], f64), residual=torch.zeros(k, a, dtype=f64, device=device),
                       Q=torch.zeros(k, 6, dtype=f64, device=device), P=torch.zeros(k, a, 3, dtype=f64, device=device),
                       L=torch.zeros(k, a, 3, dtype=f64, device=device), row_residual=torch.zeros(0, device=device))


def field_joints(scene, ref, twists=None):
    """A CPU ``FieldJoints`` from the restatement's result ``ref``."""
    import torch
    from neural_jacobian_field_amd.field_volume import FieldGrid, FieldJoints
    grid = FieldGrid(scene["origin"], scene["step"], scene["dims"])
    parts = torch.from_numpy(np.ascontiguousarray(scene["parts"])) if twists is None else twists.labels
    return FieldJoints(grid=grid, labels=parts, twists=twists, **{f: torch.from_numpy(ref[f].copy()) for f in OUTPUTS})
