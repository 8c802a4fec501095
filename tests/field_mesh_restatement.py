"""Plain numpy restatement of the isosurface semantics of ``field_volume.mesh_from_values``, written
from the specification and not from the kernels, plus the surface checks the CPU and GPU tests share.  Not a test module.

Nodes: ``(ix, iy, iz)`` of an ``nx x ny x nz`` grid has linear index ``(ix*ny + iy)*nz + iz``, global index ``b*N + linear`` and
the coordinate ``fma(i_c, step[c], origin[c])`` in fp32.  ``inside(g) = values[g] >= threshold`` (NaN: outside).  Cells:
``(nx-1)(ny-1)(nz-1)`` per batch element, local index ``(ix*(ny-1) + iy)*(nz-1) + iz``.  Each cell is cut into the six Kuhn
tetrahedra -- axis orders xyz, xzy, yxz, yzx, zxy, zyx; corners ``c0 = 0, c1 = e_a, c2 = e_a + e_b, c3 = (1, 1, 1)``.
"""
import numpy as np

DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
AXIS_ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def fma32(a, b, c):
    """Correctly rounded fp32 ``fma(a, b, c)`` of fp32 arrays.  The product of two fp32 is exact in float64; its sum with c is
    rounded to float64 TO ODD (TwoSum gives the exact residual), so the second rounding to fp32 cannot double-round."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    with np.errstate(invalid="ignore"):
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = np.isfinite(s) & (err != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def node_coordinates(origin, step, index):
    """fp32 coordinates ``[..., 3]`` of integer node indices ``[..., 3]``."""
    index = np.asarray(index)
    return np.stack([fma32(index[..., c].astype(np.float32), np.float32(step[c]), np.float32(origin[c])) for c in range(3)], -1)


def _corner_lists():
    """Per tetrahedron: the four corner offsets (tuples of 0/1) in local order c0..c3."""
    out = []
    for a, b, _ in AXIS_ORDERS:
        c1 = [0, 0, 0]
        c1[a] = 1
        c2 = list(c1)
        c2[b] = 1
        out.append(((0, 0, 0), tuple(c1), tuple(c2), (1, 1, 1)))
    return out


def _case_triangles(corners, inside):
    """Triangles of one tetrahedron case as lists of three edges, an edge being a pair of local corners (low, high).
    The winding is decided here, once per (tetrahedron, case), in exact integer arithmetic on the unit-cube corners."""
    ins = [c for c in range(4) if inside[c]]
    outs = [c for c in range(4) if not inside[c]]
    if len(ins) in (0, 4):
        return []
    if len(ins) in (1, 3):
        lone = ins[0] if len(ins) == 1 else outs[0]
        j, k, l = [c for c in range(4) if c != lone]
        tris = [[(lone, j), (lone, k), (lone, l)]]
    else:
        (i, j), (k, l) = ins, outs
        tris = [[(i, k), (i, l), (j, l)], [(i, k), (j, l), (j, k)]]
    pts = np.array(corners, dtype=np.int64)
    outward = len(ins) * pts[outs].sum(0) - len(outs) * pts[ins].sum(0)      # centroid(outside) - centroid(inside), scaled
    result = []
    for tri in tris:
        mid = [pts[u] + pts[v] for u, v in tri]                               # twice the edge mid-points
        normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
        s = int(normal @ outward)
        assert s != 0
        tri = [tuple(sorted(e)) for e in tri]
        result.append(tri if s > 0 else [tri[0], tri[2], tri[1]])
    return result


def mesh(origin, step, dims, values, threshold, valid=None):
    """-> dict(vertices [V,3] f32, vertex_node [V] i32, vertex_edge [V] u8, vertex_t [V] f32, triangles [T,3] i32,
    triangle_cell [T] i32).  ``values`` [B, N] fp32; ``valid`` [B, N] or None."""
    nx, ny, nz = dims
    values = np.asarray(values, dtype=np.float32)
    batch = values.shape[0]
    n = nx * ny * nz
    assert values.shape == (batch, n)
    thr = np.float32(threshold)
    v = values.reshape(batch, nx, ny, nz)
    inside = v >= thr
    ok = np.ones_like(inside) if valid is None else (np.asarray(valid).reshape(batch, nx, ny, nz) != 0)

    # ---- vertices: ascending (owner, k)
    cross = np.zeros((batch, nx, ny, nz, 7), dtype=bool)
    for k, (dx, dy, dz) in enumerate(DIRECTIONS):
        lo = (slice(None), slice(0, nx - dx), slice(0, ny - dy), slice(0, nz - dz))
        hi = (slice(None), slice(dx, nx), slice(dy, ny), slice(dz, nz))
        cross[lo + (k,)] = ok[lo] & ok[hi] & (inside[lo] != inside[hi])
    flat = cross.reshape(batch * n, 7)
    owner, edge = np.nonzero(flat)                                   # row-major: ascending (owner, k)
    count = owner.shape[0]
    rank = np.full((batch * n, 7), -1, dtype=np.int64)
    rank[owner, edge] = np.arange(count)
    delta = np.array(DIRECTIONS, dtype=np.int64)[edge]
    local = owner % n
    i0 = np.stack([local // (ny * nz), (local // nz) % ny, local % nz], -1)
    other = owner + delta[:, 0] * ny * nz + delta[:, 1] * nz + delta[:, 2]
    v0, v1 = values.reshape(-1)[owner], values.reshape(-1)[other]
    with np.errstate(all="ignore"):
        t = (thr - v0) / (v1 - v0)                                   # fp32, IEEE
    t = np.where(np.isfinite(t), t, np.float32(0.5))
    t = np.where(t > 0, t, np.float32(0.0))
    t = np.where(t < 1, t, np.float32(1.0)).astype(np.float32)
    x0 = node_coordinates(origin, step, i0)
    x1 = node_coordinates(origin, step, i0 + delta)
    with np.errstate(all="ignore"):
        vertices = fma32(t[:, None], x1 - x0, x0)

    # ---- triangles: cells ascending, tetrahedra in order
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    cells = cx * cy * cz
    bi, ix, iy, iz = np.meshgrid(np.arange(batch), np.arange(cx), np.arange(cy), np.arange(cz), indexing="ij")
    base = (bi * n + (ix * ny + iy) * nz + iz).reshape(-1)          # owning node of corner (0,0,0), by global cell index
    gflat_in, gflat_ok = inside.reshape(-1), ok.reshape(-1)

    def node_of(corner):
        return base + corner[0] * ny * nz + corner[1] * nz + corner[2]

    slots = np.full((batch * cells, 6, 2, 3), -1, dtype=np.int64)
    for q, corners in enumerate(_corner_lists()):
        nodes = [node_of(c) for c in corners]
        all_ok = gflat_ok[nodes[0]] & gflat_ok[nodes[1]] & gflat_ok[nodes[2]] & gflat_ok[nodes[3]]
        code = sum(gflat_in[nodes[c]].astype(np.int64) << c for c in range(4))
        for case in range(1, 15):
            sel = np.nonzero(all_ok & (code == case))[0]
            if sel.size == 0:
                continue
            pattern = [(case >> c) & 1 for c in range(4)]
            for slot, tri in enumerate(_case_triangles(corners, pattern)):
                for e, (lo, hi) in enumerate(tri):
                    d = tuple(h - l for l, h in zip(corners[lo], corners[hi]))
                    r = rank[nodes[lo][sel], DIRECTIONS.index(d)]
                    assert (r >= 0).all(), "a crossing edge of a valid tetrahedron has no vertex"
                    slots[sel, q, slot, e] = r
    emitted = slots[..., 0] >= 0                                     # [cells, 6, 2], flattened in output order
    triangles = slots[emitted]
    triangle_cell = np.broadcast_to(np.arange(batch * cells)[:, None, None], emitted.shape)[emitted]
    return dict(vertices=vertices, vertex_node=owner.astype(np.int32), vertex_edge=edge.astype(np.uint8), vertex_t=t,
                triangles=triangles.astype(np.int32).reshape(-1, 3), triangle_cell=triangle_cell.astype(np.int32))


# ---- surface checks (independent of how the mesh was made) ----------------------------------------------------------------
def directed_edge_counts(triangles):
    """dict (u, v) -> number of triangles that traverse the directed edge u -> v."""
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    pairs = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    uniq, counts = np.unique(pairs, axis=0, return_counts=True)
    return {(int(u), int(v)): int(c) for (u, v), c in zip(uniq, counts)}


def boundary_edges(triangles):
    """Directed edges whose reverse is not traversed."""
    d = directed_edge_counts(triangles)
    return [e for e in d if (e[1], e[0]) not in d]


def euler_characteristic(triangles):
    """V - E + F over the vertices the triangles reference."""
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    d = directed_edge_counts(tri)
    undirected = {(min(u, v), max(u, v)) for u, v in d}
    return np.unique(tri).size - len(undirected) + tri.shape[0]


def signed_volume(vertices, triangles):
    p = np.asarray(vertices, dtype=np.float64)[np.asarray(triangles, dtype=np.int64).reshape(-1, 3)]
    return float(np.einsum("ti,ti->t", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def assert_closed_oriented(vertices, triangles, euler):
    """Every undirected edge is used by exactly two triangles, once per direction; V - E + F == euler; positive volume."""
    tri = np.asarray(triangles).reshape(-1, 3)
    assert tri.shape[0] > 0
    d = directed_edge_counts(tri)
    assert all(c == 1 for c in d.values()), "a directed edge is traversed twice"
    assert all((v, u) in d for u, v in d), "an edge is used by one triangle only"
    assert np.unique(tri).size == np.asarray(vertices).shape[0], "unreferenced vertices"
    assert euler_characteristic(tri) == euler, euler_characteristic(tri)
    assert signed_volume(vertices, tri) > 0


def ulp_distance(a, b):
    """Largest |a - b| in units of the fp32 ulp of the larger operand (0 where equal)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if a.size == 0:
        return 0.0
    scale = np.maximum(np.abs(a), np.abs(b))
    ulp = np.spacing(np.where(scale > 0, scale, np.float32(1.0)).astype(np.float32)).astype(np.float64)
    return float((np.abs(a.astype(np.float64) - b.astype(np.float64)) / ulp).max())


# ---- analytic fields -------------------------------------------------------------------------------------------------------
def grid_points(origin, step, dims):
    idx = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    return node_coordinates(origin, step, idx)


def sphere_field(points, centre, radius):
    return (radius - np.linalg.norm(points.astype(np.float64) - np.asarray(centre), axis=-1)).astype(np.float32)


def torus_field(points, centre, major, minor):
    p = points.astype(np.float64) - np.asarray(centre)
    ring = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - major
    return (minor - np.sqrt(ring ** 2 + p[:, 2] ** 2)).astype(np.float32)


def smooth_random_field(points, seed, waves=4):
    """A sum of a few random sinusoids: smooth, many components, crosses zero inside the grid and at its border."""
    rng = np.random.default_rng(seed)
    p = points.astype(np.float64)
    out = np.zeros(p.shape[0])
    for _ in range(waves):
        out += rng.normal() * np.sin(p @ rng.normal(size=3) * 2.5 + rng.uniform(0, 6.28))
    return out.astype(np.float32)
