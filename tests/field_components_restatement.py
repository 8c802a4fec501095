"""A plain numpy restatement of the connected-component semantics of DESIGN.md section 13, written from that text (not from
the kernels): a breadth-first search over the direction table.

Nodes of a grid ``dims = (nx, ny, nz)`` have the linear index ``n = (ix*ny + iy)*nz + iz`` and, for batch element b, the global
index ``b*N + n``.  Two inside nodes of ONE batch element are adjacent iff they differ by one of the first ``connectivity / 2``
directions of the mesh table, in either sign (no wrap at the grid faces), and -- with keys -- iff their keys are equal too.
``labels`` = the smallest global index of the node's component (-1 outside), ``sizes`` = its node count (0 outside), ``count``
= the number of components."""
from collections import deque

import numpy as np

DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
CONNECTIVITIES = (6, 14)


def offsets(connectivity):
    """The ``connectivity`` neighbour offsets: the first connectivity / 2 directions and their negatives."""
    if connectivity not in CONNECTIVITIES:
        raise ValueError(connectivity)
    half = DIRECTIONS[:connectivity // 2]
    return [d for d in half] + [tuple(-c for c in d) for d in half]


def label(inside, dims, connectivity, keys=None):
    """inside [B, N] bool (keys [B, N] int) -> (labels [B, N] int32, sizes [B, N] int32, count int)."""
    inside = np.asarray(inside, dtype=bool)
    batch, nodes = inside.shape
    nx, ny, nz = dims
    assert nodes == nx * ny * nz
    labels = np.full((batch, nodes), -1, dtype=np.int32)
    sizes = np.zeros((batch, nodes), dtype=np.int32)
    nbrs = offsets(connectivity)
    count = 0
    for b in range(batch):
        ins = inside[b]
        key = None if keys is None else np.asarray(keys)[b]
        seen = np.zeros(nodes, dtype=bool)
        for start in np.flatnonzero(ins):              # ascending: the start of a search is its component's minimum
            if seen[start]:
                continue
            seen[start] = True
            queue, members = deque([int(start)]), []
            while queue:
                n = queue.popleft()
                members.append(n)
                ix, r = divmod(n, ny * nz)
                iy, iz = divmod(r, nz)
                for dx, dy, dz in nbrs:
                    jx, jy, jz = ix + dx, iy + dy, iz + dz
                    if not (0 <= jx < nx and 0 <= jy < ny and 0 <= jz < nz):
                        continue
                    m = (jx * ny + jy) * nz + jz
                    if ins[m] and not seen[m] and (key is None or key[m] == key[n]):
                        seen[m] = True
                        queue.append(m)
            members = np.asarray(members)
            assert members.min() == start
            labels[b, members] = b * nodes + start
            sizes[b, members] = members.size
            count += 1
    return labels, sizes, count


def keep(labels, sizes, min_nodes=1, largest_only=False):
    """[B, N] bool: nodes of the components of at least ``min_nodes`` nodes; ``largest_only``: per batch element only the
    component of maximal size, ties to the smallest label."""
    out = sizes >= min_nodes
    if largest_only:
        for b in range(labels.shape[0]):
            if sizes[b].max() == 0:
                continue
            first = labels[b][sizes[b] == sizes[b].max()].min()
            out[b] &= labels[b] == first
    return out


def structure(connectivity):
    """The 3x3x3 structuring element of ``scipy.ndimage.label`` for the same adjacency."""
    s = np.zeros((3, 3, 3), dtype=bool)
    s[1, 1, 1] = True
    for dx, dy, dz in offsets(connectivity):
        s[1 + dx, 1 + dy, 1 + dz] = True
    return s
