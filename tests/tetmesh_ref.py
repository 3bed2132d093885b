"""Plain-torch restatement of marching tetrahedra, the yardstick of the GPU
tests beyond the sizes of tests/golden/tetmesh.npz (tests/test_tetmesh.py
pins it to that fixture, i.e. to the reference's utils/tetmesh.py).

Semantics: a vertex is positive when sdf > 0 (0 is not).  A tet takes part
when 1-3 of its vertices are positive and all four are valid; its case is
sum(positive[i] << i).  Mesh vertices: the undirected edges (a, b), a < b,
with exactly one positive end that belong to a participating tet, each once,
ascending in (a, b).  Edges of a tet are numbered 01, 02, 03, 12, 13, 23.
Cases 1, 2, 4, 7, 8, 11, 13, 14 give one triangle, the others two; case
15 - c is case c with the winding reversed.  Faces are in tet order.
Works on any device.
"""
from __future__ import annotations

import torch

EDGE_A = (0, 0, 0, 1, 1, 2)
EDGE_B = (1, 2, 3, 2, 3, 3)
# triangles (edge numbers) of the cases with vertex 3 negative
_HALF = {1: [(0, 2, 1)], 2: [(0, 3, 4)], 3: [(1, 3, 4), (1, 4, 2)], 4: [(1, 5, 3)], 5: [(0, 2, 3), (2, 5, 3)],
         6: [(0, 1, 4), (1, 5, 4)], 7: [(2, 5, 4)]}


def triangle_table() -> torch.Tensor:
    """[16, 6] edge numbers of up to two triangles per case, -1 where none."""
    tab = torch.full((16, 6), -1, dtype=torch.long)
    for c, tris in _HALF.items():
        for q, (a, b, d) in enumerate(tris):
            tab[c, 3 * q:3 * q + 3] = torch.tensor([a, b, d])
            tab[15 - c, 3 * q:3 * q + 3] = torch.tensor([a, d, b])
    return tab


@torch.no_grad()
def marching_tetrahedra_ref(tets: torch.Tensor, sdf: torch.Tensor, valid: torch.Tensor):
    """tets [T,4] integer, sdf [V] float, valid [V] bool -> edge_ids [E,2] int64, faces [F,3] int64."""
    dev = tets.device
    V = int(sdf.numel())
    tets = tets.long().reshape(-1, 4)
    pos = sdf > 0
    if tets.shape[0] == 0:
        return torch.zeros(0, 2, dtype=torch.long, device=dev), torch.zeros(0, 3, dtype=torch.long, device=dev)
    p = pos[tets]
    n = p.sum(1)
    part = (n > 0) & (n < 4) & valid.bool()[tets].all(1)
    tt, pp = tets[part], p[part]
    case = (pp.long() * torch.tensor([1, 2, 4, 8], device=dev)).sum(1)
    ea, eb = torch.tensor(EDGE_A, device=dev), torch.tensor(EDGE_B, device=dev)
    a, b = tt[:, ea], tt[:, eb]
    key = torch.minimum(a, b) * V + torch.maximum(a, b)  # [Tp, 6]
    cross = pp[:, ea] != pp[:, eb]
    uniq = torch.unique(key[cross])  # ascending
    edge_ids = torch.stack([uniq // V, uniq % V], 1) if V else torch.zeros(0, 2, dtype=torch.long, device=dev)
    if uniq.numel() == 0:
        return edge_ids.reshape(0, 2), torch.zeros(0, 3, dtype=torch.long, device=dev)
    idx = torch.searchsorted(uniq, key)  # meaningful where `cross`
    tab = triangle_table().to(dev)[case]  # [Tp, 6]
    faces = torch.gather(idx, 1, tab.clamp(min=0)).reshape(-1, 3)
    keep = (tab.reshape(-1, 3) >= 0).all(1)
    return edge_ids, faces[keep]


def canonical_faces(faces) -> torch.Tensor:
    """Rows rotated so the smallest index comes first, then sorted: equal iff
    the two face lists are the same multiset of oriented triangles."""
    f = torch.as_tensor(faces).long().reshape(-1, 3).cpu()
    if f.shape[0] == 0:
        return f
    k = f.argmin(1)
    rot = torch.stack([f.gather(1, ((k + i) % 3)[:, None])[:, 0] for i in range(3)], 1)
    for c in (2, 1, 0):  # lexicographic: stable sorts from the last column to the first
        rot = rot[torch.sort(rot[:, c], stable=True).indices]
    return rot


def kuhn_grid(n: int, lo: float = -1.0, hi: float = 1.0, device="cpu", dtype=torch.int64):
    """A structured grid of n^3 cubic cells over [lo, hi]^3, each split into 6
    tets around its main diagonal (one per order of the three axes), which
    makes the faces of neighbouring cells match; every tet has positive
    volume (det[v1 - v0, v2 - v0, v3 - v0] > 0), so the triangles of a level
    set are consistently oriented: (n + 1)^3 points [V,3] float32 and 6 n^3
    tets [T,4] int64 (or `dtype`), cell-major."""
    m = n + 1
    ax = torch.linspace(lo, hi, m, device=device)
    pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    c = torch.arange(n, device=device, dtype=dtype)
    base = (c[:, None, None] * m * m + c[None, :, None] * m + c[None, None, :]).reshape(-1)
    step = (m * m, m, 1)
    tets = []
    for a, b, d in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        v1, v2 = base + step[a], base + step[a] + step[b]
        if (a, b, d) in ((0, 2, 1), (1, 0, 2), (2, 1, 0)):  # odd orders: swap two vertices to keep the volume positive
            v1, v2 = v2, v1
        tets.append(torch.stack([base, v1, v2, base + step[a] + step[b] + step[d]], 1))
    return pts.float().contiguous(), torch.stack(tets, 1).reshape(-1, 4).contiguous()


def is_closed_oriented(faces) -> bool:
    """Every directed edge of the triangles occurs exactly once and its reverse exactly once."""
    f = torch.as_tensor(faces).long().cpu()
    a = torch.cat([f[:, 0], f[:, 1], f[:, 2]])
    b = torch.cat([f[:, 1], f[:, 2], f[:, 0]])
    n = int(f.max()) + 1
    fwd, rev = a * n + b, b * n + a
    return bool(torch.unique(fwd).numel() == fwd.numel() and torch.equal(torch.sort(fwd).values, torch.sort(rev).values))
