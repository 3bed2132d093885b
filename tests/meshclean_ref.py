"""numpy / scipy restatement of the mesh clean-up, the yardstick of the GPU
tests beyond the meshes whose answer is known by construction
(tests/test_meshclean.py pins it to those).

Semantics (open3d's cluster_connected_triangles and the reference's
post_process_mesh, mesh_extract_tetrahedra.py:18-40): two triangles are
adjacent when they share an undirected edge (min, max) of vertex ids — a
shared vertex alone does not connect, an edge of three or more triangles
connects them all, the edges of index-degenerate triangles count like any
other.  Clusters are numbered in ascending order of their lowest triangle
index.  Area is 0.5 |cross| per triangle, in float64.  The filter drops the
triangles of clusters below the threshold, then the unreferenced vertices,
then the triangles with two equal ids; order and winding are kept.

Also the builders of the constructed meshes (strips, fans, floaters).
"""
from __future__ import annotations

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def cluster_connected_triangles_ref(vertices, faces):
    """vertices [V,3] float or None, faces [F,3] integer -> (triangle_clusters [F] int64,
    cluster_n_triangles [C] int64, cluster_area [C] float64 or None)."""
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    F = f.shape[0]
    if F == 0:
        z = np.zeros(0, np.int64)
        return z, z.copy(), (np.zeros(0, np.float64) if vertices is not None else None)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    tri = np.tile(np.arange(F, dtype=np.int64), 3)
    order = np.lexsort((tri, hi, lo))
    lo, hi, tri = lo[order], hi[order], tri[order]
    same = (lo[1:] == lo[:-1]) & (hi[1:] == hi[:-1])  # chaining a run of equal edges connects all its triangles
    g = coo_matrix((np.ones(int(same.sum()), np.int8), (tri[1:][same], tri[:-1][same])), shape=(F, F))
    n, comp = connected_components(g, directed=False)
    first = np.full(n, F, np.int64)
    np.minimum.at(first, comp, np.arange(F, dtype=np.int64))
    rank = np.empty(n, np.int64)
    rank[np.argsort(first)] = np.arange(n)
    labels = rank[comp]
    counts = np.bincount(labels, minlength=n).astype(np.int64)
    area = None
    if vertices is not None:
        v = np.asarray(vertices, np.float64).reshape(-1, 3)
        cr = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        area = np.bincount(labels, weights=0.5 * np.sqrt((cr * cr).sum(1)), minlength=n)
    return labels, counts, area


def post_process_mesh_ref(vertices, faces, cluster_to_keep=1, min_triangles=50):
    """-> (vertices [V',3] float32, faces [F',3] int64); IndexError for a bad cluster_to_keep, as the reference."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return v[:0], f
    labels, counts, _ = cluster_connected_triangles_ref(None, f)
    if cluster_to_keep < 1:
        raise IndexError(cluster_to_keep)
    n_min = max(int(np.sort(counts)[-cluster_to_keep]), min_triangles)
    f = f[counts[labels] >= n_min]
    used = np.zeros(v.shape[0], bool)
    used[f.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    f = remap[f]
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    return v[used], f.reshape(-1, 3)


# ---- constructed meshes ------------------------------------------------------------------------------------------
def strip(n: int, first_vertex: int = 0) -> np.ndarray:
    """n triangles (i, i + 1, i + 2) over n + 2 vertices, every other one flipped so the winding is consistent:
    triangle i shares the edge (i + 1, i + 2) with triangle i + 1 — one cluster."""
    i = np.arange(n, dtype=np.int64)
    f = np.stack([i, i + 1, i + 2], 1)
    f[1::2] = f[1::2][:, [1, 0, 2]]
    return f + first_vertex


def fan(n: int, centre: int, first_rim: int) -> np.ndarray:
    """n triangles (centre, r_i, r_{i + 1}) around `centre`, rim vertices first_rim .. first_rim + n — one cluster."""
    i = np.arange(n, dtype=np.int64) + first_rim
    return np.stack([np.full(n, centre, np.int64), i, i + 1], 1)


def tetrahedron(first_vertex: int) -> np.ndarray:
    """The 4 outward triangles of a tetrahedron over 4 vertices — one closed cluster."""
    return np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int64) + first_vertex


def concat(parts):
    """Face arrays, each over its own vertices numbered from 0, shifted to follow each other -> (faces, V, spans):
    spans[k] = (first triangle, end triangle) of part k."""
    out, spans, v0, t0 = [], [], 0, 0
    for f in parts:
        out.append(f + v0)
        v0 += int(f.max()) + 1
        spans.append((t0, t0 + f.shape[0]))
        t0 += f.shape[0]
    return np.concatenate(out), v0, spans


def by_first_occurrence(keys: np.ndarray) -> np.ndarray:
    """Arbitrary per-triangle cluster keys -> ids numbered in ascending order of each key's first triangle."""
    _, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    rank = np.empty(first.shape[0], np.int64)
    rank[np.argsort(first)] = np.arange(first.shape[0])
    return rank[inv.reshape(-1)]


def constructed(seed: int = 0, second_51: bool = False):
    """The constructed mesh of the tests, triangle order shuffled by `seed`: strips of 49, 50, 51 and 300
    triangles (and a second one of 51), two fans of 6 around one shared centre vertex (2 clusters), three
    triangles on one common edge (1 cluster), two index-degenerate triangles (a, a, b), (a, a, c) (1 cluster).
    -> dict(vertices [V,3] float32, faces [F,3] int64, name [F] the constructed cluster of every triangle,
    labels [F], counts [C]: the answer by construction)."""
    parts = [("s49", strip(49)), ("s50", strip(50)), ("s51", strip(51)), ("s300", strip(300))]
    if second_51:
        parts.append(("s51b", strip(51)))
    fans = np.concatenate([fan(6, 0, 1), fan(6, 0, 8)])
    parts += [("fans", fans), ("edge3", np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int64)),
              ("degen", np.array([[0, 0, 1], [0, 0, 2]], np.int64))]
    faces, V, spans = concat([f for _, f in parts])
    name = np.empty(faces.shape[0], dtype="U8")
    for (n, _), (a, b) in zip(parts, spans):
        name[a:b] = n
        if n == "fans":
            name[a:a + 6], name[a + 6:b] = "fanA", "fanB"
    rng = np.random.default_rng(seed)
    perm = rng.permutation(faces.shape[0])
    faces, name = faces[perm], name[perm]
    labels = by_first_occurrence(name)
    return dict(vertices=rng.standard_normal((V, 3)).astype(np.float32), faces=faces, name=name, labels=labels,
                counts=np.bincount(labels).astype(np.int64))


def keep_by_name(mesh, names):
    """The filter's answer by construction: the triangles of the named constructed clusters in their order,
    without the index-degenerate ones, over the vertices those clusters use, in their order."""
    v, f = mesh["vertices"], mesh["faces"]
    f = f[np.isin(mesh["name"], list(names))]
    used = np.zeros(v.shape[0], bool)
    used[f.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    return v[used], remap[f].reshape(-1, 3)


# (cluster_to_keep, min_triangles, second 51-strip) -> the constructed clusters that stay
EXPECTED_KEPT = [
    (1, 50, False, ("s300",)),
    (2, 50, False, ("s300", "s51")),
    (2, 50, True, ("s300", "s51", "s51b")),                 # the tie at the threshold keeps both
    (4, 50, False, ("s300", "s51", "s50")),                 # the 4th largest has 49: the floor of 50 drops it
    (4, 1, False, ("s300", "s51", "s50", "s49")),
    (8, 1, False, ("s300", "s51", "s50", "s49", "fanA", "fanB", "edge3", "degen")),  # degenerate: cluster kept, gone
]


def with_floaters(vertices, faces, n: int = 40, seed: int = 0, sizes=(4, 60)):
    """A mesh plus n floaters away from it: closed tetrahedra (4 triangles) and strips of sizes[0]..sizes[1]
    triangles, both ends of the range included.  Half of the floaters' vertices come before the mesh's and
    half after, and the triangle order is shuffled, so removing the floaters renumbers every vertex and
    must give back `vertices` exactly and `faces` as a multiset.  -> (vertices float32, faces int64)."""
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    counts = [sizes[1], sizes[0], sizes[0]] + [int(c) for c in rng.integers(sizes[0], sizes[1] + 1, n - 3)]
    parts = [tetrahedron(0) if (k % 2 == 1 and c >= 4) else strip(c) for k, c in enumerate(counts)]
    front, back = parts[:n // 2], parts[n // 2:]
    ff, vf, _ = concat(front)
    fb, vb, _ = concat(back)

    def positions(count):
        centre = rng.standard_normal((count, 3))
        centre *= 1.6 / np.linalg.norm(centre, axis=1, keepdims=True)
        return (centre + 0.02 * rng.standard_normal((count, 3))).astype(np.float32)

    faces_all = np.concatenate([ff, f + vf, fb + vf + v.shape[0]])
    verts_all = np.concatenate([positions(vf), v, positions(vb)])
    return verts_all, faces_all[rng.permutation(faces_all.shape[0])]
