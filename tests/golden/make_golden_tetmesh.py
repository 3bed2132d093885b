"""Generate tests/golden/tetmesh.npz from the reference's own marching
tetrahedra (utils/tetmesh.py:51-190), run on the CPU.

Run in the build container (where /root/reference exists and scipy is
installed):
    python tests/golden/make_golden_tetmesh.py
Only the DATA file written next to this script is committed: inputs (the
tets included, so no test needs scipy or the reference) and the reference's
`merged_verts_ids` [E,2] and `faces` [F,3].

Three groups of cases:
  all_*      all 16 sign cases x all 24 vertex orders of one tet, on disjoint
             vertex sets (384 tets, 1536 vertices): pins the winding of every
             triangle and the diagonal of every two-triangle case.
  del_*      scipy.spatial.Delaunay of 3000 uniform points in [-1,1]^3
             (seed 0), sdf = |p| - 0.6 with every 97th sdf exactly 0 and every
             53rd vertex invalid; tets stored as int32.
  scene_*    the tetra points (gsr_scene.tetra_points, CPU) of the
             120-Gaussian scene SCENE_KW with the reference's per-point scale
             (scene/gaussian_model.py:516-518, restated in numpy), their
             Delaunay cells, sdf = |p - centroid| - median distance, every
             31st vertex invalid.
"""
from __future__ import annotations

import importlib.util
import itertools
import math
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, os.path.join(ROOT, "geometry-grounded-gaussian-splatting_amd"))

# the scene of the `scene_*` group and of the driver tests (tests/test_gpu_tetmesh.py)
SCENE_KW = dict(P=120, aspect=64 / 96, z_range=(5.0, 7.0), log_scale_mean=math.log(0.25), opacity_std=2.5)


def _reference():
    spec = importlib.util.spec_from_file_location("ref_tetmesh", os.path.join(REF, "utils", "tetmesh.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _run(ref, pts, tets, sdf, valid):
    V = sdf.shape[0]
    _, _, faces, ids = ref.marching_tetrahedra(
        torch.from_numpy(pts)[None], torch.from_numpy(tets).long(), torch.from_numpy(sdf)[None],
        torch.zeros(1, V, 1), torch.from_numpy(valid)[None])
    return ids[0].numpy().astype(np.int64), faces[0].numpy().astype(np.int64)


def main():
    from scipy.spatial import Delaunay

    import gsr_scene as S

    ref = _reference()
    out = {}

    # ---- all cases x all vertex orders ----
    tets, sdf = [], []
    for case in range(16):
        for perm in itertools.permutations(range(4)):
            base = 4 * len(tets)
            tets.append([base + p for p in perm])
            sdf += [1.0 if (case >> perm.index(k)) & 1 else -1.0 for k in range(4)]  # tet slot i positive iff bit i
    tets = np.asarray(tets, np.int64)
    sdf = np.asarray(sdf, np.float32)
    # the case index is over tet slots: slot i holds vertex base + perm[i]
    for t, row in enumerate(tets):
        assert sum(int(sdf[v] > 0) << i for i, v in enumerate(row)) == t // 24
    pts = np.random.default_rng(1).uniform(-1, 1, size=(sdf.size, 3)).astype(np.float32)
    valid = np.ones(sdf.size, bool)
    ids, faces = _run(ref, pts, tets, sdf, valid)
    out.update(all_tets=tets.astype(np.int32), all_sdf=sdf, all_valid=valid, all_ids=ids.astype(np.int32),
               all_faces=faces.astype(np.int32))

    # ---- Delaunay of uniform points ----
    pts = np.random.default_rng(0).uniform(-1, 1, size=(3000, 3)).astype(np.float32)
    tets = Delaunay(pts.astype(np.float64)).simplices.astype(np.int32)
    sdf = (np.linalg.norm(pts.astype(np.float64), axis=1) - 0.6).astype(np.float32)
    sdf[::97] = 0.0
    valid = np.ones(3000, bool)
    valid[::53] = False
    ids, faces = _run(ref, pts, tets, sdf, valid)
    print("delaunay: T", tets.shape[0], "E", ids.shape[0], "F", faces.shape[0])
    out.update(del_pts=pts, del_tets=tets, del_sdf=sdf, del_valid=valid, del_ids=ids.astype(np.int32),
               del_faces=faces.astype(np.int32))

    # ---- tetra points of a small scene ----
    inp = S.activated_inputs(S.make_gaussians(**SCENE_KW))
    pts = S.tetra_points(inp).numpy().astype(np.float32)
    smax = inp["scales"].numpy().max(axis=1, keepdims=True) * np.float32(3.0)
    scale = np.concatenate([np.repeat(smax, 14, axis=1).reshape(-1, 1), smax], 0).astype(np.float32)
    tets = Delaunay(pts.astype(np.float64)).simplices.astype(np.int32)
    d = np.linalg.norm(pts.astype(np.float64) - pts.astype(np.float64).mean(0), axis=1)
    sdf = (d - np.median(d)).astype(np.float32)
    valid = np.ones(pts.shape[0], bool)
    valid[::31] = False
    ids, faces = _run(ref, pts, tets, sdf, valid)
    print("scene: V", pts.shape[0], "T", tets.shape[0], "E", ids.shape[0], "F", faces.shape[0])
    out.update(scene_pts=pts, scene_scale=scale, scene_tets=tets, scene_sdf=sdf, scene_valid=valid,
               scene_ids=ids.astype(np.int32), scene_faces=faces.astype(np.int32))

    path = os.path.join(OUT, "tetmesh.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
