"""Generate tests/golden/dtueval.npz from the reference's own DTU evaluation:
dtu_eval/eval.py --mode mesh, run unmodified on the CPU through runpy, and
best_fit_transform of evaluate_dtu_mesh.py.

Run in the build container (where /root/reference exists and scipy, sklearn
and tqdm are installed):
    python tests/golden/make_golden_dtueval.py
Only the DATA file written next to this script is committed: the inputs, the
recorded shuffle, and what the reference computed from them.

How the reference is run: `open3d` (not installed) is a stub whose readers
return the arrays this script wrote; ObsMask*.mat and Plane*.mat are written
with scipy.io.savemat into a temporary directory; np.random.default_rng is
replaced by a seeded generator whose shuffle records its permutation (and the
un-shuffled cloud).  evaluate_dtu_mesh.py is loaded with cv2, trimesh, skimage,
arguments, gaussian_renderer and scene stubbed: only best_fit_transform and
the scale lines (158-163, restated below) are used.

The scene: two copies, 0.11 apart, of a 13 x 13 bumpy height field at 0.9 x 0.7
spacing (many pairs of samples from different triangles within the 0.2
radius), two index-degenerate triangles, 6000 scanner points scattered around
the field (float32-representable), 400 of them lifted beyond max_dist, an
80 %-filled ObsMask at Res 0.5, plane z > -1.

The assertions at the end are what lets the tests compare integers exactly.
"""
from __future__ import annotations

import os
import runpy
import sys
import tempfile
import types

import numpy as np
import scipy.io
from scipy.spatial import cKDTree

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import dtueval_ref as R  # noqa: E402

DENSITY, MAX_DIST, SCAN = 0.2, 20.0, 1


def scene(seed=0):
    rng = np.random.default_rng(seed)
    # 0.9 x 0.7 cells, every triangle listed from its right-angle corner: l1 / thr is near 4.5 and
    # l2 / thr near 3.5, so n1 = 4 and n2 = 3, and (i + .5) / n1 + (j + .5) / n2 = 1 has no solution when one
    # of n1, n2 is even and the other odd ((2i + 1) n2 + (2j + 1) n1 is then odd, 2 n1 n2 is not)
    n, sx, sy = 13, 0.9, 0.7
    gx, gy = np.meshgrid(np.arange(n) * sx, np.arange(n) * sy, indexing="ij")
    gz = 0.25 * np.sin(0.7 * gx) * np.cos(0.5 * gy) + 0.04 * rng.standard_normal(gx.shape)
    sheet = np.stack([gx, gy, gz], -1).reshape(-1, 3)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    tris = np.concatenate([np.stack([a, b, c], 1), np.stack([d, c, b], 1)])
    vertices = np.concatenate([sheet, sheet + np.array([0.013, 0.021, 0.11])]).astype(np.float32)
    faces = np.concatenate([tris, tris + n * n, [[3, 3, 7], [5, 9, 5]]]).astype(np.int32)
    stl_xy = rng.uniform([-1.0, -1.0], [12.0, 9.5], size=(6000, 2))
    stl_z = 0.25 * np.sin(0.7 * stl_xy[:, 0]) * np.cos(0.5 * stl_xy[:, 1]) + 0.3 * rng.standard_normal(6000)
    stl = np.concatenate([stl_xy, stl_z[:, None]], 1)
    stl[:400, 2] += 35.0
    stl[400:600, 2] -= 2.5  # below the plane
    stl = stl.astype(np.float32)
    bb = np.array([[-2.0, -2.0, -3.0], [13.0, 13.0, 4.0]])
    res = 0.5
    shape = np.floor((bb[1] - bb[0]) / res).astype(int) + 1
    obs = (rng.uniform(size=tuple(shape)) < 0.8).astype(np.uint8)
    plane = np.array([0.0, 0.0, 1.0, 1.0])
    cams = rng.standard_normal((64, 3)) * 2.0
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    gt = 37.0 * cams @ q.T + np.array([10.0, -20.0, 600.0]) + 1e-3 * rng.standard_normal((64, 3))
    return dict(vertices=vertices, faces=faces, stl=stl, bb=bb, res=res, obs_mask=obs, plane=plane, cam_centers=cams,
                gt_centers=gt)


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def run_reference(s, tmp):
    class _Geom:
        pass

    def read_triangle_mesh(path):
        z, g = np.load(path), _Geom()
        g.vertices, g.triangles = z["vertices"].astype(np.float64), z["triangles"]
        return g

    def read_point_cloud(path):
        g = _Geom()
        g.points = np.load(path)["points"].astype(np.float64)
        return g

    stub("open3d", io=types.SimpleNamespace(read_triangle_mesh=read_triangle_mesh, read_point_cloud=read_point_cloud,
                                            write_point_cloud=lambda *a, **k: True),
         geometry=types.SimpleNamespace(PointCloud=_Geom), utility=types.SimpleNamespace(Vector3dVector=np.asarray))
    os.makedirs(os.path.join(tmp, "ObsMask"))
    os.makedirs(os.path.join(tmp, "Points", "stl"))
    mesh = os.path.join(tmp, "mesh.ply")
    with open(mesh, "wb") as fh:
        np.savez(fh, vertices=s["vertices"], triangles=s["faces"])
    with open(os.path.join(tmp, "Points", "stl", f"stl{SCAN:03}_total.ply"), "wb") as fh:
        np.savez(fh, points=s["stl"])
    scipy.io.savemat(os.path.join(tmp, "ObsMask", f"ObsMask{SCAN}_10.mat"),
                     {"ObsMask": s["obs_mask"], "BB": s["bb"], "Res": np.array([[s["res"]]])})
    scipy.io.savemat(os.path.join(tmp, "ObsMask", f"Plane{SCAN}.mat"), {"P": s["plane"].reshape(4, 1)})

    rec = {}
    real_rng = np.random.default_rng

    class _Shuffle:
        def shuffle(self, arr, axis=0):
            rec["data_pcd"] = arr.copy()
            rec["perm"] = real_rng(12345).permutation(arr.shape[0])
            arr[:] = arr[rec["perm"]]

    argv = sys.argv
    sys.argv = ["eval.py", "--data", mesh, "--scan", str(SCAN), "--mode", "mesh", "--dataset_dir", tmp,
                "--vis_out_dir", tmp, "--downsample_density", str(DENSITY), "--max_dist", str(MAX_DIST)]
    import sklearn.neighbors  # noqa: F401  (its own imports draw from default_rng: before the patch)

    # eval.py:81 is the one call without a seed
    np.random.default_rng = lambda *a, **k: real_rng(*a, **k) if (a or k) else _Shuffle()
    try:
        g = runpy.run_path(os.path.join(REF, "dtu_eval", "eval.py"), run_name="__main__")
    finally:
        np.random.default_rng = real_rng
        sys.argv = argv
    return g, rec


def reference_alignment(cams, gt):
    for name in ("cv2", "trimesh", "skimage", "skimage.morphology", "arguments", "gaussian_renderer", "scene"):
        stub(name, binary_dilation=None, disk=None, ModelParams=None, PipelineParams=None, get_combined_args=None,
             GaussianModel=None, Scene=None)
    m = runpy.run_path(os.path.join(REF, "evaluate_dtu_mesh.py"), run_name="reference_evaluate_dtu_mesh")
    scale_points = np.linalg.norm(cams - cams.mean(axis=0), axis=1).mean()
    scale_gt = np.linalg.norm(gt - gt.mean(axis=0), axis=1).mean()
    _, r, t = m["best_fit_transform"](cams * scale_gt / scale_points, gt)
    return scale_gt / scale_points, r, t


def main():
    s = scene()
    with tempfile.TemporaryDirectory() as tmp:
        g, rec = run_reference(s, tmp)
    pcd, perm, mask = rec["data_pcd"], rec["perm"], g["mask"]
    kept = perm[mask]
    d2s, s2d = g["dist_d2s"][:, 0], g["dist_s2d"][:, 0]
    scale, rot, t = reference_alignment(s["cam_centers"], s["gt_centers"])

    # ---- what lets the integer results be compared exactly
    r2 = DENSITY * DENSITY
    pairs = cKDTree(pcd).query_pairs(DENSITY * 1.01, output_type="ndarray")
    d = pcd[pairs[:, 0]] - pcd[pairs[:, 1]]
    gap = np.abs((d * d).sum(-1) - r2).min() / r2
    assert gap > 1e-9, f"a pair of samples lies on the radius: {gap}"
    lat_gap, ratio_gap = np.inf, np.inf
    for _, n1, n2, q1, q2, *_ in R.triangle_lattices(s["vertices"], s["faces"], DENSITY):
        lat_gap = min(lat_gap, np.abs(R.lattice(n1, n2)[1] - 1).min())
        ratio_gap = min(ratio_gap, abs(q1 - np.round(q1)), abs(q2 - np.round(q2)))
    assert lat_gap > 1e-12, f"a lattice sum lies on 1: {lat_gap}"
    assert ratio_gap > 1e-9, f"l / thr lies on an integer: {ratio_gap}"
    near = np.abs(np.concatenate([d2s, s2d]) - MAX_DIST).min() / MAX_DIST
    assert near > 1e-9, f"a nearest distance lies on max_dist: {near}"
    assert (d2s < MAX_DIST).any() and (s2d < MAX_DIST).any() and (s2d >= MAX_DIST).any()
    assert np.array_equal(s["stl"], s["stl"].astype(np.float32))

    out = dict(vertices=s["vertices"], faces=s["faces"], stl=s["stl"], obs_mask=s["obs_mask"], bb=s["bb"],
               res=np.float64(s["res"]), plane=s["plane"], density=np.float64(DENSITY), max_dist=np.float64(MAX_DIST),
               perm=perm.astype(np.int32), data_pcd=pcd, kept_index=kept.astype(np.int32),
               n_in=np.int64(g["data_in"].shape[0]), n_in_obs=np.int64(g["data_in_obs"].shape[0]),
               n_stl_above=np.int64(g["stl_above"].shape[0]), dist_d2s=d2s, dist_s2d=s2d,
               mean_d2s=np.float64(g["mean_d2s"]), mean_s2d=np.float64(g["mean_s2d"]),
               overall=np.float64(g["over_all"]), cam_centers=s["cam_centers"], gt_centers=s["gt_centers"],
               align_scale=np.float64(scale), align_R=rot, align_t=t)
    path = os.path.join(OUT, "dtueval.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes; sampled {pcd.shape[0]}, kept {kept.shape[0]}, "
          f"in {out['n_in']}, in_obs {out['n_in_obs']}, stl above {out['n_stl_above']}, "
          f"d2s < max {(d2s < MAX_DIST).mean():.3f}, s2d < max {(s2d < MAX_DIST).mean():.3f}, "
          f"means {out['mean_d2s']:.6f} {out['mean_s2d']:.6f} {out['overall']:.6f}; "
          f"gaps: radius {gap:.2e}, lattice {lat_gap:.2e}, l/thr {ratio_gap:.2e}, max_dist {near:.2e}")
    assert os.path.getsize(path) < 400_000


if __name__ == "__main__":
    main()
