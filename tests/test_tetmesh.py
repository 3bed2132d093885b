"""CPU tests of the tetrahedral mesh extraction (no GPU needed).

* tests/tetmesh_ref.py, the plain-torch restatement the GPU tests use as
  their yardstick beyond the fixture's sizes, reproduces every case of
  tests/golden/tetmesh.npz (the reference's utils/tetmesh.py run on the CPU,
  tests/golden/make_golden_tetmesh.py): edge ids equal, faces equal as
  multisets after rotating every row so its smallest index comes first —
  winding and the two-triangle cases' diagonal must match.
* gsr_mesh refuses CPU tensors and wrong shapes / dtypes (no CPU fallback),
  write_ply round-trips, gsr_scene.tetra_points_scale equals the fixture's.
"""
from __future__ import annotations

import math
import os

import numpy as np
import pytest
import torch

import tetmesh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "tetmesh.npz"))
GROUPS = ("all", "del", "scene")
# the scene of the fixture's third group (tests/golden/make_golden_tetmesh.py)
SCENE_KW = dict(P=120, aspect=64 / 96, z_range=(5.0, 7.0), log_scale_mean=math.log(0.25), opacity_std=2.5)


def group(name):
    g = {k[len(name) + 1:]: GOLD[k] for k in GOLD.files if k.startswith(name + "_")}
    return dict(g, tets=torch.from_numpy(g["tets"]), sdf=torch.from_numpy(g["sdf"]),
                valid=torch.from_numpy(g["valid"]), ids=torch.from_numpy(g["ids"]).long(),
                faces=torch.from_numpy(g["faces"]).long())


@pytest.mark.parametrize("name", GROUPS)
def test_restatement_reproduces_reference(name):
    g = group(name)
    ids, faces = R.marching_tetrahedra_ref(g["tets"], g["sdf"], g["valid"])
    assert ids.dtype == torch.int64 and faces.dtype == torch.int64
    assert torch.equal(ids, g["ids"])
    assert (ids[:, 0] < ids[:, 1]).all()
    assert torch.equal(R.canonical_faces(faces), R.canonical_faces(g["faces"]))
    if name == "del":
        assert g["tets"].dtype == torch.int32
        assert (g["tets"].shape[0], ids.shape[0], faces.shape[0]) == (19650, 1476, 2735)
    if name == "all":  # 24 orders of cases 1..14: 8 one-triangle and 6 two-triangle cases
        assert faces.shape[0] == 24 * (8 + 2 * 6)


def test_canonical_faces_only_forgives_rotation():
    f = torch.tensor([[5, 2, 9], [1, 7, 3]])
    assert torch.equal(R.canonical_faces(f), R.canonical_faces(torch.tensor([[7, 3, 1], [9, 5, 2]])))
    assert not torch.equal(R.canonical_faces(f), R.canonical_faces(torch.tensor([[5, 9, 2], [1, 7, 3]])))


def test_marching_tetrahedra_refuses_cpu_and_bad_inputs():
    import gsr_mesh as M

    V, T = 8, 3
    args = dict(vertices=torch.zeros(1, V, 3), tets=torch.zeros(T, 4, dtype=torch.int64), sdf=torch.zeros(1, V),
                scales=torch.zeros(1, V, 1), valids=torch.ones(1, V, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        M.marching_tetrahedra(**args)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        M.marching_tetrahedra_ids(args["tets"], args["sdf"][0], args["valids"][0])
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        M.alpha_cull_sdf(torch.zeros(4, 3), [], None, None, 0.0)


def _fake_device(t):
    """A CPU tensor that claims to be a device tensor, to reach the shape / dtype checks without a GPU."""

    class _T(torch.Tensor):
        @property
        def is_cuda(self):
            return True

    return t.as_subclass(_T)


@pytest.mark.parametrize("bad", ["tets_shape", "tets_dtype", "sdf_dtype", "sdf_shape", "valid_dtype", "scales_shape",
                                 "vertices_shape", "valid_len"])
def test_marching_tetrahedra_shape_and_dtype_errors(bad):
    import gsr_mesh as M

    V, T = 8, 3
    a = dict(vertices=torch.zeros(1, V, 3), tets=torch.zeros(T, 4, dtype=torch.int64), sdf=torch.zeros(1, V),
             scales=torch.zeros(1, V, 1), valids=torch.ones(1, V, dtype=torch.bool))
    if bad == "tets_shape":
        a["tets"] = torch.zeros(T, 3, dtype=torch.int64)
    elif bad == "tets_dtype":
        a["tets"] = torch.zeros(T, 4, dtype=torch.int16)
    elif bad == "sdf_dtype":
        a["sdf"] = torch.zeros(1, V, dtype=torch.float64)
    elif bad == "sdf_shape":
        a["sdf"] = torch.zeros(V)
    elif bad == "valid_dtype":
        a["valids"] = torch.ones(1, V)
    elif bad == "scales_shape":
        a["scales"] = torch.zeros(1, V)
    elif bad == "vertices_shape":
        a["vertices"] = torch.zeros(1, V, 2)
    elif bad == "valid_len":
        a["valids"] = torch.ones(1, V + 1, dtype=torch.bool)
    a = {k: _fake_device(v) for k, v in a.items()}
    with pytest.raises(RuntimeError, match="marching_tetrahedra: `"):
        M.marching_tetrahedra(**a)


def _read_ply(path):
    with open(path, "rb") as fh:
        assert fh.readline() == b"ply\n"
        assert fh.readline() == b"format binary_little_endian 1.0\n"
        counts, props = {}, {}
        while True:
            line = fh.readline().decode("ascii").split()
            if line[0] == "end_header":
                break
            if line[0] == "element":
                cur = line[1]
                counts[cur] = int(line[2])
                props[cur] = []
            elif line[0] == "property":
                props[cur].append(line[1:])
        assert props["vertex"] == [["float", "x"], ["float", "y"], ["float", "z"]]
        assert props["face"] == [["list", "uchar", "int", "vertex_indices"]]
        v = np.frombuffer(fh.read(12 * counts["vertex"]), "<f4").reshape(-1, 3)
        f = np.frombuffer(fh.read(13 * counts["face"]), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
        assert fh.read() == b""
    assert (f["n"] == 3).all()
    return v, f["v"]


def test_write_ply_round_trip(tmp_path):
    import gsr_mesh as M

    g = torch.Generator().manual_seed(0)
    v = torch.randn(37, 3, generator=g)
    f = torch.randint(0, 37, (61, 3), generator=g)
    M.write_ply(str(tmp_path / "m.ply"), v, f)
    rv, rf = _read_ply(str(tmp_path / "m.ply"))
    assert np.array_equal(rv, v.numpy()) and np.array_equal(rf, f.numpy())
    M.write_ply(str(tmp_path / "e.ply"), torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64))
    rv, rf = _read_ply(str(tmp_path / "e.ply"))
    assert rv.shape == (0, 3) and rf.shape == (0, 3)


def test_tetra_points_scale_matches_fixture():
    import gsr_scene as S

    inp = S.activated_inputs(S.make_gaussians(**SCENE_KW))
    scale = S.tetra_points_scale(inp)
    pts = S.tetra_points(inp)
    assert scale.shape == (15 * SCENE_KW["P"], 1) and pts.shape[0] == scale.shape[0]
    assert np.array_equal(scale.numpy(), GOLD["scene_scale"])
    assert np.allclose(pts.numpy(), GOLD["scene_pts"], rtol=0, atol=1e-6)
    # the 14 offsets of a Gaussian share its scale; its centre comes after every offset
    assert np.array_equal(scale[:14].numpy(), np.repeat(scale[14 * SCENE_KW["P"]:][:1].numpy(), 14, 0))


def test_grid_sphere_is_a_closed_oriented_surface():
    """The structured grid the GPU tests use, through the restatement: a sphere
    inside the grid comes out closed and consistently oriented — a check of
    the triangle table that rests on no recorded output."""
    pts, tets = R.kuhn_grid(8)
    vol = torch.linalg.det(torch.stack([pts[tets[:, i]] - pts[tets[:, 0]] for i in (1, 2, 3)], 1).double())
    assert (vol > 0).all()
    sdf = pts.norm(dim=1) - 0.62
    ids, faces = R.marching_tetrahedra_ref(tets, sdf, torch.ones(sdf.numel(), dtype=torch.bool))
    assert faces.shape[0] > 500 and R.is_closed_oriented(faces)
    assert not R.is_closed_oriented(faces[1:])
    flipped = faces.clone()
    flipped[0] = flipped[0, [0, 2, 1]]
    assert not R.is_closed_oriented(flipped)
