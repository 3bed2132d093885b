"""GPU tests of marching tetrahedra in HIP (csrc/tetmesh.hip through
gsr_mesh) and of the mesh-extraction driver around it.

Yardsticks: tests/golden/tetmesh.npz (the reference's utils/tetmesh.py on the
CPU) for the fixture's cases; beyond its sizes the plain-torch restatement
tests/tetmesh_ref.py, which tests/test_tetmesh.py pins to that fixture.  No
floating-point arithmetic is involved, so every comparison is exact: edge ids
equal, faces equal as multisets of oriented triangles (rotation of a row is
the only freedom; gsr lists faces in tet order, the reference one-triangle
tets first).  The grid case adds a check that rests on neither: the level set
of a sphere inside the grid is a closed, consistently oriented surface.
"""
from __future__ import annotations

import types

import numpy as np
import pytest
import torch

import gsr_scene as S
import tetmesh_ref as R
from test_tetmesh import SCENE_KW, group

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _mt(tets, sdf, valid):
    import gsr_mesh as M

    return M.marching_tetrahedra_ids(tets.to(DEV), sdf.to(DEV), valid.to(DEV))


def _same(got, ref):
    ids, faces = got
    rids, rfaces = ref
    assert ids.dtype == torch.int64 and faces.dtype == torch.int64
    assert ids.shape == rids.shape and faces.shape == rfaces.shape, (ids.shape, rids.shape, faces.shape, rfaces.shape)
    assert torch.equal(ids.cpu(), rids.cpu())
    assert torch.equal(R.canonical_faces(faces), R.canonical_faces(rfaces))


@pytest.fixture(scope="module")
def grid():
    """24^3 cells x 6 tets = 82 944 tets, a sphere well inside; the restatement's result computed once."""
    pts, tets = R.kuhn_grid(24)
    sdf = (pts - torch.tensor([0.03, -0.02, 0.01])).norm(dim=1) - 0.61
    valid = torch.ones(sdf.numel(), dtype=torch.bool)
    ref = R.marching_tetrahedra_ref(tets, sdf, valid)
    return dict(pts=pts, tets=tets, sdf=sdf, valid=valid, ref=ref)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("name", ["all", "del", "scene"])
def test_fixture_cases(name, dtype):
    import gsr_mesh as M

    g = group(name)
    V = g["sdf"].numel()
    gen = torch.Generator().manual_seed(5)
    verts = torch.from_numpy(g["pts"]) if "pts" in g else torch.randn(V, 3, generator=gen)
    scales = torch.from_numpy(g["scale"]) if "scale" in g else torch.rand(V, 1, generator=gen)
    verts, scales, sdf, valid = verts.to(DEV), scales.to(DEV), g["sdf"].to(DEV), g["valid"].to(DEV)
    tets = g["tets"].to(dtype).to(DEV)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):  # a non-default stream: the call takes the caller's
        out = M.marching_tetrahedra(verts[None], tets, sdf[None], scales[None], valid[None])
    stream.synchronize()
    assert [len(o) for o in out] == [1, 1, 1, 1]
    (ends, ends_sdf), mscales, faces, ids = out[0][0], out[1][0], out[2][0], out[3][0]
    _same((ids, faces), (g["ids"], g["faces"]))
    flat = ids.reshape(-1)
    assert torch.equal(ends, verts[flat].reshape(-1, 2, 3))
    assert torch.equal(ends_sdf, sdf[flat].reshape(-1, 2, 1))
    assert torch.equal(mscales, scales[flat].reshape(-1, 2, 1))
    # exactly one positive end per mesh vertex
    assert bool(((sdf[ids[:, 0]] > 0) != (sdf[ids[:, 1]] > 0)).all())


@pytest.mark.parametrize("T", [0, 1, 255, 256, 257, 70001])
def test_tet_counts_around_block_sizes(grid, T):
    """Slices of the grid's tets (a lane, a wave, a block of 256 lanes, 1024-tet blocks and their ragged ends),
    taken where the sphere passes so that even one tet crosses."""
    first = int(torch.nonzero((grid["sdf"][grid["tets"]] > 0).sum(1) % 4 != 0)[0])
    start = min(first, grid["tets"].shape[0] - T)
    tets = grid["tets"][start:start + T]
    ref = R.marching_tetrahedra_ref(tets, grid["sdf"], grid["valid"])
    assert (ref[1].shape[0] > 0) == (T > 0)
    _same(_mt(tets, grid["sdf"], grid["valid"]), ref)
    _same(_mt(tets.int(), grid["sdf"], grid["valid"].to(torch.uint8)), ref)


def test_nothing_to_extract(grid):
    tets, V = grid["tets"][:5000], grid["sdf"].numel()
    for sdf, valid in ((-torch.ones(V), grid["valid"]),           # no participating tet
                       (torch.ones(V), grid["valid"]),            # all positive
                       (torch.zeros(V), grid["valid"]),           # sdf exactly 0 is not positive
                       (grid["sdf"], torch.zeros(V, dtype=torch.bool))):  # every tet invalid
        ids, faces = _mt(tets, sdf, valid)
        assert ids.shape == (0, 2) and faces.shape == (0, 3)
        assert ids.dtype == torch.int64 and faces.dtype == torch.int64 and ids.device.type == "cuda"
    ids, faces = _mt(torch.zeros(0, 4, dtype=torch.int64), torch.zeros(0), torch.zeros(0, dtype=torch.bool))
    assert ids.shape == (0, 2) and faces.shape == (0, 3)


def test_one_invalid_vertex_removes_its_tets(grid):
    valid = grid["valid"].clone()
    valid[grid["ref"][0][::7, 0]] = False  # ends of crossing edges
    ref = R.marching_tetrahedra_ref(grid["tets"], grid["sdf"], valid)
    assert 0 < ref[1].shape[0] < grid["ref"][1].shape[0]
    _same(_mt(grid["tets"], grid["sdf"], valid), ref)


def test_duplicate_tet_gives_faces_twice_vertices_once():
    tets = torch.tensor([[0, 1, 2, 3], [0, 1, 2, 3]])
    sdf = torch.tensor([1.0, 1.0, -1.0, -1.0])  # case 3: two triangles
    valid = torch.ones(4, dtype=torch.bool)
    ids, faces = _mt(tets, sdf, valid)
    assert ids.cpu().tolist() == [[0, 2], [0, 3], [1, 2], [1, 3]]
    assert faces.shape == (4, 3) and torch.equal(faces[:2], faces[2:])
    _same((ids, faces), R.marching_tetrahedra_ref(tets, sdf, valid))


def test_fan_of_48_tets_shares_one_vertex():
    ring = torch.arange(48) + 2
    tets = torch.stack([torch.zeros(48, dtype=torch.long), torch.ones(48, dtype=torch.long), ring,
                        torch.roll(ring, -1)], 1)
    sdf = -torch.ones(50)
    sdf[0] = 1.0
    valid = torch.ones(50, dtype=torch.bool)
    ids, faces = _mt(tets, sdf, valid)
    assert ids.shape == (49, 2) and ids[0].tolist() == [0, 1]
    assert int(((ids[:, 0] == 0) & (ids[:, 1] == 1)).sum()) == 1
    assert faces.shape == (48, 3) and int((faces == 0).sum()) == 48  # every triangle uses the shared vertex once
    _same((ids, faces), R.marching_tetrahedra_ref(tets, sdf, valid))


def test_vertex_ids_above_65536():
    """V = 70 000 (17 key bits per end): the crossing edges join ids above 65 536."""
    pts, tets = R.kuhn_grid(6)  # 343 vertices
    off, V = 69000, 70000
    sdf = torch.full((V,), -1.0)
    sdf[off:off + pts.shape[0]] = pts.norm(dim=1) - 0.55
    valid = torch.ones(V, dtype=torch.bool)
    ref = R.marching_tetrahedra_ref(tets + off, sdf, valid)
    assert ref[0].shape[0] > 50 and int(ref[0].min()) > 65536
    _same(_mt(tets + off, sdf, valid), ref)
    _same(_mt((tets + off).int(), sdf, valid), ref)


@pytest.mark.parametrize("bad", [None, -1], ids=["id_equals_V", "negative_id"])
def test_vertex_id_out_of_range_raises(grid, bad):
    V = grid["sdf"].numel()
    tets = grid["tets"][:3000].clone()
    tets[1234, 2] = V if bad is None else bad
    for t in (tets, tets.int()):
        with pytest.raises(RuntimeError, match=r"outside \[0, V\)"):
            _mt(t, grid["sdf"], grid["valid"])
    with pytest.raises(RuntimeError, match="gsr: "):  # tets without vertices
        _mt(tets, torch.zeros(0), torch.zeros(0, dtype=torch.bool))
    # the library is fine afterwards
    ok = grid["tets"][:3000]
    _same(_mt(ok, grid["sdf"], grid["valid"]), R.marching_tetrahedra_ref(ok, grid["sdf"], grid["valid"]))


def test_grid_sphere(grid):
    a = _mt(grid["tets"], grid["sdf"], grid["valid"])
    b = _mt(grid["tets"], grid["sdf"], grid["valid"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])  # bit-identical runs, face order included
    _same(a, grid["ref"])
    assert torch.equal(a[1].cpu(), grid["ref"][1])  # and gsr's face order is the restatement's: tet order
    assert a[1].shape[0] > 5000 and R.is_closed_oriented(a[1])
    c = _mt(grid["tets"].int(), grid["sdf"], grid["valid"])
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


# ---- the driver -------------------------------------------------------------------------------------------------
class _Pipe:
    debug = False
    compute_cov3D_python = False


class _Model:
    def __init__(self, inp):
        self.get_xyz = inp["means3D"]
        self.get_opacity_with_3D_filter = inp["opacities"]
        self.get_scaling_with_3D_filter = inp["scales"]
        self.get_rotation = inp["rotations"]
        self.active_sh_degree = 3
        self.active_sg_degree = 0


def _views(W, H):
    """Three orbit cameras; the middle one carries a gt_mask (a disc) and the reference camera's R, T, Fx, Fy, Cx, Cy."""
    views = []
    for i, cam in enumerate(S.orbit_cameras(3, W, H)):
        cam = cam.to(DEV)
        v = types.SimpleNamespace(**{k: getattr(cam, k) for k in cam.__dataclass_fields__}, gt_mask=None)
        if i == 1:
            yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
            v.gt_mask = (((xx - W / 2) ** 2 + (yy - H / 2) ** 2) < (0.45 * H) ** 2).float()[None].to(DEV)
            v.R, v.T = cam.world_view_transform[:3, :3], cam.world_view_transform[3, :3]
            v.Fx, v.Fy = W / (2 * np.tan(cam.FoVx / 2)), H / (2 * np.tan(cam.FoVy / 2))
            v.Cx, v.Cy = (W - 1) / 2, (H - 1) / 2
        views.append(v)
    return views


def test_driver_matches_restatement(monkeypatch):
    import gsr_mesh as M

    g = group("scene")
    W, H = 96, 64
    pc = _Model({k: v.detach().contiguous().to(DEV) for k, v in S.activated_inputs(S.make_gaussians(**SCENE_KW)).items()})
    views = _views(W, H)
    pts, scale = torch.from_numpy(g["pts"]).to(DEV), torch.from_numpy(g["scale"]).to(DEV)
    cells = g["tets"].to(DEV)

    sdf, seen = M.alpha_cull_sdf(pts, views, pc, _Pipe(), 0.0)
    sdf_chunked, seen_chunked = M.alpha_cull_sdf(pts, views, pc, _Pipe(), 0.0, chunk=700)
    assert torch.equal(sdf, sdf_chunked) and torch.equal(seen, seen_chunked)
    assert sdf.shape == (pts.shape[0],) and seen.dtype == torch.bool
    assert 0.3 < float(seen.float().mean()) and bool((sdf[~seen] == 0.5).all())
    unmasked, _ = M.alpha_cull_sdf(pts, [types.SimpleNamespace(**{**vars(v), "gt_mask": None}) for v in views], pc,
                                   _Pipe(), 0.0)
    assert not torch.equal(sdf, unmasked)  # the mask removes a view from some points

    calls = []
    real = M.marching_tetrahedra_ids
    monkeypatch.setattr(M, "marching_tetrahedra_ids", lambda *a: (calls.append("hip"), real(*a))[1])
    verts, faces = M.extract_mesh(pts, scale, cells, views, pc, _Pipe(), 0.0, n_binary_steps=4)
    monkeypatch.setattr(M, "marching_tetrahedra_ids",
                        lambda t, s, v: (calls.append("ref"), R.marching_tetrahedra_ref(t, s, v))[1])
    rverts, rfaces = M.extract_mesh(pts, scale, cells, views, pc, _Pipe(), 0.0, n_binary_steps=4)
    assert calls == ["hip", "ref"]
    assert verts.dtype == torch.float32 and faces.dtype == torch.int64 and verts.shape[1] == 3
    assert faces.shape[0] > 0 and int(faces.max()) == verts.shape[0] - 1
    assert torch.equal(verts, rverts)
    assert torch.equal(R.canonical_faces(faces), R.canonical_faces(rfaces))
    assert torch.unique(faces).numel() == verts.shape[0]  # no unreferenced vertex is left
    # the bisection moved the vertices off the edge midpoints, and not past the edges' ends
    v0, _ = M.extract_mesh(pts, scale, cells, views, pc, _Pipe(), 0.0, n_binary_steps=0)
    assert v0.shape == verts.shape and not torch.equal(v0, verts)
    assert float((verts - v0).norm(dim=1).max()) <= float(scale.max())
