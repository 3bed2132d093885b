"""GPU tests of the mesh clean-up in HIP (csrc/meshclean.hip through
gsr_mesh.cluster_connected_triangles and post_process_mesh).

Yardsticks: meshes whose answer is known by construction
(meshclean_ref.constructed / EXPECTED_KEPT) and, beyond them, the numpy /
scipy restatement tests/meshclean_ref.py, which tests/test_meshclean.py pins
to those.  Everything but the area is integer work and compared exactly.

Area: per cluster, |gsr - restatement| <= 1e-9 * sum 0.5 |e1| |e2| over the
cluster's triangles.  Both sum the same float64 terms up to contraction, in
different orders; (F + 16) * 2^-53 = 3.4e-11 at F <= 3e5, so the bar has
about 30x headroom.

The deep chains (one strip of 200 000 triangles) are what breaks label
propagation and unbounded find loops; the test runner's time limit is their
guard.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import helpers as Hh
import meshclean_ref as R
import tetmesh_ref as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _dev(v, f, dtype=torch.int64):
    return (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV),
            torch.from_numpy(np.ascontiguousarray(f)).to(dtype).to(DEV))


def _clusters(v, f, dtype=torch.int64, **kw):
    import gsr_mesh as M

    out = M.cluster_connected_triangles(*_dev(v, f, dtype), **kw)
    assert out[0].dtype == torch.int64 and out[1].dtype == torch.int64 and out[0].is_cuda and out[1].is_cuda
    assert out[0].shape == (f.shape[0],)
    assert (out[2] is None) == (v is None)
    if v is not None:
        assert out[2].dtype == torch.float64 and out[2].shape == out[1].shape
    return out


def _area_ratio(got_area, v, f, ref):
    """max over the clusters of |gsr - restatement| / sum 0.5 |e1| |e2| (0 where both are 0)."""
    if f.shape[0] == 0:
        assert got_area.shape == (0,)
        return 0.0
    v = v.astype(np.float64)
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    scale = np.bincount(ref[0], weights=0.5 * np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
    err = np.abs(got_area.cpu().numpy() - ref[2])
    assert (err[scale == 0] == 0).all()
    return float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


def _same_clusters(got, ref):
    assert torch.equal(got[0].cpu(), torch.from_numpy(ref[0]))
    assert torch.equal(got[1].cpu(), torch.from_numpy(ref[1]))


def _post(v, f, *a, dtype=torch.int64, **kw):
    import gsr_mesh as M

    pv, pf = M.post_process_mesh(*_dev(v, f, dtype), *a, **kw)
    assert pv.dtype == torch.float32 and pf.dtype == torch.int64 and pv.is_cuda and pf.is_cuda
    assert pv.dim() == 2 and pv.shape[1] == 3 and pf.dim() == 2 and pf.shape[1] == 3
    return pv, pf


def _same_mesh(got, ref):
    assert torch.equal(got[0].cpu(), torch.from_numpy(ref[0]))
    assert torch.equal(got[1].cpu(), torch.from_numpy(ref[1]))


# ---- constructed clusters ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("second_51", [False, True])
def test_constructed_clusters(second_51, dtype):
    m = R.constructed(7, second_51)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):  # a non-default stream: the call takes the caller's
        got = _clusters(m["vertices"], m["faces"], dtype)
        none = _clusters(None, m["faces"], dtype)
        bounded = _clusters(None, m["faces"], dtype, num_vertices=m["vertices"].shape[0])
    stream.synchronize()
    _same_clusters(got, (m["labels"], m["counts"]))
    _same_clusters(none, (m["labels"], m["counts"]))
    _same_clusters(bounded, (m["labels"], m["counts"]))
    ref = R.cluster_connected_triangles_ref(m["vertices"], m["faces"])
    assert _area_ratio(got[2], m["vertices"], m["faces"], ref) <= 1e-9


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("k,min_triangles,second_51,names", R.EXPECTED_KEPT)
def test_constructed_filter(k, min_triangles, second_51, names, dtype):
    m = R.constructed(3, second_51)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        got = _post(m["vertices"], m["faces"], k, min_triangles, dtype=dtype)
    stream.synchronize()
    _same_mesh(got, R.keep_by_name(m, names))  # vertex order, triangle order and winding included
    f = got[1]
    assert not bool(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any())


def test_defaults_are_the_references():
    m = R.constructed(5)
    import gsr_mesh as M

    v, f = _dev(m["vertices"], m["faces"])
    _same_mesh(M.post_process_mesh(v, f), R.keep_by_name(m, ("s300",)))  # cluster_to_keep=1, floor of 50


# ---- sizes around lane, wave and block ends ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fans():
    """160 fans of 7 triangles, shuffled: prefixes cut fans apart into smaller clusters."""
    rng = np.random.default_rng(11)
    faces, V, _ = R.concat([R.fan(7, 0, 1) for _ in range(160)])
    return rng.standard_normal((V, 3)).astype(np.float32), faces[rng.permutation(faces.shape[0])]


@pytest.mark.parametrize("F", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_sizes_around_block_ends(fans, F):
    v, f = fans[0], fans[1][:F]
    ref = R.cluster_connected_triangles_ref(v, f)
    for dtype in (torch.int32, torch.int64):
        got = _clusters(v, f, dtype)
        _same_clusters(got, ref)
        assert _area_ratio(got[2], v, f, ref) <= 1e-9
    if F == 0:
        pv, pf = _post(v, f)
        assert pv.shape == (0, 3) and pf.shape == (0, 3)
        return
    C = ref[1].shape[0]
    for k in sorted({1, (C + 1) // 2, C}):
        _same_mesh(_post(v, f, k, 1), R.post_process_mesh_ref(v, f, k, 1))
        _same_mesh(_post(v, f, k, 3, dtype=torch.int32), R.post_process_mesh_ref(v, f, k, 3))


# ---- deep chain ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["index", "reversed", "shuffled"])
def test_deep_chain(order):
    n = 200_000
    f = R.strip(n)
    if order == "reversed":
        f = f[::-1]
    elif order == "shuffled":
        f = f[np.random.default_rng(2).permutation(n)]
    labels, counts, _ = _clusters(None, f, torch.int32, num_vertices=n + 2)
    assert counts.cpu().tolist() == [n] and int(labels.max()) == 0 and int(labels.min()) == 0
    v = np.zeros((n + 2, 3), np.float32)
    pv, pf = _post(v, f)
    assert pv.shape == (n + 2, 3) and torch.equal(pf.cpu(), torch.from_numpy(np.ascontiguousarray(f)))


# ---- real shape ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    """The kuhn_grid(24) sphere through marching tetrahedra in HIP, 40 floaters of 4 to 60 triangles around it, and
    the restatement's clusters of the whole, computed once."""
    import gsr_mesh as M

    pts, tets = T.kuhn_grid(24)
    sdf = (pts - torch.tensor([0.03, -0.02, 0.01])).norm(dim=1) - 0.61
    ids, faces = M.marching_tetrahedra_ids(tets.to(DEV), sdf.to(DEV), torch.ones(sdf.numel(), dtype=torch.bool, device=DEV))
    ids, faces = ids.cpu(), faces.cpu()
    a, b = pts[ids[:, 0]], pts[ids[:, 1]]
    sa, sb = sdf[ids[:, 0]][:, None], sdf[ids[:, 1]][:, None]
    verts = ((a * sb - b * sa) / (sb - sa)).float().numpy()  # the linear zero crossing of every edge
    v, f = R.with_floaters(verts, faces.numpy(), n=40, seed=4)
    return dict(verts=verts, faces=faces.numpy(), v=v, f=f, ref=R.cluster_connected_triangles_ref(v, f))


def test_sphere_with_floaters(sphere):
    s = sphere
    assert s["faces"].shape[0] > 5000 and s["ref"][1].shape[0] == 41 and int(s["ref"][1].max()) == s["faces"].shape[0]
    _same_clusters(_clusters(s["v"], s["f"]), s["ref"])
    pv, pf = _post(s["v"], s["f"], 1)
    assert torch.equal(pv.cpu(), torch.from_numpy(s["verts"]))  # every vertex renumbered back, none lost
    assert torch.equal(T.canonical_faces(pf), T.canonical_faces(s["faces"]))
    assert T.is_closed_oriented(pf)
    _same_mesh((pv, pf), R.post_process_mesh_ref(s["v"], s["f"], 1))
    _same_mesh(_post(s["v"], s["f"], 3, dtype=torch.int32), R.post_process_mesh_ref(s["v"], s["f"], 3))


def test_repeat_runs_are_bit_identical(sphere):
    s = sphere
    a, b = _clusters(s["v"], s["f"]), _clusters(s["v"], s["f"])
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(a[2].view(torch.int64), b[2].view(torch.int64))
    p, q = _post(s["v"], s["f"], 2), _post(s["v"], s["f"], 2)
    assert torch.equal(p[0].view(torch.int32), q[0].view(torch.int32)) and torch.equal(p[1], q[1])


def test_area_against_restatement(sphere):
    s = sphere
    labels, counts, area = _clusters(s["v"], s["f"])
    ratio = _area_ratio(area, s["v"], s["f"], s["ref"])
    Hh.record_margins({"cluster area |d| / sum 0.5|e1||e2|": (ratio, 1e-9)}, "cluster areas vs restatement")
    assert ratio <= 1e-9
    big = int(labels[torch.from_numpy(s["ref"][0] == s["ref"][1].argmax()).to(DEV)][0])
    assert abs(float(area[big]) - 4 * np.pi * 0.61 ** 2) < 0.05  # the sphere's cluster has the sphere's area


# ---- errors --------------------------------------------------------------------------------------------------------
def test_vertex_id_out_of_range_raises():
    import gsr_mesh as M

    m = R.constructed(1)
    V = m["vertices"].shape[0]
    for bad in (V, -1):
        f = m["faces"].copy()
        f[123, 1] = bad
        for dtype in (torch.int32, torch.int64):
            with pytest.raises(RuntimeError, match=r"gsr: mesh_clusters: a face names a vertex outside \[0, V\)"):
                _clusters(m["vertices"], f, dtype)
            with pytest.raises(RuntimeError, match=r"outside \[0, V\)"):
                _post(m["vertices"], f, dtype=dtype)
    # the library is fine afterwards
    _same_clusters(_clusters(m["vertices"], m["faces"]), (m["labels"], m["counts"]))
    v, f = _dev(m["vertices"], m["faces"])
    C = m["counts"].shape[0]
    for k in (0, C + 1):
        with pytest.raises(ValueError, match="cluster_to_keep"):
            M.post_process_mesh(v, f, cluster_to_keep=k)
    _same_mesh(M.post_process_mesh(v, f, cluster_to_keep=C, min_triangles=1),
               R.post_process_mesh_ref(m["vertices"], m["faces"], C, 1))


# ---- the driver ----------------------------------------------------------------------------------------------------
def test_extract_mesh_cluster_to_keep():
    import gsr_mesh as M
    import gsr_scene as S
    from test_gpu_tetmesh import _Model, _Pipe, _views
    from test_tetmesh import SCENE_KW, group

    g = group("scene")
    pc = _Model({k: v.detach().contiguous().to(DEV) for k, v in S.activated_inputs(S.make_gaussians(**SCENE_KW)).items()})
    views = _views(96, 64)
    pts, scale = torch.from_numpy(g["pts"]).to(DEV), torch.from_numpy(g["scale"]).to(DEV)
    cells = g["tets"].to(DEV)
    args = (pts, scale, cells, views, pc, _Pipe(), 0.0)
    plain = M.extract_mesh(*args, n_binary_steps=4)
    none = M.extract_mesh(*args, n_binary_steps=4, cluster_to_keep=None)
    assert torch.equal(plain[0], none[0]) and torch.equal(plain[1], none[1])
    assert plain[1].shape[0] > 0 and torch.unique(plain[1]).numel() == plain[0].shape[0]
    kept = M.extract_mesh(*args, n_binary_steps=4, cluster_to_keep=1)
    again = M.post_process_mesh(*plain, cluster_to_keep=1)
    assert torch.equal(kept[0], again[0]) and torch.equal(kept[1], again[1])
    _same_mesh(kept, R.post_process_mesh_ref(plain[0].cpu().numpy(), plain[1].cpu().numpy(), 1))
