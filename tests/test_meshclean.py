"""CPU tests of the mesh clean-up (no GPU needed).

* tests/meshclean_ref.py, the numpy / scipy restatement the GPU tests use as
  their yardstick, reproduces the meshes whose answer is known by
  construction: strips of 49, 50, 51 and 300 triangles, two fans that touch
  at one vertex (2 clusters), three triangles on one edge (1 cluster), two
  index-degenerate triangles, triangle order shuffled; the clusters that stay
  for every (cluster_to_keep, min_triangles) of meshclean_ref.EXPECTED_KEPT.
* gsr_mesh.cluster_connected_triangles and post_process_mesh refuse CPU
  tensors, wrong dtypes and shapes and a bad cluster_to_keep (no CPU path).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import meshclean_ref as R
import tetmesh_ref as T
from test_tetmesh import _fake_device


@pytest.mark.parametrize("second_51", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_reproduces_constructed_clusters(seed, second_51):
    m = R.constructed(seed, second_51)
    labels, counts, area = R.cluster_connected_triangles_ref(m["vertices"], m["faces"])
    assert labels.dtype == np.int64 and counts.dtype == np.int64 and area.dtype == np.float64
    assert np.array_equal(labels, m["labels"]) and np.array_equal(counts, m["counts"])
    assert sorted(counts.tolist()) == sorted([2, 3, 6, 6, 49, 50, 51, 300] + [51] * second_51)
    assert labels[0] == 0 and np.array_equal(np.unique(labels, return_index=True)[1],
                                             np.sort(np.unique(labels, return_index=True)[1]))
    for name, n in (("fanA", 6), ("fanB", 6), ("edge3", 3), ("degen", 2)):
        ids = np.unique(labels[m["name"] == name])
        assert ids.shape == (1,) and counts[ids[0]] == n
    assert labels[m["name"] == "fanA"][0] != labels[m["name"] == "fanB"][0]  # a shared vertex does not connect
    none = R.cluster_connected_triangles_ref(None, m["faces"].astype(np.int32))
    assert np.array_equal(none[0], labels) and none[2] is None


@pytest.mark.parametrize("k,min_triangles,second_51,names", R.EXPECTED_KEPT)
def test_restatement_reproduces_constructed_filter(k, min_triangles, second_51, names):
    m = R.constructed(3, second_51)
    v, f = R.post_process_mesh_ref(m["vertices"], m["faces"], k, min_triangles)
    ev, ef = R.keep_by_name(m, names)
    assert v.dtype == np.float32 and f.dtype == np.int64
    assert np.array_equal(v, ev) and np.array_equal(f, ef)
    assert not ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any()
    if "degen" in names:  # its vertices were referenced when the unreferenced ones went: they stay
        assert v.shape[0] == m["vertices"].shape[0] and np.unique(f).shape[0] == v.shape[0] - 3


def test_restatement_area_and_edge_cases():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 3], [5, 5, 5]], np.float32)
    f = np.array([[0, 1, 2], [4, 4, 4], [0, 1, 3]])
    labels, counts, area = R.cluster_connected_triangles_ref(v, f)
    assert labels.tolist() == [0, 1, 0] and counts.tolist() == [2, 1] and area.tolist() == [5.0, 0.0]
    e = R.cluster_connected_triangles_ref(v, np.zeros((0, 3), np.int64))
    assert e[0].shape == (0,) and e[1].shape == (0,) and e[2].shape == (0,)
    ev, ef = R.post_process_mesh_ref(v, np.zeros((0, 3), np.int64))
    assert ev.shape == (0, 3) and ef.shape == (0, 3)
    for bad in (0, 3):
        with pytest.raises(IndexError):
            R.post_process_mesh_ref(v, f, bad, 1)


def test_with_floaters_only_adds_small_clusters():
    m = R.constructed(0)
    v, f = R.with_floaters(m["vertices"], m["faces"], n=40, seed=1)
    _, counts, _ = R.cluster_connected_triangles_ref(None, f)
    assert counts.shape[0] == m["counts"].shape[0] + 40
    extra = sorted(counts.tolist())
    for c in m["counts"].tolist():
        extra.remove(c)
    assert min(extra) == 4 and max(extra) == 60
    pv, pf = R.post_process_mesh_ref(v, f, 1)
    ev, ef = R.keep_by_name(m, ("s300",))
    assert np.array_equal(pv, ev) and torch.equal(T.canonical_faces(pf), T.canonical_faces(ef))


def test_mesh_cleanup_refuses_cpu_tensors():
    import gsr_mesh as M

    v, f = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="cluster_connected_triangles: `faces` must be a HIP device tensor"):
        M.cluster_connected_triangles(v, f)
    with pytest.raises(RuntimeError, match="cluster_connected_triangles: `faces` must be a HIP device tensor"):
        M.cluster_connected_triangles(None, f)
    with pytest.raises(RuntimeError, match="cluster_connected_triangles: `vertices` must be a HIP device tensor"):
        M.cluster_connected_triangles(v, _fake_device(f))
    with pytest.raises(RuntimeError, match="post_process_mesh: `faces` must be a HIP device tensor"):
        M.post_process_mesh(v, f)
    with pytest.raises(RuntimeError, match="post_process_mesh: `vertices` must be a HIP device tensor"):
        M.post_process_mesh(v, _fake_device(f))
    with pytest.raises(RuntimeError, match="post_process_mesh: `vertices` must be a HIP device tensor"):
        M.post_process_mesh(None, _fake_device(f))
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        M.post_process_mesh(v.numpy(), f.numpy())


@pytest.mark.parametrize("fn", ["cluster_connected_triangles", "post_process_mesh"])
@pytest.mark.parametrize("bad", ["faces_shape", "faces_dim", "faces_dtype", "vertices_dtype", "vertices_shape",
                                 "vertices_dim"])
def test_mesh_cleanup_shape_and_dtype_errors(fn, bad):
    import gsr_mesh as M

    a = dict(vertices=torch.zeros(5, 3), faces=torch.zeros(4, 3, dtype=torch.int64))
    name = bad.split("_")[0]
    if bad == "faces_shape":
        a["faces"] = torch.zeros(4, 4, dtype=torch.int64)
    elif bad == "faces_dim":
        a["faces"] = torch.zeros(12, dtype=torch.int64)
    elif bad == "faces_dtype":
        a["faces"] = torch.zeros(4, 3, dtype=torch.int16)
    elif bad == "vertices_dtype":
        a["vertices"] = torch.zeros(5, 3, dtype=torch.float64)
    elif bad == "vertices_shape":
        a["vertices"] = torch.zeros(5, 2)
    elif bad == "vertices_dim":
        a["vertices"] = torch.zeros(1, 5, 3)
    a = {k: _fake_device(v) for k, v in a.items()}
    with pytest.raises(RuntimeError, match=f"{fn}: `{name}` must"):
        getattr(M, fn)(**a)


@pytest.mark.parametrize("k", [0, -1, 1.0, True, None, "1"])
def test_post_process_mesh_refuses_bad_cluster_to_keep(k):
    """cluster_to_keep < 1 or not an integer: ValueError before anything runs (the reference's np.sort(...)[-k]
    raises IndexError for 0 and picks a wrong cluster for a negative k)."""
    import gsr_mesh as M

    v, f = _fake_device(torch.zeros(5, 3)), _fake_device(torch.zeros(4, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="post_process_mesh: `cluster_to_keep` must be an integer >= 1"):
        M.post_process_mesh(v, f, cluster_to_keep=k)


def test_extract_mesh_takes_cluster_to_keep():
    import inspect

    import gsr_mesh as M

    p = inspect.signature(M.extract_mesh).parameters
    assert list(p)[-1] == "cluster_to_keep" and p["cluster_to_keep"].default is None
    assert p["n_binary_steps"].default == 10
