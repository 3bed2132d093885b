"""CPU tests of the DTU Chamfer evaluation (no GPU needed).

* tests/dtueval_ref.py, the numpy / scipy restatement the GPU tests use beyond
  the golden file, reproduces tests/golden/dtueval.npz (the reference's own
  dtu_eval/eval.py and best_fit_transform, see make_golden_dtueval.py): the
  sampled cloud bit for bit, the kept set and the counts exactly, distances
  within 1e-12 relative (cKDTree against sklearn's KD-tree), means within 1e-9.
* gsr_eval refuses CPU tensors, wrong dtypes and shapes (no CPU path).
* include/gsr.h declares the three calls and the ABI version is unchanged.
"""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import dtueval_ref as R
from test_tetmesh import _fake_device

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dtueval.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def ref(gold):
    return R.dtu_chamfer_ref(gold["vertices"], gold["faces"], gold["stl"], gold["obs_mask"], gold["bb"],
                             float(gold["res"]), gold["plane"], gold["perm"], float(gold["density"]), 60,
                             float(gold["max_dist"]))


def test_golden_file_is_small_and_takes_both_branches(gold):
    assert os.path.getsize(GOLD) < 400_000
    md = float(gold["max_dist"])
    assert (gold["dist_d2s"] < md).all() and (gold["dist_s2d"] < md).any() and (gold["dist_s2d"] >= md).any()
    assert gold["kept_index"].shape[0] < gold["data_pcd"].shape[0] // 2  # the thinning has work to do
    f = gold["faces"]
    assert ((f[:, 0] == f[:, 1]) | (f[:, 0] == f[:, 2]) | (f[:, 1] == f[:, 2])).sum() == 2


def test_restatement_samples_the_reference_cloud(gold, ref):
    assert ref["data_pcd"].dtype == np.float64 and np.array_equal(ref["data_pcd"], gold["data_pcd"])


def test_restatement_keeps_the_reference_points(gold, ref):
    assert np.array_equal(ref["kept_index"], gold["kept_index"])
    assert (ref["n_in"], ref["n_in_obs"], ref["n_stl_above"]) == (int(gold["n_in"]), int(gold["n_in_obs"]),
                                                                  int(gold["n_stl_above"]))


def test_restatement_distances_and_means(gold, ref):
    md = float(gold["max_dist"])
    for k in ("dist_d2s", "dist_s2d"):
        near = gold[k] < md
        assert np.array_equal(np.isfinite(ref[k]), near)
        assert np.abs(ref[k][near] - gold[k][near]).max() <= 1e-12 * gold[k][near].max()
    for k in ("mean_d2s", "mean_s2d", "overall"):
        assert abs(ref[k] - float(gold[k])) <= 1e-9 * abs(float(gold[k]))


def test_restatement_alignment(gold):
    scale, rot, t = R.align_ref(gold["cam_centers"], gold["gt_centers"])
    assert abs(scale - float(gold["align_scale"])) <= 1e-10 * float(gold["align_scale"])
    assert np.abs(rot - gold["align_R"]).max() <= 1e-10 and np.abs(t - gold["align_t"]).max() <= 1e-10 * 600


def test_align_to_dtu_matches_the_reference(gold):
    """Host code: runs without a GPU."""
    import gsr_eval as E

    scale, rot, t = E.align_to_dtu(torch.from_numpy(gold["cam_centers"]), gold["gt_centers"])
    assert abs(scale - float(gold["align_scale"])) <= 1e-10 * float(gold["align_scale"])
    assert np.abs(rot - gold["align_R"]).max() <= 1e-10 and np.abs(t - gold["align_t"]).max() <= 1e-10 * 600
    assert abs(np.linalg.det(rot) - 1) <= 1e-12
    moved = E.apply_alignment(torch.from_numpy(gold["cam_centers"]), scale, rot, t).numpy()
    assert moved.dtype == np.float64 and np.abs(moved - gold["gt_centers"]).max() < 0.01  # the scene's 1e-3 noise
    # a reflected target takes the reflection fix: still a rotation
    _, rot2, _ = E.align_to_dtu(gold["cam_centers"], gold["gt_centers"] * np.array([1.0, 1.0, -1.0]))
    assert abs(np.linalg.det(rot2) - 1) <= 1e-12
    with pytest.raises(RuntimeError):
        E.align_to_dtu(np.zeros((4, 2)), np.zeros((4, 2)))


@pytest.mark.parametrize("bad", ["cpu", "f16", "shape", "faces_dtype", "faces_shape", "perm_dtype", "perm_len",
                                 "mask_dtype"])
def test_entry_points_refuse_bad_arguments(bad):
    import gsr_eval as E

    pts = _fake_device(torch.zeros(5, 3, dtype=torch.float64))
    v, f = _fake_device(torch.zeros(4, 3)), _fake_device(torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        if bad == "cpu":
            E.nearest_distance(torch.zeros(5, 3, dtype=torch.float64), pts, 1.0)
        elif bad == "f16":
            E.downsample_points(_fake_device(torch.zeros(5, 3, dtype=torch.float16)), 0.2)
        elif bad == "shape":
            E.nearest_distance(pts, _fake_device(torch.zeros(5, 2, dtype=torch.float64)), 1.0)
        elif bad == "faces_dtype":
            E.sample_mesh_points(v, _fake_device(torch.zeros(2, 3, dtype=torch.int16)))
        elif bad == "faces_shape":
            E.sample_mesh_points(v, _fake_device(torch.zeros(2, 4, dtype=torch.int64)))
        elif bad == "perm_dtype":
            E.downsample_points(pts, 0.2, perm=_fake_device(torch.arange(5, dtype=torch.int32)))
        elif bad == "perm_len":
            E.downsample_points(pts, 0.2, perm=_fake_device(torch.arange(4)))
        elif bad == "mask_dtype":
            E.dtu_chamfer(v, f, _fake_device(torch.zeros(3, 3)), _fake_device(torch.zeros(2, 2, 2)), np.zeros((2, 3)),
                          0.5, np.zeros(4))
    with pytest.raises(RuntimeError):
        E.sample_mesh_points(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64))


def test_header_declares_the_calls_and_keeps_the_abi():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "gsr.h")).read()
    for name in ("gsr_mesh_sample_points", "gsr_points_downsample", "gsr_points_nearest"):
        assert f"int {name}(" in header
    from diff_gaussian_rasterization import _C

    assert _C.ABI_VERSION == 20
