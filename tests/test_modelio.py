"""Model files on the host (gsr_model): the header, the numpy restatement of both directions
(tests/modelio_ref.py), every refusal of the header parser, the row length through the ABI, and what a
checkpoint may contain.  No device: the kernels are in tests/test_gpu_modelio.py.

plyfile is not a dependency of this project; where it can be imported the restatement is held to it, otherwise
that parity is restated and not run.
"""
from __future__ import annotations

import io

import numpy as np
import pytest
import torch

import modelio_ref as R

HEADER_2_1_0 = (b"ply\n"
                b"format binary_little_endian 1.0\n"
                b"element vertex 2\n"
                b"property float x\n"
                b"property float y\n"
                b"property float z\n"
                b"property float nx\n"
                b"property float ny\n"
                b"property float nz\n"
                b"property float f_dc_0\n"
                b"property float f_dc_1\n"
                b"property float f_dc_2\n"
                b"property float opacity\n"
                b"property float scale_0\n"
                b"property float scale_1\n"
                b"property float scale_2\n"
                b"property float rot_0\n"
                b"property float rot_1\n"
                b"property float rot_2\n"
                b"property float rot_3\n"
                b"property float filter_3D\n"
                b"end_header\n")


def _gm():
    import gsr_model

    return gsr_model


# ------------------------------------------------------------------ header
def test_header_literal():
    assert _gm().ply_header(2, 1, 0) == HEADER_2_1_0
    assert R.header(2, [(n, "float") for n in R.names(1, 0)]) == HEADER_2_1_0


@pytest.mark.parametrize("M,G", [(16, 0), (4, 2)])
def test_header_property_list(M, G):
    gm = _gm()
    head = gm.ply_header(5, M, G)
    count, props, end = R.parse_header(head)
    assert count == 5 and end == len(head)
    assert props == [(n, "float") for n in R.names(M, G)]
    assert len(props) == 18 + 3 * (M - 1) + 7 * G
    assert [n for n, _ in R.parse_header(gm.ply_header(5, M, G, exclude_filter=True))[1]] == R.names(M, G, True)


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("sh,sg", [(0, 0), (3, 0), (1, 2), (3, 7)])
def test_restatement_round_trip_bit_for_bit(sh, sg):
    raw = R.make_raw(9, sh, sg, seed=sh + sg, special_rows=(0, 4, 8))
    assert np.isnan(raw["xyz"][0]).any() and (raw["xyz"].view(np.uint32) == 0x80000000).any()
    data = R.save_bytes(raw)
    M, G = R.degrees(raw)
    assert len(data) == len(_gm().ply_header(9, M, G)) + 9 * 4 * (18 + 3 * (M - 1) + 7 * G)
    back = R.load(data)
    for k in R.FIELDS:
        assert R.bits_equal(back[k], raw[k]), k


def test_restatement_transposes_f_rest():
    """A guard on tests/modelio_ref.py alone (it runs no code of gsr_model, and passes without it): the
    reference the other tests compare with has the reference's one transposition."""
    raw = R.make_raw(3, 2, 1)
    att = R.rows(raw)
    K = 8
    for c in range(3):
        for k in range(K):
            assert np.array_equal(att[:, 9 + c * K + k], raw["features_rest"][:, k, c])
    assert not att[:, 3:6].any()
    assert np.array_equal(att[:, -1], raw["filter_3D"][:, 0])


def test_restatement_reads_the_awkward_layout():
    """A guard on tests/modelio_ref.py alone (it runs no code of gsr_model, and passes without it): the file
    the GPU test loads has a reversed order, uchar after z (odd stride) and doubles that no float32 holds."""
    raw = R.make_raw(7, 1, 2, special_rows=(0, 6))
    data = R.build_file(raw, reverse=True, uchar_after_z=True, double_prefixes=("scale_", "opacity"), drop_sg=True)
    count, props, _ = R.parse_header(data)
    stride = sum({"float": 4, "double": 8, "uchar": 1}[t] for _, t in props)
    assert stride % 2 == 1 and props[0][0] == "filter_3D"
    got = R.load(data)
    assert got["sg_axis"].shape == (7, 0, 3) and got["sg_sharpness"].shape == (7, 0)
    for k in ("xyz", "features_dc", "features_rest", "rotation", "filter_3D"):
        assert R.bits_equal(got[k], raw[k]), k
    el, _ = R.read_structured(data)
    d = np.asarray(el["scale_1"])
    with np.errstate(over="ignore", under="ignore"):
        assert (d.astype(np.float32).astype(np.float64) != d).any()  # the doubles do not round-trip
    assert not R.bits_equal(got["scaling"], raw["scaling"])


def test_plyfile_parity():
    plyfile = pytest.importorskip("plyfile")
    raw = R.make_raw(6, 1, 2, special_rows=(0, 5))
    M, G = R.degrees(raw)
    att = R.rows(raw)
    elements = np.empty(6, dtype=[(n, "f4") for n in R.names(M, G)])
    elements[:] = list(map(tuple, att))
    buf = io.BytesIO()
    plyfile.PlyData([plyfile.PlyElement.describe(elements, "vertex")]).write(buf)
    assert buf.getvalue() == R.save_bytes(raw)
    el = plyfile.PlyData.read(io.BytesIO(R.save_bytes(raw))).elements[0]
    for c, n in enumerate(R.names(M, G)):
        assert R.bits_equal(np.asarray(el[n]), att[:, c]), n


# ------------------------------------------------------------------ the header parser
def _write(tmp_path, data, name="m.ply"):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def _file(props, count=2, fmt="binary_little_endian", payload=None, extra_lines=()):
    lines = ["ply", f"format {fmt} 1.0", f"element vertex {count}"]
    lines += [f"property {t} {n}" for n, t in props] + list(extra_lines) + ["end_header"]
    width = {"float": 4, "double": 8, "uchar": 1, "int": 4}
    stride = sum(width[t.split()[-1]] if not t.startswith("list") else 0 for _, t in props)
    body = b"\0" * (count * stride) if payload is None else payload
    return ("\n".join(lines) + "\n").encode() + body


def _props(M=4, G=2, drop=(), types=None):
    types = types or {}
    return [(n, types.get(n, "float")) for n in R.names(M, G) if n not in drop]


def test_read_ply_header_accepts(tmp_path):
    gm = _gm()
    raw = R.make_raw(5, 1, 2)
    h = gm.read_ply_header(_write(tmp_path, R.save_bytes(raw)))
    assert (h.count, h.sh_degree, h.sg_degree, h.stride, h.has_filter) == (5, 1, 2, 4 * 41, True)
    assert h.payload_offset == len(gm.ply_header(5, 4, 2))
    assert [(n, t) for n, t, _ in h.properties] == [(n, "float") for n in R.names(4, 2)]
    assert [o for _, _, o in h.properties] == list(range(0, 4 * 41, 4))
    off, code = h.column_tables()
    assert list(off[:3]) == [0, 4, 8] and list(off[3:6]) == [-1, -1, -1] and off[-1] == 160 and not code.any()
    # another order, other types between the floats, doubles, no SG, trailing elements
    data = R.build_file(raw, reverse=True, uchar_after_z=True, double_prefixes=("scale_", "opacity"), drop_sg=True)
    h = gm.read_ply_header(_write(tmp_path, data, "b.ply"))
    assert (h.count, h.sh_degree, h.sg_degree) == (5, 1, 0) and h.stride == 4 * 27 + 3 + 4 * 4
    off, code = h.column_tables()
    names = R.names(4, 0)
    at = {n: o for n, _, o in h.properties}
    assert off[names.index("z")] == at["z"] and at["blue"] == at["z"] - 3 and at["red"] == at["z"] - 1 and at["z"] % 4 == 3
    assert [int(c) for c in code] == [int(n.startswith("scale_") or n == "opacity") for n in names]
    h = gm.read_ply_header(_write(tmp_path, _file(_props(1, 0, drop=("filter_3D",))), "c.ply"),
                           allow_missing_filter=True)
    assert not h.has_filter and h.column_tables()[0][-1] == -1


REFUSALS = [
    ("ascii", _file(_props(), fmt="ascii"), "ascii"),
    ("big-endian", _file(_props(), fmt="binary_big_endian"), "binary_big_endian"),
    ("list", _file(_props() + [("vertex_indices", "list uchar int")]), "vertex_indices"),
    ("short payload", _file(_props(), count=3, payload=b"\0" * (3 * 4 * 41 - 1)), "shorter than count x stride"),
    ("missing x", _file(_props(drop=("x",))), "`x`"),
    ("missing opacity", _file(_props(drop=("opacity",))), "`opacity`"),
    ("missing f_dc_1", _file(_props(drop=("f_dc_1",))), "`f_dc_1`"),
    ("missing scale_2", _file(_props(drop=("scale_2",))), "scale_"),
    ("missing rot_0", _file(_props(drop=("rot_0",))), "rot_"),
    ("missing filter", _file(_props(drop=("filter_3D",))), "`filter_3D`"),
    ("f_rest count", _file(_props(drop=("f_rest_8",))), "f_rest_"),
    ("f_rest not a degree", _file(_props(M=3)), "f_rest_"),
    ("sg counts", _file(_props(drop=("sg_color_5",))), "sg_color_"),
    ("sg sharpness", _file(_props(drop=("sg_sharpness_1",))), "sg_sharpness_"),
    ("int column", _file(_props(types={"opacity": "int"})), "`opacity`"),
    ("uchar column", _file(_props(types={"f_rest_3": "uchar"})), "`f_rest_3`"),
]


@pytest.mark.parametrize("data,match", [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_read_ply_header_refuses(tmp_path, data, match):
    with pytest.raises(ValueError, match=match):
        _gm().read_ply_header(_write(tmp_path, data))


def test_load_ply_checks_the_degrees_before_any_device_work(tmp_path):
    path = _write(tmp_path, R.save_bytes(R.make_raw(3, 1, 2)))
    with pytest.raises(ValueError, match="sh_degree = 3"):
        _gm().load_ply(path, sh_degree=3)
    with pytest.raises(ValueError, match="sg_degree = 0"):
        _gm().load_ply(path, sg_degree=0)


def test_max_iteration(tmp_path):
    gm = _gm()
    with pytest.raises(ValueError, match="no point_cloud"):
        gm.max_iteration(str(tmp_path))
    for n in ("iteration_7", "iteration_30", "iteration_x", "other"):
        (tmp_path / "point_cloud" / n).mkdir(parents=True)
    assert gm.max_iteration(str(tmp_path)) == 30


# ------------------------------------------------------------------ the ABI's host entries
def test_row_floats_and_block_rows_through_the_table():
    from diff_gaussian_rasterization import _abi

    L = _abi.load()
    for M in (1, 4, 9, 16):
        for G in (0, 1, 2, 7):
            A = L.gsr_model_row_floats(M, G)
            assert A == 18 + 3 * (M - 1) + 7 * G == len(R.names(M, G))
            Rb = L.gsr_model_block_rows(A)
            assert 4 <= Rb <= 256 and Rb % 4 == 0 and Rb * A * 4 <= 32 * 1024
    assert L.gsr_model_row_floats(0, 0) == 0 and L.gsr_model_row_floats(1, -1) == 0
    assert L.gsr_model_block_rows(8192) == 1 and L.gsr_model_block_rows(8193) == 0 and L.gsr_model_block_rows(0) == 0
    assert L.gsr_model_block_rows(4000) == 2  # (fewer than 4 rows: not rounded to a multiple of 4)
    assert [L.gsr_model_unpack_block_rows(s) for s in (0, 1, 4 * 63, 4 * 112, 32736, 32737)] == [0, 256, 129, 73, 1, 0]


# ------------------------------------------------------------------ checkpoints
def _walk(x, where="capture()"):
    if x is None or isinstance(x, (torch.Tensor, bool, int, float, str)):
        assert not isinstance(x, torch.nn.Parameter), f"{where} is a Parameter"
        return
    if isinstance(x, dict):
        assert type(x) is dict, f"{where} is a {type(x).__name__}"
        for k, v in x.items():
            assert isinstance(k, (int, str)), f"{where} has the key {k!r}"
            _walk(v, f"{where}[{k!r}]")
    elif isinstance(x, list):
        assert type(x) is list, f"{where} is a {type(x).__name__}"
        for n, v in enumerate(x):
            _walk(v, f"{where}[{n}]")
    else:
        raise AssertionError(f"{where} is a {type(x).__name__}")


@pytest.mark.parametrize("app", ["no", "gs", "gof", "pgsr"])
def test_capture_holds_plain_data_only(app):
    import gsr_scene as S
    from gsr_train import TrainGaussians

    raw = S.make_gaussians(12, sh_degree=1, sg_degree=2)
    g = TrainGaussians(raw, spatial_lr_scale=2.5, sh_degree=1, sg_degree=2)
    g.create_app_model(3, app, lr={"gs_final": 0.0005} if app == "gs" else None)
    for group in g.optimizer.param_groups:  # (per-parameter state as after one step; no kernel involved)
        for p in group["params"]:
            g.optimizer.state[p] = {"step": torch.tensor(1.0), "exp_avg": torch.zeros_like(p),
                                    "exp_avg_sq": torch.ones_like(p)}
    state = g.capture()
    assert isinstance(state, tuple) and len(state) == 19 + 4
    for n, item in enumerate(state):  # the tuple itself is the one container that is not a list or a dict
        _walk(item, f"capture()[{n}]")
    assert state[:2] == (1, 2) and state[15] == 2.5 and state[16] == app
    assert state[2] is not g._xyz and state[2].data_ptr() == g._xyz.data_ptr()
    assert (state[17] is not None) == (app == "gof") and (state[18] is not None) == (app != "no")
    assert state[21] == 0.01 and state[22] == ({"gs_final": 0.0005} if app == "gs" else {})
    buf = io.BytesIO()
    torch.save((state, 9), buf)
    buf.seek(0)
    loaded, it = torch.load(buf, weights_only=True)
    assert it == 9 and len(loaded) == len(state)
    # restore on the host: fresh leaves with the saved bits, the groups by name with their rates and state
    h = TrainGaussians(S.make_gaussians(12, sh_degree=1, sg_degree=2, seed=3), sh_degree=0, sg_degree=0)
    h.restore(loaded)
    assert (h.active_sh_degree, h.active_sg_degree, h.spatial_lr_scale, h.app_model.value) == (1, 2, 2.5, app)
    assert torch.equal(h._xyz, g._xyz) and h._xyz.is_leaf and h._xyz.requires_grad
    assert h._xyz.data_ptr() != loaded[2].data_ptr()
    assert [(x["name"], x["lr"]) for x in h.optimizer.param_groups] == \
           [(x["name"], x["lr"]) for x in g.optimizer.param_groups]
    for gh, gg in zip(h.optimizer.param_groups, g.optimizer.param_groups):
        assert isinstance(gh["betas"], tuple) and len(gh["params"]) == len(gg["params"])
        for ph, pg in zip(gh["params"], gg["params"]):
            assert torch.equal(ph, pg)
            sh_, sg_ = h.optimizer.state[ph], g.optimizer.state[pg]
            assert float(sh_["step"]) == 1.0 and not sh_["step"].is_cuda
            assert torch.equal(sh_["exp_avg"], sg_["exp_avg"]) and torch.equal(sh_["exp_avg_sq"], sg_["exp_avg_sq"])
    if app == "gs":
        assert h.exposure_scheduler_args(30000) == pytest.approx(0.0005)
