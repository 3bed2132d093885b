"""GPU tests of the model files (gsr_model, csrc/modelio.hip) against the numpy restatement of
the reference's save_ply / load_ply (tests/modelio_ref.py).

Everything is bit-exact: tensors and rows are compared on their uint32 view, files byte for byte.  The sizes
are taken from R = gsr_model_block_rows(A), the rows one workgroup owns, so that block seams, a block of one
row and a ragged last block are all met; the unpack kernel sizes its blocks from the file's row bytes
(gsr_model_unpack_block_rows), so its seams are met as well.  NaNs with payloads, -0, the infinities and
denormals sit in the first row, the last row and the two rows at the first seam of either kernel.
"""
from __future__ import annotations

import math
import os

import numpy as np
import pytest
import torch

import modelio_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DEGREES = [(0, 0), (3, 0), (1, 2), (3, 7)]


def _gm():
    import gsr_model

    return gsr_model


def _block_rows(sh, sg):
    from diff_gaussian_rasterization import _abi

    L = _abi.load()
    return L.gsr_model_block_rows(L.gsr_model_row_floats((sh + 1) ** 2, sg))


def _unpack_rows(stride):
    """Rows per workgroup of the unpack kernel for file rows of `stride` bytes (it differs from the pack's R)."""
    from diff_gaussian_rasterization import _abi

    return _abi.load().gsr_model_unpack_block_rows(stride)


def _row_bytes(sh, sg):
    return 4 * (18 + 3 * ((sh + 1) ** 2 - 1) + 7 * sg)


def _sizes(sh, sg):
    Rb = _block_rows(sh, sg)
    return [0, 1, 63, 64, 65, Rb - 1, Rb, Rb + 1, 2 * Rb + 1]


_CASES = {}


def _case(P, sh, sg, seam=None):
    """(the model as numpy arrays, as RawGaussians on the device), made once per size.  The special values sit
    in the first and last rows and on both sides of the first seam of the pack kernel, of the unpack kernel
    for the canonical file, and of `seam` (the rows per workgroup of another file layout) when given."""
    import gsr_scene as S

    key = (P, sh, sg, seam)
    if key not in _CASES:
        Rb, Ru = _block_rows(sh, sg), _unpack_rows(_row_bytes(sh, sg))
        rows = (0, P - 1, Rb - 1, Rb, Ru - 1, Ru) + ((seam - 1, seam) if seam else ())
        raw = R.make_raw(P, sh, sg, seed=P + 7 * sh + sg, special_rows=rows)
        dev = S.RawGaussians(*[torch.from_numpy(raw[k]).to(DEV) for k in
                               ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity", "sg_axis",
                                "sg_sharpness", "sg_color", "filter_3D")])
        _CASES[key] = (raw, dev)
    return _CASES[key]


def _same_bits(t, want, what):
    got = t.detach().cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32).reshape(want.shape) != want.view(np.uint32))
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}"


def _same_model(got, want, what):
    for k in R.FIELDS:
        _same_bits(getattr(got, k), want[k], f"{what} {k}")


# ------------------------------------------------------------------ pack
@pytest.mark.parametrize("sh,sg", DEGREES)
def test_pack_rows_bit_exact(sh, sg):
    gm = _gm()
    for P in _sizes(sh, sg):
        raw, dev = _case(P, sh, sg)
        tensors, _, M, G = gm._tensors(dev)
        rows = gm.pack_rows(tensors, M, G)
        _same_bits(rows, R.rows(raw), f"P={P}")


def test_pack_rows_from_unaligned_tensors():
    """Tensors that start 4 bytes off a 16-byte boundary (views into a larger buffer) take the kernel's
    dword path; the rows are the same."""
    gm = _gm()
    sh, sg = 1, 2
    P = 2 * _block_rows(sh, sg) + 3
    raw, dev = _case(P, sh, sg)
    tensors, _, M, G = gm._tensors(dev)
    shifted = []
    for t in tensors:
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        shifted.append(v)
    _same_bits(gm.pack_rows(shifted, M, G), R.rows(raw), "shifted")
    _same_bits(gm.pack_rows(tensors, M, G, r0=1, n=P - 2), R.rows(raw)[1:-1], "rows 1 .. P-2")


# ------------------------------------------------------------------ file
@pytest.mark.parametrize("sh,sg", DEGREES)
def test_save_ply_is_the_reference_file(sh, sg, tmp_path):
    gm = _gm()
    for P in _sizes(sh, sg):
        raw, dev = _case(P, sh, sg)
        path = str(tmp_path / f"m{P}.ply")
        gm.save_ply(dev, path)
        with open(path, "rb") as f:
            assert f.read() == R.save_bytes(raw), P


@pytest.mark.parametrize("chunk_rows", [100, 101, 1])
def test_save_ply_in_chunks(chunk_rows, tmp_path):
    """Chunk seams inside the kernel's blocks (100 rows, a multiple of 4: the 16-byte path; 101 and 1: chunks
    that start off a 16-byte boundary)."""
    raw, dev = _case(257, 1, 2)
    path = str(tmp_path / "sub" / "dir" / "m.ply")  # (the directory is made)
    _gm().save_ply(dev, path, chunk_rows=chunk_rows)
    with open(path, "rb") as f:
        assert f.read() == R.save_bytes(raw)


# ------------------------------------------------------------------ unpack
@pytest.mark.parametrize("sh,sg", DEGREES)
def test_load_ply_returns_the_tensors(sh, sg, tmp_path):
    gm = _gm()
    Ru = _unpack_rows(_row_bytes(sh, sg))
    for P in sorted(set(_sizes(sh, sg) + [Ru - 1, Ru, Ru + 1, 2 * Ru + 1])):  # (the unpack kernel's own seams too)
        raw, _ = _case(P, sh, sg)
        path = str(tmp_path / f"m{P}.ply")
        with open(path, "wb") as f:
            f.write(R.save_bytes(raw))
        got = gm.load_ply(path, device=DEV)
        _same_model(got, raw, f"P={P}")
        assert got.xyz.device == DEV and got.features_rest.shape == (P, (sh + 1) ** 2 - 1, 3)
    _same_model(gm.load_ply(path, sh_degree=sh, sg_degree=sg, device=DEV, chunk_rows=100), raw, "chunks of 100")


@pytest.mark.parametrize("chunk_rows", [None, 100, 150])  # (150: a workgroup seam inside a chunk)
def test_load_ply_awkward_layout(chunk_rows, tmp_path):
    """Reversed property order, three uchar after z (an odd stride: every block but the first starts
    unaligned), scale_* and opacity as doubles no float32 holds, no SG properties."""
    gm = _gm()
    sh, sg = 3, 2
    P = 2 * _block_rows(sh, sg) + 1
    stride = _row_bytes(sh, 0) + 3 + 4 * 4  # (no SG columns, three uchar, four columns 4 bytes wider)
    Ru = _unpack_rows(stride)
    assert Ru < P  # more than one workgroup; the special values straddle its first seam
    raw, _ = _case(P, sh, sg, seam=Ru)
    data = R.build_file(raw, reverse=True, uchar_after_z=True, double_prefixes=("scale_", "opacity"), drop_sg=True)
    path = str(tmp_path / "awkward.ply")
    with open(path, "wb") as f:
        f.write(data)
    h = gm.read_ply_header(path)
    assert h.stride == stride and h.stride % 2 == 1 and h.sg_degree == 0
    want = R.load(data)
    assert not R.bits_equal(want["scaling"], raw["scaling"])  # (the rounding is exercised)
    got = gm.load_ply(path, device=DEV, chunk_rows=chunk_rows)
    _same_model(got, want, "awkward")
    _same_bits(got.xyz, raw["xyz"], "awkward xyz")


def test_load_ply_allow_missing_filter(tmp_path):
    gm = _gm()
    raw, _ = _case(65, 1, 2)
    data = R.build_file(raw, drop_filter=True)
    path = str(tmp_path / "nofilter.ply")
    with open(path, "wb") as f:
        f.write(data)
    with pytest.raises(ValueError, match="filter_3D"):
        gm.load_ply(path, device=DEV)
    got = gm.load_ply(path, device=DEV, allow_missing_filter=True)
    want = R.load(data, allow_missing_filter=True)
    assert not want["filter_3D"].any()
    _same_model(got, want, "no filter")


def test_offsets_past_two_to_the_31():
    """P A 4 > 2^31 bytes of rows (SH 3, SG 7): the global offsets of both kernels are 64-bit.  The reference
    here is the torch chain on the device (the restatement's transposes and one cat), and the numpy restatement
    on the last rows, the ones whose byte offsets lie past 2^31."""
    import gsr_scene as S

    gm = _gm()
    sh, sg, P = 3, 7, 4_800_001
    A = _row_bytes(sh, sg) // 4
    assert P * A * 4 > 2 ** 31
    gen = torch.Generator(device=DEV).manual_seed(3)
    shapes = ((P, 3), (P, 1, 3), (P, 15, 3), (P, 3), (P, 4), (P, 1), (P, sg, 3), (P, sg), (P, sg, 3), (P, 1))
    raw = S.RawGaussians(*[torch.randn(s, generator=gen, device=DEV) for s in shapes])
    tensors, _, M, G = gm._tensors(raw)
    rows = gm.pack_rows(tensors, M, G)
    want = torch.cat((raw.xyz, torch.zeros_like(raw.xyz), raw.features_dc.transpose(1, 2).flatten(1),
                      raw.features_rest.transpose(1, 2).flatten(1), raw.opacity, raw.scaling, raw.rotation,
                      raw.sg_axis.flatten(1), raw.sg_sharpness, raw.sg_color.flatten(1), raw.filter_3D), dim=1)
    assert torch.equal(rows.view(torch.int32), want.view(torch.int32))
    del want
    tail = {k: getattr(raw, k)[-300:].cpu().numpy() for k in R.FIELDS}
    _same_bits(rows[-300:], R.rows(tail), "the last 300 rows")
    # and back: the rows as a file's payload, unpacked in one call
    from diff_gaussian_rasterization import _abi

    off = torch.arange(0, 4 * A, 4, dtype=torch.int32, device=DEV)
    code = torch.zeros(A, dtype=torch.int32, device=DEV)
    outs = [torch.empty_like(t) for t in tensors]
    _abi.call(DEV, "gsr_model_unpack_rows", P, M, G, 4 * A, rows.data_ptr(), off.data_ptr(), code.data_ptr(),
              *[t.data_ptr() for t in outs], _abi.stream(DEV))
    for (name, _), got, t in zip(gm.TENSORS, outs, tensors):
        assert torch.equal(got.view(torch.int32), t.view(torch.int32)), name


# ------------------------------------------------------------------ argument errors
def test_save_ply_refuses_what_it_would_have_to_copy(tmp_path):
    import gsr_scene as S

    gm = _gm()
    _, dev = _case(65, 1, 2)
    fields = list(S.RawGaussians.__dataclass_fields__)
    path = str(tmp_path / "never.ply")

    def with_(name, t):
        return S.RawGaussians(*[t if f == name else getattr(dev, f) for f in fields])

    wide = torch.zeros(65, 6, device=DEV)
    with pytest.raises(ValueError, match="`scaling` must be contiguous"):
        gm.save_ply(with_("scaling", wide[:, ::2]), path)
    with pytest.raises(ValueError, match="`rotation` must be float32"):
        gm.save_ply(with_("rotation", dev.rotation.double()), path)
    with pytest.raises(ValueError, match="`opacity` must be on a HIP device"):
        gm.save_ply(with_("opacity", dev.opacity.cpu()), path)
    with pytest.raises(ValueError, match="`sg_color` must have shape"):
        gm.save_ply(with_("sg_color", dev.sg_color[:, :1].contiguous()), path)
    assert not os.path.exists(path)


def test_abi_argument_errors():
    from diff_gaussian_rasterization import _abi

    L = _abi.load()
    P, M, G = 8, 4, 0
    A = L.gsr_model_row_floats(M, G)
    stride = 4 * A
    t = [torch.zeros(P * w, device=DEV) for w in (3, 3, 3 * (M - 1), 1, 3, 4, 1, 1, 1, 1)]
    p = [x.data_ptr() for x in t]
    rows = torch.zeros(P * stride, dtype=torch.uint8, device=DEV)
    off = torch.arange(0, stride, 4, dtype=torch.int32, device=DEV)
    code = torch.zeros(A, dtype=torch.int32, device=DEV)
    st = _abi.stream(DEV)

    def unpack(stride=stride, off=off, code=code, rows_ptr=rows.data_ptr(), P=P):
        return L.gsr_model_unpack_rows(P, M, G, stride, rows_ptr, off.data_ptr(), code.data_ptr(), *p, st)

    assert unpack() == 0
    past = off.clone()
    past[A - 1] = stride - 3  # (a float that ends one byte past the row)
    assert unpack(off=past) != 0 and b"past `stride`" in L.gsr_last_error()
    dbl = code.clone()
    dbl[A - 1] = 1  # (the last column as a double: 8 bytes from stride - 4)
    assert unpack(code=dbl) != 0 and b"past `stride`" in L.gsr_last_error()
    assert unpack(stride=stride - 1) != 0
    normals = off.clone()
    normals[3:6] = torch.tensor([-7, stride, 1 << 30], dtype=torch.int32)  # (nx ny nz: entries ignored)
    assert unpack(off=normals) == 0
    bad = code.clone()
    bad[2] = 2
    assert unpack(code=bad) != 0 and b"type" in L.gsr_last_error()
    assert unpack(rows_ptr=rows.data_ptr() + 4) != 0 and b"aligned" in L.gsr_last_error()
    assert unpack(rows_ptr=None) != 0 and unpack(P=-1) != 0 and unpack(stride=0) != 0
    assert unpack(stride=40000) != 0 and b"tile" in L.gsr_last_error()
    assert unpack(P=0, rows_ptr=None) == 0
    out = torch.zeros(P * A, device=DEV)
    assert L.gsr_model_pack_rows(P, M, G, *p, out.data_ptr(), st) == 0
    assert L.gsr_model_pack_rows(P, M, G, *p, None, st) != 0
    assert L.gsr_model_pack_rows(P, M, G, None, *p[1:], out.data_ptr(), st) != 0 and b"`xyz`" in L.gsr_last_error()
    assert L.gsr_model_pack_rows(-1, M, G, *p, out.data_ptr(), st) != 0
    assert L.gsr_model_pack_rows(P, 0, G, *p, out.data_ptr(), st) != 0
    assert L.gsr_model_pack_rows(P, M, 2000, *p, out.data_ptr(), st) != 0 and b"tile" in L.gsr_last_error()
    assert L.gsr_model_pack_rows(0, M, G, *([None] * 11), st) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the model directory
def test_model_directory_and_render(tmp_path):
    import gsr_scene as S
    from gaussian_renderer import render
    from gsr_train import TrainGaussians, _Pipe, orbit_views

    gm = _gm()
    raw = S.make_gaussians(500, sh_degree=3, sg_degree=0, aspect=48 / 64).to(DEV)
    early = S.RawGaussians(*[getattr(raw, f) * 0.5 for f in raw.__dataclass_fields__])
    root = str(tmp_path / "out")
    gm.save_model(early, root, 7)
    path = gm.save_model(TrainGaussians(raw), root, 30)  # (a TrainGaussians and a RawGaussians are both taken)
    assert path == os.path.join(root, "point_cloud", "iteration_30", "point_cloud.ply") and os.path.isfile(path)
    got, it = gm.load_model(root, -1, device=DEV)
    assert it == 30
    for f in raw.__dataclass_fields__:
        assert torch.equal(getattr(got, f).view(torch.int32), getattr(raw, f).view(torch.int32)), f
    got7, it7 = gm.load_model(root, 7, device=DEV)
    assert it7 == 7 and torch.equal(got7.xyz, early.xyz)
    view = orbit_views(1, 64, 48, DEV)[0]
    with torch.no_grad():
        img = render(view, TrainGaussians(got), _Pipe(), torch.zeros(3, device=DEV), 0.0, require_depth=False)["render"]
    assert img.shape == (3, 48, 64) and bool(torch.isfinite(img).all()) and float(img.abs().sum()) > 0


# ------------------------------------------------------------------ resume
def _grads(g, seed):
    """Fixed synthetic gradients for every parameter of the optimizer (the raster backward's float atomics
    make real gradients differ from run to run; FusedAdam is elementwise and does not)."""
    gen = torch.Generator().manual_seed(seed)
    for group in g.optimizer.param_groups:
        for p in group["params"]:
            p.grad = (torch.randn(p.shape, generator=gen) * 1e-3).to(p.device)


def _step(g, seed, iteration):
    _grads(g, seed)
    g.update_learning_rate(iteration)
    g.optimizer.step()
    g.optimizer.zero_grad(set_to_none=True)


def _snapshot(g):
    out = {"filter_3D": g.filter_3D, "max_radii2D": g.max_radii2D, "xyz_gradient_accum": g.xyz_gradient_accum,
           "xyz_gradient_accum_abs": g.xyz_gradient_accum_abs, "denom": g.denom}
    groups = []
    for group in g.optimizer.param_groups:
        groups.append((group["name"], group["lr"]))
        for n, p in enumerate(group["params"]):
            st = g.optimizer.state[p]
            out[f"{group['name']}.{n}"] = p.detach()
            out[f"{group['name']}.{n}.exp_avg"] = st["exp_avg"]
            out[f"{group['name']}.{n}.exp_avg_sq"] = st["exp_avg_sq"]
            out[f"{group['name']}.{n}.step"] = st["step"]
    return groups, out


def test_resume_from_checkpoint_is_bit_equal(tmp_path):
    import gsr_train

    gm = _gm()
    step, view, nearest = gsr_train.synthetic_training_setup(300, 64, 48, sh_degree=1, sg_degree=2, device="cuda",
                                                             seed=5)
    a = step.g
    a.create_app_model(2, "gs", lr={"gs_final": 0.002, "iterations": 100})
    a.compute_3D_filter([view, nearest])
    gen = torch.Generator().manual_seed(11)
    a.denom = torch.full((300, 1), 4.0, device=DEV)
    a.xyz_gradient_accum = (torch.rand(300, 1, generator=gen) * 0.004).to(DEV)  # mean gradient up to 0.001
    a.xyz_gradient_accum_abs = (torch.rand(300, 1, generator=gen) * 0.008).to(DEV)
    a.max_radii2D = (torch.rand(300, generator=gen) * 20).to(DEV)
    for it in (1, 2, 3):
        _step(a, 100 + it, it)
    path = str(tmp_path / "chkpnt3.pth")
    gm.save_checkpoint(a, 3, path)
    state, it = torch.load(path, weights_only=True)  # plain data only
    assert it == 3 and len(state) == 23

    def continue_(g, noise):
        for it in (4, 5):
            _step(g, 100 + it, it)
        kw = {"noise": noise} if noise is not None else {"generator": torch.Generator().manual_seed(1)}
        return g.densify_and_prune(0.0002, 0.05, 4.0, None, **kw)

    probe, it = gm.load_checkpoint(path, device=DEV)  # (only to learn how many rows of noise the plan wants)
    assert it == 3
    C, S, _ = continue_(probe, None)
    assert C + S > 0
    noise = torch.randn(C + 2 * S, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    b, _ = gm.load_checkpoint(path, device=DEV)
    for attr in ("_xyz", "_features_rest", "_sg_color", "_appearance_embeddings"):
        p = getattr(b, attr)
        assert p.is_leaf and p.requires_grad and p.data_ptr() != getattr(a, attr).data_ptr()
    assert b.app_model is a.app_model and b.percent_dense == a.percent_dense
    assert b.spatial_lr_scale == a.spatial_lr_scale and b._app_lr == a._app_lr
    assert continue_(a, noise) == continue_(b, noise) == (C, S, probe.last_densify["pruned"])
    groups_a, snap_a = _snapshot(a)
    groups_b, snap_b = _snapshot(b)
    assert groups_a == groups_b and [n for n, _ in groups_a][-1] == "appearance_embeddings"
    assert groups_a[-1][1] == a.exposure_scheduler_args(5) != gsr_train.TrainGaussians.APP_LR["gs_init"]
    assert snap_a.keys() == snap_b.keys()
    for k in snap_a:
        x, y = snap_a[k], snap_b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, k
        assert torch.equal(x.cpu().contiguous().view(torch.int32), y.cpu().contiguous().view(torch.int32)), k
    assert snap_a["xyz.0"].shape[0] == 300 + C + S - probe.last_densify["pruned"]
    # training goes on from the restored model
    b.compute_3D_filter([view, nearest])
    loss = gsr_train.TrainStep(b, fused_rgb_loss=True).step(view, nearest)
    assert math.isfinite(float(loss))
