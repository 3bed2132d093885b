"""CPU tests of tests/viewgrads_ref.py, the float64 reference of
view_color_grads_kernel (csrc/view_grads.hip): the rebuilt rows are the
autograd gradients of the forward's colour model, the two layout packers
round-trip, and the tolerance constants C_KIND still cover the float32
restatement on every input family of tests/test_gpu_viewgrads.py."""
import numpy as np
import pytest
import torch

import viewgrads_ref as VR


def _autograd_rows(inp, sh_degree, SHM, sg_degree, SGM):
    """Gradients of sum_v sum(rgb_v * dR_v) in float64 torch, with the colour model of preprocess_fwd.hip /
    oracle color_from_shsg: rgb = sum_k Y_k(d) sh_k + sum_l sg_color_l exp(lambda_l (a_l . d - 1)) + 0.5, the SG
    axis as given (un-normalised), the direction d = normalize(mean - campos) detached."""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))  # noqa: E731
    g = torch.Generator().manual_seed(1)
    P = inp["means3D"].shape[0]
    shs = torch.randn(P, SHM, 3, dtype=torch.float64, generator=g).requires_grad_(True)
    axis = t(inp["sg_axis"]).requires_grad_(True)
    lam = t(inp["sg_sharpness"]).requires_grad_(True)
    col = t(inp["sg_color"]).requires_grad_(True)
    means, rows, campos = t(inp["means3D"]), t(inp["rows"]), t(inp["campos"])
    n = (sh_degree + 1) ** 2
    loss = torch.zeros((), dtype=torch.float64)
    for v in range(rows.shape[0]):
        do = means - campos[v]
        d = (do / do.norm(dim=1, keepdim=True)).detach()
        Y, _ = VR.sh_basis(d[:, 0], d[:, 1], d[:, 2], sh_degree)
        rgb = sum(Y[k][:, None] * shs[:, k] for k in range(n)) + 0.5
        for l in range(sg_degree):
            rgb = rgb + col[:, l] * torch.exp(lam[:, l] * ((axis[:, l] * d).sum(1) - 1.0))[:, None]
        loss = loss + (rgb * (rows[v] / VR.SH_C0)).sum()
    loss.backward()
    z = torch.zeros_like
    return {"sh": shs.grad, "sg_axis": axis.grad if axis.grad is not None else z(axis),
            "sg_sharpness": lam.grad if lam.grad is not None else z(lam),
            "sg_color": col.grad if col.grad is not None else z(col)}


@pytest.mark.parametrize("sg_degree", [0, 3, 7])
@pytest.mark.parametrize("sh_degree", [0, 1, 2, 3])
def test_rebuild_is_the_colour_model_s_gradient(sh_degree, sg_degree):
    """rebuild(float64) equals, to 1e-12 relative per element, the autograd gradients of the forward's colour
    model summed over the views; rows past the active degrees are zero in both."""
    P, n_views, SHM, SGM = 40, 3, 16, 7
    inp = VR.make_inputs(P, n_views, SGM, seed=10 * sh_degree + sg_degree)
    got, _ = VR.rebuild(inp["rows"], inp["campos"], inp["means3D"], sh_degree, SHM, sg_degree, SGM, inp["sg_axis"],
                        inp["sg_sharpness"], inp["sg_color"], dtype=np.float64)
    want = _autograd_rows(inp, sh_degree, SHM, sg_degree, SGM)
    for kind in VR.KINDS:
        w = want[kind].numpy()
        assert got[kind].shape == w.shape, kind
        assert np.any(w) or kind != "sh"
        assert np.all(np.abs(got[kind] - w) <= 1e-12 * np.abs(w)), (kind, float(np.abs(got[kind] - w).max()))
    assert not got["sh"][:, (sh_degree + 1) ** 2:].any()
    for kind in VR.KINDS[1:]:
        assert not got[kind][:, sg_degree:].any(), kind
        assert sg_degree == 0 or got[kind][:, :sg_degree].any(), kind


@pytest.mark.parametrize("P,n_views,chunk", [(1, 1, 1), (13, 3, 1), (13, 3, 5), (13, 3, 13), (13, 3, 20), (512, 2, 256),
                                             (513, 2, 256), (0, 2, 4)])
def test_packers_round_trip(P, n_views, chunk):
    r = np.random.default_rng(P + chunk)
    rows = r.normal(size=(n_views, P, 3)).astype(np.float32)
    campos = r.normal(size=(n_views, 3)).astype(np.float32)
    flat = VR.pack_flat(rows, campos)
    assert flat.shape == (n_views * (3 * P + 4),) and flat.dtype == np.float32
    rows2, cam2 = VR.unpack_flat(flat, n_views, P)
    assert np.array_equal(rows2, rows) and np.array_equal(cam2, campos)
    gathered, cam4 = VR.pack_chunked(rows, campos, chunk)
    assert gathered.shape == (3 * n_views * P,) and cam4.shape == (n_views, 4)
    rows3, cam3 = VR.unpack_chunked(gathered, cam4, n_views, P, chunk)
    assert np.array_equal(rows3, rows) and np.array_equal(cam3, campos)
    # the layout itself, element by element (view_grads.hip's header): Gaussian i of view v in range [b, b + len)
    for i in range(0, P, max(1, P // 7)):
        b = i // chunk * chunk
        ln = min(chunk, P - b)
        for v in range(n_views):
            assert np.array_equal(gathered[3 * n_views * b + 3 * v * ln + 3 * (i - b):][:3], rows[v, i])
            assert np.array_equal(flat[v * (3 * P + 4) + 3 * i:][:3], rows[v, i])
    if chunk >= P:  # one range: the chunked layout is the views' rows one after the other
        assert np.array_equal(gathered, rows.reshape(-1))


def test_dc_sum_is_sequential_float32():
    rows = np.array([[[1.0, 1e8, -0.0]], [[2.0 ** -24, 1.0, -0.0]], [[2.0 ** -24, -1e8, 0.0]]], dtype=np.float32)
    got = VR.dc_sum_f32(rows)
    assert got.dtype == np.float32
    assert got.tolist() == [[1.0, 0.0, 0.0]]  # (1 + u) + u rounds to 1 twice; (1e8 + 1) - 1e8 = 0
    assert not np.signbit(got).any()


def _measure():
    """{kind: (worst |f32 - f64| / (2^-24 S), family)} over every input family."""
    worst = {k: (0.0, None) for k in VR.KINDS}
    for name in VR.FAMILIES:
        lo, _ = VR.family_rebuild(name, np.float32)
        hi, S = VR.family_rebuild(name, np.float64)
        for kind in VR.KINDS:
            assert lo[kind].dtype == np.float32 and hi[kind].dtype == np.float64
            if not hi[kind].size:
                continue
            err = np.abs(lo[kind].astype(np.float64) - hi[kind])
            assert np.all(err[S[kind] == 0.0] == 0.0), (name, kind)
            live = S[kind] > 0.0
            if live.any():
                c = float((err[live] / (VR.U * S[kind][live])).max())
                if c > worst[kind][0]:
                    worst[kind] = (c, name)
    return worst


def test_tolerance_constants_cover_the_float32_restatement():
    """C_KIND (the GPU tests' bar is 4 C_KIND 2^-24 S per element) is still at least the float32 restatement's
    worst error on the GPU tests' input families."""
    worst = _measure()
    for kind, (c, name) in worst.items():
        print(f"[c_kind] {kind}: {c:.3f} (family {name}); constant {VR.C_KIND[kind]}")
    for kind, (c, name) in worst.items():
        assert VR.C_KIND[kind] >= c, (kind, c, name)
