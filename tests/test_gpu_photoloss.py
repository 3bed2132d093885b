"""GPU tests of the fused photometric loss (csrc/photoloss.hip, gsr_loss) against the float64 restatement
tests/photoloss_ref.py: mask composite, the four appearance modes, L1 and "valid" SSIM, with the gradients
w.r.t. the image, the embedding and the gain.

Bars.  Values within 1e-6 absolute and dL/dimage within 1e-5 relative L2 (the project's SSIM bars,
tests/test_gpu_ssim.py); per pixel and for the embedding and gain gradients the float64 yardstick form
e_gpu <= 2 e_fp32 + floor (helpers.Yardstick), e_fp32 the error of the same restatement in fp32 torch.
PHOTO_FLOOR: the measured e_gpu where the fp32 restatement is exact, rounded up to a power of ten.
The figures are next to the constant.

Sign ties.  A pixel whose float64 |t - g| is below 1e-6 max(1, |g|) may take either sign: it is left out of the
per-pixel comparisons, and a sum over pixels (embedding gradient) gets the slack 2 sum_ties |term| / sum |term|.
The share of such pixels is asserted <= 0.1 % before anything is compared (expected about 1e-5 for these inputs).
"""
from __future__ import annotations

import pytest
import torch

import helpers as Hh
import photoloss_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# Measured on an MI355X over the parity and L1-only cases of this file (832 comparisons): none with e_fp32 == 0 had
# e_gpu > 0 (where the fp32 restatement is exact, e.g. the L1-only gradient of one rounded constant, so is the
# kernel), and the largest e_gpu anywhere was 1.8e-5 beside an e_fp32 of the same size.  The floor is therefore the
# one of the SSIM stencil this kernel shares (tests/test_gpu_ssim.py SSIM_FLOOR, measured 3.5e-8, rounded up).
PHOTO_FLOOR = 1e-7
LAM = 0.2
SHAPES = [(11, 11), (12, 33), (17, 33), (47, 95), (64, 96), (70, 100)]
L1_ONLY_SHAPES = [(1, 1), (5, 7)]
MODES = ["no", "gs", "pgsr", "gain"]
MASKS = ["none", "half", "ones", "zeros", "exact_half"]


def _pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(shape, generator=g)
    b = (a + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    return a, b


def _mask(kind, H, W):
    if kind == "none":
        return None
    if kind == "half":  # a cut across the tile seams: columns below W/2 + 1 and rows above 2 are inside
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        return ((xs <= W // 2) & (ys >= 2)).float()
    return torch.full((H, W), {"ones": 1.0, "zeros": 0.0, "exact_half": 0.5}[kind])


def _crop(H, W):
    if H >= 32 and W >= 32:  # the GOF centre crop
        Hc, Wc = H // 32 * 32, W // 32 * 32
        return ((H - Hc) // 2, (W - Wc) // 2, Hc, Wc)
    return (H // 4, W // 4, max(1, H - H // 2), max(1, W - W // 2))


def _params(mode, H, W, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    if mode == "gs":
        return {"embedding": torch.eye(3, 4) + 0.05 * torch.randn(3, 4, generator=g)}
    if mode == "pgsr":
        return {"embedding": 0.1 * torch.randn(2, generator=g)}
    if mode == "gain":
        crop = _crop(H, W)
        return {"gain": 0.5 + torch.rand(3, crop[2], crop[3], generator=g), "crop": crop}
    return {}


def _evaluate(kind, a, b, mode, mask, bg, params, lam=LAM, with_ssim=True, loss=lambda v: v):
    """{'vals': (loss, l1, ssim), 'image' / 'embedding' / 'gain': gradients} on the device ('gpu'), in fp32 torch
    or in float64 torch."""
    import gsr_loss

    cast = {"gpu": lambda t: t.to(DEV), "fp32": lambda t: t.clone(), "f64": lambda t: t.double()}[kind]
    x = cast(a).requires_grad_(True)
    leaves = {"image": x}
    kw = {"app_model": mode}
    for k, v in params.items():
        if k == "crop":
            kw[k] = v
        else:
            kw[k] = leaves[k] = cast(v).requires_grad_(True)
    m = None if mask is None else cast(mask)
    c = None if bg is None else cast(bg)
    if kind == "gpu":
        vals = (gsr_loss.rgb_loss(x, cast(b), mask=m, bg=c, lambda_dssim=lam, **kw) if with_ssim
                else (gsr_loss.l1_loss(x, cast(b), mask=m, bg=c, **kw),) * 2 + (torch.zeros((), device=DEV),))
    else:
        vals = R.rgb_loss(x, cast(b), mask=m, bg=c, lambda_dssim=lam, with_ssim=with_ssim, **kw)
    loss(vals[0]).backward()
    out = {"vals": tuple(float(v.detach()) for v in vals)}
    for k, t in leaves.items():
        assert torch.isfinite(t.grad).all(), (kind, k)
        out[k] = t.grad.detach().cpu().double()
    return out


def _ties(a, b, mode, mask, bg, params):
    """[3,H,W] bool: the pixels whose sign is open (float64 |t - g| < 1e-6 max(1, |g|)), spread to the entries of
    dL/dimage they reach (GS: the three channels of the pixel); and the same over the L1's region alone."""
    kw = {k: (v if k == "crop" else v.double()) for k, v in params.items()}
    m = None if mask is None else mask.double()
    c = None if bg is None else bg.double()
    d = R.l1_terms(a.double(), b.double(), mask=m, bg=c, app_model=mode, **kw)
    g = R.composite(b.double(), m, c)
    top, left, Hc, Wc = params.get("crop", (0, 0) + tuple(a.shape[-2:]))
    open_ = d.abs() < 1e-6 * g[:, top:top + Hc, left:left + Wc].abs().clamp_min(1.0)
    share = float(open_.float().mean())
    assert share <= 1e-3, share  # the cap, before anything is compared
    full = torch.zeros(a.shape, dtype=torch.bool)
    full[:, top:top + Hc, left:left + Wc] = open_.any(dim=0, keepdim=True).expand_as(open_) if mode == "gs" else open_
    return full, open_


def _bands(H, W):
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    border = (ys < 5) | (ys >= H - 5) | (xs < 5) | (xs >= W - 5)
    seam = torch.zeros(H, W, dtype=torch.bool)
    for s in range(32, W, 32):
        seam |= (xs >= s - 5) & (xs < s + 5)
    for s in range(16, H, 16):
        seam |= (ys >= s - 5) & (ys < s + 5)
    seam &= ~border
    return border, seam, ~border & ~seam


def _emb_scale_and_slack(a, b, mode, mask, bg, params, open_, count_scale):
    """Per embedding entry, (1 - lambda)/N sum |term| and the ties' slack 2 sum_ties |term| / sum |term|."""
    x = a.double()
    ones = torch.ones_like(x[0])
    if mode == "gs":  # E[c,k]: sign_c x_k, E[c,3]: sign_c
        terms = [[x[k].abs() for k in range(3)] + [ones] for _ in range(3)]
        tie = [open_[c] for c in range(3) for _ in range(4)]
        flat = [t for row in terms for t in row]
    else:  # e0: sign_c exp(e0) x_c summed over c, e1: sign_c
        e0 = float(torch.exp(params["embedding"][0].double()))
        flat = [(e0 * x).abs(), torch.ones_like(x)]
        tie = [open_, open_]
    scale = torch.tensor([float(t.sum()) for t in flat]) * count_scale
    slack = torch.tensor([float(t[m].sum()) / max(float(t.sum()), 1e-300) * 2.0 for t, m in zip(flat, tie)])
    return scale, slack


def _compare(what, a, b, mode, mask, bg, params, lam=LAM, with_ssim=True, loss=lambda v: v, values=True):
    H, W = a.shape[-2:]
    full_ties, open_ = _ties(a, b, mode, mask, bg, params)
    gpu, f32, f64 = (_evaluate(k, a, b, mode, mask, bg, params, lam, with_ssim, loss) for k in ("gpu", "fp32", "f64"))
    if values:
        for name, v, r in zip(("loss", "l1", "ssim"), gpu["vals"], f64["vals"]):
            assert abs(v - r) <= 1e-6, (what, name, v, r)
    g, g32, gr = (torch.where(full_ties, torch.zeros(()).double(), t["image"]) for t in (gpu, f32, f64))
    if float(gr.norm()) > 0 and values:
        assert float((g - gr).norm() / gr.norm()) <= 1e-5, what
    scale = max(float(gr.abs().max()), 1e-300)
    yard = Hh.Yardstick(what)
    for name, band in zip(("border", "seam", "rest"), _bands(H, W)):
        if int(band.sum()):
            yard.add(name, float((g - gr)[:, band].abs().max()) / scale, float((g32 - gr)[:, band].abs().max()) / scale,
                     PHOTO_FLOOR)
    if "embedding" in params:
        n_l1 = 3 * H * W
        lam_eff = lam if with_ssim else 0.0
        v = torch.tensor(f64["vals"][0], dtype=torch.float64, requires_grad=True)
        loss(v).backward()
        up = abs(float(v.grad))
        sc, slack = _emb_scale_and_slack(a, b, mode, mask, bg, params, open_, up * (1.0 - lam_eff) / n_l1)
        eg = ((gpu["embedding"] - f64["embedding"]).flatten().abs() / sc - slack).clamp_min(0.0)
        e32 = (f32["embedding"] - f64["embedding"]).flatten().abs() / sc
        yard.add("embedding", float(eg.max()), float(e32.max()), PHOTO_FLOOR)
    if "gain" in params:
        keep = ~open_
        gs = max(float(f64["gain"].abs().max()), 1e-300)
        yard.add("gain", float((gpu["gain"] - f64["gain"])[keep].abs().max()) / gs,
                 float((f32["gain"] - f64["gain"])[keep].abs().max()) / gs, PHOTO_FLOOR)
    yard.check()


# ------------------------------------------------------------------ 1-3: parity, ties, embedding and gain gradients
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_parity_per_mode_mask_background(H, W, mode):
    a, b = _pair((3, H, W), 11)
    params = _params(mode, H, W, 11)
    for kind in MASKS:
        for bg in (torch.zeros(3), torch.ones(3)):
            if kind == "none" and float(bg[0]) == 1.0:
                continue  # (no mask: the background is not read)
            _compare(f"photo {mode} {H}x{W} mask={kind} bg={float(bg[0]):.0f}", a, b, mode, _mask(kind, H, W), bg, params)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H,W", L1_ONLY_SHAPES + [(47, 95)])
def test_l1_only_switch(H, W, mode):
    a, b = _pair((3, H, W), 12)
    params = _params(mode, H, W, 12)
    for kind in ("none", "half"):
        _compare(f"photo l1-only {mode} {H}x{W} mask={kind}", a, b, mode, _mask(kind, H, W), torch.ones(3), params,
                 with_ssim=False)


# ------------------------------------------------------------------ 4: exactness where it is owed
def _gpu(a, b, grad=True, l1_only=False, **kw):
    import gsr_loss

    x = a.to(DEV).requires_grad_(grad)
    kw = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}
    if l1_only:
        vals = (gsr_loss.l1_loss(x, b.to(DEV), **kw),)
    else:
        vals = gsr_loss.rgb_loss(x, b.to(DEV), **kw)
    if grad:
        vals[0].backward()
    return tuple(v.detach().clone() for v in vals), x.grad


def test_identity_embeddings_equal_mode_no_bit_for_bit():
    a, b = _pair((3, 47, 95), 13)
    (v0, g0) = _gpu(a, b)
    for mode, emb in (("pgsr", torch.zeros(2)), ("gs", torch.eye(3, 4))):
        v, g = _gpu(a, b, app_model=mode, embedding=emb)
        assert torch.equal(v[1], v0[1]) and torch.equal(g, g0), mode


def test_image_equal_to_ground_truth_has_zero_l1_half():
    import gsr_loss

    a, _ = _pair((3, 47, 95), 14)
    for mode in MODES:
        params = _params(mode, 47, 95, 14)
        if mode == "gs":
            params["embedding"] = torch.eye(3, 4)
        if mode == "pgsr":
            params["embedding"] = torch.zeros(2)
        if mode == "gain":
            params["gain"] = torch.ones_like(params["gain"])
        x = a.to(DEV).requires_grad_(True)
        leaves = {k: v.to(DEV).requires_grad_(True) for k, v in params.items() if k != "crop"}
        l1 = gsr_loss.l1_loss(x, a.to(DEV), app_model=mode, crop=params.get("crop"), **leaves)
        l1.backward()
        assert float(l1.detach()) == 0.0 and not x.grad.any(), mode
        for k, t in leaves.items():
            assert not t.grad.any(), (mode, k)
        # the full call: l1 == 0, and the gradient is the SSIM half alone
        x2 = a.to(DEV).requires_grad_(True)
        v = gsr_loss.rgb_loss(x2, a.to(DEV), app_model=mode, crop=params.get("crop"),
                              **{k: t.detach() for k, t in leaves.items()})
        v[0].backward()
        x3 = a.to(DEV).requires_grad_(True)
        gsr_loss.rgb_loss(x3, a.to(DEV))[0].backward()
        assert float(v[1]) == 0.0 and torch.equal(x2.grad, x3.grad), mode


def test_mask_of_ones_is_no_mask_and_mask_of_zeros_is_the_background():
    a, b = _pair((3, 47, 95), 15)
    bg = torch.tensor([0.25, 1.0, 0.0])
    for mode in MODES:
        params = _params(mode, 47, 95, 15)
        v0, g0 = _gpu(a, b, app_model=mode, **params)
        v1, g1 = _gpu(a, b, app_model=mode, mask=torch.ones(47, 95), bg=bg, **params)
        assert all(torch.equal(p, q) for p, q in zip(v0, v1)) and torch.equal(g0, g1), mode
        v2, g2 = _gpu(a, b, app_model=mode, mask=torch.zeros(47, 95), bg=bg, **params)
        v3, g3 = _gpu(a, bg.view(3, 1, 1).expand(3, 47, 95).contiguous(), app_model=mode, **params)
        assert all(torch.equal(p, q) for p, q in zip(v2, v3)) and torch.equal(g2, g3), mode


# ------------------------------------------------------------------ 5: consistency with what exists
def test_ssim_equals_fused_ssim_bit_for_bit():
    import fused_ssim as FS

    a, b = _pair((3, 47, 95), 16)
    v, _ = _gpu(a, b, lambda_dssim=0.2)
    s = FS.fused_ssim(a.to(DEV).unsqueeze(0), b.to(DEV).unsqueeze(0), padding="valid")
    assert torch.equal(v[2], s.detach())


def test_lambda_one_gradient_equals_fused_ssim_gradient_bit_for_bit():
    """The backward spells out the roundings of ssim_bwd_kernel (csrc/photoloss.hip), so with lambda = 1, where the
    L1 half is exactly zero, the two gradients are the same bits."""
    import fused_ssim as FS

    a, b = _pair((3, 47, 95), 16)
    x = a.to(DEV).requires_grad_(True)
    (1.0 - FS.fused_ssim(x.unsqueeze(0), b.to(DEV).unsqueeze(0), padding="valid")).backward()
    _, g1 = _gpu(a, b, lambda_dssim=1.0)
    print("[photo] lambda=1 gradient against 1 - fused_ssim: max |diff| / max |g| =",
          float((g1 - x.grad).abs().max() / x.grad.abs().max()))
    assert torch.equal(g1, x.grad)


def test_l1_only_equals_full_call_l1_bit_for_bit():
    a, b = _pair((3, 47, 95), 16)
    for mode in MODES:
        params = _params(mode, 47, 95, 16)
        m = _mask("half", 47, 95)
        full, _ = _gpu(a, b, grad=False, app_model=mode, mask=m, **params)
        only, _ = _gpu(a, b, grad=False, l1_only=True, app_model=mode, mask=m, **params)
        assert torch.equal(full[1], only[0]), mode


# ------------------------------------------------------------------ 6: determinism and layouts
def test_deterministic():
    a, b = _pair((3, 47, 95), 17)
    for mode in MODES:
        params = _params(mode, 47, 95, 17)
        runs = []
        for _ in range(2):
            import gsr_loss

            x = a.to(DEV).requires_grad_(True)
            leaves = {k: v.to(DEV).requires_grad_(True) for k, v in params.items() if k != "crop"}
            v = gsr_loss.rgb_loss(x, b.to(DEV), mask=_mask("half", 47, 95).to(DEV), app_model=mode,
                                  crop=params.get("crop"), **leaves)
            v[0].backward()
            runs.append([t.detach() for t in v] + [x.grad] + [t.grad for t in leaves.values()])
        assert all(torch.equal(p, q) for p, q in zip(*runs)), mode


def test_layouts():
    import gsr_loss

    H, W = 37, 53
    a, b = _pair((3, H, W), 18)
    a, b = a.to(DEV), b.to(DEV)
    e = torch.tensor([0.05, -0.02], device=DEV)

    def run(leaf, view):
        v = gsr_loss.rgb_loss(view, b, app_model="pgsr", embedding=e)
        v[0].backward()
        g, leaf.grad = leaf.grad, None
        return [t.detach() for t in v], g

    x = a.clone().requires_grad_(True)
    want_v, want_g = run(x, x)
    same = lambda v: all(torch.equal(p, q) for p, q in zip(v, want_v))  # noqa: E731
    x4 = a[None].clone().requires_grad_(True)  # [1,3,H,W]
    v, g = run(x4, x4)
    assert same(v) and torch.equal(g[0], want_g)
    cl = a.permute(1, 2, 0).contiguous().requires_grad_(True)  # channels last
    view = cl.permute(2, 0, 1)
    assert not view.is_contiguous()
    v, g = run(cl, view)
    assert same(v) and torch.equal(g.permute(2, 0, 1), want_g)
    big = torch.full((3, H + 5, W + 5), 9.0, device=DEV)  # a crop of a larger tensor
    big[:, 3:-2, 1:-4] = a
    big.requires_grad_(True)
    v, g = run(big, big[:, 3:-2, 1:-4])
    assert same(v) and torch.equal(g[:, 3:-2, 1:-4], want_g) and not g[:, :3].any()
    flat = torch.zeros(a.numel() + 1, device=DEV)  # 4 bytes off a 16-byte boundary
    flat[1:] = a.flatten()
    flat.requires_grad_(True)
    view = flat[1:].view(a.shape)
    assert view.data_ptr() % 16 == 4
    v, g = run(flat, view)
    assert same(v) and torch.equal(g[1:].view(a.shape), want_g)


# ------------------------------------------------------------------ 7: upstream gradients
@pytest.mark.parametrize("case", ["w=-3", "w=1e-6", "squared"])
@pytest.mark.parametrize("mode", MODES)
def test_upstream_gradient(mode, case):
    loss = (lambda v: v ** 2) if case == "squared" else (lambda v: float(case[2:]) * v)
    a, b = _pair((3, 37, 53), 19)
    _compare(f"photo upstream {mode} {case}", a, b, mode, _mask("half", 37, 53), torch.ones(3), _params(mode, 37, 53, 19),
             loss=loss, values=False)


# ------------------------------------------------------------------ 8: argument errors
def test_argument_errors():
    import gsr_loss

    a, b = _pair((3, 37, 53), 20)
    a, b = a.to(DEV), b.to(DEV)
    torch.cuda.synchronize()
    gain = torch.ones(3, 32, 32, device=DEV)
    bad = [dict(app_model=7), dict(app_model="gs"), dict(app_model="pgsr"), dict(app_model="gain", crop=(0, 0, 32, 32)),
           dict(app_model="gain", gain=gain, crop=(6, 0, 32, 32)), dict(app_model="gain", gain=gain, crop=(0, 22, 32, 32)),
           dict(app_model="gain", gain=gain, crop=(-1, 0, 32, 32))]
    for kw in bad:
        with pytest.raises(RuntimeError):
            gsr_loss.rgb_loss(a, b, **kw)
    for H, W in ((10, 40), (40, 10)):
        s, t = _pair((3, H, W), 21)
        with pytest.raises(RuntimeError):
            gsr_loss.rgb_loss(s.to(DEV), t.to(DEV))
        assert float(gsr_loss.l1_loss(s.to(DEV), t.to(DEV))) > 0  # the L1-only switch takes any size
    torch.cuda.synchronize()  # (nothing was launched that could fault)


# ------------------------------------------------------------------ 9: the training step
def _rel(x, y):
    return float((x.double() - y.double()).norm() / max(float(y.double().norm()), 1e-30))


def test_train_step_fused_rgb_loss_matches_unfused():
    import gsr_train

    res = []
    for fused in (True, False):
        step, view, nearest = gsr_train.synthetic_training_setup(300, 64, 48, seed=5)
        step = gsr_train.TrainStep(step.g, fused_rgb_loss=fused)
        loss = float(step.step(view, nearest))
        res.append((loss, {k: p.detach().clone() for k, p in step.g.named_parameters()}))
    (l1, p1), (l0, p0) = res
    assert abs(l1 - l0) <= 1e-5 * abs(l0), (l1, l0)
    for k in p0:
        assert _rel(p1[k], p0[k]) <= 1e-3, (k, _rel(p1[k], p0[k]))


def test_train_step_pgsr_with_mask():
    import gsr_loss
    import gsr_train

    step, view, nearest = gsr_train.synthetic_training_setup(300, 64, 48, seed=5)
    g = step.g
    g.create_app_model(8, "pgsr")
    with pytest.raises(RuntimeError):
        gsr_train.TrainStep(g)  # an appearance model without the fused loss
    H, W = view.image_height, view.image_width
    view.gt_mask = _mask("half", H, W).to(DEV)
    view.uid = 3
    bg = torch.tensor([1.0, 1.0, 1.0], device=DEV)
    step = gsr_train.TrainStep(g, bg=bg, fused_rgb_loss=True)
    seen = {}
    real = gsr_loss.rgb_loss

    def spy(image, gt, **kw):  # the rendered image and the loss of the first call
        out = real(image, gt, **kw)
        seen.setdefault("call", (image.detach().cpu().double(), kw["embedding"].detach().cpu().double(), float(out[0].detach())))
        return out

    gsr_loss.rgb_loss = spy
    try:
        losses = [float(step.step(view, nearest)) for _ in range(3)]
    finally:
        gsr_loss.rgb_loss = real
    assert all(torch.isfinite(torch.tensor(losses)))
    img, emb, got = seen["call"]
    want = R.rgb_loss(img, view.original_image.cpu().double(), mask=view.gt_mask.cpu().double(), bg=bg.cpu().double(),
                      app_model="pgsr", embedding=emb, lambda_dssim=gsr_train.LAMBDA_DSSIM)[0]
    assert abs(got - float(want)) <= 1e-6, (got, float(want))
    e = g._appearance_embeddings.detach()
    others = [k for k in range(8) if k != 3]
    assert e[3].abs().min() > 0 and not e[others].any()
    st = g.optimizer.state[g._appearance_embeddings]
    assert not st["exp_avg"][others].any() and not st["exp_avg_sq"][others].any()
    before = e.clone()
    g.densify_and_prune(0.0002, 0.005, 5.0, None)
    assert torch.equal(g._appearance_embeddings.detach(), before)
    names = [gr["name"] for gr in g.optimizer.param_groups]
    assert names.count("appearance_embeddings") == 1 and g.optimizer.param_groups[-1]["params"][0] is g._appearance_embeddings
    # a masked view without the fused loss is refused too
    step, view, nearest = gsr_train.synthetic_training_setup(300, 64, 48, seed=5)
    view.gt_mask = _mask("half", H, W).to(DEV)
    with pytest.raises(RuntimeError):
        step.step(view, nearest)


def test_fused_adam_takes_embedding_rows_and_conv_weights():
    """create_app_model's groups: a [num_cameras, 2] parameter, 4-D convolution weights (with a gradient that is
    not contiguous) and the 16-parameter chunking, against torch.optim.Adam."""
    import gsr_loss
    from gsr_optim import FusedAdam

    torch.manual_seed(0)
    nets = [gsr_loss.AppearanceNetwork(67, 3).to(DEV) for _ in range(2)]
    nets[1].load_state_dict(nets[0].state_dict())
    embs = [torch.nn.Parameter(torch.zeros(8, 2, device=DEV)) for _ in range(2)]
    opts = [cls([{"params": [e], "lr": 1e-3, "name": "appearance_embeddings"},
                 {"params": list(n.parameters()), "lr": 1e-3, "name": "appearance_network"}], lr=0.0, eps=1e-15)
            for cls, e, n in ((FusedAdam, embs[0], nets[0]), (torch.optim.Adam, embs[1], nets[1]))]
    gen = torch.Generator(device="cpu").manual_seed(1)
    for _ in range(2):
        grads = [torch.randn(p.shape, generator=gen).to(DEV) for p in nets[0].parameters()]
        ge = torch.zeros(8, 2, device=DEV)
        ge[3] = torch.tensor([0.5, -2.0], device=DEV)
        for e, n in zip(embs, nets):
            e.grad = ge.clone()
            for p, gr in zip(n.parameters(), grads):
                p.grad = gr.clone()
        w = nets[0].conv2.weight
        w.grad = w.grad.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)  # same values, not contiguous
        assert not w.grad.is_contiguous()
        for o in opts:
            o.step()
    assert _rel(embs[0], embs[1]) <= 1e-6 and not embs[0][[0, 1, 2, 4, 5, 6, 7]].any()
    for p, q in zip(nets[0].parameters(), nets[1].parameters()):
        assert _rel(p, q) <= 1e-6
