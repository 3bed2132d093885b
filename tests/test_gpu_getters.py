"""GPU tests of the activation getters (csrc/optim.hip scale_opacity_kernel,
normalize_rows_kernel) called directly through gsr_optim, values and
gradients, against tests/train_ref.py in float64.

Judged per row: a row's error is max|a - ref| over its elements / max|ref|
of that row (absolute where the row's reference is zero), so that a wrong
row is not hidden by the tensor's largest one.  Rows are built in kinds
(saturated or ordinary opacity logits x filter sizes; zero, tiny, huge and
ordinary quaternion rows); within a kind the rows are conditioned alike, and
the worst row of each kind (for scale_opacity: of each group of rows that are
conditioned alike, see test_scale_opacity_rows) is held to the float64 yardstick
(helpers.Yardstick): e_gpu <= 2 e_fp32 + GETTER_FLOOR, with the same getters
evaluated by torch in fp32 on the CPU as the yardstick.
"""
from __future__ import annotations

import pytest
import torch

import gsr_optim
import helpers as Hh
import train_ref as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# e_gpu measured for the groups whose fp32 yardstick is exact against float64, rounded up to a power of ten.
# Measured on an MI355X: in all 57 comparisons with e_fp32 == 0 (zero rows, dL/do without an upstream gradient
# on the opacity) e_gpu is 0 too, so the floor is 0.  Worst e_gpu / e_fp32 elsewhere: scale_opacity 1.37 (P = 4099,
# o = 5, f = 1e3 e^s, dL/ds: 2.44e-7 against 1.79e-7), normalize_rows 1.25 (D = 7, |x| = 1e18, dx: 3.64e-7 against
# 2.91e-7).  Split into all 24 opacity x filter kinds at P = 257, 11 rows a kind, the first measurement had opacity
# at o = 0, f = 1e3 e^s at 2.81e-7 against 0.98e-7, both under 3 fp32 ulps: too small a sample for a factor 2,
# hence the groups of test_scale_opacity_rows.
GETTER_FLOOR = 0.0

O_KINDS = (-30.0, -5.0, 0.0, 5.0, 30.0, None)  # None: random logits
F_KINDS = ("0", "1e-6 e^s", "e^s", "1e3 e^s")


def _so_inputs(P, seed):
    """s uniform in [-12, 3]; row i has opacity kind i % 6 and filter kind (i // 6) % 4: all 24 combinations."""
    g = torch.Generator().manual_seed(seed)
    s = torch.rand(P, 3, generator=g) * 15.0 - 12.0
    o = torch.randn(P, 1, generator=g) * 3.0
    i = torch.arange(P)
    for k, val in enumerate(O_KINDS):
        if val is not None:
            o[i % 6 == k] = val
    fk = (i // 6) % 4
    es = torch.exp(s[:, :1].double())
    f = (es * torch.tensor([0.0, 1e-6, 1.0, 1e3], dtype=torch.float64)[fk][:, None]).float()
    kind = (i % 6) * 4 + fk
    return s, o, f, kind


def _so_eval(fn, s, o, f, up_s, up_o):
    s, o = s.clone().requires_grad_(True), o.clone().requires_grad_(True)
    scales, op = fn(s, o, f)
    loss = 0.0
    if up_s is not None:
        loss = loss + (scales * up_s).sum()
    if up_o is not None:
        loss = loss + (op * up_o).sum()
    loss.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731  (an unused output's input)
    return scales.detach(), op.detach(), zero(s), zero(o)


def _by_kind(yard, name, kind, n_kinds, a_gpu, a_f32, ref, floor, labels, rows=None):
    """One yardstick comparison per kind: the worst row of the kind (among `rows`) on either side."""
    e_gpu, e_f32 = Hh.row_errs(a_gpu, ref), Hh.row_errs(a_f32, ref)
    for k in range(n_kinds):
        sel = (kind == k) if rows is None else (kind == k) & rows
        if int(sel.sum()):
            yard.add(f"{name}[{labels(k)}]", float(e_gpu[sel].max()), float(e_f32[sel].max()), floor)


def _scale_opacity_quotient(s, o, f):
    """train_ref.scale_opacity with the coefficient as sqrt(det1 / det2): in fp32 the reference's
    det1.sqrt() * det2.rsqrt() overflows in its backward (d rsqrt(x) = -x^-1.5 / 2 with x = det2 down to 5e-32
    for log-scales near -12, times det1's own 1 / (2 sqrt(det1))), this form does not."""
    q = torch.exp(s).square()
    a = q + f.square()
    return a.sqrt(), torch.sigmoid(o) * (q.prod(dim=1) / a.prod(dim=1)).sqrt()[:, None]


O_CLASS = ("fixed o", "o=30", "random o")  # alike in conditioning: 1 - sigmoid(o) cancels at 30, and for large random o


@pytest.mark.parametrize("upstream", ["both", "scales", "opacity"])
@pytest.mark.parametrize("P", [0, 1, 255, 256, 257, 4099])
def test_scale_opacity_rows(P, upstream):
    """Row errors, the worst row of a group of rows against the worst fp32 row of the same group.  The groups
    hold rows that are conditioned alike and, but for P = 1, at least 40 of them (with the 11 rows one of the 24
    kinds has at P = 257 the maxima of two equally good evaluations scatter by more than the factor 2; the 24
    kinds are judged one by one at P = 4099, 170 rows each):
      scales, opacity   one group (every row is a chain of exp, squares, products, sqrt);
      dL/do             by the opacity logit: the fixed ones below 30, 30, random;
      dL/ds             by the filter: 0, 1e-6 e^s (where autograd's 1 - q/a cancels in fp32), e^s, 1e3 e^s.
    Where the reference's own fp32 getter gives a non-finite dL/ds (its backward overflows for small scales
    whenever the opacity has an upstream gradient: 1 or 2 rows of 257, 35 of 4099; the float64 reference and the
    kernel stay finite), the row's yardstick is the quotient form of the same getter in fp32 instead, within the
    row's own group (one or two rows are no group of their own).  Where dL/ds is exactly 0 (f = 0 and no upstream
    gradient on the scales), the float64 autograd value is rounding noise around 1e-17: those rows are left out
    of the groups and the kernel must give exactly 0."""
    s, o, f, kind = _so_inputs(P, 20 + P)
    g = torch.Generator().manual_seed(21)
    up_s = torch.randn(P, 3, generator=g) if upstream in ("both", "scales") else None
    up_o = torch.randn(P, 1, generator=g) if upstream in ("both", "opacity") else None
    dbl = lambda t: None if t is None else t.double()  # noqa: E731
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    ref = _so_eval(T.scale_opacity, s.double(), o.double(), f.double(), dbl(up_s), dbl(up_o))
    f32 = _so_eval(T.scale_opacity, s, o, f, up_s, up_o)
    quo = _so_eval(_scale_opacity_quotient, s, o, f, up_s, up_o)
    gpu = tuple(t.cpu() for t in _so_eval(gsr_optim.scaling_n_opacity_with_3D_filter, s.to(DEV), o.to(DEV), f.to(DEV),
                                          dev(up_s), dev(up_o)))
    for name, a, r in zip(("scales", "opacity", "ds", "do"), gpu, ref):
        assert a.shape == r.shape and torch.isfinite(a).all() and torch.isfinite(r).all(), name
    for a in f32[:2] + f32[3:] + quo:
        assert torch.isfinite(a).all()
    o_kind, f_kind = kind // 4, kind % 4
    o_class = torch.where(o_kind == O_KINDS.index(30.0), 1, torch.where(o_kind == O_KINDS.index(None), 2, 0))
    overflow = ~torch.isfinite(f32[2]).all(dim=1)
    zero_ds = (f_kind == 0) if up_s is None else torch.zeros(P, dtype=torch.bool)
    print(f"[yard] scale_opacity P={P} upstream={upstream}: {int(overflow.sum())} rows overflow in the fp32 getter")
    assert torch.equal(gpu[2][zero_ds], torch.zeros(int(zero_ds.sum()), 3))
    assert float(ref[2][zero_ds].abs().max()) <= 1e-12 if int(zero_ds.sum()) else True
    yard = Hh.Yardstick(f"scale_opacity P={P} upstream={upstream}")
    one = torch.zeros(P, dtype=torch.long)
    label = lambda k: f"o={O_KINDS[k // 4]} f={F_KINDS[k % 4]}"  # noqa: E731
    ds_rows = ~zero_ds
    f32_ds = torch.where(overflow[:, None], quo[2], f32[2])
    _by_kind(yard, "scales", one, 1, gpu[0], f32[0], ref[0], GETTER_FLOOR, lambda k: "all")
    _by_kind(yard, "opacity", one, 1, gpu[1], f32[1], ref[1], GETTER_FLOOR, lambda k: "all")
    _by_kind(yard, "do", o_class, 3, gpu[3], f32[3], ref[3], GETTER_FLOOR, lambda k: O_CLASS[k])
    _by_kind(yard, "ds", f_kind, 4, gpu[2], f32_ds, ref[2], GETTER_FLOOR, lambda k: "f=" + F_KINDS[k], rows=ds_rows)
    if P >= 2400:
        for name, a, b, r in zip(("scales", "opacity", "do"), gpu[:2] + gpu[3:], f32[:2] + f32[3:], ref[:2] + ref[3:]):
            _by_kind(yard, name, kind, 24, a, b, r, GETTER_FLOOR, label)
        _by_kind(yard, "ds", kind, 24, gpu[2], f32_ds, ref[2], GETTER_FLOOR, label, rows=ds_rows)
    if P:
        yard.check()


def test_scale_opacity_non_contiguous_scaling():
    """A [:, :3] slice of a [P, 4] tensor: the wrapper's .contiguous() makes it right, bit for bit."""
    P = 257
    s, o, f, _ = _so_inputs(P, 22)
    up_s, up_o = torch.randn(P, 3, generator=torch.Generator().manual_seed(23)).to(DEV), torch.ones(P, 1, device=DEV)
    want = _so_eval(gsr_optim.scaling_n_opacity_with_3D_filter, s.to(DEV), o.to(DEV), f.to(DEV), up_s, up_o)
    wide = torch.cat([s, torch.full((P, 1), 1e30)], dim=1).to(DEV).requires_grad_(True)
    sl = wide[:, :3]
    assert not sl.is_contiguous()
    oo = o.to(DEV).requires_grad_(True)
    scales, op = gsr_optim.scaling_n_opacity_with_3D_filter(sl, oo, f.to(DEV))
    ((scales * up_s).sum() + (op * up_o).sum()).backward()
    assert torch.equal(scales, want[0]) and torch.equal(op, want[1])
    assert torch.equal(wide.grad[:, :3], want[2]) and torch.equal(oo.grad, want[3])
    assert torch.equal(wide.grad[:, 3], torch.zeros(P, device=DEV))


ROW_KINDS = ("random", "zero", "0.999e-12", "1.001e-12", "1e-13", "1e-11", "1e-30", "1e18", "1 and 1e-25")


def _rows(n, D, seed):
    """Row i is of kind i % 9.  The rows at the branch point of F.normalize (|x| = eps = 1e-12) lie 1e-3 to
    either side of it, 1e4 fp32 ulps, so that float64, fp32 and the kernel take the same branch."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, D, generator=g, dtype=torch.float64)
    x = torch.where(x.abs() < 0.05, 0.05, x)
    kind = torch.arange(n) % len(ROW_KINDS)
    unit = x / x.norm(dim=1, keepdim=True)
    for k, name in enumerate(ROW_KINDS):
        r = kind == k
        if name == "zero":
            x[r] = 0.0
        elif name == "1 and 1e-25":
            x[r] = 1e-25
            x[r, 0] = 1.0
        elif name != "random":
            x[r] = unit[r] * float(name)
    return x.float(), kind


def _nr_eval(fn, x, up):
    x = x.clone().requires_grad_(True)
    y = fn(x)
    (y * up).sum().backward()
    return y.detach(), x.grad


@pytest.mark.parametrize("n", [0, 1, 257])
@pytest.mark.parametrize("layout", ["D4", "D4_off4", "D1", "D3", "D7"])
def test_normalize_rows(layout, n):
    D = int(layout[1])
    x, kind = _rows(n, D, 30 + D)
    up = torch.randn(n, D, generator=torch.Generator().manual_seed(31))
    # float64 and fp32 take the same branch of max(|x|, eps) for every row (no row needs excluding)
    len64 = x.double().norm(dim=1)
    len32 = x.norm(dim=1)
    assert torch.equal(len64 > 1e-12, len32 > torch.tensor(1e-12, dtype=torch.float32))
    assert float(((len64 - 1e-12).abs() / 1e-12).min()) > 5e-4 if n else True
    ref = _nr_eval(T.normalize_rows, x.double(), up.double())
    f32 = _nr_eval(T.normalize_rows, x, up)
    if "off4" in layout:
        base = torch.zeros(4 * n + 1, device=DEV)
        base[1:] = x.flatten().to(DEV)
        base.requires_grad_(True)
        xv = base[1:].view(n, 4)
        assert n == 0 or xv.data_ptr() % 16 == 4  # contiguous, so the wrapper passes it on as it is
        y = gsr_optim.normalize_rows(xv)
        (y * up.to(DEV)).sum().backward()
        gpu = (y.detach(), base.grad[1:].view(n, 4))
        assert float(base.grad[0]) == 0.0
    else:
        gpu = _nr_eval(gsr_optim.normalize_rows, x.to(DEV), up.to(DEV))
        assert n == 0 or D != 4 or gpu[0].data_ptr() % 16 == 0
    yard = Hh.Yardstick(f"normalize_rows {layout} n={n}")
    for name, a, b, r in zip(("y", "dx"), gpu, f32, ref):
        assert a.shape == r.shape and torch.isfinite(a).all(), name
        _by_kind(yard, name, kind, len(ROW_KINDS), a.cpu(), b, r, GETTER_FLOOR, lambda k: ROW_KINDS[k])
    if n:
        yard.check()
