"""GPU tests of the training update (csrc/optim.hip):
FusedAdam against torch.optim.Adam (the reference's optimizer,
scene/gaussian_model.py:347-351) and the densification statistics against
the reference's own torch statements (gaussian_model.py:818-821,
train.py:236-237).  The oracle here is torch on the CPU, fp32.

Tolerances: Adam state and parameters max|a-b| <= 2e-6 * max|b| + 1e-12
(same fp32 formula, different rounding of sqrt/division); statistics exact
except the x/y norm (<= 1 ulp).

The edge tests below (grid-stride and group walk, mixed alignment, more than
16 parameters, separate batches, the eps = 1e-15 range, 300 steps) judge
FusedAdam in the float64 yardstick form instead (helpers.Yardstick): per
tensor, e = max|a - ref| / max|ref| against tests/train_ref.adam_step in
float64, and e_gpu <= 2 e_fp32 + ADAM_FLOOR with torch.optim.Adam in fp32 on
the CPU as the yardstick.
"""
from __future__ import annotations

import math

import pytest
import torch

import gsr_optim
import helpers as Hh
import train_ref as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# the Gaussian parameter groups of GaussianModel (xyz, f_dc, f_rest, opacity, scaling, rotation, sg_*)
SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,),
          "sg_axis": (7, 3), "sg_sharpness": (7,), "sg_color": (7, 3)}
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 5e-2, "scaling": 5e-3, "rotation": 1e-3,
       "sg_axis": 1e-3, "sg_sharpness": 1e-3, "sg_color": 1e-4}


def _groups(P, seed, device):
    g = torch.Generator().manual_seed(seed)
    return [{"params": [torch.nn.Parameter(torch.randn((P,) + s, generator=g).to(device))], "lr": LRS[k], "name": k}
            for k, s in SHAPES.items()]


def _pair(P, seed):
    ref = _groups(P, seed, "cpu")
    mine = _groups(P, seed, DEV)
    o_ref = torch.optim.Adam(ref, lr=0.0, eps=1e-15, foreach=False)
    o_mine = gsr_optim.FusedAdam(mine, lr=0.0, eps=1e-15)
    return ref, mine, o_ref, o_mine


def _close(a, b, rtol=2e-6):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max()) <= rtol * float(b.abs().max()) + 1e-12


@pytest.mark.parametrize("P", [1, 7, 10007])
def test_fused_adam_matches_torch_adam(P):
    ref, mine, o_ref, o_mine = _pair(P, 0)
    g = torch.Generator().manual_seed(1)
    for it in range(4):
        for gr, gm in zip(ref, mine):
            grad = torch.randn(gr["params"][0].shape, generator=g) * 10 ** (-it)
            if it == 2:
                grad[: max(1, P // 3)] = 0.0  # zero gradients still decay the moments
            gr["params"][0].grad = grad.clone()
            gm["params"][0].grad = grad.to(DEV)
        if it == 1:  # the reference's xyz learning-rate schedule edits param_groups in place
            for o in (o_ref, o_mine):
                for grp in o.param_groups:
                    if grp["name"] == "xyz":
                        grp["lr"] = 1.1e-4
        o_ref.step()
        o_mine.step()
        for gr, gm in zip(ref, mine):
            pr, pm = gr["params"][0], gm["params"][0]
            assert _close(pm, pr), (gr["name"], it)
            sr, sm = o_ref.state[pr], o_mine.state[pm]
            assert set(sm) == set(sr) and float(sm["step"]) == float(sr["step"])
            assert _close(sm["exp_avg"], sr["exp_avg"]) and _close(sm["exp_avg_sq"], sr["exp_avg_sq"])


def test_fused_adam_survives_densification_state_edits():
    """cat_tensors_to_optimizer / _prune_optimizer (gaussian_model.py) replace
    params and their exp_avg/exp_avg_sq in the state dict; the next step
    must use the new tensors (here: a pruned, non-16-B-aligned view too)."""
    ref, mine, o_ref, o_mine = _pair(1000, 2)
    for gr, gm in zip(ref, mine):
        gr["params"][0].grad = torch.ones_like(gr["params"][0]) * 0.1
        gm["params"][0].grad = torch.ones_like(gm["params"][0]) * 0.1
    o_ref.step()
    o_mine.step()
    keep = torch.arange(1000) % 3 != 0
    for o, dev in ((o_ref, "cpu"), (o_mine, DEV)):
        for grp in o.param_groups:
            old = grp["params"][0]
            st = o.state.pop(old)
            new = torch.nn.Parameter(old.detach()[keep.to(dev)].contiguous())
            st["exp_avg"] = st["exp_avg"][keep.to(dev)].contiguous()
            st["exp_avg_sq"] = st["exp_avg_sq"][keep.to(dev)].contiguous()
            grp["params"][0] = new
            o.state[new] = st
            new.grad = torch.full_like(new, -0.05)
    o_ref.step()
    o_mine.step()
    for gr, gm in zip(o_ref.param_groups, o_mine.param_groups):
        assert _close(gm["params"][0], gr["params"][0]), gr["name"]
    # an unaligned (offset-1) but contiguous parameter takes the scalar path
    base = torch.zeros(1001, device=DEV)
    p = torch.nn.Parameter(base[1:])
    o = gsr_optim.FusedAdam([p], lr=0.1)
    p.grad = torch.ones(1000, device=DEV)
    o.step()
    assert torch.allclose(p.detach(), torch.full((1000,), -0.1, device=DEV), rtol=1e-6)


def test_densify_stats_matches_reference_statements():
    P = 5003
    g = torch.Generator().manual_seed(3)
    vgrad = torch.randn(P, 3, generator=g)
    radii = torch.randint(-1, 4, (P,), generator=g, dtype=torch.int32)
    state = {k: torch.rand(P, 1, generator=g) for k in ("accum", "accum_abs", "denom")}
    max_r = torch.rand(P, generator=g) * 3
    # reference (train.py:236-237, gaussian_model.py:818-821), on CPU
    vis = radii > 0
    r_max = max_r.clone()
    r_max[vis] = torch.max(r_max[vis], radii[vis])
    r_acc, r_abs, r_den = state["accum"].clone(), state["accum_abs"].clone(), state["denom"].clone()
    r_acc[vis] += torch.norm(vgrad[vis, :2], dim=-1, keepdim=True)
    r_abs[vis] += torch.norm(vgrad[vis, 2:], dim=-1, keepdim=True)
    r_den[vis] += 1

    class G:
        pass

    gm = G()
    gm.max_radii2D = max_r.to(DEV)
    gm.xyz_gradient_accum, gm.xyz_gradient_accum_abs, gm.denom = (state[k].to(DEV) for k in ("accum", "accum_abs",
                                                                                               "denom"))
    vp = torch.zeros(P, 3, device=DEV, requires_grad=True)
    vp.grad = vgrad.to(DEV)
    gsr_optim.add_densification_stats(gm, vp, radii.to(DEV))
    assert torch.equal(gm.max_radii2D.cpu(), r_max)
    assert torch.equal(gm.denom.cpu(), r_den) and torch.equal(gm.xyz_gradient_accum_abs.cpu(), r_abs)
    assert torch.allclose(gm.xyz_gradient_accum.cpu(), r_acc, rtol=2e-7, atol=0)


# ---------------------------------------------------------------- edges, in the float64 yardstick form
# e_gpu measured where torch's fp32 Adam is exact against float64 (e_fp32 == 0), rounded up to a power of ten.
# Measured on an MI355X over the 411 comparisons below: in the 6 with e_fp32 == 0 (zero gradients and moments)
# e_gpu is 0 too, so the floor is 0 and those results are held to be exact.  Worst e_gpu / e_fp32 elsewhere: 1.10
# (300 steps, f_rest at t = 100: 3.36e-7 against 3.05e-7).  In the eps range the kernel and torch's fp32 agree to
# the printed digits on both moments (g = 1e-18, g^2 an fp32 denormal: exp_avg_sq 5.17e-7 both; g = 1e-22, g^2
# underflows: 1.0 both; preloaded 1e-38..1e-45: 2.18e-7 both): the kernel keeps fp32 denormals as the CPU does.
ADAM_FLOOR = 0.0


class Trio:
    """The same Adam run three ways: tests/train_ref.adam_step in float64 (the reference), torch.optim.Adam in
    fp32 on the CPU (the yardstick) and FusedAdam on the device, one single-tensor group per parameter."""

    def __init__(self, tensors, lrs, betas=None, eps=1e-15):
        self.eps = eps
        self.p64, self.m64, self.v64, self.step, self.lr, self.betas = [], [], [], [], [], []
        self.cpu, self.gpu = [], []
        self.o_cpu = self.o_gpu = None
        for k, (t, lr) in enumerate(zip(tensors, lrs)):
            self.add(t, lr, betas[k] if betas else (0.9, 0.999))

    def add(self, t, lr, betas=(0.9, 0.999)):
        self.p64.append(t.double().clone())
        self.m64.append(torch.zeros_like(t, dtype=torch.float64))
        self.v64.append(torch.zeros_like(t, dtype=torch.float64))
        self.step.append(0)
        self.lr.append(lr)
        self.betas.append(betas)
        pc, pg = torch.nn.Parameter(t.clone()), torch.nn.Parameter(t.to(DEV))
        self.cpu.append(pc)
        self.gpu.append(pg)
        gc, gg = ({"params": [p], "lr": lr, "betas": betas} for p in (pc, pg))
        if self.o_cpu is None:
            self.o_cpu = torch.optim.Adam([gc], lr=0.0, eps=self.eps, foreach=False)
            self.o_gpu = gsr_optim.FusedAdam([gg], lr=0.0, eps=self.eps)
        else:
            self.o_cpu.add_param_group(gc)
            self.o_gpu.add_param_group(gg)

    def preload(self, k, m, v, step):
        """Adam state as a long run leaves it: moments m, v after `step` steps."""
        self.m64[k], self.v64[k], self.step[k] = m.double().clone(), v.double().clone(), step
        self.o_cpu.state[self.cpu[k]] = {"step": torch.tensor(float(step)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        self.o_gpu.state[self.gpu[k]] = {"step": torch.tensor(float(step)), "exp_avg": m.to(DEV),
                                         "exp_avg_sq": v.to(DEV)}

    def set_lr(self, k, lr):
        self.lr[k] = lr
        self.o_cpu.param_groups[k]["lr"] = lr
        self.o_gpu.param_groups[k]["lr"] = lr

    def update(self, grads):
        """One step; grads[k] is None for a parameter without a gradient this step."""
        for k, g in enumerate(grads):
            self.cpu[k].grad = None if g is None else g.clone()
            self.gpu[k].grad = None if g is None else g.to(DEV)
            if g is not None:
                self.step[k] += 1
                self.p64[k], self.m64[k], self.v64[k] = T.adam_step(self.p64[k], g.double(), self.m64[k], self.v64[k],
                                                                    self.lr[k], self.step[k], self.betas[k], self.eps)
        self.o_cpu.step()
        self.o_gpu.step()

    def compare(self, yard, tag=""):
        for k in range(len(self.p64)):
            sc, sg = self.o_cpu.state[self.cpu[k]], self.o_gpu.state[self.gpu[k]]
            if self.step[k] == 0:
                assert len(sc) == 0 and len(sg) == 0
                continue
            assert float(sg["step"]) == float(sc["step"]) == self.step[k], (k, sg["step"], sc["step"], self.step[k])
            for name, ref, c, g in (("p", self.p64[k], self.cpu[k], self.gpu[k]),
                                    ("m", self.m64[k], sc["exp_avg"], sg["exp_avg"]),
                                    ("v", self.v64[k], sc["exp_avg_sq"], sg["exp_avg_sq"])):
                assert torch.isfinite(g).all(), (tag, k, name)
                yard.add(f"{tag}{name}{k}", Hh.max_err(g, ref), Hh.max_err(c, ref), ADAM_FLOOR)


def _carve(sizes, pad=16, misalign=()):
    """Offsets of groups of `sizes` floats in one buffer: every group starts on a 16-byte boundary (or 4 bytes
    past one for the indices in `misalign`) with at least `pad` sentinel floats on either side."""
    offs, cur = [], pad
    for k, n in enumerate(sizes):
        offs.append(cur + (1 if k in misalign else 0))
        cur += (n + 1 + 3) // 4 * 4 + pad
    inside = torch.zeros(cur, dtype=torch.bool)
    for o, n in zip(offs, sizes):
        inside[o:o + n] = True
    return offs, cur, inside


SENTINEL = -7.25


def _one_launch(sizes, lrs, steps, seed, mis_p=(), mis_g=(), mis_m=(), mis_v=()):
    """`steps` Adam steps over groups of `sizes` floats, each step one gsr_adam_step launch over views carved out
    of four sentinel-filled buffers, against float64 and torch's fp32 Adam; also checks every float outside the
    groups (at least 16 on either side of each) untouched."""
    from diff_gaussian_rasterization import _C

    assert len(sizes) <= _C.MAX_ADAM_GROUPS
    gen = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(n, generator=gen) for n in sizes]
    grads = [[torch.randn(n, generator=gen) * 10.0 ** (-2 * it) for n in sizes] for it in range(steps)]
    # float64 reference and the fp32 yardstick
    ref = [(p.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64))
           for p, n in zip(p0, sizes)]
    cpu = [torch.nn.Parameter(p.clone()) for p in p0]
    o_cpu = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(cpu, lrs)], lr=0.0, eps=1e-15, foreach=False)
    bufs, views, masks = {}, {}, {}
    for name, mis in (("p", mis_p), ("g", mis_g), ("m", mis_m), ("v", mis_v)):
        offs, total, inside = _carve(sizes, misalign=mis)
        b = torch.full((total,), SENTINEL, device=DEV)
        bufs[name], masks[name] = b, inside.to(DEV)
        views[name] = [b[o:o + n] for o, n in zip(offs, sizes)]
        for k, (o, n) in enumerate(zip(offs, sizes)):
            assert (b[o:o + n].data_ptr() % 16 == 0) == (k not in mis) or n == 0
    for k in range(len(sizes)):
        views["p"][k].copy_(p0[k])
        views["m"][k].zero_()
        views["v"][k].zero_()
    for it in range(steps):
        for k in range(len(sizes)):
            views["g"][k].copy_(grads[it][k])
            cpu[k].grad = grads[it][k].clone()
            ref[k] = T.adam_step(ref[k][0], grads[it][k].double(), ref[k][1], ref[k][2], lrs[k], it + 1)
        g_before = bufs["g"].clone()
        _C.adam_step([(views["p"][k], views["g"][k], views["m"][k], views["v"][k]) for k in range(len(sizes))],
                     lrs, float(it + 1), 0.9, 0.999, 1e-15)
        o_cpu.step()
        assert torch.equal(bufs["g"], g_before)  # gradients are read only
    for name in ("p", "m", "v"):
        out = bufs[name][~masks[name]]
        assert torch.equal(out, torch.full_like(out, SENTINEL)), f"{name}: a float outside the groups was written"
    yard = Hh.Yardstick(f"adam one launch {sizes[:3]}.. mis p{mis_p} g{mis_g} m{mis_m} v{mis_v}")
    for k, n in enumerate(sizes):
        st = o_cpu.state[cpu[k]]
        for name, r, c in (("p", ref[k][0], cpu[k]), ("m", ref[k][1], st["exp_avg"]), ("v", ref[k][2], st["exp_avg_sq"])):
            yard.add(f"{name}{k}", Hh.max_err(views[name][k], r), Hh.max_err(c, r), ADAM_FLOOR)
    yard.check()


def test_adam_grid_stride_and_group_walk():
    """More float4 than the capped grid has lanes (2,100,009 against 8192 workgroups x 256 = 2,097,152): the grid is
    capped, every thread walks from the first group into the seventh (3.4M floats) or beyond, and threads 0..2856
    run a second iteration of the grid-stride loop, in which they cross from the first group over the empty one
    and four more into the last two within one stride."""
    sizes = [5_000_003, 0, 1, 2, 3, 5, 3_400_001, 7]
    assert sum((n + 3) // 4 for n in sizes) > 8192 * 256
    _one_launch(sizes, [1e-3 * (k + 1) for k in range(len(sizes))], steps=2, seed=10)


@pytest.mark.parametrize("which", ["param", "grad", "exp_avg", "exp_avg_sq"])
def test_adam_mixed_alignment_in_one_launch(which):
    """The middle group 4 bytes off a 16-byte boundary in one of its four buffers, its neighbours aligned: that
    group alone takes the scalar path."""
    kw = {"param": "mis_p", "grad": "mis_g", "exp_avg": "mis_m", "exp_avg_sq": "mis_v"}[which]
    _one_launch([1001, 1000, 999], [1e-3, 2e-3, 3e-3], steps=2, seed=11, **{kw: (1,)})


@pytest.mark.parametrize("n_params", [17, 33])
def test_adam_more_parameters_than_one_launch_holds(n_params):
    """FusedAdam splits its batch into launches of MAX_ADAM_GROUPS = 16: 17 -> 2, 33 -> 3."""
    from diff_gaussian_rasterization import _C

    assert _C.MAX_ADAM_GROUPS == 16
    gen = torch.Generator().manual_seed(12)
    trio = Trio([torch.randn(5 + 3 * k, generator=gen) for k in range(n_params)],
                [1e-4 * (k + 1) for k in range(n_params)])
    for it in range(2):
        trio.update([torch.randn(5 + 3 * k, generator=gen) for k in range(n_params)])
    yard = Hh.Yardstick(f"adam {n_params} parameters")
    trio.compare(yard)
    yard.check()


def test_adam_separate_batches():
    """Parameters that cannot share a launch: different betas, a parameter added after 3 steps (its step count
    lags), and one whose gradient is None on alternate steps (its step count must not advance then)."""
    gen = torch.Generator().manual_seed(13)
    n = [301, 77, 130, 64]
    trio = Trio([torch.randn(n[k], generator=gen) for k in range(3)], [1e-3, 2e-3, 3e-3],
                betas=[(0.9, 0.999), (0.8, 0.99), (0.9, 0.999)])
    yard = Hh.Yardstick("adam separate batches")
    for it in range(7):
        if it == 3:
            trio.add(torch.randn(n[3], generator=gen), 4e-3)
        grads = [torch.randn(n[k], generator=gen) for k in range(len(trio.p64))]
        if it % 2 == 1:
            grads[2] = None
        trio.update(grads)
        trio.compare(yard, f"it{it}.")
    assert trio.step == [7, 7, 4, 4]
    yard.check()


def _cpu_keeps_denormals():
    return float(torch.tensor(1e-40) * torch.tensor(1.0)) != 0.0 and float(torch.tensor(1e-20).square()) != 0.0


@pytest.mark.parametrize("case", ["zero", "1e-7", "1e-12", "1e-18", "1e-22", "tiny_v"])
def test_adam_eps_range(case):
    """Where eps = 1e-15 decides the step: gradients that are zero from the first step (nothing moves, nothing is
    NaN), gradients whose squares are fp32 normals (1e-7, 1e-12), denormals (1e-18) and underflow (1e-22), and
    exp_avg_sq decayed to 1e-38..1e-45 under zero gradients.  Parameters start at zero in all but the zero case,
    so that the displacement itself is judged.  The yardstick (torch fp32 on the CPU) must keep denormals."""
    assert _cpu_keeps_denormals()
    P = 4099
    gen = torch.Generator().manual_seed(14)
    yard = Hh.Yardstick(f"adam eps range {case}")
    if case == "zero":
        p0 = torch.randn(P, generator=gen)
        trio = Trio([p0], [5e-2])
        for it in range(3):
            trio.update([torch.zeros(P)])
        assert torch.equal(trio.gpu[0].detach().cpu(), p0)
        st = trio.o_gpu.state[trio.gpu[0]]
        assert torch.equal(st["exp_avg"].cpu(), torch.zeros(P)) and torch.equal(st["exp_avg_sq"].cpu(), torch.zeros(P))
    elif case == "tiny_v":
        trio = Trio([torch.zeros(P)], [5e-2])
        m = (torch.rand(P, generator=gen) - 0.5) * 2e-20
        v = 10.0 ** (-38.0 - 7.0 * torch.rand(P, generator=gen).double())
        trio.preload(0, m, v.float(), 2000)
        for it in range(3):
            trio.update([torch.zeros(P)])
    else:
        mag = float(case)
        trio = Trio([torch.zeros(P)], [5e-2])
        for it in range(3):
            sign = torch.where(torch.rand(P, generator=gen) < 0.5, -1.0, 1.0)
            trio.update([(sign * mag * (0.5 + torch.rand(P, generator=gen).double())).float()])
    trio.compare(yard)
    yard.check()


def _xyz_lr(it, n, lr_init=1.6e-4, lr_final=1.6e-6):
    """The reference's position learning-rate schedule (log-linear from lr_init to lr_final), over n steps."""
    t = min(max(it / n, 0.0), 1.0)
    return math.exp((1.0 - t) * math.log(lr_init) + t * math.log(lr_final))


def test_adam_long_run():
    """300 steps over the nine parameter shapes at P = 257, gradients re-drawn every step at magnitudes cycling
    through 1e-3..1e1, the xyz learning rate decayed every step: the bias corrections from t = 1 to t = 300."""
    P, n_steps = 257, 300
    gen = torch.Generator().manual_seed(15)
    names = list(SHAPES)
    trio = Trio([torch.randn((P,) + SHAPES[k], generator=gen) for k in names], [LRS[k] for k in names])
    yard = Hh.Yardstick("adam 300 steps")
    for it in range(1, n_steps + 1):
        mag = 10.0 ** (-3.0 + 4.0 * ((it * 7) % 11) / 10.0)
        trio.set_lr(names.index("xyz"), _xyz_lr(it, n_steps))
        trio.update([torch.randn((P,) + SHAPES[k], generator=gen) * mag for k in names])
        if it in (1, 10, 100, 300):
            trio.compare(yard, f"t{it}.")
    yard.check()


# ---------------------------------------------------------------- densification statistics at their sizes
def _stats_case(P, radii, seed=3):
    g = torch.Generator().manual_seed(seed)
    vgrad = torch.randn(P, 3, generator=g)
    state = {k: torch.rand(P, 1, generator=g) for k in ("accum", "accum_abs", "denom")}
    max_r = torch.rand(P, generator=g) * 3
    vis = radii > 0
    r_max = max_r.clone()
    r_max[vis] = torch.max(r_max[vis], radii[vis])
    r_acc, r_abs, r_den = state["accum"].clone(), state["accum_abs"].clone(), state["denom"].clone()
    r_acc[vis] += torch.norm(vgrad[vis, :2], dim=-1, keepdim=True)
    r_abs[vis] += torch.norm(vgrad[vis, 2:], dim=-1, keepdim=True)
    r_den[vis] += 1

    class G:
        pass

    gm = G()
    gm.max_radii2D = max_r.to(DEV)
    gm.xyz_gradient_accum, gm.xyz_gradient_accum_abs, gm.denom = (state[k].to(DEV) for k in ("accum", "accum_abs",
                                                                                               "denom"))
    vp = torch.zeros(P, 3, device=DEV, requires_grad=True)
    vp.grad = vgrad.to(DEV)
    gsr_optim.add_densification_stats(gm, vp, radii.to(DEV))
    assert torch.equal(gm.max_radii2D.cpu(), r_max)
    assert torch.equal(gm.denom.cpu(), r_den) and torch.equal(gm.xyz_gradient_accum_abs.cpu(), r_abs)
    assert torch.allclose(gm.xyz_gradient_accum.cpu(), r_acc, rtol=2e-7, atol=0)
    return gm, max_r, state


@pytest.mark.parametrize("P", [0, 1, 255, 256, 257, 5003])
def test_densify_stats_sizes(P):
    radii = torch.randint(-1, 4, (P,), generator=torch.Generator().manual_seed(4), dtype=torch.int32)
    if P == 1:
        radii[:] = 2
    _stats_case(P, radii)


@pytest.mark.parametrize("P", [257, 5003])
def test_densify_stats_nothing_visible(P):
    """Every radius <= 0: all four buffers stay bit-identical."""
    radii = -torch.randint(0, 3, (P,), generator=torch.Generator().manual_seed(5), dtype=torch.int32)
    assert int((radii == 0).sum()) > 0 and int((radii < 0).sum()) > 0
    gm, max_r, state = _stats_case(P, radii)
    assert torch.equal(gm.max_radii2D.cpu(), max_r)
    assert torch.equal(gm.xyz_gradient_accum.cpu(), state["accum"])
    assert torch.equal(gm.xyz_gradient_accum_abs.cpu(), state["accum_abs"])
    assert torch.equal(gm.denom.cpu(), state["denom"])


@pytest.mark.parametrize("P", [257, 5003])
def test_densify_stats_everything_visible(P):
    radii = torch.randint(1, 5, (P,), generator=torch.Generator().manual_seed(6), dtype=torch.int32)
    gm, max_r, state = _stats_case(P, radii)
    assert torch.equal(gm.denom.cpu(), state["denom"] + 1)
