"""Plain-torch restatement of the reference's densification, with the random
draw as an explicit tensor (CPU or GPU; the yardstick of the HIP path beyond
the fixture's sizes, and tools/bench_densify.py's baseline).

densify_and_prune_ref   GaussianModel.densify_and_prune (scene/gaussian_model.py:
                        797-816): clone, then split over the array the clones
                        were appended to (their gradients padded with 0), then
                        the opacity prune, each pass as boolean-mask indexing
                        and torch.cat over the parameters and Adam moments.
compute_3D_filter_ref   :225-262;  reset_opacity_ref  :521-539.

tests/test_densify.py checks all three against tests/golden/densify.npz, the
reference's own code run on the CPU.
"""
from __future__ import annotations

import torch
from torch import nn

# optimizer group name -> attribute (gaussian_model.py densification_postfix)
NAMES = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity",
         "scaling": "_scaling", "rotation": "_rotation", "sg_axis": "_sg_axis", "sg_sharpness": "_sg_sharpness",
         "sg_color": "_sg_color"}
LRS = {"xyz": 0.00016, "f_dc": 0.0013, "f_rest": 0.00011, "opacity": 0.05, "scaling": 0.005, "rotation": 0.001,
       "sg_axis": 0.002, "sg_sharpness": 0.095, "sg_color": 0.00064}


class RefGaussians:
    """The state densification edits: nine raw parameters, filter_3D, the four statistics and
    an Adam with the reference's named single-parameter groups."""

    def __init__(self, params: dict, device="cpu", optimizer_cls=torch.optim.Adam, sg_groups=None):
        for name, attr in NAMES.items():
            setattr(self, attr, nn.Parameter(torch.as_tensor(params[name], dtype=torch.float32).to(device).clone()))
        P = self._xyz.shape[0]
        self.percent_dense = 0.01
        self.filter_3D = torch.zeros(P, 1, device=device)
        self.xyz_gradient_accum = torch.zeros(P, 1, device=device)
        self.xyz_gradient_accum_abs = torch.zeros(P, 1, device=device)
        self.denom = torch.zeros(P, 1, device=device)
        self.max_radii2D = torch.zeros(P, device=device)
        if sg_groups is None:
            sg_groups = self._sg_color[0].numel() > 0 if P else True
        names = [n for n in NAMES if sg_groups or not n.startswith("sg_")]
        self.optimizer = optimizer_cls([{"params": [getattr(self, NAMES[n])], "lr": LRS[n], "name": n} for n in names],
                                       lr=0.0, eps=1e-15)

    def set_stats(self, accum, accum_abs, denom):
        dev = self._xyz.device
        self.xyz_gradient_accum = torch.as_tensor(accum, dtype=torch.float32).reshape(-1, 1).to(dev).clone()
        self.xyz_gradient_accum_abs = torch.as_tensor(accum_abs, dtype=torch.float32).reshape(-1, 1).to(dev).clone()
        self.denom = torch.as_tensor(denom, dtype=torch.float32).reshape(-1, 1).to(dev).clone()

    def set_moments(self, moments: dict):
        """moments: name -> (exp_avg, exp_avg_sq); the state of a parameter after `step` steps."""
        for group in self.optimizer.param_groups:
            if group["name"] in moments:
                p = group["params"][0]
                m, v = moments[group["name"]]
                self.optimizer.state[p] = {"step": torch.tensor(1.0),
                                           "exp_avg": torch.as_tensor(m, dtype=torch.float32).to(p.device).clone(),
                                           "exp_avg_sq": torch.as_tensor(v, dtype=torch.float32).to(p.device).clone()}

    def moments(self, name):
        for group in self.optimizer.param_groups:
            if group["name"] == name:
                st = self.optimizer.state.get(group["params"][0])
                return None if not st else (st["exp_avg"], st["exp_avg_sq"])
        return None


def rotation_matrices(q):
    """utils/general_utils.py build_rotation: R(q / |q|), q = (r, x, y, z)."""
    norm = torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    r, x, y, z = (q / norm[:, None]).unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def _groups(g):
    return {grp["name"]: grp for grp in g.optimizer.param_groups if grp.get("name") in NAMES}


def _set(g, name, tensor, moments):
    """Replace a parameter (and its moments when it has state), as the reference's helpers do."""
    attr = NAMES[name]
    new = nn.Parameter(tensor.requires_grad_(True))
    grp = _groups(g).get(name)
    if grp is not None:
        st = g.optimizer.state.pop(grp["params"][0], None)
        grp["params"][0] = new
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = moments
            g.optimizer.state[new] = st
    setattr(g, attr, new)


def _append(g, new: dict):
    """cat_tensors_to_optimizer: extend every parameter, zero moments for the new rows."""
    for name, attr in NAMES.items():
        old, ext = getattr(g, attr).detach(), new[name]
        mo = g.moments(name)
        moments = None if mo is None else tuple(torch.cat((m, torch.zeros_like(ext)), dim=0) for m in mo)
        _set(g, name, torch.cat((old, ext), dim=0), moments)
    n = g._xyz.shape[0]
    dev = g._xyz.device
    g.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
    g.xyz_gradient_accum_abs = torch.zeros((n, 1), device=dev)
    g.denom = torch.zeros((n, 1), device=dev)
    g.max_radii2D = torch.zeros(n, device=dev)


def _prune(g, remove):
    """prune_points: keep ~remove in every parameter, moment and statistic."""
    keep = ~remove
    for name, attr in NAMES.items():
        mo = g.moments(name)
        moments = None if mo is None else tuple(m[keep] for m in mo)
        _set(g, name, getattr(g, attr).detach()[keep], moments)
    g.xyz_gradient_accum = g.xyz_gradient_accum[keep]
    g.xyz_gradient_accum_abs = g.xyz_gradient_accum_abs[keep]
    g.denom = g.denom[keep]
    g.max_radii2D = g.max_radii2D[keep]


def _sampled_xyz(g, mask, eps, repeat):
    stds = torch.exp(g._scaling.detach()[mask]).repeat(repeat, 1)
    rots = rotation_matrices(g._rotation.detach()[mask]).repeat(repeat, 1, 1)
    return torch.bmm(rots, (stds * eps).unsqueeze(-1)).squeeze(-1) + g._xyz.detach()[mask].repeat(repeat, 1)


def quantile_ref(values, q):
    """torch.quantile's linear rule in fp32 on a sort (no element limit): rank = q (n - 1),
    lerp(sorted[floor], sorted[ceil], rank - floor)."""
    s = torch.sort(values.reshape(-1)).values
    rank = torch.as_tensor(q, dtype=torch.float32, device=s.device) * (s.numel() - 1)
    lo = rank.floor().long().clamp(0, s.numel() - 1)
    hi = rank.ceil().long().clamp(0, s.numel() - 1)
    return torch.lerp(s[lo], s[hi], rank - lo.float())


@torch.no_grad()
def densify_and_prune_ref(g, max_grad, min_opacity, extent, noise, use_torch_quantile=True):
    """Returns ((clone - before, split - clone, split - prune), Q, noise rows used).  `noise`
    holds at least C + 2 S rows of standard-normal draws: rows [0, C) for the clones, then
    [C, C + 2 S) for the split (children copy 0, then copy 1)."""
    grads = g.xyz_gradient_accum / g.denom
    grads[grads.isnan()] = 0.0
    grads_abs = g.xyz_gradient_accum_abs / g.denom
    grads_abs[grads_abs.isnan()] = 0.0
    ratio = (torch.norm(grads, dim=-1) >= max_grad).float().mean()
    Q = torch.quantile(grads_abs.reshape(-1), 1 - ratio) if use_torch_quantile else \
        quantile_ref(grads_abs, 1 - ratio)
    limit = g.percent_dense * extent
    before = g._xyz.shape[0]

    # clone
    big = torch.max(torch.exp(g._scaling.detach()), dim=1).values > limit
    mask = (torch.norm(grads, dim=-1) >= max_grad) & ~big
    C = int(mask.sum())
    new = {name: getattr(g, attr).detach()[mask] for name, attr in NAMES.items()}
    new["xyz"] = _sampled_xyz(g, mask, noise[:C].to(grads), 1)
    _append(g, new)
    clone = g._xyz.shape[0]

    # split, over originals then clones (gradients of the clones: 0)
    n = g._xyz.shape[0]
    pg = torch.zeros(n, device=grads.device)
    pg[:before] = grads.squeeze(-1)
    pga = torch.zeros(n, device=grads.device)
    pga[:before] = grads_abs.squeeze(-1)
    big = torch.max(torch.exp(g._scaling.detach()), dim=1).values > limit
    mask = ((pg >= max_grad) & big) | (pga >= Q)
    S = int(mask.sum())
    new = {name: getattr(g, attr).detach()[mask].repeat(*([2] + [1] * (getattr(g, attr).dim() - 1)))
           for name, attr in NAMES.items()}
    new["xyz"] = _sampled_xyz(g, mask, noise[C:C + 2 * S].to(grads), 2)
    new["scaling"] = torch.log(torch.exp(g._scaling.detach()[mask]).repeat(2, 1) / (0.8 * 2))
    _append(g, new)
    _prune(g, torch.cat((mask, torch.zeros(2 * S, device=mask.device, dtype=torch.bool))))
    split = g._xyz.shape[0]

    # opacity prune
    _prune(g, (torch.sigmoid(g._opacity.detach()) < min_opacity).squeeze(-1))
    prune = g._xyz.shape[0]
    return (clone - before, split - clone, split - prune), float(Q), C + 2 * S


@torch.no_grad()
def compute_3D_filter_ref(xyz, cameras, dtype=torch.float32):
    """gaussian_model.py:225-262 in `dtype`: ([P,1] filter, seen mask)."""
    xyz = xyz.detach().to(dtype)
    distance = torch.full((xyz.shape[0],), float("inf"), device=xyz.device, dtype=dtype)
    seen = torch.zeros(xyz.shape[0], device=xyz.device, dtype=torch.bool)
    focal = 0.0
    for cam in cameras:
        R = torch.as_tensor(cam.R).to(xyz)
        T = torch.as_tensor(cam.T).to(xyz)
        xyz_cam = xyz @ R + T[None, :]
        z = xyz_cam[:, 2]
        uv = (xyz_cam[:, :2] / z.unsqueeze(-1)).abs()
        bx, by = cam.image_width / cam.Fx * 0.575, cam.image_height / cam.Fy * 0.575
        valid = (z > 0.2) & (uv[:, 0] <= bx) & (uv[:, 1] <= by)
        distance = torch.where(valid, torch.minimum(distance, z), distance)
        seen |= valid
        focal = max(focal, cam.Fx)
    distance[~seen] = distance[seen].max()  # (raises when nothing is seen, as the reference)
    return (distance / focal * (0.2 ** 0.5))[..., None], seen


@torch.no_grad()
def reset_opacity_values(scaling, opacity, filter_3D, dtype=torch.float32):
    """The new raw opacities of reset_opacity (gaussian_model.py:521-539) in `dtype`, with x =
    min(opacity_with_filter, 0.01) / coef (the argument of the inverse sigmoid)."""
    s, o, f = scaling.detach().to(dtype), opacity.detach().to(dtype), filter_3D.detach().to(dtype)
    sq = torch.square(torch.exp(s))
    coef = torch.sqrt(sq.prod(dim=1) / (sq + torch.square(f)).prod(dim=1))
    cur = torch.sigmoid(o) * coef[..., None]
    x = torch.min(cur, torch.ones_like(cur) * 0.01) / coef[..., None]
    return torch.log(x / (1 - x)), x


@torch.no_grad()
def reset_opacity_ref(g):
    new, _ = reset_opacity_values(g._scaling, g._opacity, g.filter_3D)
    mo = g.moments("opacity")
    _set(g, "opacity", new, None if mo is None else (torch.zeros_like(new), torch.zeros_like(new)))
