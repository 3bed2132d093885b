"""Generate tests/golden/photoloss.npz from the reference's own Python code:
utils/loss_utils.py:90-123 L1_loss_appearance over its four appearance models
(scene/gaussian_model.py App_model) and scene/appearance_network.py
AppearanceNetwork, in fp32 on the CPU, with the autograd gradients.

Run where the reference tree exists (as tests/golden/make_golden.py, whose
stubs for the reference's unavailable imports this script uses):
    python tests/golden/make_golden_photoloss.py
Only the data file is committed: inputs, the network's weights, values and
gradients.  To keep the file small the network's weights are 15 levels of a
per-tensor scale (stored as int8) and the images multiples of 1/4096 (stored as
uint16): the values the reference is given, so both are exact.

Cases: NO, GS, GOF, PGSR at 64 x 96 and 70 x 100 (the GOF centre crop of the
second: 64 x 96 at top 3, left 2).
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

SIZES = ((64, 96), (70, 100))


def _reference():
    MG._install_stubs()
    gm = importlib.import_module("scene.gaussian_model")
    scene = sys.modules["scene"]
    scene.GaussianModel, scene.Camera = gm.GaussianModel, object  # `from scene import GaussianModel, Camera`
    MG._stub("fused_ssim", fused_ssim=lambda *a, **k: None)
    MG._stub("warp_patch_ncc")
    MG._stub("gaussian_renderer", sample_depth=lambda *a, **k: None, render=lambda *a, **k: None)
    lu = importlib.import_module("utils.loss_utils")
    an = importlib.import_module("scene.appearance_network")
    return gm.GaussianModel.App_model, lu.L1_loss_appearance, an.AppearanceNetwork


class _Gaussians:
    """What L1_loss_appearance reads of a GaussianModel."""

    def __init__(self, app_model, embeddings, network=None):
        self.app_model, self._emb, self.appearance_network = app_model, embeddings, network

    def get_apperance_embedding(self, idx):
        return self._emb[idx]


def main():
    App, l1_app, Network = _reference()
    rng = np.random.default_rng(20240611)
    torch.manual_seed(7)
    out = {}
    net = Network(3 + 64, 3)
    with torch.no_grad():
        for k, p in net.state_dict().items():
            scale = float(p.abs().max()) / 7.0
            q = torch.round(p / scale).clamp(-7, 7)
            p.copy_(q * scale)
            out[f"net.{k}.q"] = q.numpy().astype(np.int8)
            out[f"net.{k}.scale"] = np.float32(scale)
    view = 2
    for H, W in SIZES:
        tag = f"{H}x{W}"
        qa = rng.integers(0, 4096, (3, H, W)).astype(np.uint16)
        qb = np.clip(np.round(qa + 409.6 * rng.standard_normal(qa.shape)), 0, 4096).astype(np.uint16)
        a, b = qa.astype(np.float32) / 4096, qb.astype(np.float32) / 4096
        out[f"image.{tag}.q4096"], out[f"gt.{tag}.q4096"] = qa, qb
        embs = {
            "no": None,
            "gs": (np.eye(3, 4)[None] + 0.05 * rng.standard_normal((4, 3, 4))).astype(np.float32),
            "gof": (0.5 * rng.standard_normal((4, 64))).astype(np.float32),
            "pgsr": (0.1 * rng.standard_normal((4, 2))).astype(np.float32),
        }
        for name, member in (("no", App.NO), ("gs", App.GS), ("gof", App.GOF), ("pgsr", App.PGSR)):
            img = torch.tensor(a, requires_grad=True)
            emb = None if embs[name] is None else torch.tensor(embs[name], requires_grad=True)
            net.zero_grad()
            l1 = l1_app(img, torch.tensor(b), _Gaussians(member, emb, net if name == "gof" else None), view)
            l1.backward()
            out[f"{name}.{tag}.l1"] = l1.detach().numpy()
            out[f"{name}.{tag}.dimage"] = img.grad.numpy()
            if emb is not None:
                out[f"{name}.{tag}.embeddings"] = embs[name]
                out[f"{name}.{tag}.dembeddings"] = emb.grad.numpy()
            if name == "gof":
                out[f"gof.{tag}.dconv3_weight"] = net.conv3.weight.grad.numpy().copy()
                out[f"gof.{tag}.dconv3_bias"] = net.conv3.bias.grad.numpy().copy()
    out["view"] = np.int64(view)
    path = os.path.join(MG.OUT, "photoloss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
