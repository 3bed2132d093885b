"""Generate tests/golden/tnteval.npz from the reference's own histogram rule:
eval_tnt/evaluation.py's get_f1_score_histo2, imported unmodified with `open3d`
and `matplotlib` stubbed (neither is called by that function).

Run in the build container (where /root/reference exists):
    python tests/golden/make_golden_tnteval.py
Only the DATA file written next to this script is committed: the two distance
arrays, tau, plot_stretch, and what the reference computed from them.

The arrays (3000 and 2500 values, tau = 0.01) include values exactly on a bin
edge (the edges are numpy's own arange values), the last edge itself, values
at 5 tau and beyond, zeros, and none within 1e-9 of tau (asserted below, which
is what lets precision and recall be compared exactly).
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
TAU, STRETCH = 0.01, 5


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def distances(seed, n):
    rng = np.random.default_rng(seed)
    edges = np.arange(0, TAU * STRETCH, TAU / 100)
    d = np.abs(rng.normal(0.0, 0.012, size=n))
    d[:40] = edges[rng.integers(0, edges.shape[0], size=40)]  # exactly on a bin edge
    d[:40][np.abs(d[:40] - TAU) < 1e-9] = edges[7]
    d[40:44] = edges[-1]                                       # the last edge: the closed end
    d[44:50] = [TAU * STRETCH, TAU * STRETCH * 1.5, 1.0, 0.0, 0.0, np.nextafter(edges[-1], 1.0)]
    near = np.abs(d - TAU) < 1e-9
    d[near] += 1e-6
    return rng.permutation(d)


def main():
    stub("open3d")
    stub("matplotlib", pyplot=stub("matplotlib.pyplot"))
    sys.path.insert(0, os.path.join(REF, "eval_tnt"))
    import evaluation  # noqa: E402  (the reference's file, unmodified)

    d1, d2 = distances(1, 3000), distances(2, 2500)
    for d in (d1, d2):
        assert np.abs(d - TAU).min() > 1e-9, "a distance lies on tau"
    with contextlib.redirect_stdout(io.StringIO()):
        p, r, f, e1, c1, e2, c2 = evaluation.get_f1_score_histo2(TAU, "", STRETCH, d1, d2)
    path = os.path.join(OUT, "tnteval.npz")
    np.savez_compressed(path, tau=np.float64(TAU), plot_stretch=np.int64(STRETCH), d1=d1, d2=d2,
                        precision=np.float64(p), recall=np.float64(r), fscore=np.float64(f), edges_source=e1,
                        cum_source=c1, edges_target=e2, cum_target=c2)
    print(f"{path}: {os.path.getsize(path)} bytes; precision {p:.6f} recall {r:.6f} fscore {f:.6f}, "
          f"{e1.shape[0]} edges, cum ends {c1[-1]:.4f} {c2[-1]:.4f}")
    assert os.path.getsize(path) < 200_000


if __name__ == "__main__":
    main()
