"""Golden vectors of the reference's ``Gaussians.initialize_scale``: runs the REFERENCE ITSELF on the clouds of
tests/knn_restatement.py and stores inputs and outputs as tests/golden/knn_<cloud>_n<N>.npz.

Needs a checkout of the reference (dcaustin33/intro_to_gaussian_splatting) where oracle/capture_golden.py looks for it; it is
imported through that script's own importer, which stubs the absent third-party ``plyfile`` module, and never copied --
this script writes data only.  The method is called on a plain object carrying ``points`` and
``scales = 0.001 * ones``: not through the constructor, which writes a ``.ply``.  The reference's three sorted distances
are not returned by the method; they are recorded where the method itself takes their mean.

    python tools/capture_knn_golden.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT_DIR = os.path.join(ROOT, "tests", "golden")


def _import_reference():
    sys.path.insert(0, ROOT)
    from oracle import capture_golden          # its importer: stubs plyfile, puts the reference on the path

    return capture_golden._import_reference()[1]


def capture(Gaussians, points: np.ndarray):
    """(scales (n, 3), dist3 (n, 3)) as the reference computes them on the CPU, float32."""
    import torch

    carrier = types.SimpleNamespace(points=torch.from_numpy(points.copy()),
                                    scales=0.001 * torch.ones((points.shape[0], 3), dtype=torch.float32))
    seen = []
    mean = torch.Tensor.mean

    def recording_mean(self, *a, **k):
        seen.append(self.detach().clone())
        return mean(self, *a, **k)

    torch.Tensor.mean = recording_mean
    try:
        Gaussians.initialize_scale(carrier)
    finally:
        torch.Tensor.mean = mean
    assert len(seen) == 1 and seen[0].shape[0] == points.shape[0], [tuple(s.shape) for s in seen]
    dist3 = torch.full((points.shape[0], 3), float("inf"), dtype=torch.float32)
    dist3[:, :seen[0].shape[1]] = seen[0]
    return carrier.scales.numpy().astype(np.float32), dist3.numpy()


def main() -> None:
    import knn_restatement as kr

    Gaussians = _import_reference()
    for kind, n in kr.FIXTURES:
        points = kr.cloud(kind, n)
        scales, dist3 = capture(Gaussians, points)
        path = os.path.join(OUT_DIR, kr.fixture_name(kind, n) + ".npz")
        np.savez_compressed(path, points=points, scales=scales, dist3=dist3)
        print("%s: scales %.6g .. %.6g, %d bytes" % (os.path.basename(path), float(scales.min()), float(scales.max()),
                                                     os.path.getsize(path)))


if __name__ == "__main__":
    main()
