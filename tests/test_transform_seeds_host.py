"""The committed rotation seeds of the frame-invariance tests (tests/transform_cases.py: SEEDS) obey their rule, on the CPU:
with the seed, the oracle's own before / after pair of frames -- the C restatement of the reference over the numpy
restatement of the transform, cameras moved by GaussianScene._move_views -- stays within the pixel tolerance everywhere,
no earlier seed does, and every Gaussian stays clear of the near test (z_view >= 0.2) and of the far plane (100) in both
frames.  No GPU code is involved in the choice."""
import numpy as np
import pytest

import transform_cases as tc


@pytest.mark.parametrize("name,kind", tc.CASES)
def test_the_committed_seed_is_the_first_the_oracle_accepts(tmp_path, name, kind):
    seed = tc.SEEDS[(name, kind)]
    for candidate in range(seed + 1):
        before, after, z0, z1 = tc.oracle_pair(name, kind, candidate, tmp_path / str(candidate))
        worst = float(np.abs(after - before).max())
        print("%s, %s, seed %d: the oracle's own pair differs by %.3g; z_view %.2f .. %.2f -> %.2f .. %.2f"
              % (name, kind, candidate, worst, z0.min(), z0.max(), z1.min(), z1.max()))
        assert before.max() > 0.5                      # a frame, not a black one
        assert (worst <= tc.PIXEL_TOLERANCE) == (candidate == seed)
    s = tc.KINDS[kind][0]
    assert z0.min() >= 0.4 and z1.min() >= 0.4 and z0.max() <= 50.0 and z1.max() <= 50.0
    assert np.abs(z1 - s * z0).max() <= 1e-5 * z1.max()


def test_the_normalize_scene_keeps_its_frame_in_the_oracle(tmp_path):
    """normalize() has no seed to choose (R = I, s and t follow from the cameras): the scene it is tried on is one whose
    oracle pair stays within the tolerance and whose Gaussians stay clear of the near test after shrinking."""
    before, after, z0, z1 = tc.oracle_pair(tc.NORMALIZE_SCENE, "normalize", None, tmp_path)
    worst = float(np.abs(after - before).max())
    print("normalize: the oracle's own pair differs by %.3g; z_view %.2f .. %.2f -> %.2f .. %.2f (s = %.4f)"
          % (worst, z0.min(), z0.max(), z1.min(), z1.max(), z1.max() / z0.max()))
    assert before.max() > 0.5 and worst <= tc.PIXEL_TOLERANCE
    assert z1.min() >= 0.4 and z1.max() <= 50.0
