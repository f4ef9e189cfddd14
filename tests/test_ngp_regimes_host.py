"""The regimes of tests/test_gpu_ngp_regimes.py on the CPU checker alone: each regime's inputs must actually be the regime (rays behind
the camera, a step that varies and meets both clamps, a camera inside the box, ...) and must not be trivial -- a frame without a sample,
or without a ray that saturates, would let the GPU comparison pass while testing nothing.  The checker's loop is
tests/ngp_regimes.render on oracle.oracle with the f32 network of oracle.ngp; the GPU file asserts the same on the GPU's own counts.

With the real network the checker gives: cascades 0.66 between the clamps / 0.34 at dt_max on the issue's bitfield, whose level-1 ellipsoid
(semi-axes 0.7 / 0.9 / 0.7) holds no cell outside the unit cube -- 0 samples with max |xyz| > 1 -- and 0.72 / 0.28 with 8 574 such samples
on the regime's second bitfield (level 1 reaching x = +-1.4); var_dt 0.75 at dt_min / 0.25 between; grid512 every step at dt_max
(0.00677 < dt_min 0.02706), 128 samples on the longest ray.

Printed per run (pytest -s): the shares of marched samples whose step equals dt_min / lies strictly between / equals dt_max, the largest
per-ray count and the number of rays with weights_sum > 0.5."""
import numpy as np
import pytest

import ngp_regimes as R


def _report(regime, run, f):
    lo, mid, hi = R.step_shares(run, f["steps"])
    dt_min, dt_max = R.step_bounds(run)
    print("%-12s rays %5d  samples %6d  dt_min %.5f dt_max %.5f  shares == dt_min %.3f  between %.3f  == dt_max %.3f  max count %3d  "
          "rays with weight > 0.5: %d  rays without a sample: %d  samples with max |xyz| > 1: %d"
          % (run.label, run.ro.shape[0], f["steps"].size, dt_min, dt_max, lo, mid, hi, int(f["ray_counts"].max()),
             int((f["weights_sum"] > 0.5).sum()), int((f["ray_counts"] == 0).sum()), int((f["reach"] > 1).sum())))


@pytest.mark.parametrize("regime", R.REGIMES)
def test_regime_inputs_meet_their_conditions(regime):
    frames = [R.checker_frame(regime, i) for i in range(len(R.runs(regime)))]
    for run, f in zip(R.runs(regime), frames):
        _report(regime, run, f)
        assert f["steps"].size == int(f["ray_counts"].sum())
    R.check_common(regime, frames)
    R.check_regime(regime, frames)


def test_axis_rays_are_the_listed_ones():
    """exact zeros and the two negative zeros survive the way into the arrays both sides read"""
    run = R.runs("axis")[0]
    assert run.rd.dtype == np.float32 and np.signbit(run.rd[4, :2]).all() and not np.signbit(run.rd[0, :2]).any()
    assert (run.rd[[0, 1, 4, 5]] == [0, 0, 1]).all() and (run.rd[2] == [1, 0, 0]).all() and (run.rd[3] == [0, -1, 0]).all()
    # no origin on a box plane along a zero direction component (far is NaN there, in the reference as well)
    on_plane = (np.abs(run.ro) == 1) & (run.rd == 0)
    assert not on_plane.any()
