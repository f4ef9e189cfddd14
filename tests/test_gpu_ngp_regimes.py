"""The hash-grid NeRF frame (BASELINE cfg2) against the CPU checker outside the one regime tests/test_gpu_ngp.py covers (the frontal
camera, bound 1, one cascade, a 128^3 grid, a constant step): rays with dz < 0 and along +-x, two cascades, a step that varies and meets
dt_min / dt_max, a camera inside the box, a box that is not the cube, 64^3 and 512^3 grids, axis-aligned rays with exact and negative
zeros, an odd frame, another encoder (tests/ngp_regimes.py lists the runs; tests/test_ngp_regimes_host.py holds their inputs to the
conditions that make them the regime, on the CPU).  The only source of expected f32 values is the reference's loop on oracle.oracle and
oracle.ngp (ngp_regimes.checker_frame).  Per run, a ladder -- every comparison np.array_equal, no tolerance:

  1. operators   the same host loop on lz_march_rays / lz_composite_rays / lz_near_far_from_aabb around FusedHashgridNeRF.forward (f32)
                 == the checker: image, depth, weights_sum, per-ray counts.  The GPU's own counts meet the regime's conditions.
  2. loop mode   HashgridRenderer(mode="loop"), schedule (1, 8), f32 net and f32 net on half tables == the checker: image, image_raw,
                 depth, weights_sum, ray_counts; state[3] == 1, state[5] == ray_counts.sum()
  3. fused mode  HashgridRenderer(mode="fused", cap="reference"), the same two nets == the CHECKER (not loop mode)
  4. f16 net     no bit-exact CPU reference (the MFMA fixes the accumulation order): the host loop of step 1 around the GPU f16 forward,
                 as test_f16_renderer_equals_the_host_loop arranges it; loop mode and fused mode equal it bit for bit, counts included.
                 Step 1 holds that host loop's march and compositing to the checker in the same run."""
import functools

import numpy as np
import pytest
import torch

import ngp_regimes as R

pytestmark = pytest.mark.gpu
KEYS = ("image", "image_raw", "depth", "weights_sum", "ray_counts")
RUN_PARAMS = [pytest.param(r, i, id="%s-%d" % (r, i)) for r, i in R.RUN_IDS]


@functools.lru_cache(maxsize=None)
def nets(encoder):
    """GenericHashgridNeRF(seed=3) on the GPU and its three fused networks"""
    from lzzx_nerf_amd.ngp import FusedHashgridNeRF
    g = R.model(torch.device("cuda"), encoder)
    out = dict(g=g, f32=FusedHashgridNeRF(g.enc, g.sigma_net, g.color_net), half=FusedHashgridNeRF(g.enc, g.sigma_net, g.color_net, half_tables=True),
               f16=FusedHashgridNeRF(g.enc, g.sigma_net, g.color_net, precision="f16"))
    assert out["half"].precision == "f32" and out["half"].table.dtype == torch.float16
    return out


@functools.lru_cache(maxsize=None)
def host_loop_frame(regime, index, net):
    """the reference's loop on the GPU operators around nets(...)[net].forward; traced.  Shared: not written into"""
    run = R.runs(regime)[index]
    out = R.render(R.GpuOps, nets(run.encoder)[net].forward, run, trace=True)
    for v in out.values():
        v.setflags(write=False)
    return out


def renderer_frame(run, net, mode):
    from lzzx_nerf_amd.ngp import HashgridRenderer
    dev = R.GpuOps.to
    r = HashgridRenderer(nets(run.encoder)[net], dev(R.bitfield(run.bits)), bound=run.bound, cascade=run.cascade, grid_size=run.grid_size,
                         aabb=dev(run.aabb), min_near=run.min_near, budget_factor=1, n_step_cap=8, mode=mode, cap="reference")
    got = r.render(dev(run.ro), dev(run.rd), dt_gamma=run.dt_gamma, max_steps=run.max_steps, T_thresh=run.T_thresh, count_samples=True)
    torch.cuda.synchronize()
    out = {k: got[k].cpu().numpy() for k in KEYS}
    out["ray_counts"] = out["ray_counts"].astype(np.int64)
    out["state"] = got["state"].cpu().numpy()
    return out


def assert_equals(got, want, keys, what):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert np.array_equal(got[k], want[k], equal_nan=False), (what, k, int((got[k] != want[k]).sum()), got[k].size)


def assert_renderer(run, net, mode, want):
    got = renderer_frame(run, net, mode)
    assert_equals(got, want, KEYS, (run.label, net, mode))
    assert int(got["state"][3]) == 1 and int(got["state"][5]) == int(got["ray_counts"].sum()) == int(want["ray_counts"].sum())


# ---- 1. the operators ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime,index", RUN_PARAMS)
def test_operators_equal_the_checker(regime, index):
    want = R.checker_frame(regime, index)
    got = host_loop_frame(regime, index, "f32")
    assert_equals(got, want, ("nears", "fars", "ray_counts", "steps", "reach", "weights_sum", "depth", "image_raw", "image"), (regime, index))


@pytest.mark.parametrize("regime", R.REGIMES)
def test_regime_conditions_on_the_gpu_counts(regime):
    """tests/test_ngp_regimes_host.py's conditions, on what the GPU operators marched and composited"""
    frames = [host_loop_frame(regime, i, "f32") for i in range(len(R.runs(regime)))]
    R.check_common(regime, frames)
    R.check_regime(regime, frames)


# ---- 2. / 3. the two renderers against the checker --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["loop", "fused"])
@pytest.mark.parametrize("net", ["f32", "half"])
@pytest.mark.parametrize("regime,index", RUN_PARAMS)
def test_renderer_equals_the_checker(regime, index, net, mode):
    assert_renderer(R.runs(regime)[index], net, mode, R.checker_frame(regime, index, half=net == "half"))


# ---- 4. the f16 net ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["loop", "fused"])
@pytest.mark.parametrize("regime,index", RUN_PARAMS)
def test_f16_renderer_equals_the_host_loop(regime, index, mode):
    want = host_loop_frame(regime, index, "f16")
    assert (want["weights_sum"] > 0.5).any() and want["ray_counts"].max() > 8
    assert_renderer(R.runs(regime)[index], "f16", mode, want)
