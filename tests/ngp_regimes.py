"""Shared by tests/test_ngp_regimes_host.py (CPU) and tests/test_gpu_ngp_regimes.py (GPU): the regimes in which the hash-grid NeRF frame
(BASELINE cfg2) is held to the CPU checker, and the reference's inference loop (renderer.py:495-561: march_rays -> network ->
composite_rays("plain") -> compaction, n_step = max(min(N // n_alive, 8), 1)) written once over a small operator interface --
tests/test_gpu_cfg2_render._render with bound, cascade, grid_size, aabb, min_near, dt_gamma, T_thresh and max_steps passed through where
that one hard-codes 1, 128, 0.05.  `CpuOps` is oracle.oracle; `GpuOps` the raymarching operators of the package (lz_march_rays,
lz_composite_rays, lz_near_far_from_aabb).  TEST INFRASTRUCTURE ONLY.

Rays are made once, on the CPU (oracle.get_rays), and the same arrays go to both sides: they are inputs here, not the code under test.
Every run of a regime is a `Run`; `runs(regime)` lists them (`inside` has one per min_near, `axis` one per bitfield)."""
import functools
import types

import numpy as np

from conftest import ellipsoid_bitfield
from lzzx_nerf_amd.synthetic import orbit_pose, synthetic_camera
from oracle import ngp as ONGP
from oracle import oracle as O

F32 = np.float32
SQRT3F = F32(1.7320508075688772)

REGIMES = ("behind", "side", "cascades", "var_dt", "inside", "aabb", "grid64", "grid512", "axis", "odd", "encoder", "bound15")
SMALL_ENCODER = dict(num_levels=16, level_dim=2, base_resolution=4, log2_hashmap_size=12, desired_resolution=512)

N_RUNS = {"cascades": 2, "inside": 2, "axis": 2, "bound15": 2}      # every other regime is one run
RUN_IDS = tuple((r, i) for r in REGIMES for i in range(N_RUNS.get(r, 1)))

AXIS_O = np.array([(0, 0, -3), (0.1, 0.05, -3), (-3, 0, 0), (0, 3, 0), (0, 0, -3), (0.5, 0.5, -3), (0, 0, 3)], F32)
AXIS_D = np.array([(0, 0, 1), (0, 0, 1), (1, 0, 0), (0, -1, 0), (-0.0, -0.0, 1), (0, 0, 1), (0, 0, -1)], F32)


@functools.lru_cache(maxsize=None)
def bitfield(kind):
    """"full": the ellipsoid; "holes": the same with a quarter of its bytes cleared (the seed of test_gpu_ngp_fused.py); "two": cascade 0
    full, cascade 1 holes; "two_wide": cascade 1 an
    ellipsoid with holes whose long axis, at twice the size, reaches x = +-1.4, past the unit cube; "ones"; "e64": the ellipsoid on a 64^3 grid; "rand512": 512^3 / 8 bytes in Morton order, each 0 or 255"""
    if kind == "full":
        return ellipsoid_bitfield()[0]
    if kind == "holes":
        full = bitfield("full")
        holes = full & np.where(np.random.default_rng(5).random(full.shape) < 0.25, 0, 255).astype(full.dtype)
        assert 0 < int(np.unpackbits(holes).sum()) < int(np.unpackbits(full).sum())
        return holes
    if kind == "two":
        return np.concatenate([bitfield("full"), bitfield("holes")])
    if kind == "two_wide":
        wide = ellipsoid_bitfield(semi=(0.7, 0.4, 0.3))[0]
        mask = np.where(np.random.default_rng(6).random(wide.shape) < 0.25, 0, 255).astype(wide.dtype)
        return np.concatenate([bitfield("full"), wide & mask])
    if kind == "ones":
        return np.full(128 ** 3 // 8, 255, np.uint8)
    if kind == "e64":
        return ellipsoid_bitfield(grid_size=64)[0]
    if kind == "rand512":
        return np.where(np.random.default_rng(512).random(512 ** 3 // 8) < 0.5, 0, 255).astype(np.uint8)
    raise KeyError(kind)


def _camera(pose=None, H=40, W=40, zoom=1.0):
    front, intr = synthetic_camera(H, W)
    intr = [intr[0] / zoom, intr[1] / zoom, intr[2], intr[3]]
    ro, rd = O.get_rays(front if pose is None else pose, intr, H, W)
    return np.ascontiguousarray(ro), np.ascontiguousarray(rd)


def _run(label, ro, rd, bits, **kw):
    r = dict(label=label, ro=ro, rd=rd, bits=bits, bound=1.0, cascade=1, grid_size=128, aabb=None, min_near=0.05, dt_gamma=1 / 256,
             T_thresh=1e-4, max_steps=128, encoder="default")
    r.update(kw)
    if r["aabb"] is None:
        b = r["bound"]
        r["aabb"] = [-b, -b, -b, b, b, b]
    r["aabb"] = np.array(r["aabb"], F32)
    return types.SimpleNamespace(**r)


@functools.lru_cache(maxsize=None)
def runs(regime):
    """the runs of a regime, as the issue's table sets them"""
    out = _runs(regime)
    assert len(out) == N_RUNS.get(regime, 1)
    return out


def _runs(regime):
    if regime == "behind":
        return (_run("behind", *_camera(orbit_pose(230)), "holes"),)
    if regime == "side":
        return (_run("side", *_camera(orbit_pose(157)), "holes"),)
    if regime == "cascades":
        return tuple(_run("cascades-" + b, *_camera(orbit_pose(157)), b, bound=2.0, cascade=2, dt_gamma=1 / 64) for b in ("two", "two_wide"))
    if regime == "var_dt":
        return (_run("var_dt", *_camera(orbit_pose(157)), "holes", max_steps=256),)
    if regime == "inside":
        pose = np.eye(4, dtype=F32)
        pose[2, 3] = -0.9
        ro, rd = _camera(pose, zoom=4.0)
        return tuple(_run("inside-%g" % mn, ro, rd, "holes", min_near=mn, max_steps=64) for mn in (0.05, 0.2))
    if regime == "aabb":
        return (_run("aabb", *_camera(zoom=3.0), "full", aabb=[-1, -0.5, -1, 1, 0.5, 1]),)
    if regime == "grid64":
        return (_run("grid64", *_camera(orbit_pose(157)), "e64", grid_size=64),)
    if regime == "grid512":
        return (_run("grid512", *_camera(), "rand512", grid_size=512, T_thresh=1e-2),)
    if regime == "axis":
        return tuple(_run("axis-" + b, AXIS_O.copy(), AXIS_D.copy(), b) for b in ("full", "ones"))
    if regime == "odd":
        return (_run("odd", *_camera(H=37, W=41), "holes"),)
    if regime == "encoder":
        return (_run("encoder", *_camera(), "holes", encoder="small"),)
    if regime == "bound15":
        # 2 bound = 3 is no power of two: the box-to-unit mapping's reciprocal multiply and a true division differ here (tests/bound_cases.py)
        # "two": no sample leaves the unit cube; "two_wide": its level-1 ellipsoid, at 1.5 times the size, reaches x = +-1.05 -- samples of
        # the outer level, whose box is [-1.5, 1.5]^3
        return tuple(_run("bound15-" + b, *_camera(orbit_pose(157)), b, bound=1.5, cascade=2) for b in ("two", "two_wide"))
    raise KeyError(regime)


def step_bounds(run):
    """(dt_min, dt_max) of the march as raymarching.cu:380-381 forms them, in float: the clamp is inverted when dt_min > dt_max"""
    dt_min = F32(2) * SQRT3F / F32(run.max_steps)
    dt_max = F32(2) * SQRT3F * F32(1 << (run.cascade - 1)) / F32(run.grid_size)
    return dt_min, dt_max


# ---- the network -------------------------------------------------------------------------------------------------------------------
def model(device, encoder="default"):
    """synthetic.GenericHashgridNeRF(seed=3); encoder "small": its table replaced by a second GridEncoder built as get_encoder does
    (16 levels from 4 to 512 in a 2^12 table: most levels hashed), seeded on its own"""
    import torch

    from lzzx_nerf_amd.encoding import get_encoder
    from lzzx_nerf_amd.synthetic import GenericHashgridNeRF
    g = GenericHashgridNeRF(device, seed=3)
    if encoder == "small":
        enc, dim = get_encoder("hashgrid", **SMALL_ENCODER)
        assert dim == 32
        enc.embeddings.data.copy_(torch.rand(enc.embeddings.shape, generator=torch.Generator().manual_seed(12)) * 2 - 1)
        g.enc = enc.to(device)
    return g


def checker_net(g, half):
    """oracle.ngp.network on the module's weights and table (half: the table rounded to f16, as test_gpu_ngp.make does)"""
    W = dict(s0=g.sigma_net.net[0].weight, s1=g.sigma_net.net[1].weight, c0=g.color_net.net[0].weight, c1=g.color_net.net[1].weight)
    W = {k: v.detach().cpu().numpy() for k, v in W.items()}
    e = g.enc
    emb = e.embeddings.detach().cpu().numpy()
    offsets = e.offsets.cpu().numpy()
    want = O.grid_offsets(3, e.num_levels, e.per_level_scale, e.base_resolution, e.log2_hashmap_size)
    assert np.array_equal(want, offsets), "oracle.grid_offsets and the module's offsets differ"
    return ONGP.network(W, emb.astype(np.float16) if half else emb, offsets, e.per_level_scale, e.base_resolution)


# ---- the operators -----------------------------------------------------------------------------------------------------------------
class CpuOps:
    near_far = staticmethod(O.near_far_from_aabb)

    @staticmethod
    def march(n_alive, n_step, alive, t, ro, rd, run, bits, nears, fars):
        return O.march_rays(n_alive, n_step, alive, t, ro, rd, run.bound, bits, run.cascade, run.grid_size, nears, fars, 128, None,
                            run.dt_gamma, run.max_steps)

    @staticmethod
    def composite(n_alive, n_step, alive, t, sig, rgb, dl, ws, dep, img, T):
        O.composite_rays("plain", n_alive, n_step, alive, t, sig, rgb, dl, ws, dep, img, T_thresh=T)

    to = staticmethod(lambda a: np.ascontiguousarray(a))
    np_ = staticmethod(lambda a: a)
    zeros = staticmethod(lambda *s: np.zeros(s, F32))
    arange = staticmethod(lambda n: np.arange(n, dtype=np.int32))
    copy = staticmethod(lambda a: a.copy())
    compact = staticmethod(lambda a: np.ascontiguousarray(a[a >= 0]))


class GpuOps:
    @staticmethod
    def near_far(ro, rd, aabb, mn):
        from lzzx_nerf_amd import raymarching as R
        return R.near_far_from_aabb(ro, rd, aabb, mn)

    @staticmethod
    def march(n_alive, n_step, alive, t, ro, rd, run, bits, nears, fars):
        from lzzx_nerf_amd import raymarching as R
        return R.march_rays(n_alive, n_step, alive, t, ro, rd, run.bound, bits, run.cascade, run.grid_size, nears, fars, 128, False,
                            run.dt_gamma, run.max_steps)

    @staticmethod
    def composite(n_alive, n_step, alive, t, sig, rgb, dl, ws, dep, img, T):
        from lzzx_nerf_amd import raymarching as R
        R.composite_rays(n_alive, n_step, alive, t, sig, rgb, dl, ws, dep, img, T)

    @staticmethod
    def to(a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def zeros(*s):
        import torch
        return torch.zeros(*s, device="cuda")

    @staticmethod
    def arange(n):
        import torch
        return torch.arange(n, dtype=torch.int32, device="cuda")

    np_ = staticmethod(lambda a: a.cpu().numpy())
    copy = staticmethod(lambda a: a.clone())
    compact = staticmethod(lambda a: a[a >= 0])


def render(ops, net, run, trace=False):
    """run_cuda, inference branch (renderer.py:495-561), on either backend -> dict of numpy arrays: image (blended on white, clamped),
    image_raw, depth, weights_sum, ray_counts, nears, fars; with trace the marched samples' deltas[:, 0] and max |xyz| as well"""
    ro, rd, aabb, bits = ops.to(run.ro), ops.to(run.rd), ops.to(run.aabb), ops.to(bitfield(run.bits))
    N = run.ro.shape[0]
    nears, fars = ops.near_far(ro, rd, aabb, run.min_near)
    ws, dep, img = ops.zeros(N), ops.zeros(N), ops.zeros(N, 3)
    alive = ops.arange(N)
    t = ops.copy(nears)
    counts = np.zeros(N, np.int64)
    steps, reach = [], []
    step = 0
    while step < run.max_steps:
        n_alive = alive.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        xyzs, dirs, dl = ops.march(n_alive, n_step, alive, t, ro, rd, run, bits, nears, fars)
        sig, rgb = net(xyzs, dirs, run.bound)
        d0 = ops.np_(dl)[: n_alive * n_step, 0]
        np.add.at(counts, ops.np_(alive), (d0 != 0).reshape(n_alive, n_step).sum(1))
        if trace:
            steps.append(d0[d0 != 0])
            reach.append(np.abs(ops.np_(xyzs)[: n_alive * n_step]).max(1)[d0 != 0])
        ops.composite(n_alive, n_step, alive, t, sig, rgb, dl, ws, dep, img, run.T_thresh)
        alive = ops.compact(alive)
        step += n_step
    ws, dep, img = ops.np_(ws), ops.np_(dep), ops.np_(img)
    out = dict(image=np.clip(img + (1 - ws)[:, None], 0, 1).astype(F32), image_raw=img, depth=dep, weights_sum=ws, ray_counts=counts,
               nears=ops.np_(nears), fars=ops.np_(fars))
    if trace:
        out["steps"] = np.concatenate(steps) if steps else np.zeros(0, F32)
        out["reach"] = np.concatenate(reach) if reach else np.zeros(0, F32)
    return out


# ---- the checker's frames, computed once per process ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cpu_model(encoder):
    import torch
    return model(torch.device("cpu"), encoder)


@functools.lru_cache(maxsize=None)
def checker_frame(regime, index, half=False):
    """run `index` of `regime` through the loop on the CPU checker (f32 net, or the f32 net on half tables); traced.  Shared: do not write
    into the arrays"""
    run = runs(regime)[index]
    out = render(CpuOps, checker_net(_cpu_model(run.encoder), half), run, trace=True)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- the conditions the inputs must meet (on anyone's counts: the checker's on the CPU, the GPU's own in the GPU file) ------------------
def step_shares(run, steps):
    """shares of the marched samples whose step equals dt_min, lies strictly between, equals dt_max"""
    dt_min, dt_max = step_bounds(run)
    n = max(steps.size, 1)
    return float((steps == dt_min).sum()) / n, float(((steps > dt_min) & (steps < dt_max)).sum()) / n, float((steps == dt_max).sum()) / n


def check_common(regime, frames):
    """every regime, per run: a ray with weights_sum > 0.5, a ray without a sample, a ray with more than 8, no NaN.  `axis` marches seven
    rays on two bitfields: on all-ones each of them crosses two units of occupied cells, so "a ray without a sample" is asked of the
    regime's runs together there (the ray at x = y = 0.5 on the ellipsoid).  Not asked of grid512 (the issue: half of its cells are set)."""
    for f in frames:
        for k in ("image", "image_raw", "depth", "weights_sum", "nears", "fars"):
            assert not np.isnan(f[k]).any(), (regime, k)
        assert (f["weights_sum"] > 0.5).any(), regime
        assert f["ray_counts"].max() > 8, regime
    empty = [bool((f["ray_counts"] == 0).any()) for f in frames]
    if regime == "axis":
        assert any(empty), regime
    elif regime != "grid512":
        assert all(empty), regime


def check_regime(regime, frames):
    """what the issue asks of each regime's inputs, on traced frames (one per run)"""
    rs = runs(regime)
    run, f = rs[0], frames[0]
    dz = run.rd[:, 2]
    lo, mid, hi = step_shares(run, f["steps"])
    dt_min, dt_max = step_bounds(run)
    if regime == "behind":
        assert (dz < 0).all()
    elif regime == "side":
        assert (dz < 0).mean() >= 1 / 3 and (dz > 0).mean() >= 1 / 3
    elif regime == "cascades":
        # the issue's bitfield ("two"): its level-1 ellipsoid has semi-axes 0.7 / 0.9 / 0.7, so no occupied cell and no sample lies outside
        # the unit cube, whatever the camera or the step.  The second run ("two_wide": 1.4 / 0.8 / 0.6, seen along x) is there for that condition, and
        # meets the step-share conditions as well.
        for r, g in zip(rs, frames):
            lo, mid, hi = step_shares(r, g["steps"])
            assert mid >= 0.1 and hi >= 0.1, (lo, mid, hi)
        assert int((frames[1]["reach"] > 1).sum()) >= 100
    elif regime == "var_dt":
        assert lo >= 0.1 and mid >= 0.1, (lo, mid, hi)
    elif regime == "inside":
        for r, g in zip(rs, frames):
            assert (g["nears"] == F32(r.min_near)).all()
        assert not np.array_equal(frames[0]["image"], frames[1]["image"])
    elif regime == "aabb":
        assert (f["nears"] > 1e30).any() and not (f["nears"] > 1e30).all()
    elif regime == "grid512":
        assert dt_min > dt_max and f["steps"].size > 0 and (f["steps"] == dt_max).all()
    elif regime == "odd":
        assert int((run.rd[:, 0] == 0).sum()) >= 37
    elif regime == "bound15":
        assert int((frames[1]["reach"] > 1).sum()) >= 100          # samples in cascade 1, where the box is [-1.5, 1.5]^3
    elif regime == "axis":
        for g in frames:
            assert (g["nears"] == 2).all() and (g["fars"] == 4).all()
