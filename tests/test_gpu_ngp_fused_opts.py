"""HashgridRenderer(mode="fused") with what the frame machinery offers next to the frame itself (lz_ngp_frame_render_opts /
lz_ngp_frame_finish): tiles of one frame under the reference's cap (frame_rays_total, fused_begin / fused_finish and the summed
histogram), occupancy clipping, perturb / noises and the RGB24 output.  Every comparison is torch.equal on image, image_raw,
weights_sum, depth and ray_counts plus state[5]; no tolerances.  The 48 x 48-ray ellipsoid scene and the GenericHashgridNeRF(seed=3) nets
are tests/test_gpu_ngp_fused.py's."""
import numpy as np
import pytest
import torch

import ngp_regimes as R
from test_gpu_ngp_fused import KEYS, LZF_CEFF, NETS, _sub, assert_same, nets, scene  # noqa: F401  (nets, scene: module-scoped fixtures)

pytestmark = pytest.mark.gpu
H = W = 48
CASE_B = dict(max_steps=16, T_thresh=1e-4)       # test_gpu_ngp_fused_spp.py's case B on the full ellipsoid: C_eff > 16
# three unequal contiguous row tiles.  The first -- the 13 top rows, mostly rays that miss the ellipsoid -- replays another schedule when
# it is rendered on its own (few rays alive against its own ray count: fatter chunks past the cap); test_tiles_are_the_frame asserts that.
ROW_TILES = ((0, 13), (13, 30), (30, 48))
ALL_S = (1, 2, 4, 8, 16, 0)


def clone(res):
    return {k: v.clone() for k, v in res.items()}


def renderer(net, bits, mode="fused", **ctor):
    from lzzx_nerf_amd.ngp import HashgridRenderer
    return HashgridRenderer(net, bits, mode=mode, **{"bound": 1.0, **ctor})


def frame(net, bits, ro, rd, mode="fused", ctor=None, **kw):
    out = clone(renderer(net, bits, mode, **(ctor or {})).render(ro, rd, count_samples=True, **kw))
    torch.cuda.synchronize()
    return out


def assert_frame(got, want):
    assert_same(want, got)
    assert int(got["state"][5]) == int(want["state"][5])


@pytest.fixture(scope="module")
def frames_b(nets, scene):
    """precision -> (loop, whole-frame fused) of case B: computed once, shared, not written into"""
    cache = {}

    def get(precision):
        if precision not in cache:
            cache[precision] = tuple(frame(nets[precision], scene["full"], scene["ro"], scene["rd"], mode=m, **CASE_B) for m in ("loop", "fused"))
        return cache[precision]
    return get


# ---- 1. tiles are the frame ------------------------------------------------------------------------------------------------------------
def tile_indices(split):
    rows = torch.arange(H * W, device="cuda").reshape(H, W)
    if split == "rows":
        return [rows[a:b].reshape(-1) for a, b in ROW_TILES]
    return [rows[k::3].reshape(-1) for k in range(3)]             # interleaved stripes of three tiles


def render_tiles(net, bits, ro, rd, tiles, S_of, total, **kw):
    """every tile on its own renderer: fused_begin on all, the histograms summed in place, fused_finish on all
    -> (the tiles put back into pixel order, sum of state[5], the tiles' own histograms)"""
    rs = [renderer(net, bits, steps_per_pass=S) for S in S_of]
    ctxs = []
    for r, idx in zip(rs, tiles):
        r.frame_rays_total = total
        ctxs.append(r.fused_begin(ro[idx].contiguous(), rd[idx].contiguous(), count_samples=True, **kw))
        assert ctxs[-1]["deferred"] and ctxs[-1]["hist"].shape == (kw["max_steps"] + 1,) and ctxs[-1]["hist"].dtype == torch.int32
    own = [c["hist"].clone() for c in ctxs]
    summed = torch.stack(own).sum(0).to(torch.int32)
    for c in ctxs:
        c["hist"].copy_(summed)
    outs = [r.fused_finish(c) for r, c in zip(rs, ctxs)]
    torch.cuda.synchronize()
    full = {}
    for k in KEYS:
        full[k] = torch.empty((ro.shape[0],) + tuple(outs[0][k].shape[1:]), dtype=outs[0][k].dtype, device="cuda")
        for idx, o in zip(tiles, outs):
            full[k][idx] = o[k]
    return full, sum(int(o["state"][5]) for o in outs), own, outs


@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("split", ["rows", "interleaved"])
@pytest.mark.parametrize("S_of", [(1, 1, 1), (4, 4, 4), (0, 0, 0), (16, 1, 4)], ids=["S1", "S4", "auto", "mixed"])
def test_tiles_are_the_frame(nets, scene, frames_b, precision, split, S_of):
    from lzzx_nerf_amd.dist import cap_schedule_from_histogram
    loop, whole = frames_b(precision)
    c_eff = int(whole["state"][LZF_CEFF])
    assert c_eff > 16 and int(whole["state"][9]) > 0
    tiles = tile_indices(split)
    assert sorted(torch.cat(tiles).tolist()) == list(range(H * W)) and len({int(t.numel()) for t in tiles}) == (3 if split == "rows" else 1)
    got, samples, own, outs = render_tiles(nets[precision], scene["full"], scene["ro"], scene["rd"], tiles, S_of, H * W, **CASE_B)
    for want in (whole, loop):
        assert_same(want, got)
        assert samples == int(want["state"][5])
    for o in outs:
        assert int(o["state"][LZF_CEFF]) == c_eff                 # every tile replayed the frame's schedule
    assert cap_schedule_from_histogram(torch.stack(own).sum(0).tolist(), H * W, 16)[0] == c_eff
    if split == "rows":
        # the condition on the input: some tile's own schedule is not the frame's, and that tile rendered alone is not the frame's pixels
        lone = [k for k, (h, idx) in enumerate(zip(own, tiles)) if cap_schedule_from_histogram(h.tolist(), int(idx.numel()), 16)[0] != c_eff]
        print("frame C_eff %d; tiles' own C_eff %s" % (c_eff, [cap_schedule_from_histogram(h.tolist(), int(i.numel()), 16)[0] for h, i in zip(own, tiles)]))
        assert lone
        idx = tiles[lone[0]]
        alone = frame(nets[precision], scene["full"], scene["ro"][idx].contiguous(), scene["rd"][idx].contiguous(), ctor=dict(steps_per_pass=S_of[lone[0]]),
                      **CASE_B)
        assert int(alone["state"][LZF_CEFF]) != c_eff
        differs = (alone["ray_counts"] != whole["ray_counts"][idx]) | (alone["image_raw"] != whole["image_raw"][idx]).any(1)
        print("rays of tile %d that differ when it is rendered alone: %d of %d" % (lone[0], int(differs.sum()), idx.numel()))
        assert int(differs.sum()) >= 1


def test_tiles_whole_in_begin_and_bad_total(nets, scene, frames_b):
    """cap "per_ray" and frame_rays_total = None return from fused_begin complete; frame_rays_total < N raises"""
    loop, whole = frames_b("f32")
    ro, rd = scene["ro"], scene["rd"]
    r = renderer(nets["f32"], scene["full"])
    ctx = r.fused_begin(ro, rd, count_samples=True, **CASE_B)
    assert not ctx["deferred"] and ctx["hist"] is None
    torch.cuda.synchronize()
    done = clone(dict(image=r._fbuf["out"], image_raw=r._fbuf["image"], weights_sum=r._fbuf["weights_sum"], depth=r._fbuf["depth"],
                      ray_counts=r._fbuf["ray_counts"], state=r._fbuf["state"]))
    assert_frame(done, whole)                                      # before fused_finish
    assert_frame(r.fused_finish(ctx), whole)
    per_ray = frame(nets["f32"], scene["full"], ro, rd, ctor=dict(cap="per_ray"), **CASE_B)
    r = renderer(nets["f32"], scene["full"], cap="per_ray")
    r.frame_rays_total = H * W                                     # no schedule under this cap: nothing to defer
    ctx = r.fused_begin(ro, rd, count_samples=True, **CASE_B)
    assert not ctx["deferred"] and ctx["hist"] is None
    assert_frame(r.fused_finish(ctx), per_ray)
    r = renderer(nets["f32"], scene["full"])
    r.frame_rays_total = H * W - 1
    with pytest.raises(ValueError, match="frame_rays_total"):
        r.fused_begin(ro, rd, **CASE_B)
    with pytest.raises(ValueError, match="frame_rays_total"):
        r.render(ro, rd, **CASE_B)
    with pytest.raises(RuntimeError, match="fused"):
        renderer(nets["f32"], scene["full"], mode="loop").fused_begin(ro, rd, **CASE_B)


def test_an_empty_tile_adds_nothing(nets, scene, frames_b):
    """a tile without rays next to a tile that holds the whole frame: zero histogram words, empty outputs"""
    loop, whole = frames_b("f32")
    tiles = [torch.arange(H * W, device="cuda"), torch.arange(0, device="cuda")]
    got, samples, own, outs = render_tiles(nets["f32"], scene["full"], scene["ro"], scene["rd"], tiles, (1, 4), H * W, **CASE_B)
    assert int(own[1].abs().sum()) == 0 and outs[1]["image"].shape == (0, 3) and outs[1]["ray_counts"].shape == (0,)
    assert_same(whole, got)
    assert samples == int(whole["state"][5])
    # through render(): the empty tile still takes part in the exchange (a collective between ranks), with zero words
    seen = []
    r = renderer(nets["f32"], scene["full"])
    r.frame_rays_total, r.cap_exchange = H * W, seen.append
    e = torch.empty(0, 3, device="cuda")
    o = r.render(e, e, count_samples=True, rgb24=True, **CASE_B)
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0].shape == (17,) and int(seen[0].abs().sum()) == 0
    assert o["image"].shape == (0, 3) and o["image_rgb24"].shape == (0, 3) and o["ray_counts"].shape == (0,) and int(o["state"][5]) == 0


# ---- 2. dist.ShardedFrame.configure ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", NETS)
def test_sharded_frame_configure(nets, scene, frames_b, precision):
    from lzzx_nerf_amd.dist import ShardedFrame
    loop, whole = frames_b(precision)
    sf = ShardedFrame(H, W, 0, 1, device="cuda", steps_per_pass=4, cap="reference")
    r = renderer(nets[precision], scene["full"], cap="per_ray")
    r.frame_rays_total, r.cap_exchange = 1, print
    assert sf.configure(r) is r
    assert (r.cap, r.steps_per_pass, r.frame_rays_total, r.cap_exchange) == ("reference", 4, None, None)
    got = clone(r.render(scene["ro"], scene["rd"], count_samples=True, **CASE_B))
    torch.cuda.synchronize()
    assert r.last_steps_per_pass == 4
    assert_frame(got, whole)
    assert_frame(got, loop)
    # what configure sets for a frame of several ranks, on the one rank there is: the frame's ray count and the exchange (called once,
    # between the two phases, with the histogram)
    seen = []
    r.frame_rays_total, r.cap_exchange = sf.H * sf.W, lambda h: seen.append(h.clone()) or sf.sum_over_ranks(h)
    got = clone(r.render(scene["ro"], scene["rd"], count_samples=True, **CASE_B))
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0].shape == (17,) and int(seen[0].sum()) == H * W and int(seen[0][16]) == int(whole["state"][9])
    assert_frame(got, whole)


# ---- 3. occupancy clipping -------------------------------------------------------------------------------------------------------------
def assert_box_inside(r):
    box, aabb = r.occupied_bounds().cpu(), r.aabb.cpu()
    assert bool((box[:3] > aabb[:3]).all()) and bool((box[3:] < aabb[3:]).all()), (box, aabb)


@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("bits", ["holes", "full", "two"])
def test_clip_equals_unclipped_and_loop(nets, scene, precision, bits):
    """clip_to_occupancy on == off == the loop, at every S under both caps (per_ray: the loop under the schedule (1, 1)); "two": two
    cascades, the bound-2 scene of test_fused_two_cascades"""
    net = nets[precision]
    if bits == "two":
        b, (ro, rd), ctor, kw = torch.cat([scene["full"], scene["holes"]]), _sub(scene, 1200, 9), dict(bound=2.0), dict(max_steps=64)
    else:
        b, (ro, rd), ctor, kw = scene[bits], (scene["ro"], scene["rd"]), {}, dict(CASE_B)
    for cap in ("reference", "per_ray"):
        loop = frame(net, b, ro, rd, mode="loop", ctor=dict(n_step_cap=8 if cap == "reference" else 1, **ctor), **kw)
        off = frame(net, b, ro, rd, ctor=dict(cap=cap, **ctor), **kw)
        assert_frame(off, loop)
        assert int(loop["ray_counts"].max()) >= 16 and int((loop["ray_counts"] == 0).sum()) > 0
        for S in ALL_S:
            r = renderer(net, b, cap=cap, steps_per_pass=S, clip_to_occupancy=True, **ctor)
            assert r.clip_to_occupancy and r.occupancy_margin == 8
            on = clone(r.render(ro, rd, count_samples=True, **kw))
            torch.cuda.synchronize()
            assert_box_inside(r)
            assert_frame(on, off)
            assert_frame(on, loop)
            # the clipped march ends are in use: inside the aabb's far on the rays that meet the box at all
            t_end, fars = r._fbuf["t_end"], r._fbuf["fars"]
            assert bool((t_end <= fars).all()) and int((t_end < fars).sum()) > 0


@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("fill", [0, 255])
def test_clip_uniform_bitfields(nets, scene, precision, fill):
    bits = torch.full_like(scene["full"], fill)
    ro, rd = _sub(scene, 700, 7)
    loop = frame(nets[precision], bits, ro, rd, mode="loop", max_steps=24)
    for S in (1, 4):
        on = frame(nets[precision], bits, ro, rd, ctor=dict(clip_to_occupancy=True, steps_per_pass=S), max_steps=24)
        assert_frame(on, loop)
    assert (int(loop["ray_counts"].sum()) == 0) == (fill == 0)


@pytest.mark.parametrize("precision", NETS)
def test_clip_follows_the_bitfield(nets, scene, precision):
    """an in-place change of the bitfield: a version bump is seen by itself, a write behind torch's back after invalidate_occupancy()"""
    net, ro, rd = nets[precision], scene["ro"], scene["rd"]
    want = {k: frame(net, scene[k], ro, rd, mode="loop", **CASE_B) for k in ("holes", "full")}
    r = renderer(net, torch.zeros_like(scene["full"]), clip_to_occupancy=True)
    none = clone(r.render(ro, rd, count_samples=True, **CASE_B))
    assert int(none["ray_counts"].sum()) == 0 and bool((r.occupied_bounds() > 1e30).all())      # no occupied cell: a box no ray reaches
    box0 = r.occupied_bounds()
    assert r.occupied_bounds() is box0                              # cached
    r.bitfield.copy_(scene["holes"])                                # bumps the version
    assert_frame(clone(r.render(ro, rd, count_samples=True, **CASE_B)), want["holes"])
    assert r.occupied_bounds() is not box0
    assert_box_inside(r)
    box1, version = r.occupied_bounds(), r.bitfield._version
    r.bitfield.zero_()
    assert_frame(clone(r.render(ro, rd, count_samples=True, **CASE_B)), none)
    r.bitfield.data.copy_(scene["full"])                            # .data: the same memory, no version bump
    assert r.bitfield._version == version + 1
    r.invalidate_occupancy()
    assert_frame(clone(r.render(ro, rd, count_samples=True, **CASE_B)), want["full"])
    assert r.occupied_bounds() is not box1
    torch.cuda.synchronize()


# ---- 4. perturb ------------------------------------------------------------------------------------------------------------------------
def draws(n, seed=11):
    u = torch.rand(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    u[0] = 0.0
    assert float(u.min()) == 0.0 and float(u.max()) < 1.0
    return u.cuda()


@pytest.mark.parametrize("precision", NETS)
def test_perturb_fused_equals_loop(nets, scene, precision):
    net, ro, rd = nets[precision], scene["ro"], scene["rd"]
    u = draws(ro.shape[0])
    for bits, kw in (("holes", dict(max_steps=128)), ("full", CASE_B)):
        loop = frame(net, scene[bits], ro, rd, mode="loop", noises=u, **kw)
        plain = frame(net, scene[bits], ro, rd, mode="loop", **kw)
        assert not torch.equal(loop["depth"], plain["depth"])       # the draws move the samples
        for S in (1, 4, 16):
            assert_frame(frame(net, scene[bits], ro, rd, ctor=dict(steps_per_pass=S), noises=u, **kw), loop)
        zero = torch.zeros_like(u)
        assert_frame(frame(net, scene[bits], ro, rd, noises=zero, **kw), plain)
        assert_frame(frame(net, scene[bits], ro, rd, mode="loop", noises=zero, **kw), plain)


@pytest.mark.parametrize("mode", ["loop", "fused"])
def test_perturb_arguments(nets, scene, mode):
    ro, rd = _sub(scene, 300, 3)
    r = renderer(nets["f32"], scene["holes"], mode)
    for bad in (draws(299), draws(301), draws(1)):
        with pytest.raises(RuntimeError, match="one value per ray"):
            r.render(ro, rd, max_steps=32, noises=bad)
    torch.manual_seed(5)
    a = clone(r.render(ro, rd, max_steps=32, perturb=True, count_samples=True))
    torch.manual_seed(5)
    u = torch.rand(300, dtype=torch.float32, device="cuda")          # what perturb draws without noises
    b = clone(r.render(ro, rd, max_steps=32, noises=u, count_samples=True))
    torch.cuda.synchronize()
    assert_frame(a, b)
    assert not torch.equal(a["depth"], r.render(ro, rd, max_steps=32)["depth"])


def checker_loop(net, run, noises):
    """ngp_regimes.render's loop on the CPU checker with the draws handed to march_rays on the FIRST iteration only
    (renderer.py:344,521)"""
    O, ops = R.O, R.CpuOps
    ro, rd, aabb, bits = run.ro, run.rd, run.aabb, R.bitfield(run.bits)
    N = ro.shape[0]
    nears, fars = O.near_far_from_aabb(ro, rd, aabb, run.min_near)
    ws, dep, img = ops.zeros(N), ops.zeros(N), ops.zeros(N, 3)
    alive, t = ops.arange(N), nears.copy()
    counts = np.zeros(N, np.int64)
    step = 0
    while step < run.max_steps:
        n_alive = alive.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        xyzs, dirs, dl = O.march_rays(n_alive, n_step, alive, t, ro, rd, run.bound, bits, run.cascade, run.grid_size, nears, fars, 128,
                                      noises if step == 0 else None, run.dt_gamma, run.max_steps)
        sig, rgb = net(xyzs, dirs, run.bound)
        np.add.at(counts, alive, (dl[: n_alive * n_step, 0] != 0).reshape(n_alive, n_step).sum(1))
        ops.composite(n_alive, n_step, alive, t, sig, rgb, dl, ws, dep, img, run.T_thresh)
        alive = ops.compact(alive)
        step += n_step
    return dict(image=np.clip(img + (1 - ws)[:, None], 0, 1).astype(np.float32), image_raw=img, depth=dep, weights_sum=ws, ray_counts=counts)


def test_perturb_equals_the_checker():
    """the f32 net, 40 x 40 rays (ngp_regimes' "side" run), both modes and S = 4 against the CPU checker: np.array_equal"""
    from test_gpu_ngp_regimes import assert_equals, nets as regime_nets
    run = R.runs("side")[0]
    u = draws(run.ro.shape[0], seed=12)
    want = checker_loop(R.checker_net(R.model(torch.device("cpu"), run.encoder), False), run, u.cpu().numpy())
    plain = R.checker_frame("side", 0)
    assert not np.array_equal(want["depth"], plain["depth"]) and (want["weights_sum"] > 0.5).any() and want["ray_counts"].max() > 8
    dev = R.GpuOps.to
    keys = ("image", "image_raw", "depth", "weights_sum", "ray_counts")
    for mode, S in (("loop", 1), ("fused", 1), ("fused", 4)):
        r = renderer(regime_nets(run.encoder)["f32"], dev(R.bitfield(run.bits)), mode, bound=run.bound, cascade=run.cascade, grid_size=run.grid_size,
                     aabb=dev(run.aabb), min_near=run.min_near, steps_per_pass=S)
        o = r.render(dev(run.ro), dev(run.rd), dt_gamma=run.dt_gamma, max_steps=run.max_steps, T_thresh=run.T_thresh, count_samples=True, noises=u)
        torch.cuda.synchronize()
        got = {k: o[k].cpu().numpy() for k in keys}
        got["ray_counts"] = got["ray_counts"].astype(np.int64)
        assert_equals(got, want, keys, (mode, S))


# ---- 5. RGB24 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("mode", ["loop", "fused"])
def test_rgb24(nets, scene, precision, mode):
    ro, rd = _sub(scene, 900, 13)
    bg = torch.rand(900, 3, generator=torch.Generator().manual_seed(17)).cuda()
    plain = frame(nets[precision], scene["holes"], ro, rd, mode=mode, max_steps=32, bg_color=bg)
    assert "image_rgb24" not in plain
    for S in ((1, 4) if mode == "fused" else (1,)):
        r = renderer(nets[precision], scene["holes"], mode, steps_per_pass=S)
        r.render(ro, rd, max_steps=32, bg_color=bg, rgb24=True)          # allocates the buffer that is then filled with a sentinel
        buf = (r._fbuf if mode == "fused" else r._buf)["out_rgb24"]
        buf.fill_(77)
        o = clone(r.render(ro, rd, max_steps=32, bg_color=bg, rgb24=True, count_samples=True))
        torch.cuda.synchronize()
        assert_frame(o, plain)
        want = (o["image"] * 255).to(torch.uint8)
        assert o["image_rgb24"].dtype == torch.uint8 and o["image_rgb24"].shape == (900, 3)
        assert torch.equal(o["image_rgb24"], want)
        assert int((want != 77).sum()) > 2000 and int(want.max()) > 200 and int(want.min()) < 50
    e = torch.empty(0, 3, device="cuda")
    o = renderer(nets[precision], scene["holes"], mode).render(e, e, max_steps=32, rgb24=True)
    assert o["image_rgb24"].dtype == torch.uint8 and o["image_rgb24"].shape == (0, 3)


# ---- 6. all options at once ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", NETS)
@pytest.mark.parametrize("n", [1, 5, 37 * 29])
def test_all_options_at_once(nets, scene, precision, n):
    """clipping, draws, RGB24 and the two-call frame (the tile holds the whole frame: frame_rays_total = n) into NaN-prefilled outputs"""
    ro, rd = _sub(scene, n, 100 + n)
    u = draws(n, seed=n)
    kw = dict(CASE_B, bg_color=0.3, noises=u, rgb24=True, count_samples=True)
    want = clone(renderer(nets[precision], scene["full"], "loop").render(ro, rd, **kw))
    for S in (1, 8, 0):
        r = renderer(nets[precision], scene["full"], steps_per_pass=S, clip_to_occupancy=True)
        r.frame_rays_total = n
        r.render(ro, rd, **kw)                                      # allocates the buffers that are then poisoned
        for k in ("out", "image", "weights_sum", "depth", "t_end"):
            r._fbuf[k].fill_(float("nan"))
        r._fbuf["ray_counts"].fill_(-12345)
        r._fbuf["out_rgb24"].fill_(77)
        got = r.render(ro, rd, **kw)
        torch.cuda.synchronize()
        for k in KEYS:
            assert not bool(torch.isnan(got[k].float()).any()), k
        assert not bool(torch.isnan(r._fbuf["t_end"]).any())
        assert_frame(got, want)
        assert torch.equal(got["image_rgb24"], want["image_rgb24"]) and torch.equal(got["image_rgb24"], (got["image"] * 255).to(torch.uint8))
