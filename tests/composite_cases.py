"""Shared inputs of the training-compositing tests and a float64 autograd model of the operation (no GPU, no checker).

composite_rays_train* (raymarching.py:283-660) turns per-sample (sigma, rgb, ambient(s), uncertainty, dt, t) into per-ray sums and carries
every training step's gradient back.  The device kernels are pinned bit for bit to the CPU checker, the checker restates the reference's
kernel: neither says that the backward IS the derivative of the forward.  `model64` does: the forward written from its definition in
torch float64, the gradients by autograd.  tests/test_composite_model_host.py holds the model to closed forms and to central differences
of its own forward, measures the checker against it (MEASURED / BARS below), and tests/test_gpu_composite_model.py holds the kernels of
both sample layouts to the same bars.

CASES: rays tables [N, 3] = (id, offset, count) -- ids a random permutation, offsets = base + exclusive scan of the counts, counts always
containing 0, 1 and the edges of the kernels' 8-sample chunk (7, 8, 9, 15, 16, 17) and 33, shuffled so that empty rays sit inside groups
-- N around the 64-ray group, a counter base of 0 or 200 (rows in front of the first ray that no ray owns), and one of two endings: a tail
of 37 unowned rows, or a buffer cut inside a ray's range so that a suffix of the rays is dropped (raymarching.cu:457)."""
import functools

import numpy as np
import torch

# variant -> (n_amb, amb_weighted, has_unc), as the *_v entries of the C ABI take them
VARIANTS = {"ambient": (1, 0, 0), "sigma": (1, 1, 0), "uncertainty": (1, 0, 1), "triplane": (2, 0, 1)}
EDGE_COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 33)
T_THRESH = 1e-4
NEAR_REL = 1e-3          # a ray whose T after a visited sample is this close (relative) to T_thresh may stop a sample earlier / later in f32
NEAR_CAP = 0.02          # at most this share of a case's rays may be that close (asserted per case on the host)
TAIL = 37


def group_size():
    from lzzx_nerf_amd import _lib
    return int(_lib.load().lz_train_group_size())


def step_rows(rays, M):
    """ray-major row -> step-major row for every sample a ray owns: dict-free numpy restatement of the header's formula.
    rays [N, 3] (id, ray-major offset, count) in processing order; returns (src, dst): sample k of rays[i] sits at ray-major row src and
    step-major row dst (dropped rays own nothing)."""
    rays = np.asarray(rays, np.int64)
    src, dst = [], []
    G = group_size()
    for g0 in range(0, len(rays), G):
        grp = rays[g0:g0 + G]
        c = np.where(grp[:, 1] + grp[:, 2] <= M, grp[:, 2], 0)
        if c.max(initial=0) == 0:
            continue
        gb = grp[0, 1]
        alive = c[None, :] > np.arange(c.max())[:, None]                 # [k, j]
        pos = np.cumsum(alive.reshape(-1)).reshape(alive.shape) - 1       # k-major running index
        k, j = np.nonzero(alive)
        dst.append(gb + pos[k, j])
        src.append(grp[j, 1] + k)
    if not src:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(src), np.concatenate(dst)


# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
def _make_case(name, seed, N, base, ending, counts=None, T_thresh=T_THRESH, opaque=0):
    rng = np.random.default_rng(seed)
    if counts is None:
        counts = np.concatenate([np.array(EDGE_COUNTS), rng.integers(0, 40, N - len(EDGE_COUNTS))])
        rng.shuffle(counts)
    counts = np.asarray(counts, np.int64)
    assert len(counts) == N
    offs = base + np.concatenate([[0], np.cumsum(counts)[:-1]])
    ids = rng.permutation(N)
    rays = np.stack([ids, offs, counts], 1).astype(np.int32)
    total = base + int(counts.sum())
    if ending == "tail":
        M = total + TAIL
    else:                        # the last few rays do not fit, and M lands inside the range of the first of them
        p = max(i for i in range(N - 2) if counts[i] >= 2)
        M = int(offs[p] + counts[p] // 2)
    sigma = rng.uniform(0, 80, M)
    sigma[rng.random(M) < 0.2] = 0.0
    dt = rng.uniform(0.005, 0.03, M)
    t = np.full(M, 2.0)
    for o, c in zip(offs, counts):              # t increasing from 2 along every ray that fits
        if o + c <= M:
            t[o:o + c] = 2.0 + np.cumsum(dt[o:o + c])
    if opaque:                                  # alpha == 1 and T == 0 exactly, in float32 and in float64 (sigma dt >= 50)
        sigma[rng.choice(np.arange(base, total), opaque, replace=False)] = 1e4
    return case_from_arrays(name, rays, M, sigma, np.stack([dt, t], 1), rng.uniform(0, 1, (M, 3)), rng.uniform(0, 1, M),
                            rng.uniform(0, 1, M), rng.uniform(0, 1, M), T_thresh, rng, base=base, ending=ending)


def case_from_arrays(name, rays, M, sigma, deltas, rgb, amb0, amb1, unc, T_thresh, rng, upstream=None, **extra):
    """a case from explicit per-sample arrays (float32 copies are what every implementation reads); upstream gradients N(0, 1) from rng,
    except those given in `upstream`"""
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    rays = np.ascontiguousarray(rays, np.int32)
    N = len(rays)
    offs, counts = rays[:, 1].astype(np.int64), rays[:, 2].astype(np.int64)
    kept = (counts > 0) & (offs + counts <= M)
    owner = np.full(M, -1, np.int64)            # the position in rays[] of the ray that owns a row; -1: no ray's
    for n in np.nonzero(kept)[0]:
        owner[offs[n]:offs[n] + counts[n]] = n
    case = dict(name=name, N=N, M=M, T_thresh=T_thresh, rays=rays, kept=kept, owner=owner, sigma=f32(sigma), deltas=f32(deltas),
                rgb=f32(rgb), amb0=f32(amb0), amb1=f32(amb1), unc=f32(unc), **extra)
    for k, shape in (("g_weights_sum", N), ("g_amb0_sum", N), ("g_amb1_sum", N), ("g_unc_sum", N), ("g_depth", N), ("g_image", (N, 3)),
                     ("g_xyzs", (M, 3)), ("g_dirs", (M, 3))):          # upstream gradients; the last two feed the march's backward
        case[k] = f32(rng.normal(size=shape))
    for k, v in (upstream or {}).items():
        assert case[k].shape == np.shape(v)
        case[k] = f32(v).copy()
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)             # shared among the tests: nobody edits a case
    return case


def _build_cases():
    cases = []
    for i, N in enumerate((63, 64, 65, 130)):
        for j, base in enumerate((0, 200)):
            ending = "tail" if (i + j) % 2 == 0 else "drop"          # both endings under both bases
            cases.append(_make_case(f"n{N}_b{base}_{ending}", 100 + 10 * i + j, N, base, ending))
    # one kept ray of 9 samples behind 200 unowned rows, a tail behind it: the first ray is also the last
    cases.append(_make_case("n1_b200_tail", 7, 1, 200, "tail", counts=[9]))
    # the buffer ends inside the FIRST ray: every ray is dropped, all outputs and every gradient row are zero
    cases.append(_make_case("n3_b200_all_dropped", 9, 3, 200, "drop", counts=[9, 0, 5]))
    # T_thresh = 0 never stops a ray; a few opaque samples make T exactly 0 and the walk goes on over zero weights
    cases.append(_make_case("n65_b200_tail_T0", 8, 65, 200, "tail", T_thresh=0.0, opaque=12))
    return {c["name"]: c for c in cases}


CASES = _build_cases()
CASE_NAMES = list(CASES)


# ------------------------------------------------------------------------------------------------------------------------------------
# the float64 model
# ------------------------------------------------------------------------------------------------------------------------------------
def forward64(variant, case, sigma, rgb, amb0, amb1, unc):
    """the forward from its definition, float64 torch (differentiable in the five per-sample inputs, [M] / [M, 3] tensors in ray-major
    rows).  alpha = 1 - exp(-sigma dt), w = alpha T, image += w rgb, depth += w t, ws += w, unc_sum += w unc, ambient sums over the
    visited samples unweighted (weighted by w in the `sigma` variant), T *= 1 - alpha, the ray stops after the first sample that leaves
    T < T_thresh; an empty or dropped ray gives zeros.  Returns (outputs by RAY ID, near by position in rays[], visited per sample row)."""
    na, aw, hu = VARIANTS[variant]
    rays, M, N, th = case["rays"].astype(np.int64), case["M"], case["N"], case["T_thresh"]
    off, cnt, kept = rays[:, 1], rays[:, 2], case["kept"]
    C = int(max(cnt[kept].max(initial=0), 1))
    k = np.arange(C)
    valid = kept[:, None] & (k[None, :] < cnt[:, None])                      # [N, C]: sample k of ray n exists
    rows = torch.from_numpy(np.where(valid, off[:, None] + k[None, :], 0))
    valid = torch.from_numpy(valid)
    dl = torch.from_numpy(case["deltas"].astype(np.float64))
    dt, t = dl[:, 0][rows], dl[:, 1][rows]
    alpha = 1.0 - torch.exp(-sigma[rows] * dt)
    T = torch.ones(N, dtype=torch.float64)
    alive = torch.ones(N, dtype=torch.bool)
    near = torch.zeros(N, dtype=torch.bool)
    zero = torch.zeros(N, dtype=torch.float64)
    ws_cols, vis_cols = [], []
    for s in range(C):
        vis = alive & valid[:, s]
        ws_cols.append(torch.where(vis, alpha[:, s] * T, zero))
        vis_cols.append(vis)
        T = torch.where(vis, T * (1.0 - alpha[:, s]), T)
        Tn = T.detach()
        near |= vis & ((Tn - th).abs() < NEAR_REL * th)                       # (an empty band at T_thresh = 0: nothing stops there)
        alive = vis & ~(Tn < th)                                              # the sample that crossed the threshold was included
    w = torch.stack(ws_cols, 1)                                               # [N, C]
    visited = torch.stack(vis_cols, 1).to(torch.float64)
    ids = torch.from_numpy(rays[:, 0])
    by_id = lambda v: torch.zeros_like(v).index_copy(0, ids, v)
    amb_w = w if aw else visited
    out = dict(weights_sum=by_id(w.sum(1)), depth=by_id((w * t).sum(1)), image=by_id((w[:, :, None] * rgb[rows]).sum(1)),
               amb0_sum=by_id((amb_w * amb0[rows]).sum(1)))
    out["amb1_sum"] = by_id((amb_w * amb1[rows]).sum(1)) if na > 1 else None
    out["unc_sum"] = by_id((w * unc[rows]).sum(1)) if hu else None
    visited_row = torch.zeros(M, dtype=torch.bool)
    visited_row[rows[visited > 0]] = True
    return out, near, visited_row


def loss64(variant, case, out):
    """sum of upstream gradient x output over every output EXCEPT depth (grad_depth is not propagated, raymarching.py:323)"""
    g = lambda k: torch.from_numpy(case[k].astype(np.float64))
    loss = (g("g_weights_sum") * out["weights_sum"]).sum() + (g("g_image") * out["image"]).sum() + (g("g_amb0_sum") * out["amb0_sum"]).sum()
    if out["amb1_sum"] is not None:
        loss = loss + (g("g_amb1_sum") * out["amb1_sum"]).sum()
    if out["unc_sum"] is not None:
        loss = loss + (g("g_unc_sum") * out["unc_sum"]).sum()
    return loss


def inputs64(case):
    return [torch.from_numpy(case[k].astype(np.float64)) for k in ("sigma", "rgb", "amb0", "amb1", "unc")]


def _model64(variant, case):
    na, aw, hu = VARIANTS[variant]
    leaves = [x.requires_grad_(True) for x in inputs64(case)]
    out, near, visited = forward64(variant, case, *leaves)
    grads = torch.autograd.grad(loss64(variant, case, out), leaves, allow_unused=True)
    np64 = lambda v: None if v is None else v.detach().numpy()
    gs, gr, ga0, ga1, gu = [np.zeros(tuple(x.shape)) if g is None else g.numpy() for g, x in zip(grads, leaves)]
    grads = dict(grad_sigmas=gs, grad_rgbs=gr, grad_amb0=ga0, grad_amb1=ga1 if na > 1 else None, grad_unc=gu if hu else None)
    near = near.numpy()
    near_id = np.zeros(case["N"], bool)
    near_id[case["rays"][:, 0]] = near
    near_row = np.zeros(case["M"], bool)                                       # rows of the rays in `near`
    own = case["owner"] >= 0
    near_row[own] = near[case["owner"][own]]
    return dict(out={k: np64(v) for k, v in out.items()}, grads=grads, near=near, near_id=near_id, near_row=near_row, visited=visited.numpy())


@functools.lru_cache(maxsize=None)
def _model64_cached(variant, name):
    return _model64(variant, CASES[name])


def model64(variant, case):
    """float64 outputs (by ray id), the five gradient arrays of loss64 (ray-major rows, None where the variant has no such input) and
    `near` (by position in rays[]; `near_id` by ray id, `near_row` per sample row) and `visited` (per sample row: the walk took it).  Cached per (variant, case) for the shared CASES."""
    if CASES.get(case["name"]) is case:
        return _model64_cached(variant, case["name"])
    return _model64(variant, case)


def march_backward64(case):
    """march_rays_train's backward in float64: xyz = o + t d, dirs = d, so grad_o = sum g_xyz and grad_d = sum (t g_xyz + g_dirs) over
    the kept samples of a ray; an empty or dropped ray gets zero.  Rows by POSITION in rays[]."""
    rays = case["rays"].astype(np.int64)
    gx, gd, t = case["g_xyzs"].astype(np.float64), case["g_dirs"].astype(np.float64), case["deltas"][:, 1].astype(np.float64)
    go, gdd = np.zeros((case["N"], 3)), np.zeros((case["N"], 3))
    for n in np.nonzero(case["kept"])[0]:
        o, c = rays[n, 1], rays[n, 2]
        go[n] = gx[o:o + c].sum(0)
        gdd[n] = (t[o:o + c, None] * gx[o:o + c] + gd[o:o + c]).sum(0)
    return go, gdd


# ------------------------------------------------------------------------------------------------------------------------------------
# what a comparison with the model compares, and how far the float32 checker is from it
# ------------------------------------------------------------------------------------------------------------------------------------
def quantities(variant, out, grads):
    """{bar key: array} of one variant's outputs and gradients (dict access by the checker's names works for the model, the checker and
    device results alike).  The ambient channel has two keys each way: unweighted sums of up to 40 values in [0, 1) against sums weighted
    by w <= 1, and an unweighted ambient gradient that is the upstream value itself (no arithmetic: the bar is 0)."""
    na, aw, hu = VARIANTS[variant]
    q = dict(weights_sum=out["weights_sum"], depth=out["depth"], image=out["image"], grad_sigmas=grads["grad_sigmas"],
             grad_rgbs=grads["grad_rgbs"])
    amb, gamb = ("amb_sum_weighted", "grad_amb_weighted") if aw else ("amb_sum", "grad_amb")
    q[amb] = out["amb0_sum"] if na < 2 else np.stack([out["amb0_sum"], out["amb1_sum"]], -1)
    q[gamb] = grads["grad_amb0"] if na < 2 else np.stack([grads["grad_amb0"], grads["grad_amb1"]], -1)
    if hu:
        q["unc_sum"], q["grad_unc"] = out["unc_sum"], grads["grad_unc"]
    return q


PER_RAY = ("weights_sum", "depth", "image", "amb_sum", "amb_sum_weighted", "unc_sum", "grad_rays_o", "grad_rays_d")   # the rest: per sample row

# MEASURED[k]: the largest |checker - model64| of quantity k over every case and variant above, rays in `near` left out, measured by
# tests/test_composite_model_host.py::test_checker_is_within_the_recorded_bars_of_the_model on the CPU (it prints the table with -s and
# asserts that no figure here exceeds what it measures).  Magnitudes: depth 2-5, the unweighted ambient sums up to ~20, the gradients up
# to ~3, grad_rays_d (sums of ~20 terms t g_xyz + g_dirs, t ~ 2-3) up to ~50.
MEASURED = {
    "weights_sum": 2.45633185014249e-07,
    "depth": 7.747240795552557e-07,
    "image": 2.3905914259270133e-07,
    "amb_sum": 4.447996616363525e-06,
    "amb_sum_weighted": 1.71319881170362e-07,
    "unc_sum": 1.61064126924515e-07,
    "grad_sigmas": 1.302948019615835e-08,
    "grad_rgbs": 1.990008446917102e-07,
    "grad_amb": 0.0,
    "grad_amb_weighted": 1.3290413880540086e-07,
    "grad_unc": 1.7412308239705965e-07,
    "grad_rays_o": 2.6971101760864258e-06,
    "grad_rays_d": 1.2862760996767975e-05,
}
# The device kernels run the checker's operation sequence bit for bit, so their expected distance from the model IS the measured one; the
# factor covers the spread between cases, nothing else.
BAR_FACTOR = 4.0
BARS = {k: BAR_FACTOR * v for k, v in MEASURED.items()}


def max_abs_diff(got, want, skip=None):
    """largest |got - want| over the elements whose leading index is not in `skip` (bool mask over the first axis or None)"""
    d = np.abs(np.asarray(got, np.float64) - want)
    if skip is not None:
        d = d[~skip]
    return float(d.max(initial=0.0))
