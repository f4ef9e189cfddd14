"""Register budget of the training march and training compositing kernels, from build.py's per-kernel report (lib/kernel_resources.json).
All 25 take rules from csrc/lz_composite_train.h -- the drop rule, the ray header, the per-sample step, the zero rows, the group walk, the
march start; which kernel takes which is in DESIGN.md -- so a change there must not cost any of them scratch, a spill, a wave of
occupancy, or move its LDS size (the launches rely on it)."""
import json
import os

import pytest

VARIANTS = ("Li0ELb0ELb0E", "Li1ELb0ELb0E", "Li1ELb1ELb0E", "Li1ELb0ELb1E", "Li2ELb0ELb1E")     # <NAMB, AMBW, UNC> as mangled

# mangled prefix: (occupancy at least, LDS bytes exactly)
BUDGET = {}
for _v in VARIANTS:
    BUDGET["_Z24lz_k_composite_train_fwdI%sE" % _v] = (2, 18464)
    BUDGET["_Z24lz_k_composite_train_bwdI%sE" % _v] = (2, 28736)
    BUDGET["_Z26lz_k_composite_train_fwd_gI%sE" % _v] = (5 if _v == "Li0ELb0ELb0E" else 4, 0)
    BUDGET["_Z26lz_k_composite_train_bwd_gI%sE" % _v] = (5 if _v in ("Li0ELb0ELb0E", "Li1ELb0ELb0E") else 4, 0)
BUDGET.update({
    "_Z22lz_k_march_train_countP": (8, 1024),
    "_Z22lz_k_march_train_writeP": (3, 47104),
    "_Z30lz_k_march_train_write_groupedP": (8, 1024),
    "_Z25lz_k_march_train_backwardP": (8, 0),
    "_Z33lz_k_march_train_backward_groupedP": (8, 0),
})


def _raymarch_resources():
    from lzzx_nerf_amd import build as B
    if not os.path.exists(B.RESOURCES) or not B.up_to_date():
        B.build(force=True)
    return json.load(open(B.RESOURCES))["lz_raymarch.hip"]


def test_budget_covers_every_training_kernel():
    names = [k for k in _raymarch_resources() if "lz_k_composite_train_" in k or "lz_k_march_train_" in k]
    assert len(names) == len(BUDGET) == 25, sorted(names)


@pytest.mark.parametrize("prefix", sorted(BUDGET))
def test_raymarch_kernel_resources(prefix):
    res = _raymarch_resources()
    names = [k for k in res if k.startswith(prefix)]
    assert len(names) == 1, names
    r = res[names[0]]
    occupancy, lds = BUDGET[prefix]
    assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, r
    assert r["occupancy"] >= occupancy, r
    assert r.get("lds", 0) == lds, r
