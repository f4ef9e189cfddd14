#!/usr/bin/env python3
"""The A/B rule of profiles/r7_lean_stream_ab.json applied to a directory of bench.py result lines.

    python tools/ab_rule.py <dir> [--baseline parent] > profiles/<name>_ab.json

<dir> holds <variant>_<alternation>.json, each the JSON line of one `bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline` run, the
library builds alternating on one box.  A variant counts as a gain over the baseline when EVERY run of it is faster than EVERY run of the
baseline AND the mean difference is at least five times the larger of the two min-max spreads."""
import glob
import json
import os
import re
import sys


def main():
    d = sys.argv[1]
    base = sys.argv[sys.argv.index("--baseline") + 1] if "--baseline" in sys.argv else "parent"
    runs = {}
    for p in sorted(glob.glob(os.path.join(d, "*_[0-9]*.json"))):
        m = re.match(r"(.+)_(\d+)\.json$", os.path.basename(p))
        lines = [l for l in open(p).read().strip().splitlines() if l.startswith("{")]
        if not m or not lines:
            continue
        r = json.loads(lines[-1])
        roof = r.get("roofline", {})
        runs.setdefault(m.group(1), []).append({"alternation": int(m.group(2)), "ms_per_step": r["ms_per_step"],
                                                "kernel_avg_launch_ms": roof.get("avg_launch_ms"), "roofline_frac": r.get("roofline_frac")})
    stats = {}
    for v, rs in runs.items():
        ms = [x["ms_per_step"] for x in rs]
        stats[v] = {"mean": round(sum(ms) / len(ms), 4), "min": min(ms), "max": max(ms), "spread": round(max(ms) - min(ms), 4)}
    against = {}
    for v in runs:
        if v == base or base not in runs:
            continue
        diff = stats[base]["mean"] - stats[v]["mean"]
        need = 5 * max(stats[base]["spread"], stats[v]["spread"])
        every = stats[v]["max"] < stats[base]["min"]
        against[v] = {"mean_difference_ms": round(diff, 4), "percent": round(100 * diff / stats[base]["mean"], 2), "every_run_faster": every,
                      "five_times_larger_spread_ms": round(need, 4), "counts_as_gain": bool(every and diff >= need)}
    json.dump({"baseline": base, "runs": runs, "stats": stats, "against_" + base: against}, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
