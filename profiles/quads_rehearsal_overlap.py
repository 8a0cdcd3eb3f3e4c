#!/usr/bin/env python3
"""Per-kernel statistics and the two-chain overlap of a `rocprofv3 --kernel-trace --stats` run of
profiles/time_quads_rehearsal.py (the rocpd SQLite database rocprofv3 writes):
    python3 profiles/quads_rehearsal_overlap.py RESULTS.db
Prints one JSON object: per kernel name the calls, total and mean microseconds; and for each kind of work on the exchange
stream during the two-chain runs (partition-boundary launch, RCCL send / receive kernel, pack / unpack) how many of its
launches ran while an interior launch of the solver's stream was running, and for how long on average."""
import json
import sqlite3
import sys


def main():
    db = sqlite3.connect(sys.argv[1])
    rows = db.execute("select name, stream_id, start, end, grid_x, workgroup_x from kernels order by start").fetchall()
    stats = {}
    for name, _, t0, t1, _, _ in rows:
        s = stats.setdefault(name.split("(")[0], [0, 0.0])
        s[0] += 1
        s[1] += (t1 - t0) / 1e3
    stage = [r for r in rows if "sw2d_quad_stage_kernel" in r[0]]
    # the solver's stream runs the interior launches (two chains), the whole-share launches (stream order) and the whole
    # mesh: three grid sizes, the interior one the smallest; the exchange stream runs pack, send / receive, unpack, boundary
    solver = max({r[1] for r in stage}, key=lambda s: sum(1 for r in stage if r[1] == s))
    inner_grid = min(r[4] for r in stage if r[1] == solver)
    inner = [r for r in stage if r[1] == solver and r[4] == inner_grid]
    t_lo, t_hi = inner[0][2], inner[-1][3]
    chain_b = [r for r in rows if r[1] != solver and t_lo <= r[2] <= t_hi]
    out = {"kernels": {k: {"calls": v[0], "total_us": round(v[1], 1), "mean_us": round(v[1] / v[0], 2)}
                       for k, v in sorted(stats.items(), key=lambda kv: -kv[1][1])},
           "interior_launches": len(inner),
           "mean_us_interior_launch": round(sum((r[3] - r[2]) / 1e3 for r in inner) / len(inner), 2)}
    for label, key in (("boundary_launch", "sw2d_quad_stage_kernel"), ("send_recv", "nccl"), ("pack_unpack", "bdg_halo")):
        mine = [r for r in chain_b if key in r[0]]
        side = []
        for _, _, b0, b1, _, _ in mine:
            side.append(max((min(b1, i1) - max(b0, i0) for _, _, i0, i1, _, _ in inner if i0 < b1 and b0 < i1), default=0) / 1e3)
        out[label] = {"launches": len(mine), "mean_us": round(sum((r[3] - r[2]) / 1e3 for r in mine) / max(len(mine), 1), 2),
                      "beside_an_interior_launch": sum(1 for v in side if v > 0),
                      "mean_us_side_by_side": round(sum(side) / max(len(side), 1), 2)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
