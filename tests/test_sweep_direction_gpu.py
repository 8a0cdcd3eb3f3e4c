"""Whole-mesh stage launches of the triangle solver alternate the direction in which every XCD walks its chunk of tiles
(StageParams::sweepBack, csrc/hip/sw2d_stage_tile.hpp); BDG_SW2D_SWEEP=forward, read when a solver is created, keeps every
launch forward. The order in which tiles run cannot change a result: both solvers must leave the same bits, on meshes small
enough that a wrong mapping (a tile taken twice, a tile skipped, a ragged last tile) shows: 286 elements (five 64-lane tiles,
a grid smaller than 8) and 650 elements (11 tiles: not a multiple of 8). Partitioned launches never sweep back.

The crossover to the one-tile-per-wave kernel and the tile walk of the state-once kernel are read once per process, so the
cases run in child processes."""
import json
import os
import sys

import pytest

from conftest import launch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCRIPT = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import blitzdg_amd.pyblitzdg as dg
from blitzdg_amd import sw2d
from blitzdg_amd.halo import LocalGroupSw2d
assert "torch" not in sys.modules
spec = json.loads(sys.argv[2])
SWITCH = "BDG_SW2D_SWEEP"


def fields(x, y, a):
    return (10.0 + a * np.exp(-10 * x * x - 10 * y * y), 0.3 * a * np.sin(3 * x + 1) * np.cos(2 * y),
            0.3 * a * np.cos(2 * x) * np.sin(3 * y - 1), 1.0 + 0.2 * a * np.cos(2 * x + y))


def sources(x, y):
    return {"zx": -0.5 + 0 * x, "zy": 0.5 * y, "f": 1e-1 * (1.0 + 0.5 * y), "CD": 2.5e-2}


def mesh_of(m):
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(m["nx"], m["ny"], shuffleSeed=m.get("seed", 0))
    return mesh


def created(forward, env, make):
    # the switches a case names are read when the solver is created (or per call: they stay set until the case is over)
    os.environ.update(env)
    if forward:
        os.environ[SWITCH] = "forward"
    try:
        return make()
    finally:
        os.environ.pop(SWITCH, None)


def run_single(c):
    nodes = dg.TriangleNodesProvisioner(c["order"], mesh_of(c["mesh"]))
    if c["kind"] in ("rk2", "ssprk2"):
        nodes.buildFilter(0.9 * c["order"], c["order"])
    ctx = nodes.dgContext()
    x, y = ctx.x, ctx.y
    four = c["kind"] == "four"
    out = {}
    for forward in (True, False):
        kw = dict(fields=4, sources=sources(x, y)) if four else {}
        s = created(forward, c.get("env", {}), lambda: sw2d.Sw2dSolver(nodes=nodes, flags=c.get("flags", 0), **kw))
        put = (lambda a: s.setState4(*fields(x, y, a))) if four else (lambda a: s.setState(*fields(x, y, a)[:3]))
        put(1.0)
        dt = 0.5 * s.computeDt(0.65)[0]
        if c["kind"] == "rk2":
            s.stepRK2(dt, 2, filter=True)
        elif c["kind"] == "ssprk2":
            s.stepSSPRK2(dt, 2, sponge=3.0)
        else:
            s.lserk4Stages(dt, 13)     # 2 steps + 3 stages
            put(0.7)                   # mid-step: the stage count restarts, the sweep parity does not
            s.lserk4Stages(dt, 7)
        out[forward] = (s.getState4() if four else s.getState(), s.backwardLaunches)
        s.close()
    for k in c.get("env", {}):
        os.environ.pop(k, None)
    (a, back_fwd), (b, back_def) = out[True], out[False]
    return {"equal": [bool(np.array_equal(p, q)) for p, q in zip(a, b)], "hu_max": float(np.abs(b[1]).max()),
            "finite": bool(all(np.isfinite(p).all() for p in b)), "backward": [back_fwd, back_def]}


def run_split(c):
    res = {}
    for forward in (True, False):
        g = created(forward, {}, lambda: LocalGroupSw2d(mesh_of(c["mesh"]), c["order"], 2))
        try:
            dt = None
            for a, n in ((1.0, 13), (0.7, 7)):
                g.set_initial_state(lambda x, y: fields(x, y, a)[:3])
                if dt is None:
                    dt = 0.5 * min(s.computeDt(0.65)[0] for s in g.solvers)
                g.lserk4_stages(dt, n)
            res[forward] = (g.gather_state(), [s.backwardLaunches for s in g.solvers],
                            [(p.num_interior, p.num_owned) for p in g.plans])
        finally:
            g.close()
    (a, back_fwd, parts), (b, back_def, _) = res[True], res[False]
    return {"equal": [bool(np.array_equal(p, q)) for p, q in zip(a, b)], "hu_max": float(np.abs(b[1]).max()),
            "finite": bool(all(np.isfinite(p).all() for p in b)), "backward": [back_fwd, back_def], "parts": parts}


print("RESULT " + json.dumps([run_split(c) if c["kind"] == "split" else run_single(c) for c in spec]))
"""

SWITCHES = ("BDG_SW2D_SWEEP", "BDG_SW2D_SMALL_LAUNCH", "BDG_SW2D_TILE_INTERLEAVE", "BDG_SW2D_FULL_STAGE_TRAFFIC",
            "BDG_SW2D_TRACER_PASS", "BDG_SW2D_AFFINE_VARIANT")


def _run(spec, process_env):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(process_env)
    r = launch([sys.executable, "-c", _SCRIPT, ROOT, json.dumps(spec)], env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, r.stdout[-2000:]
    return json.loads(line[-1][len("RESULT "):])


def _check(results, spec):
    assert len(results) == len(spec)
    for c, got in zip(spec, results):
        assert all(got["equal"]), (c, got)
        assert got["finite"] and got["hu_max"] > 1e-4, (c, got)   # (a state that is not at rest)
        back_forward, back_default = got["backward"]
        assert back_forward == 0, (c, got)                        # the switch: no launch walked backwards
        assert back_default > 0, (c, got)                         # the default solver really alternated


def _meshes():
    """286 elements as built; 650 shuffled elements as given and renumbered."""
    from blitzdg_amd import sw2d
    ragged = {"nx": 13, "ny": 11}
    shuffled = {"nx": 25, "ny": 13, "seed": 5}
    return [(ragged, 0), (shuffled, sw2d.KEEP_ORDER), (shuffled, sw2d.REORDER)]


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_unrolled_kernel_is_bit_identical_in_both_directions(order):
    """BDG_SW2D_SMALL_LAUNCH=0: the unrolled kernel also on these meshes; gathers through the face links (stage kinds FIRST, MID
    and LAST in both directions: 20 launches, odd number per step) and through vmapP with the residual in and out."""
    spec = [{"kind": "lserk", "order": order, "mesh": m, "flags": f, "env": e}
            for m, f in _meshes() for e in ({}, {"BDG_SW2D_FULL_STAGE_TRAFFIC": "1"})]
    if order == 4:
        spec += [{"kind": k, "order": 4, "mesh": m, "flags": f} for m, f in _meshes()[:2] for k in ("rk2", "ssprk2")]
    _check(_run(spec, {"BDG_SW2D_SMALL_LAUNCH": "0"}), spec)


@pytest.mark.parametrize("interleave", ["0", "1"])
def test_matrix_core_kernels_are_bit_identical_in_both_directions(interleave):
    """Default crossover: N = 4 on the one-tile-per-wave matrix-core kernel, N = 5, 6, 8 on the state-once kernel, whose waves
    walk several tiles -- side by side (BDG_SW2D_TILE_INTERLEAVE=1, the default) or a chunk each (=0); per-node geometry at
    N = 4 runs the same kernel's NODAL instance."""
    from blitzdg_amd import sw2d
    spec = [{"kind": "lserk", "order": n, "mesh": m, "flags": f} for n in (4, 5, 6, 8) for m, f in _meshes()]
    spec += [{"kind": k, "order": 4, "mesh": _meshes()[1][0], "flags": sw2d.KEEP_ORDER} for k in ("rk2", "ssprk2")]
    spec += [{"kind": "lserk", "order": 4, "mesh": m, "flags": f | sw2d.NODAL_GEOMETRY} for m, f in _meshes()[:2]]
    _check(_run(spec, {"BDG_SW2D_TILE_INTERLEAVE": interleave}), spec)


@pytest.mark.parametrize("small_launch", [None, "0"])
def test_four_fields_with_sources_and_the_tracer_in_its_own_launch(small_launch):
    """BDG_SW2D_TRACER_PASS=1: the tracer is a launch of its own behind the three-field launch (N = 4: the unrolled kernels
    with BDG_SW2D_SMALL_LAUNCH=0, N = 8: the state-once kernel with sources, then the tracer pass): two launches over the same
    elements in one evaluation, in opposite directions."""
    from blitzdg_amd import sw2d
    spec = [{"kind": "four", "order": n, "mesh": {"nx": 25, "ny": 13, "seed": 5}, "flags": sw2d.KEEP_ORDER,
             "env": {"BDG_SW2D_TRACER_PASS": "1"}} for n in (4, 8)]
    got = _run(spec, {} if small_launch is None else {"BDG_SW2D_SMALL_LAUNCH": small_launch})
    _check(got, spec)
    for g in got:   # 20 evaluations of two launches each: every evaluation has one backward launch
        assert g["backward"][1] == 20, g


def test_two_way_split_ignores_the_switch():
    """Partitioned launches (interior and partition-boundary) always walk forward: the interior launch orders its ring tiles
    last because they wait in the kernel for the previous boundary launch. Bit-identical with and without the switch, and no
    launch of either rank counted as backward."""
    spec = [{"kind": "split", "order": 4, "mesh": {"nx": 24, "ny": 20}}]
    got = _run(spec, {})
    g = got[0]
    assert all(g["equal"]) and g["finite"] and g["hu_max"] > 1e-4, g
    assert g["backward"] == [[0, 0], [0, 0]], g
    assert all(0 < i < o for i, o in g["parts"]), g
