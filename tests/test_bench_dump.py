"""bench.py --dump-outputs DIR: the state the timed stages computed, as float64 .npy files of at most 64 MB in all (a fixed,
seeded sample of element columns beyond that), the same bits in every run with the same arguments, so that two builds can
be compared output for output."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("h", "hu", "hv")


def _load(d):
    return [np.load(os.path.join(d, f"{n}.npy")) for n in FIELDS]


def test_dump_keeps_a_small_state_whole_and_samples_the_headline_state_the_same_way_every_time(tmp_path):
    import bench
    rng = np.random.default_rng(0)
    small = [rng.standard_normal((15, 300)) for _ in FIELDS]
    bench.dump_outputs(str(tmp_path / "small"), dict(zip(FIELDS, small)))
    for got, a in zip(_load(tmp_path / "small"), small):
        assert got.dtype == np.float64 and np.array_equal(got, a)

    # the headline's shape, 15 x 10^6 per field; every entry holds its element index (plus the field's number)
    k = 10**6
    big = {n: np.broadcast_to(np.arange(k, dtype=np.float64) + i, (15, k)) for i, n in enumerate(FIELDS)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big)
    assert sum(os.path.getsize(tmp_path / "a" / f"{n}.npy") for n in FIELDS) <= 64e6
    kept = None
    for i, (a, b) in enumerate(zip(_load(tmp_path / "a"), _load(tmp_path / "b"))):
        assert a.dtype == np.float64 and np.array_equal(a, b)
        cols = a[0] - i
        assert (a == a[0]).all() and np.array_equal(cols, np.unique(cols)) and 0 <= cols[0] and cols[-1] < k
        assert kept is None or np.array_equal(cols, kept)   # the same elements of every field
        kept = cols
    assert len(kept) >= 100000


@pytest.mark.gpu
def test_dump_is_the_state_after_warmup_plus_steps_stages_from_the_initial_state(tmp_path):
    """Two runs of bench.py with the clock ramp on (its length depends on the clocks) dump the same bits, and these are the
    state after exactly warm-up + steps LSERK4 stages from bench.py's initial state: --steps sets the timed stages."""
    import bench
    import blitzdg_amd.pyblitzdg as dg
    from blitzdg_amd import sw2d
    from conftest import launch

    warmup, steps = 3, 7
    for d in ("a", "b"):
        out = launch([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup),
                      "--cells", "60x40", "--no-also", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / d)],
                     cwd=ROOT, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == steps and line["config"]["elements"] == 4800

    mesh = dg.MeshManager()
    mesh.buildBoxMesh(60, 40)
    nodes = dg.TriangleNodesProvisioner(bench.ORDER, mesh)
    ctx = nodes.dgContext()
    solver = sw2d.Sw2dSolver(nodes=nodes, g=bench.G, device=0)
    solver.setState(*bench.initial_state(ctx.x, ctx.y))
    dt, _ = solver.computeDt(bench.CFL)
    solver.lserk4Stages(dt, warmup + steps - 1)
    one_short = solver.getState()
    solver.lserk4Stages(dt, 1)
    ref = solver.getState()
    for d in ("a", "b"):
        for got, r in zip(_load(tmp_path / d), ref):
            assert got.dtype == np.float64 and np.array_equal(got, r)
    assert not np.array_equal(one_short[1], ref[1])
