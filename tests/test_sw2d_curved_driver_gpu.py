"""The curved solver's driver on the device -- adaptive dt, blow-up check, the six output fields (sw2d_curved_driver_kernel.hpp;
reference sw2d_curved.py:231-302) -- against the NumPy restatement of tests/curved_driver_ref.py. The conditions of the cases
are checked without a GPU by tests/test_curved_driver_cases.py.

Meshes (tests/curved_cases.py): K = 8 (less than one 64-lane row), K = 84 = 64 + 20 (a ragged second row; shuffled: the curved
elements scattered over both rows). Every test here fails without the driver calls."""
import re

import numpy as np
import pytest

import curved_cases as cc
import curved_driver_ref as ref

pytestmark = pytest.mark.gpu

_SOLVERS = {}


def setup(order, mesh, shuffle=0):
    """(case, solver with the driver enabled: H = 1, c = sqrt(g)), made once per (order, mesh, shuffle)."""
    key = (order, mesh, shuffle)
    if key not in _SOLVERS:
        c = cc.problem(order, mesh[0], mesh[1], shuffle=shuffle)
        s = cc.solver(c)
        s.enableDriver(c.ctx, H=np.full_like(c.x, ref.H0), c=ref.wave_speed(c))
        _SOLVERS[key] = (c, s)
    return _SOLVERS[key]


def adaptive_setup(name):
    kw = ref.ADAPTIVE_CASES[name][0]
    c, s = setup(kw["order"], (kw["nx"], kw["ny"]), kw.get("shuffle", 0))
    return ref.case(name), s   # (the reference's own case object: same arguments, same tables)


def owned_dt(c, q, cs, cfl, owned):
    """The NumPy formula over the first `owned` elements."""
    K = c.K
    nf = np.asarray(c.ctx.vmapM).size // K
    import types
    ctx = types.SimpleNamespace(Fscale=c.ctx.Fscale[:, :owned], vmapM=np.asarray(c.ctx.vmapM).reshape(-1)[:nf * owned])
    cs = cs if np.ndim(cs) == 0 else cs[:, :owned]
    return ref.compute_dt(ctx, c.order, [a[:, :owned] for a in q], cs, cfl)


# ---- 1. computeDt

@pytest.mark.parametrize("order", range(1, 9))
def test_compute_dt_is_the_numpy_formula_bit_for_bit_on_one_ragged_row(order):
    c, s = setup(order, cc.SMALL_MESH)
    s.setState(*c.q)
    q = s.getState()
    assert s.computeDt(0.75) == ref.compute_dt(c.ctx, order, q, ref.wave_speed(c), 0.75)
    carr = ref.wave_speed(c) * (1.0 + 0.2 * np.sin(3 * c.x + c.y))
    s.enableDriver(c.ctx, H=np.full_like(c.x, ref.H0), c=carr)        # a second call replaces the tables
    try:
        assert s.computeDt(0.3) == ref.compute_dt(c.ctx, order, q, carr, 0.3)
    finally:
        s.enableDriver(c.ctx, H=np.full_like(c.x, ref.H0), c=ref.wave_speed(c))


@pytest.mark.parametrize("order", [3, 4])
@pytest.mark.parametrize("array_c", [False, True])
def test_compute_dt_finds_the_maximum_in_every_part_of_two_rows(order, array_c):
    """K = 84: the maximum planted in element 0, 63, 64 and 83 in turn, by scaling that element's momentum."""
    c, s = setup(order, cc.INSTANCE_MESH)
    cs = ref.wave_speed(c) * (1.0 + 0.2 * np.sin(3 * c.x + c.y)) if array_c else ref.wave_speed(c)
    s.enableDriver(c.ctx, H=np.full_like(c.x, ref.H0), c=cs)
    try:
        base = ref.compute_dt(c.ctx, order, c.q, cs, 0.25)[0]
        seen = set()
        for k in (0, 63, 64, 83):
            q = [a.copy() for a in c.q]
            q[1][:, k] *= 40.0
            q[2][:, k] *= 40.0
            s.setState(*q)
            got = s.computeDt(0.25)
            assert got == ref.compute_dt(c.ctx, order, s.getState(), cs, 0.25), k
            assert got[0] < 0.5 * base, k          # the planted element does hold the maximum
            seen.add(got[0])
        assert len(seen) == 4
    finally:
        s.enableDriver(c.ctx, H=np.full_like(c.x, ref.H0), c=ref.wave_speed(c))


# ---- 2. blow-up, owned elements

def test_blow_up_raises_and_ghost_columns_are_neither_read_nor_written():
    from blitzdg_amd import _capi as C
    c = cc.problem(3, *cc.INSTANCE_MESH)
    s = cc.solver(c)                        # a solver of its own: set_partition stays with it
    H = np.full_like(c.x, ref.H0)
    cs = ref.wave_speed(c)
    s.enableDriver(c.ctx, H=H, c=cs)
    q = [a.copy() for a in c.q]
    q[0][5, 83] = np.nan
    s.setState(*q)
    with pytest.raises(C.NumericalInstability):
        s.computeDt(0.25)
    s.setState(c.q[0] * 1e9, *c.q[1:])
    with pytest.raises(C.NumericalInstability):
        s.computeDt(0.25)
    s.setState(*c.q)
    s.computeDt(0.25)

    owned = 70
    C.check(C.lib.bdg_sw2d_curved_set_partition(s._h, 0, owned, None, 0))
    want = owned_dt(c, c.q, cs, 0.25, owned)
    assert s.computeDt(0.25) == want
    q = [a.copy() for a in c.q]
    q[0][2, 75] = np.nan          # a NaN and a huge speed in ghost columns
    q[1][:, 80] *= 1e12
    s.setState(*q)
    assert s.computeDt(0.25) == want
    # outputs: the ghost columns stay as the caller passed them
    IM, _ = c.nodes.splitOperators()
    for lat in (None, IM):
        out = [np.full((c.ctx.numLocalPoints, c.K), 7.0) for _ in ref.FIELDS]
        C.check(C.lib.bdg_sw2d_curved_output_fields(s._h, C.ptr(lat), *[C.ptr(o) for o in out]))
        assert all((o[:, owned:] == 7.0).all() for o in out)
        assert all(np.isfinite(o[:, :owned]).all() and (o[:, :owned] != 7.0).any() for o in out)
    r, bound = ref.lattice(IM, q[0][:, :owned])
    assert (np.abs(out[4][:, :owned] - r) <= bound).all()
    nodal = s.outputFields()
    assert np.array_equal(nodal["u"][:, :owned], (q[1] / q[0])[:, :owned]) and (nodal["u"][:, owned:] == 0).all()


# ---- 3. runAdaptive

@pytest.mark.parametrize("name", sorted(ref.ADAPTIVE_CASES))
def test_run_adaptive_is_the_scripts_loop(name):
    c, s = adaptive_setup(name)
    n = ref.ADAPTIVE_CASES[name][1]
    cs = ref.wave_speed(c)
    # (a) one call
    s.setState(*c.q)
    dt0, _ = s.computeDt(ref.CFL)
    t_a, dt_a, steps = s.runAdaptive(ref.CFL, np.inf, maxSteps=n)
    q_a = s.getState()
    assert steps == n
    # (b) n calls of one step
    s.setState(*c.q)
    t, dt = 0.0, None
    for _ in range(n):
        t, dt, st = s.runAdaptive(ref.CFL, np.inf, t=t, dt=dt, maxSteps=1)
        assert st == 1
    assert (t, dt) == (t_a, dt_a) and all(np.array_equal(a, b) for a, b in zip(s.getState(), q_a))
    # (c) by hand
    s.setState(*c.q)
    t, dt, dts = 0.0, dt0, []
    for _ in range(n):
        s.stepRK2(dt, 1, filter=True)
        t += dt
        dts.append(dt)
        dt, _ = s.computeDt(ref.CFL)
        assert dt == ref.compute_dt(c.ctx, c.order, s.getState(), cs, ref.CFL)[0]
    assert (t, dt) == (t_a, dt_a) and all(np.array_equal(a, b) for a, b in zip(s.getState(), q_a))
    assert len(set(dts)) == n
    # the reference loop
    loop, last_dt = ref.adaptive_loop(name)
    scale = max(np.abs(a).max() for a in loop[-1][2])
    err = max(np.abs(a - b).max() for a, b in zip(q_a, loop[-1][2])) / scale
    dt_err = max(abs(a - b) / b for a, b in zip(dts + [dt_a], [d for d, _, _ in loop] + [last_dt]))
    print(name, "state error", err, "largest relative dt error", dt_err)
    assert err < ref.STATE_TOL and dt_err < ref.STATE_TOL
    assert abs(t_a - loop[-1][1]) < ref.STATE_TOL * loop[-1][1]
    # final_time below t: nothing runs
    assert s.runAdaptive(ref.CFL, t_a - 1.0, t=t_a, dt=dt_a) == (t_a, dt_a, 0)
    assert all(np.array_equal(a, b) for a, b in zip(s.getState(), q_a))


# ---- 4. outputFields

def check_outputs(c, s, q, tag):
    IM, _ = c.nodes.splitOperators()
    H = np.full_like(c.x, ref.H0)
    worst = {}
    for lat in (None, IM):
        got = s.outputFields(lat)
        want = ref.output_reference(c.ctx, q, H, lat)
        assert tuple(got) == ref.FIELDS
        for k in ref.FIELDS:
            r, bound = want[k]
            err = np.abs(got[k].astype(np.longdouble) - r)
            if lat is None and k != "vort":
                assert np.array_equal(got[k], r), (tag, k)
                continue
            ratio = float((err / bound).max())
            worst[(k, lat is not None)] = ratio
            assert (err <= bound).all(), (tag, k, lat is not None, ratio)
    print(tag, "largest error / bound:", {f"{k}{'+IM' if lat else ''}": round(v, 4) for (k, lat), v in worst.items()})
    # a subset of the fields: the same values
    some = s.outputFields(None, fields=("vort", "B"))
    full = s.outputFields(None)
    assert tuple(some) == ("vort", "B") and all(np.array_equal(some[k], full[k]) for k in some)
    return worst


@pytest.mark.parametrize("order", range(1, 9))
def test_output_fields_on_one_ragged_row(order):
    c, s = setup(order, cc.SMALL_MESH)
    s.setState(*c.q)
    check_outputs(c, s, s.getState(), f"N{order} K8")


@pytest.mark.parametrize("order", [3, 4])
def test_output_fields_on_two_rows_with_scattered_curved_elements(order):
    c, s = setup(order, cc.INSTANCE_MESH, cc.INSTANCE_SHUFFLE)
    assert (c.deformed < 64).any() and (c.deformed >= 64).any()
    s.setState(*c.q)
    check_outputs(c, s, s.getState(), f"N{order} K84 shuffled")


# ---- 5. rigid rotation

@pytest.mark.parametrize("order", [4, 8])
def test_rigid_rotation_has_vorticity_two_on_curved_elements(order):
    c, s = setup(order, cc.INSTANCE_MESH if order == 4 else cc.SMALL_MESH, cc.INSTANCE_SHUFFLE if order == 4 else 0)
    assert c.deformed.size > 0
    h = np.ones_like(c.x)
    s.setState(h, -c.y, c.x, 0.5 * h)
    vort = s.outputFields(fields=("vort",))["vort"]
    bound = ref.vorticity_bound(c.ctx, -c.y, c.x)
    err = np.abs(vort - 2.0)
    print(f"N{order}: largest |vort - 2| / bound", (err / bound).max(), "on curved elements", (err / bound)[:, c.deformed].max())
    assert (err <= bound).all()


# ---- 6. *.vtu

def point_data(path, name):
    raw = open(path, "rb").read()
    head, rest = raw.split(b"<AppendedData encoding=\"raw\">", 1)
    blob = rest[rest.index(b"_") + 1:]
    m = re.search(r'<DataArray type="Float64" Name="%s" format="appended" offset="(\d+)"/>' % name, head.decode())
    off = int(m.group(1))
    nbytes = int(np.frombuffer(blob[off:off + 8], dtype="<u8")[0])
    return np.frombuffer(blob[off + 8:off + 8 + nbytes], dtype="<f8")


def test_write_solver_fields_writes_the_six_files(tmp_path):
    import blitzdg_amd.pyblitzdg as dg
    c, s = setup(3, cc.INSTANCE_MESH, cc.INSTANCE_SHUFFLE)
    s.setState(*c.q)
    q = s.getState()
    out = dg.VtkOutputter(c.nodes)
    dev, host = tmp_path / "dev", tmp_path / "host"
    for d in (dev, host):
        d.mkdir()
    paths = out.writeSolverFields(s, 50, directory=str(dev))
    assert [p.split("/")[-1] for p in paths] == [f"{k}0000050.vtu" for k in ref.FIELDS]
    IM, tri = c.nodes.splitOperators()
    cut = lambda a: np.asarray(a, dtype=np.float64)[tri.T, :].transpose(0, 2, 1).reshape(3, -1)  # noqa: E731  (the writer's cut)
    H = np.full_like(c.x, ref.H0)
    f = ref.pointwise_fields(q, H)
    f["vort"] = ref.vorticity(c.ctx, f["u"], f["v"])
    want = ref.output_reference(c.ctx, q, H, IM)
    for k in ref.FIELDS:
        hp = host / out.generateFileName(k, 50)
        out.writeFieldToFile(str(hp), f[k], k)
        got, exp = point_data(dev / hp.name, k), point_data(hp, k)
        assert got.shape == exp.shape and got.size == 3 * c.order ** 2 * c.K
        # the order in which the file holds the corners of the cut: whichever reproduces the host's file
        lat = cut(IM @ f[k])
        flat = [o for o in "CF" if np.allclose(lat.ravel(o), exp, rtol=0, atol=1e-12 * np.abs(exp).max())]
        assert len(flat) == 1, (k, flat)
        bound = cut(want[k][1]).ravel(flat[0])
        assert (np.abs(got - exp) <= bound).all(), (k, (np.abs(got - exp) / bound).max())
        head_dev = open(dev / hp.name, "rb").read().split(b"<AppendedData")[0]
        assert head_dev == open(hp, "rb").read().split(b"<AppendedData")[0]


# ---- 7. refusals

def test_refusals():
    from blitzdg_amd import _capi as C
    c = cc.problem(2, *cc.SMALL_MESH)
    s = cc.solver(c)
    s.setState(*c.q)
    for call in (lambda: s.computeDt(0.25), lambda: s.runAdaptive(0.25, 1.0, dt=1e-3), lambda: s.outputFields(),
                 lambda: s.timeDriver("dt", 1)):
        with pytest.raises(C.BdgError, match="enable_driver") as e:
            call()
        assert e.value.code == C.BDG_ERR_ARGUMENT
    bad = types_ctx(c.ctx)
    bad.vmapM = np.asarray(c.ctx.vmapM).reshape(-1).copy()
    bad.vmapM[5] += c.ctx.numLocalPoints                      # one entry moved to another element
    with pytest.raises(C.BdgError, match="not a node of that element"):
        s.enableDriver(bad, c=1.0)
    with pytest.raises(C.BdgError, match="enable_driver"):    # ... and nothing was changed
        s.computeDt(0.25)
    bad.vmapM = np.asarray(c.ctx.vmapM).reshape(-1).copy()
    nf = bad.vmapM.size // c.K
    bad.vmapM[nf + 1], bad.vmapM[nf + 2] = bad.vmapM[nf + 2], bad.vmapM[nf + 1]   # element 1 lists its face nodes in another order
    with pytest.raises(C.BdgError, match="differs from element 0"):
        s.enableDriver(bad, c=1.0)
    with pytest.raises(ValueError, match="c is required"):
        s.enableDriver(c.ctx)
    s.enableDriver(c.ctx, c=ref.wave_speed(c))                # H = None: eta = h
    assert np.array_equal(s.outputFields()["eta"], c.q[0])
    assert s.timeDriver("dt", 2) > 0 and s.timeDriver("output", 2) > 0


def test_run_adaptive_refuses_a_solver_with_a_communicator():
    """A solver on rank 0's share of a 2-way split, its communicator a loopback through the real transport (as
    test_sw2d_curved_gpu.test_native_curved_exchange_through_real_rccl_loopback makes one)."""
    import blitzdg_amd.pyblitzdg as dg
    from blitzdg_amd import _capi as C
    from blitzdg_amd.halo import build_plan
    from blitzdg_amd.sw2d_curved import NativeDistributedSw2dCurved
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(6, 4)
    mesh.partitionMesh(2)
    plan = build_plan(mesh.elements, mesh.vertices, mesh.EToE, mesh.elementPartitionMap, 0, 2, bctype=mesh.bcType)
    nat = NativeDistributedSw2dCurved(plan, 2, cc.deform, g=cc.G, filter_args=(1.8, 2), loopback=True)
    s = nat.solver
    s.enableDriver(nat.ctx, c=0.2)
    nat.set_initial_state(lambda x, y: cc.fields(x, y))
    with pytest.raises(C.BdgError, match="communicator") as e:
        s.runAdaptive(0.25, 1.0)
    assert e.value.code == C.BDG_ERR_ARGUMENT
    assert s.computeDt(0.25)[0] > 0                            # the rank-local dt is still there


def types_ctx(ctx):
    import types
    return types.SimpleNamespace(**{k: getattr(ctx, k) for k in ("Fscale", "vmapM", "Dr", "Ds", "rx", "sx", "ry", "sy")})
