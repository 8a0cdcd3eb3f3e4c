"""The time steppers of every sw2d kernel family against the CPU oracle (three fields) and a NumPy replay (four fields).

The combine steps (MODE_COMBINE: midpoint RK2 of sw2d-simple, src/sw2d-simple/main.cpp:132-151; SSP-RK2 + sponge of the tidal
driver, src/sw2d/main.cpp:211-235) and the LSERK4 stages are compiled separately in every family, each with its own epilogue, and
the filter reaches them through pre-multiplied operator images. A wrong RK coefficient, a sponge on the wrong field or a wrong
filtered image conserves mass and keeps the symmetry, so only a comparison with a reference catches it.

The ragged mesh: a shuffled 23 x 19 box, K = 874 elements. 14 workgroups of 64 (ceil(K/64) % 8 = 6, so the XCD tile remap at the
top of every vector kernel takes its `xcd < r8` branch both ways), K % 64 = 26 and K % 16 = 10 (ragged last wave and last
matrix-core tile). Each case runs in the mesh's element order (KEEP_ORDER) and renumbered (REORDER: the face links through the
permutation).

Which kernel a pinned BDG_SW2D_AFFINE_VARIANT runs (the numbers are the values of AffineVariant in sw2d_launch.hpp; sw2d_order.hip:
stageAffine with launchAffine, launchStream and launchRolled; sw2d_device.hip: launchStage, which takes 5, 6 and 7 to stageMfma,
stageMfma2 and stageMfma3). A pinned variant bypasses the small-launch crossover. "split" is the rolled field-split kernel
(sw2d_stage_affine_rolled_kernel, FIELDS = 1, one field per wave); "unrolled" is sw2d_stage_affine_kernel (LSERK at N <= 4: the
face-link FIRST / MID / LAST instances; combine with a sponge: the SPONGE instance).

  variant  N      LSERK stage                          combine (RK2, SSP-RK2 +- sponge)
  0        1-6    unrolled                             unrolled
           7-8    split                                split
  1        1-8    split                                split
  2, 3     1-5    streamed, 2 / 3 waves per SIMD       streamed, 2 / 3 waves per SIMD
           6-8    split                                split
  4        1-6    rolled, three fields per lane        rolled, three fields per lane
           7-8    split                                split
  5        1-8    matrix cores, whole tile (mfma)      matrix cores, whole tile
  6        1-8    matrix cores, face by face (mfma2)   matrix cores, face by face
  7        1-8    matrix cores, state once (mfma3)     matrix cores, state once
  8        1-5    lean kernel, 2 waves per SIMD        as variant 0
           6-8    as variant 0                         as variant 0
  9        1-5    in-wave LDS exchange (xchg)          as variant 0
           6-8    as variant 0                         as variant 0

Without a pin, N <= 4 runs variant 0 on launches of at least kSmallLaunch[N] elements (4 000 / 10 000 / 160 000 / 160 000) and
variant 5 below; N >= 5 runs variant 7. The crossover tests hold the default to the oracle on both sides of it, and bit for bit to
the family the rule names.

The four-field solvers (tracer only; variant D: tracer, Coriolis array, drag, bed slope) take their combine steps on the unrolled
source kernel with the tracer fused (N <= 4), the state-once matrix-core source kernel (N = 5, 6 with the tracer; N = 8 with the
tracer as a second phase), the rolled kernel (BDG_SW2D_ROLLED_SOURCES), the two-wave matrix-core kernels
(BDG_SW2D_SOURCES_TWO_WAVE) or with the tracer in its own pass (BDG_SW2D_TRACER_PASS). The sponge relaxes hu and hv only
(src/sw2d/main.cpp:223-235); h and the tracer are written unsponged.

Tolerances: states per field to 1e-11 of the field's own size (assert_fields_close), dt bit for bit.
"""
import itertools

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
from blitzdg_amd import sw2d
from conftest import oracle_from, relmax, seeded_fields, tables_from_nodes
from regimes import SOURCE_ENVS, assert_fields_close, regime_fields

pytestmark = pytest.mark.gpu

STATE_TOL = 1e-11
CFL = 0.65
SPONGE = 0.05
RAGGED = (23, 19, 7)              # nx, ny, shuffle seed: K = 874
# kSmallLaunch (sw2d_device.hip): the launch size from which N <= 4 runs the unrolled kernel instead of the matrix cores
SMALL_LAUNCH = {1: 4000, 2: 10000, 3: 160000, 4: 160000}
# (nx, ny) just above and just below the crossover, each with ceil(K/64) % 8 != 0, K % 64 != 0 and K % 16 != 0
CROSSOVER_MESHES = {1: {"above": (49, 41), "below": (44, 45)}, 2: {"above": (71, 71), "below": (70, 71)},
                    3: {"above": (283, 283), "below": (282, 283)}, 4: {"above": (283, 283), "below": (282, 283)}}


def _assert_ragged(K):
    assert -(-K // 64) % 8 != 0 and K % 64 != 0 and K % 16 != 0, K


def _box(order, nx, ny, seed):
    m = dg.MeshManager()
    m.buildBoxMesh(nx, ny, shuffleSeed=seed)
    nodes = dg.TriangleNodesProvisioner(order, m)
    nodes.buildFilter(0.9 * order, order)
    return nodes, tables_from_nodes(nodes)


def _amplified(q):
    """The state with 20 times the momentum: large enough that the sponge x /= 1 + s x^2 changes hu and hv visibly."""
    return q[0], 20.0 * q[1], 20.0 * q[2]


_RAGGED = {}


def _ragged(order):
    """The ragged mesh at `order` with its tables and the oracle, shared by every test of this module."""
    if order not in _RAGGED:
        nodes, t = _box(order, *RAGGED)
        _assert_ragged(t["rx"].shape[1])
        _RAGGED[order] = (nodes, t, oracle_from(t, threads=4))
    return _RAGGED[order]


_REF3 = {}


def _reference3(order):
    """Oracle results of every stepper on the ragged mesh, computed once per order and shared by the ten variants and both
    element orders."""
    if order in _REF3:
        return _REF3[order]
    nodes, t, o = _ragged(order)
    x, y = t["x"], t["y"]
    zero = [np.zeros_like(x) for _ in range(3)]
    r = {"q0": seeded_fields(x, y, seed=order), "q1": seeded_fields(x, y, seed=order + 100)}
    r["dt"] = dt = o.dt(*r["q0"], CFL, order)
    r["lserk13"] = o.lserk4_stages(*r["q0"], zero, dt, 0, 13)[:3]
    r["lserk7"] = o.lserk4_stages(*r["q1"], zero, dt, 0, 7)[:3]      # after setState: stage 0, residual zero
    for filt in (True, False):
        r["rk2", filt] = o.step_rk2(*r["q0"], dt, 3, filter=filt)
    r["qs"] = _amplified(r["q0"])
    r["dts"] = dts = 0.3 * o.dt(*r["qs"], CFL, order)
    for filt, sp in itertools.product((True, False), (0.0, SPONGE)):
        r["ssp", filt, sp] = o.step_ssprk2(*r["qs"], dts, 2, filter=filt, sponge=sp)
    for filt in (True, False):     # the sponge must matter: far more than the tolerance, on both momentum fields
        for c in (1, 2):
            assert relmax(r["ssp", filt, SPONGE][c], r["ssp", filt, 0.0][c]) > 1e4 * STATE_TOL
    # the jumpy state (a depth that jumps at every face) for one short run of each stepper, at a quarter of the CFL step
    r["qj"] = qj = regime_fields(x, y, "jumpy", seed=order)
    r["dtj_cfl"] = o.dt(*qj, CFL, order)
    dtj = r["dtj"] = 0.25 * r["dtj_cfl"]
    r["jumpy", "lserk"] = o.lserk4_stages(*qj, zero, dtj, 0, 4)[:3]
    r["jumpy", "rk2"] = o.step_rk2(*qj, dtj, 1, filter=True)
    r["jumpy", "ssp"] = o.step_ssprk2(*qj, dtj, 1, filter=True, sponge=SPONGE)
    for k in ("lserk", "rk2", "ssp"):
        assert r["jumpy", k][0].min() > 0
    _REF3[order] = r
    return r


@pytest.mark.parametrize("flags", [sw2d.KEEP_ORDER, sw2d.REORDER], ids=["keep", "reorder"])
@pytest.mark.parametrize("variant", range(10))
@pytest.mark.parametrize("order", range(1, 9))
def test_every_three_field_family_steps_like_the_oracle(order, variant, flags, monkeypatch):
    """One pinned family (module docstring table) on the ragged mesh: computeDt bit for bit; 13 LSERK4 stages (two steps and
    three stages: FIRST, MID and LAST twice), setState part-way through a step, 7 more stages; midpoint RK2 with and without the
    filter; SSP-RK2 with the filter on and off and the sponge on and off; and one short run of each stepper on the jumpy state."""
    monkeypatch.setenv("BDG_SW2D_AFFINE_VARIANT", str(variant))
    r = _reference3(order)
    nodes = _ragged(order)[0]
    s = sw2d.Sw2dSolver(nodes=nodes, flags=flags)
    assert s.isRenumbered == (flags == sw2d.REORDER)
    s.setState(*r["q0"])
    dt, _ = s.computeDt(CFL)
    assert dt == r["dt"]
    s.stepLSERK4(dt, 2)
    s.lserk4Stages(dt, 3)
    assert_fields_close(s.getState(), r["lserk13"], STATE_TOL, what="13 LSERK4 stages")
    s.setState(*r["q1"])
    s.lserk4Stages(dt, 7)
    assert_fields_close(s.getState(), r["lserk7"], STATE_TOL, what="7 LSERK4 stages after setState")
    for filt in (True, False):
        s.setState(*r["q0"])
        s.stepRK2(dt, 3, filter=filt)
        assert_fields_close(s.getState(), r["rk2", filt], STATE_TOL, what=f"RK2 filter={filt}")
    for filt, sp in itertools.product((True, False), (0.0, SPONGE)):
        s.setState(*r["qs"])
        s.stepSSPRK2(r["dts"], 2, filter=filt, sponge=sp)
        assert_fields_close(s.getState(), r["ssp", filt, sp], STATE_TOL, what=f"SSP-RK2 filter={filt} sponge={sp}")
    qj, dtj = r["qj"], r["dtj"]
    runs = {"lserk": lambda: s.lserk4Stages(dtj, 4), "rk2": lambda: s.stepRK2(dtj, 1, filter=True),
            "ssp": lambda: s.stepSSPRK2(dtj, 1, filter=True, sponge=SPONGE)}
    for name, run in runs.items():
        s.setState(*qj)
        if name == "lserk":
            assert s.computeDt(CFL)[0] == r["dtj_cfl"]
        run()
        got = s.getState()
        assert got[0].min() > 0
        assert relmax(got[1], qj[1]) > 1e-3       # the state moved
        assert_fields_close(got, r["jumpy", name], STATE_TOL, what=f"jumpy {name}")
    s.close()


def _crossover_params():
    return [pytest.param(order, side, id=f"N{order}-{side}") for order in sorted(CROSSOVER_MESHES) for side in ("above", "below")]


@pytest.mark.parametrize("order,side", _crossover_params())
def test_default_dispatch_on_both_sides_of_the_small_launch_crossover(order, side, monkeypatch):
    """No pin: RK2 + filter, SSP-RK2 + filter + sponge and the adaptive driver loop (runAdaptive, src/sw2d-simple/main.cpp:121-171)
    match the oracle just above and just below kSmallLaunch[N], and leave the same bits as a solver pinned to the family the
    crossover rule names (variant 0 above, variant 5 below)."""
    nx, ny = CROSSOVER_MESHES[order][side]
    nodes, t = _box(order, nx, ny, 5)
    K = t["rx"].shape[1]
    _assert_ragged(K)
    assert (K >= SMALL_LAUNCH[order]) == (side == "above")
    o = oracle_from(t, threads=4)
    x, y = t["x"], t["y"]
    q0 = seeded_fields(x, y, seed=order)
    qs = _amplified(q0)
    dt = o.dt(*q0, CFL, order)
    dts = 0.3 * o.dt(*qs, CFL, order)
    ref_rk2 = o.step_rk2(*q0, dt, 2, filter=True)
    ref_ssp = o.step_ssprk2(*qs, dts, 2, filter=True, sponge=SPONGE)
    steps, ot, odt, q = 5, 0.0, dt, q0          # the loop body of test_adaptive_driver_loop_matches_reference_loop_body
    for _ in range(steps):
        q = o.step_rk2(*q, odt, 1, filter=True)
        odt = o.dt(*q, CFL, order)
        ot += odt

    runs = {}
    for pin in (None, 0 if side == "above" else 5):
        if pin is None:
            monkeypatch.delenv("BDG_SW2D_AFFINE_VARIANT", raising=False)
        else:
            monkeypatch.setenv("BDG_SW2D_AFFINE_VARIANT", str(pin))
        s = sw2d.Sw2dSolver(nodes=nodes)
        s.setState(*q0)
        s.stepRK2(dt, 2, filter=True)
        rk2 = s.getState()
        s.setState(*qs)
        s.stepSSPRK2(dts, 2, filter=True, sponge=SPONGE)
        ssp = s.getState()
        s.setState(*q0)
        tt, dd, n = s.runAdaptive(CFL, finalTime=1e9, maxSteps=steps)
        runs[pin] = (rk2, ssp, s.getState(), tt, dd, n)
        s.close()

    rk2, ssp, adaptive, tt, dd, n = runs[None]
    assert_fields_close(rk2, ref_rk2, STATE_TOL, what="RK2 + filter")
    assert_fields_close(ssp, ref_ssp, STATE_TOL, what="SSP-RK2 + filter + sponge")
    assert n == steps
    assert abs(tt - ot) / ot < 1e-12 and abs(dd - odt) / odt < 1e-12
    assert_fields_close(adaptive, q, STATE_TOL, what="runAdaptive")
    pinned = [v for k, v in runs.items() if k is not None][0]
    for a, b in zip(runs[None][:3], pinned[:3]):
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    assert runs[None][3:] == pinned[3:]


# ---------------------------------------------------------------- four-field solvers in combine mode

FOUR_FIELD_ORDERS = (2, 4, 5, 6, 8)
_REF4 = {}


def _reference4(order, kind):
    """NumPy replay (oracle_np.sw2d_rhs4) of RK2 +- filter and SSP-RK2 +- filter with the sponge on the ragged mesh, once per
    (order, solver kind), shared by the source switches."""
    from oracle.oracle_np import sw2d_rhs4
    from partition_cases import filtered, four_field_problem, replay_rk2, replay_ssprk2
    if (order, kind) in _REF4:
        return _REF4[order, kind]
    _, t, o = _ragged(order)
    q0, src, args = four_field_problem(t, order, kind)       # the state, sources and (zx, zy, g, f, CD) the partitioned cases step too
    h, hu, hv = q0[:3]
    plain = lambda q: list(sw2d_rhs4(*q, *args, t))          # noqa: E731
    rhs = {False: plain, True: filtered(plain, t["Filter"])}

    def rk2(q, dt, n, filt):
        return replay_rk2(rhs[filt], q, dt, n)

    def ssp(q, dt, n, filt, sp):
        return replay_ssprk2(rhs[filt], q, dt, n, sp)

    dt = 0.3 * o.dt(h, hu, hv, CFL, order)
    r = {"q0": q0, "dt": dt, "src": src}
    for filt in (True, False):
        r["rk2", filt] = rk2(q0, dt, 2, filt)
        r["ssp", filt] = ssp(q0, dt, 2, filt, SPONGE)
    unsponged = ssp(q0, dt, 2, False, 0.0)
    for c in (1, 2):
        assert relmax(r["ssp", False][c], unsponged[c]) > 1e4 * STATE_TOL
    _REF4[order, kind] = r
    return r


@pytest.mark.parametrize("env", list(SOURCE_ENVS))
@pytest.mark.parametrize("kind", ["tracer", "variantD"])
@pytest.mark.parametrize("order", FOUR_FIELD_ORDERS)
def test_four_field_combine_steps_match_the_numpy_replay(order, kind, env, monkeypatch):
    """The tracer-only solver (fields=4) and variant D (fields=4 with sources) in combine mode, through the default kernels and every
    switch that selects another form: RK2 with and without the filter, SSP-RK2 with and without the filter and a scalar sponge.
    The sponge relaxes hu and hv only (src/sw2d/main.cpp:223-235): a kernel that relaxed h or the tracer, or skipped hv, fails
    here field by field."""
    for k, v in SOURCE_ENVS[env].items():
        monkeypatch.setenv(k, v)
    r = _reference4(order, kind)
    t = _ragged(order)[1]
    s = sw2d.Sw2dSolver(tables=t, fields=4, sources=r["src"])
    dt = r["dt"]
    for filt in (True, False):
        s.setState4(*r["q0"])
        s.stepRK2(dt, 2, filter=filt)
        assert_fields_close(s.getState4(), r["rk2", filt], STATE_TOL, what=f"RK2 filter={filt}")
        s.setState4(*r["q0"])
        s.stepSSPRK2(dt, 2, filter=filt, sponge=SPONGE)
        assert_fields_close(s.getState4(), r["ssp", filt], STATE_TOL, what=f"SSP-RK2 filter={filt} sponge={SPONGE}")
    s.close()
