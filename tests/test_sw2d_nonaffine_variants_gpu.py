"""Every instance of the per-node-geometry variant kernels (sw2d_vn_kernel.hpp) against an np.longdouble reference.

launchStage takes variants B, C and D to these kernels when the tables are not those of straight-sided elements.
sw2d_order.hip compiles them per order 1..8: sw2d_stage_vn_kernel<N, MODE, PHYS> and sw2d_filter_rows_kernel<N, MODE, PHYS>
for MODE in RHS / LSERK / COMBINE and PHYS 1 (variants C and D) / 2 (variant B), and sw2d_vn_speed_kernel<N>. A sponge on the
wrong field, sx and ry exchanged, a drag sign, a per-face maximum that stops one node early or a wrong ca / cb in the filter
pass conserve mass and keep every symmetry, so each instance is launched here by an assertion against the reference
(tests/nonaffine_cases.py: oracle_np.sw2d_rhs4 / sw2d_rhs_b in np.longdouble on longdouble tables, rounded at the comparison).

  mesh    a shuffled, smoothly deformed 13 x 11 box, K = 286: five workgroups of 64 elements, the last wave of 30
          (blockIdx.x > 0 and a ragged wave behind full ones at every order), two speed blocks of 256, the second of 30
          (sw2d_vb_speed_reduce_kernel with nblocks = 2). At N = 1 the deformed elements are still straight: NODAL_GEOMETRY
          asks for the per-node path. Every solver asserts `not usesAffineGeometry`.
  order   1 .. 8
  set     B    three fields, enableVariantB: a bed that jumps at every face (hMstar != hM), open boundary on the left edge
               at a time when the tide is -2.5 m, drag, Coriolis, a sponge array (zero on the right part) or a scalar   PHYS 2
          D    four fields, zx / zy / f arrays, CD                                                                       PHYS 1
          C    four fields, scalar f, no slopes, no drag (vp.fcor == nullptr, vp.zx == nullptr)                         PHYS 1
          T    four fields, no sources (vp.sources == 0)                                                                 PHYS 1
          D3   three fields with the sources of D (a 192-thread launch of PHYS 1)                                        PHYS 1
  The Python layer refuses none of the five sets.

  instance (per order; PHYS 1 by D, C, T, D3; PHYS 2 by B)      test
  stage_vn<RHS>                                                 test_rhs (filter False; as the first pass of every filtered call)
  stage_vn<RHS> -> raw, filter_rows<RHS>                        test_rhs (filter True)
  stage_vn<LSERK>                                               test_lserk4_stages, test_jumpy_state
  stage_vn<COMBINE>                                             test_midpoint_rk2 (ca = 1, cb = 0), test_ssprk2 (ca = cb = 0.5,
                                                                sponge), filter False
  filter_rows<COMBINE>                                          test_midpoint_rk2, test_ssprk2, test_jumpy_state, filter True
  filter_rows<LSERK>   (both PHYS)                              NO PUBLIC CALL REACHES IT: lserk4Stages / stepLSERK4 never filter
  vn_speed + vb_speed_reduce (nblocks = 2)                      every call of set B; test_rhs holds globalSpeed itself
  sponge branches of COMBINE: PHYS 2 array / PHYS 2 scalar      test_ssprk2[B] (two solvers); the array also in test_jumpy_state[B]
                              PHYS 1 scalar on hu, hv only      test_ssprk2[D, C, T, D3] (h and hN of the reference are unrelaxed)

Step sizes: the reference dt at CFL 0.65 on the host tables for the smooth state, a quarter of it for the jumpy one. For B the
model time is checked as well: frozen inside a step, moved on after the fifth LSERK4 stage and after each RK2 / Heun step, and
left alone by computeRHS.

Tolerances are the project's (tests/test_sw2d_gpu.py): one RHS 1e-12, multi-step states 1e-11, of each field's own size.
The float64 evaluation of the reference is within 6.5e-14 (RHS; N = 7, set D) and 8.1e-14 (state after 13 LSERK4 stages;
N = 8, set D) of the longdouble one (tests/test_nonaffine_cases.py, sets B and D).
Measured on one MI355X: largest RHS error 8.3e-14 (N = 7, set C, smooth state, filtered), largest state error 8.9e-14 (N = 8,
set C, 13 LSERK4 stages), largest error of globalSpeed 1.7e-16 (N = 3); 200 tests in 28 s, the slowest 0.74 s
(test_lserk4_stages[N8-C]), the references included. No test exposed a defect in the kernels, launchVn or buildNodalVariantOps.

Arithmetic-only edits to sw2d_vn_kernel.hpp tried against this module in a scratch build, each in the instances of ONE order
so that no edit can hide another (first test of that order that failed, in the order pytest runs them; unedited: all pass):
  sx and ry exchanged in the row loop (N = 1)                               test_rhs[N1-B]
  per-face lam maximum stopped one node early, PHYS 1 (N = 2)               test_rhs[N2-D]
  sponge also on c == 0 in the PHYS 2 COMBINE store (N = 3)                 test_ssprk2[N3-B]  (the only one: the filtered calls
                                                                            take the filter pass, RK2 on B runs without a sponge)
  p.sponge instead of the sponge field in sw2d_filter_rows_kernel (N = 4)   test_ssprk2[N4-B]  (then test_jumpy_state[N4-B])
  ca and cb swapped in the filter pass's COMBINE (N = 5)                    test_midpoint_rk2[N5-B]  (every set fails it; Heun cannot
                                                                            see this edit: its first update has qbase == qin and
                                                                            its second ca == cb)
  drag sign of RHS3 flipped in PHYS 1 (N = 6)                               test_rhs[N6-D]  (D and D3 only: C and T have no drag)
  zx term dropped (N = 7)                                                   test_rhs[N7-D]  (D and D3 only)
  tags >> (j + 1) for tags >> j in the stage kernel (N = 8)                 test_rhs[N8-B]
Every edit changed a test."""
import pytest

import nonaffine_cases as C
from blitzdg_amd import sw2d
from conftest import relmax
from regimes import assert_fields_close

pytestmark = pytest.mark.gpu

RHS_TOL = 1e-12
STATE_TOL = 1e-11
MOVED = 1e4 * STATE_TOL     # a stepping test that left the state where it was proves nothing

cases = pytest.mark.parametrize("order,fs", [pytest.param(n, s, id=f"N{n}-{s}") for n in range(1, 9) for s in C.SETS])


def _solver(order, fs, sponge_array=True):
    c = C.make_case(order, fs)
    flags = sw2d.KEEP_ORDER | (sw2d.NODAL_GEOMETRY if order == 1 else 0)
    s = sw2d.Sw2dSolver(tables=c.t, g=C.G, flags=flags, fields=c.fields, sources=c.sources)
    if fs == "B":
        v = c.vb
        s.enableVariantB(v["H"], v["Hx"], v["Hy"], mapO=v["mapO"], CD=v["CD"], f=v["f"], sponge=v["sponge"] if sponge_array else None)
        s.time = c.time0
    assert not s.usesAffineGeometry
    assert s.K == 286 and s.fields == c.fields
    return s


def _set(s, q, time0=None):
    (s.setState4 if len(q) == 4 else s.setState)(*q)
    if time0 is not None:
        s.time = time0


def _get(s):
    return s.getState4() if s.fields == 4 else s.getState()


def _rhs(s, q, filt):
    return (s.computeRHS4 if len(q) == 4 else s.computeRHS)(*q, filter=filt)


def _state_close(s, ref, start, what):
    got = _get(s)
    errs = assert_fields_close(got, ref, STATE_TOL, what=what)
    print(f"{what}: state " + " ".join(f"{e:.2e}" for e in errs))
    for a, b in zip(ref, start):
        assert relmax(a, b) > MOVED, f"{what}: the state hardly moved"
    return max(errs)


@cases
def test_rhs(order, fs):
    """RHS and Filter . RHS on the smooth and the jumpy state; B: globalSpeed against the reference maximum, time unchanged."""
    s = _solver(order, fs)
    r = C.reference(order, fs, "rhs")
    for kind in ("smooth", "jumpy"):
        q = r["q0"] if kind == "smooth" else r["qj"]
        for filt in (False, True):
            errs = assert_fields_close(_rhs(s, q, filt), r[kind, filt], RHS_TOL, what=f"N{order} {fs} {kind} filter={filt}")
            print(f"N{order} {fs} {kind} filter={filt}: rhs " + " ".join(f"{e:.2e}" for e in errs))
            if fs == "B":
                lam = s.globalSpeed
                print(f"N{order} {fs} {kind}: speed {abs(lam - r[kind, 'speed']) / r[kind, 'speed']:.2e}")
                assert abs(lam - r[kind, "speed"]) <= RHS_TOL * r[kind, "speed"]
                assert s.time == r["time0"]
    s.close()


@cases
def test_lserk4_stages(order, fs):
    """13 stages as 8 + 5, then setState part-way through a step and 7 more (stage 0 again, residual zero)."""
    s = _solver(order, fs)
    r = C.reference(order, fs, "lserk")
    _set(s, r["q0"], r["time0"])
    s.lserk4Stages(r["dt"], 8)
    if fs == "B":
        assert s.time == r["time8"]         # moved on after the fifth stage, frozen since
    s.lserk4Stages(r["dt"], 5)
    _state_close(s, r[13], r["q0"], f"N{order} {fs} lserk 13")
    if fs == "B":
        assert s.time == r["time13"]
    _set(s, r["q1"])                        # the model time goes on
    s.lserk4Stages(r["dt"], 7)
    _state_close(s, r[7], r["q1"], f"N{order} {fs} lserk 7 after setState")
    if fs == "B":
        assert s.time == r["time7"]
    s.close()


@cases
def test_midpoint_rk2(order, fs):
    """3 steps of the midpoint RK2 as 1 + 2, with and without the filter (B: without the sponge array, which would relax
    these combine steps too; test_jumpy_state[B] runs RK2 with it)."""
    s = _solver(order, fs, sponge_array=False)
    r = C.reference(order, fs, "rk2")
    for filt in (True, False):
        _set(s, r["q0"], r["time0"])
        s.stepRK2(r["dt"], 1, filter=filt)
        s.stepRK2(r["dt"], 2, filter=filt)
        _state_close(s, r[filt], r["q0"], f"N{order} {fs} rk2 filter={filt}")
        if fs == "B":
            assert s.time == r["time"]
    s.close()


@cases
def test_ssprk2(order, fs):
    """2 Heun steps with the sponge, filter on and off: the scalar sponge everywhere (hu and hv only; h and hN unrelaxed), and
    for B the sponge array as well."""
    r = C.reference(order, fs, "ssprk2")
    for name in (("array", "scalar") if fs == "B" else ("scalar",)):
        s = _solver(order, fs, sponge_array=name == "array")
        for filt in (True, False):
            _set(s, r["q0"], r["time0"])
            # with the array in place the scalar argument must be ignored
            s.stepSSPRK2(r["dt"], 2, filter=filt, sponge=C.SPONGE_SCALAR)
            _state_close(s, r[name, filt], r["q0"], f"N{order} {fs} ssprk2 {name} filter={filt}")
            if fs == "B":
                assert s.time == r["time"]
        s.close()
    if fs == "B":   # the two sponges are told apart by far more than the tolerance
        for i in (1, 2):
            assert relmax(r["array", False][i], r["scalar", False][i]) > MOVED


@cases
def test_jumpy_state(order, fs):
    """One step of each stepper on the jumpy state at a quarter of the CFL step, filtered where the stepper can filter."""
    s = _solver(order, fs)
    r = C.reference(order, fs, "jumpy")
    _set(s, r["qj"], r["time0"])
    s.stepLSERK4(r["dtj"], 1)
    _state_close(s, r["lserk"], r["qj"], f"N{order} {fs} jumpy lserk")
    _set(s, r["qj"], r["time0"])
    s.stepRK2(r["dtj"], 1, filter=True)
    _state_close(s, r["rk2"], r["qj"], f"N{order} {fs} jumpy rk2")
    _set(s, r["qj"], r["time0"])
    s.stepSSPRK2(r["dtj"], 1, filter=True, sponge=C.SPONGE_SCALAR)
    _state_close(s, r["ssprk2"], r["qj"], f"N{order} {fs} jumpy ssprk2")
    s.close()
