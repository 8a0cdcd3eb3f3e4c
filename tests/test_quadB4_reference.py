"""tests/quadrefB4.py, the definition of variant B with a passive tracer (four fields), held to tests/quadrefB.py and to its own
properties. No GPU.

  * Components 1 to 3 of rhsB4 equal quadrefB.rhsB bit for bit in float64: shear and jitter meshes (13 x 11, K = 143, the
    x = -1 side open), a bed that jumps at every face, a time where the tide is not zero, drag, Coriolis, the four regimes of
    tests/regimes.py, N = 1, 4, 8, 12.
  * The float64 rhsB4 stays within LD_TOL = 2.5e-13 of max|RHS| per field of its np.longdouble evaluation, which is what
    licenses holding the GPU to 1e-12 (one RHS) and 1e-11 (stepped states) against the latter. The bed jumps by a fifth of the
    smallest depth at most and the tide is positive at the evaluation time, so every star depth is positive; the reference
    has no NaN (asserted: a condition on the inputs).
  * Constancy: with hN = c h and Nopen = c, r4 = c r1 in longdouble to rounding.
  * With Nopen != c only the elements that touch the open side differ.
  * bdg_sw2dq_enable_variant_b4 refuses a NULL handle, with a NULL descriptor or a bad count beside it, without touching a
    GPU (a live handle needs one: those refusals are in tests/test_sw2d_quadsB4_gpu.py)."""
import ctypes

import numpy as np
import pytest

import quadref_ld as Q
import quadrefB as B
import quadrefB4 as B4
from regimes import REGIMES, assert_fields_close
from test_quadB_reference import LD_TOL, regime_problem

ORDERS = (1, 4, 8, 12)
T0 = 37.0
cases = pytest.mark.parametrize("mesh,order", [pytest.param(m, n, id=f"{m}-N{n}") for m in Q.MESHES for n in ORDERS])


def problem4(nodes, t, regime, seed):
    """test_quadB_reference.regime_problem with a tracer that jumps at every face and one concentration per open node."""
    q, vb = regime_problem(nodes, t, regime, seed)
    q.append(Q.tracer(q[0], t["x"], t["y"], seed))
    vb["tracer"] = B4.open_tracer(t)
    return q, vb


@cases
def test_components_1_to_3_are_quadrefB_bit_for_bit(mesh, order):
    nodes, t = B.mesh_tables(mesh, order)
    for regime in REGIMES:
        q, vb = problem4(nodes, t, regime, seed=order)
        assert abs(B.tide_value(T0, vb["tide"])) > 0 and vb["CD"] > 0 and vb["f"] != 0
        got = B4.rhsB4(*q, t, vb, time=T0, return_speed=True)
        want = B.rhsB(*q[:3], t, vb, time=T0, return_speed=True)
        for c in range(3):
            assert np.array_equal(got[c], want[c]), (regime, c)
        assert got[4] == want[3]


@cases
def test_float64_definition_is_within_a_quarter_of_the_gpu_tolerance(mesh, order):
    Q.require_extended_precision()
    nodes, t = B.mesh_tables(mesh, order)
    tl = Q.to_ld(t)
    worst = 0.0
    for regime in REGIMES:
        q, vb = problem4(nodes, t, regime, seed=order)
        H = vb["H"].ravel("F")
        jump = np.abs(H[t["vmapM"]] - H[t["vmapP"]]).max()
        assert 0.01 * q[0].min() < jump < q[0].min() and B.tide_value(T0, vb["tide"]) > 0      # every star depth is positive
        ref = B4.rhsB4(*B.to_ld(q), tl, B4.vb_ld(vb), time=T0)
        got = B4.rhsB4(*q, t, vb, time=T0)
        assert all(a.dtype == B.LD and np.all(np.isfinite(a)) for a in ref)
        assert all(np.all(np.isfinite(a)) for a in got)
        errs = assert_fields_close(got, Q.f64(ref), LD_TOL, what=f"{mesh} N{order} {regime}")
        worst = max(worst, *errs)
    print(f"{mesh} N{order}: float64 against longdouble, largest per-field error {worst:.2e}")


@cases
def test_a_uniform_concentration_gives_c_times_the_mass_equation(mesh, order):
    """The bound. Every term of r4 is c times a term of r1 up to the roundings on its way: the concentration (c h) / h, the star
    product, the flux product and quotient, the jump, the two normal products, the speed product, the halves, Fscale, the
    metric factors: fewer than 16 elementary operations; then one dot product with a row of Dr, Ds or Lift, whose
    accumulation is at most Np + 4 Nfp additions long. So each side is off by at most (Np + 4 Nfp + 16) eps sum|terms|
    (the standard gamma_n bound), and the difference of the two sides by twice that."""
    Q.require_extended_precision()
    nodes, t = B.mesh_tables(mesh, order)
    tl = Q.to_ld(t)
    c = B.LD(0.37)
    eps = np.finfo(B.LD).eps
    mult = 2 * (t["x"].shape[0] + t["nx"].shape[0] + 16)
    for regime in REGIMES:
        q, vb = problem4(nodes, t, regime, seed=order)
        ql = B.to_ld(q[:3])
        vb["tracer"] = c
        r = B4.rhsB4(*ql, c * ql[0], tl, B4.vb_ld(vb), time=T0, return_terms=True)
        r1, r4, terms = r[0], r[3], r[4]
        assert np.abs(r4).max() > 0
        excess = (np.abs(r4 - c * r1) / (mult * eps * terms)).max()
        print(f"{mesh} N{order} {regime}: |r4 - c r1| at most {float(excess):.2e} of the bound")
        assert excess <= 1


@pytest.mark.parametrize("mesh", Q.MESHES)
def test_the_open_concentration_reaches_only_the_elements_on_the_open_side(mesh):
    nodes, t = B.mesh_tables(mesh, 4)
    q, vb = problem4(nodes, t, "jumpy", seed=4)
    c = 0.37
    q[3] = c * q[0]
    nfn = t["nx"].shape[0]
    touching = np.unique(np.asarray(t["mapO"]) // nfn)
    assert 0 < touching.size < q[0].shape[1]
    a = B4.rhsB4(*q, t, dict(vb, tracer=c), time=T0)
    b = B4.rhsB4(*q, t, dict(vb, tracer=c + 0.5), time=T0)
    for i in range(3):
        assert np.array_equal(a[i], b[i])
    differs = np.nonzero((a[3] != b[3]).any(axis=0))[0]
    assert np.array_equal(differs, touching)
    # one value per node in the order of mapO: the same numbers given per node are the scalar's
    per_node = B4.rhsB4(*q, t, dict(vb, tracer=np.full(len(t["mapO"]), c)), time=T0)
    assert np.array_equal(per_node[3], a[3])


def test_steppers_step_the_tracer_as_the_depth():
    """One Heun step with a sponge: hN and h are not divided, hu and hv are; first three fields as quadrefB's steppers."""
    nodes, t = B.mesh_tables("shear", 2)
    q, vb = problem4(nodes, t, "jumpy", seed=2)
    dt = 1e-3
    got, time = B4.heun_steps(q, t, vb, dt, 2, time=T0, sponge_coeff=2.0)
    want, time3 = B.heun_steps(q[:3], t, vb, dt, 2, time=T0, sponge_coeff=2.0)
    assert time == time3 and len(got) == 4
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    r = B4.rhsB4(*q, t, vb, time=T0)
    q1 = [a + dt * b for a, b in zip(q, r)]
    q1 = [q1[0], B.sponge(q1[1], 2.0), B.sponge(q1[2], 2.0), q1[3]]
    r = B4.rhsB4(*q1, t, vb, time=T0)
    assert np.array_equal(B4.heun_steps(q, t, vb, dt, 1, time=T0, sponge_coeff=2.0)[0][3], 0.5 * (q[3] + q1[3] + dt * r[3]))
    for fn, n in ((B4.rk2_steps, 2), (B4.lserk4_stages, 7)):
        a, b = fn(q, t, vb, dt, n, time=T0), getattr(B, fn.__name__)(q[:3], t, vb, dt, n, time=T0)
        assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[-1] == b[-1] and len(a[0]) == 4


def test_bad_arguments_are_refused_without_a_gpu():
    """A solver handle needs a GPU, so every call here has a NULL handle and is refused for that before the library looks at the
    rest: what this shows is that the entry exists, reports BDG_ERR_ARGUMENT and dereferences nothing, whatever else is NULL or
    wrong. The NULL descriptor and the bad counts on a live handle are in tests/test_sw2d_quadsB4_gpu.py."""
    from blitzdg_amd import _capi as C
    lib, ARG = C.lib, C.BDG_ERR_ARGUMENT
    a, one = np.zeros((4, 1)), np.ones(1)
    d = C.Sw2dVbDesc(C.ptr(a), C.ptr(a), C.ptr(a), None, 0, 0.0, 0.0, 3.0, 100.0, 0.0, None)
    assert lib.bdg_sw2dq_enable_variant_b4(None, ctypes.byref(d), C.ptr(one), 1) == ARG          # NULL handle
    assert lib.bdg_sw2dq_enable_variant_b4(None, None, C.ptr(one), 1) == ARG                     # NULL handle, NULL descriptor
    assert lib.bdg_sw2dq_enable_variant_b4(None, ctypes.byref(d), C.ptr(one), 7) == ARG          # NULL handle, bad count
    assert lib.bdg_sw2dq_enable_variant_b4(None, ctypes.byref(d), None, -1) == ARG
    assert b"bdg_sw2dq_enable_variant_b4" in C.lib.bdg_last_error()
