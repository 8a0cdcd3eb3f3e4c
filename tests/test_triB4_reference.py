"""tests/trirefB4.py, the definition of variant B with a passive tracer on triangles, held to oracle_np.sw2d_rhs_b and to its
own properties. No GPU.

The problem is conftest.variant_b_setup (open left edge whose nodes stay in the wall list too, sloping bed, drag, Coriolis, a
time where the tide is not zero) on coarse_box.msh and on buildBoxMesh(13, 11), N = 1, 4, 8, with a tracer that jumps at every
face (hN = h times one random concentration per element in [0.2, 0.9]) and one concentration per open-boundary node.

  * Components 1 to 3 of rhsB4 equal sw2d_rhs_b bit for bit, and its speed is the maximum of sw2d_rhs_b's two speed arrays.
  * r4 in float64 stays within LD_TOL = 2.5e-13 of max|r4| of its np.longdouble evaluation, which is what licenses holding the
    GPU to 1e-12 (one RHS) and 1e-11 (stepped states) against the float64 one. Conditions on the inputs, asserted: every star
    depth is positive, |tide| > 0.1, no NaN in the reference.
  * Constancy: with hN = c h and Nopen = c, r4 = c r1 within the gamma_n bound of tests/test_quadB4_reference.py.
  * With Nopen != c only the elements that touch the open side differ; one value per node equals the scalar bit for bit.
  * The steppers leave h, hu, hv identical to the three-field ones, and hN is not sponged.
  * bdg_sw2d_enable_variant_b4 refuses a NULL handle whatever else is NULL or wrong, without touching a GPU."""
import ctypes

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import trirefB4 as T
from oracle import oracle_np
from quadref_ld import require_extended_precision
from test_quadB_reference import LD_TOL

ORDERS = (1, 4, 8)
MESHES = ("coarse", "box13x11")
cases = pytest.mark.parametrize("mesh,order", [pytest.param(m, n, id=f"{m}-N{n}") for m in MESHES for n in ORDERS])

_cache = {}


def setup(mesh, order, coarse_mesh):
    key = (mesh, order)
    if key not in _cache:
        if mesh == "coarse":
            m = coarse_mesh
        else:
            m = dg.MeshManager()
            m.buildBoxMesh(13, 11)
        _cache[key] = T.problem(order, m, seed=order)
    nodes, t, ex, q, p = _cache[key]
    return t, ex, [a.copy() for a in q], p


def args3(p):
    return p["H"], p["Hx"], p["Hy"], p["g"], p["f"], p["CD"]


@cases
def test_components_1_to_3_are_sw2d_rhs_b_bit_for_bit(mesh, order, coarse_mesh):
    t, ex, q, p = setup(mesh, order, coarse_mesh)
    assert abs(oracle_np.tide_elevation(ex["time"])) > 0.1 and p["CD"] > 0 and p["f"] != 0
    got = T.rhsB4(*q, *args3(p), ex["time"], t, p["mapO"], p["tracer"], return_speed=True)
    want = oracle_np.sw2d_rhs_b(*q[:3], *args3(p), ex["time"], t, p["mapO"])
    for c in range(3):
        assert np.array_equal(got[c], want[c]), c
    spdM, spdP = oracle_np.sw2d_rhs_b(*q[:3], *args3(p), ex["time"], t, p["mapO"], speeds_only=True)
    assert got[4] == max(spdM.max(), spdP.max())
    assert got[3].shape == q[0].shape and np.abs(got[3]).max() > 0


@cases
def test_float64_r4_is_within_a_quarter_of_the_gpu_tolerance(mesh, order, coarse_mesh):
    require_extended_precision()
    t, ex, q, p = setup(mesh, order, coarse_mesh)
    time = ex["time"]
    assert abs(oracle_np.tide_elevation(time)) > 0.1
    lam = T.global_speed(*q[:3], p["H"], p["g"], time, t, p["mapO"])
    got, star = T.tracer_rhs(*q, p["H"], lam, time, t, p["mapO"], p["tracer"], return_star=True)
    assert star > 0                                           # every star depth is positive
    # the tracer jumps at every face
    hN = q[3].flatten("F")
    N = (q[3] / q[0]).flatten("F")
    interior = np.asarray(t["vmapM"]) != np.asarray(t["vmapP"])
    assert np.abs(N[t["vmapM"]] - N[t["vmapP"]])[interior].min() > 0 and hN.min() > 0
    ref = T.rhs4_ld(*q, p["H"], p["g"], time, t, p["mapO"], p["tracer"])
    assert ref.dtype == T.LD and np.all(np.isfinite(ref)) and np.all(np.isfinite(got))
    err = np.abs(got - ref.astype(np.float64)).max() / np.abs(ref).max()
    print(f"{mesh} N{order}: float64 r4 against longdouble {float(err):.2e} of max|r4|")
    assert err <= LD_TOL


@cases
def test_a_uniform_concentration_gives_c_times_the_mass_equation(mesh, order, coarse_mesh):
    """The bound is tests/test_quadB4_reference.py's with three faces: every term of r4 is c times a term of r1 up to fewer than
    16 roundings on its way, then one dot product with a row of Dr, Ds or Lift of at most Np + 3 Nfp additions: each side is
    off by at most (Np + 3 Nfp + 16) eps sum|terms|, the difference of the two sides by twice that. Evaluated in longdouble."""
    require_extended_precision()
    t, ex, q, p = setup(mesh, order, coarse_mesh)
    tl = T.to_ld(t)
    c = T.LD(0.37)
    eps = np.finfo(T.LD).eps
    mult = 2 * (t["x"].shape[0] + t["nx"].shape[0] + 16)
    ql = [a.astype(T.LD) for a in q[:3]]
    Hl, Hxl, Hyl = (p[k].astype(T.LD) for k in ("H", "Hx", "Hy"))
    time = ex["time"]
    r1 = oracle_np.sw2d_rhs_b(*ql, Hl, Hxl, Hyl, p["g"], p["f"], p["CD"], time, tl, p["mapO"])[0]
    spdM, spdP = oracle_np.sw2d_rhs_b(*ql, Hl, Hxl, Hyl, p["g"], p["f"], p["CD"], time, tl, p["mapO"], speeds_only=True)
    lam = max(spdM.max(), spdP.max())
    r4, terms = T.tracer_rhs(*ql, c * ql[0], Hl, lam, time, tl, p["mapO"], c, return_terms=True)
    assert r1.dtype == T.LD and r4.dtype == T.LD and np.abs(r4).max() > 0
    excess = (np.abs(r4 - c * r1) / (mult * eps * terms)).max()
    print(f"{mesh} N{order}: |r4 - c r1| at most {float(excess):.2e} of the bound")
    assert excess <= 1


@pytest.mark.parametrize("mesh", MESHES)
def test_the_open_concentration_reaches_only_the_elements_on_the_open_side(mesh, coarse_mesh):
    t, ex, q, p = setup(mesh, 4, coarse_mesh)
    c = 0.37
    q[3] = c * q[0]
    nfn = t["nx"].shape[0]
    touching = np.unique(np.asarray(p["mapO"]) // nfn)
    assert 0 < touching.size < q[0].shape[1]
    # variant_b_setup leaves every open node in the wall list too: the order "walls, then the open boundary" is exercised
    assert set(p["mapO"].tolist()) <= set(np.asarray(t["mapW"]).tolist())
    a = T.rhsB4(*q, *args3(p), ex["time"], t, p["mapO"], c)
    b = T.rhsB4(*q, *args3(p), ex["time"], t, p["mapO"], c + 0.5)
    for i in range(3):
        assert np.array_equal(a[i], b[i])
    differs = np.nonzero((a[3] != b[3]).any(axis=0))[0]
    assert np.array_equal(differs, touching)
    per_node = T.rhsB4(*q, *args3(p), ex["time"], t, p["mapO"], np.full(len(p["mapO"]), c))
    assert np.array_equal(per_node[3], a[3])


def test_steppers_step_the_tracer_as_the_depth(coarse_mesh):
    t, ex, q, p = setup("coarse", 2, coarse_mesh)
    dt, time = 1e-3, ex["time"]
    sp = oracle_np.build_sponge_coeff(t, p["mapO"], 2.0, 0.5)
    assert sp.max() > 0
    got, tend = T.heun_steps(q, p, dt, 2, time=time, sponge=sp)
    want = oracle_np.step_ssprk2_b(*q[:3], *args3(p), time, dt, 2, t, p["mapO"], sponge=sp)
    assert tend == want[3] and len(got) == 4
    for a, b in zip(got, want[:3]):
        assert np.array_equal(a, b)
    # hN is not sponged: one Heun step by hand
    r = T.rhsB4(*q, *args3(p), time, t, p["mapO"], p["tracer"])
    q1 = [a + dt * b for a, b in zip(q, r)]
    q1 = [q1[0], q1[1] / (1.0 + sp * q1[1] * q1[1]), q1[2] / (1.0 + sp * q1[2] * q1[2]), q1[3]]
    r = T.rhsB4(*q1, *args3(p), time, t, p["mapO"], p["tracer"])
    one = T.heun_steps(q, p, dt, 1, time=time, sponge=sp)[0]
    assert np.array_equal(one[3], 0.5 * (q[3] + q1[3] + dt * r[3]))
    assert not np.array_equal(one[1], 0.5 * (q[1] + q1[1] + dt * r[1]))      # ... and hu is

    # RK2 + filter and LSERK4 stages against three-field loops written on sw2d_rhs_b
    def rhs3(s, tm, filt):
        r3 = oracle_np.sw2d_rhs_b(*s, *args3(p), tm, t, p["mapO"])
        return [t["Filter"] @ a for a in r3] if filt else list(r3)

    s, tm = q[:3], time
    for _ in range(2):
        s1 = [a + 0.5 * dt * b for a, b in zip(s, rhs3(s, tm, True))]
        s = [a + dt * b for a, b in zip(s, rhs3(s1, tm, True))]
        tm = tm + dt
    got, tend = T.rk2_steps(q, p, dt, 2, time=time)
    assert tend == tm and all(np.array_equal(a, b) for a, b in zip(got, s)) and not np.array_equal(got[3], q[3])
    s, res, tm = q[:3], [np.zeros_like(a) for a in q[:3]], time
    for i in range(7):
        r3 = rhs3(s, tm, False)
        res = [dg.LSERK4.rk4a[i % 5] * x + dt * y for x, y in zip(res, r3)]
        s = [x + dg.LSERK4.rk4b[i % 5] * y for x, y in zip(s, res)]
        if i % 5 == 4:
            tm = tm + dt
    got, _, tend = T.lserk4_stages(q, p, dt, 7, time=time)
    assert tend == tm and all(np.array_equal(a, b) for a, b in zip(got, s)) and not np.array_equal(got[3], q[3])


def test_bad_arguments_are_refused_without_a_gpu():
    """A solver handle needs a GPU, so every call here has a NULL handle and is refused for that before the library looks at
    the rest: the entry exists, reports BDG_ERR_ARGUMENT and dereferences nothing, whatever else is NULL or wrong. The
    refusals on a live handle are in tests/test_sw2d_triB4_gpu.py."""
    from blitzdg_amd import _capi as C
    lib, ARG = C.lib, C.BDG_ERR_ARGUMENT
    a, one = np.zeros((3, 1)), np.ones(1)
    d = C.Sw2dVbDesc(C.ptr(a), C.ptr(a), C.ptr(a), None, 0, 0.0, 0.0, 3.0, 100.0, 0.0, None)
    assert lib.bdg_sw2d_enable_variant_b4(None, ctypes.byref(d), C.ptr(one), 1) == ARG          # NULL handle
    assert lib.bdg_sw2d_enable_variant_b4(None, None, C.ptr(one), 1) == ARG                     # NULL handle, NULL descriptor
    assert lib.bdg_sw2d_enable_variant_b4(None, ctypes.byref(d), C.ptr(one), 7) == ARG          # NULL handle, bad count
    assert lib.bdg_sw2d_enable_variant_b4(None, ctypes.byref(d), None, -1) == ARG
    assert b"bdg_sw2d_enable_variant_b4" in C.lib.bdg_last_error()
