"""Eddy viscosity, constant or Smagorinsky, on the triangle solver (bdg_sw2d_enable_viscosity, the two passes of
csrc/hip/sw2d_viscosity_kernel.hpp behind every evaluation's own launches) against tests/triviscosity_ref.py.

The inputs are tridiff_ref.inputs: conftest.variant_b_setup on buildBoxMesh(13, 11) -- K = 286: more than one 64-lane wave and
ragged against 64 -- whose velocity is noise at every node, with nu0 a scalar or an (Np, K) field and Cs = 2 (not physical: on
this coarse mesh it makes max(nu - nu0) >= nu0, which test_triviscosity_reference.py asserts). Orders 1 to 8 on straight-sided
tables (flags = 0) and on per-node tables (NODAL_GEOMETRY), on four kinds of solver: "A" (three fields), "B" (variant B, three
fields), "D" (four fields with bed slope, Coriolis and drag) and "B4" (variant B with a tracer, the tracer's diffusion, source
and decay on as well). Per (order, geometry):

  test_rhs              computeRHS / computeRHS4 with viscosity minus the REFERENCE advective right-hand side equals
                        (0, T_u, T_v[, T]), and its filtered form, to RHS_TOL of max|T|: scalar nu0 alone (A), a nu0 field
                        alone (B), a field plus Smagorinsky (A, B, D, B4). Plane 0 (plane 3, B's globalSpeed) is bit for bit
                        that of the same solver without viscosity; on B4 plane 3 equals the diffusion-only solver's
  test_eddy_viscosity   eddyViscosity() of the resident state against eddy_viscosity                      1e-11 of max nu
  test_lserk4_stages    7 stages as 4 + 3 on A and B4                                                     STATE_TOL
  test_rk2_filter_steps 2 midpoint-RK2 + filter steps on B and D                                          STATE_TOL
  test_heun_steps       3 Heun steps with the sponge (array on B, scalar on A): fails if T is added after the division

then a mesh smaller than a tile, a shuffled mesh renumbered on the device, the step size, repeatability, device bytes and the
refusals. Tolerances are the project's: one RHS 1e-12, stepped states 1e-11 of max|field| (test_triviscosity_reference.py: the
float64 definition stays within LD_TOL = 2.5e-13 of its longdouble evaluation at every order). References are computed once per
order and shared by the geometry forms.

Measured on one MI355X: largest error of a term 2.9e-13 of max|T| (N = 8, straight-sided), per-node form at most 7.0e-15;
eddyViscosity() 5.0e-14 of max nu (N = 8, straight-sided), per-node form 3.2e-16; largest state error 6.5e-14 (N = 8,
straight-sided, LSERK4 stages), per-node form at most 1.4e-15; 20 adaptive steps take the standard deviation of u from 0.068
to 0.059 while dt follows nu_max from 3.221e-6 to 3.235e-6; 93 tests in 3.3 s."""
import numpy as np
import pytest

import trirefB4 as TB
import tridiff_ref as R
import triviscosity_ref as V
from blitzdg_amd import _capi as C
from blitzdg_amd import halo, sw2d
from conftest import relmax
from oracle import oracle_np as onp
from regimes import assert_fields_close

pytestmark = pytest.mark.gpu

RHS_TOL = 1e-12
STATE_TOL = 1e-11
NU_TOL = 1e-11
G = 9.81
ORDERS = tuple(range(1, 9))
FORMS = {"affine": 0, "nodal": sw2d.NODAL_GEOMETRY}
SPONGE_SCALAR = 1e-3
D_F, D_CD = 0.07, 2.5e-3
NF = {"A": 3, "B": 3, "D": 4, "B4": 4}

cases = pytest.mark.parametrize("order,form", [pytest.param(n, f, id=f"N{n}-{f}") for n in ORDERS for f in FORMS])

_REF, _MISC = {}, {}


def kwkey(kw):
    return tuple(sorted(kw.items()))


def slopes(order, **kw):
    key = ("slopes", order, kwkey(kw))
    if key not in _MISC:
        t = V.inputs(order, **kw)[1]
        _MISC[key] = onp.bed_slopes(0.3 * np.sin(2 * t["x"]) * np.cos(t["y"]), t)
    return _MISC[key]


def step_size(order, **kw):
    key = ("dt", order, kwkey(kw))
    if key not in _MISC:
        _, t, ex, q, p, _ = V.inputs(order, **kw)
        lam = TB.global_speed(*q[:3], p["H"], G, ex["time"], t, p["mapO"])
        _MISC[key] = 0.1 * (2.0 / max(kw.get("nx", 13), kw.get("ny", 11))) / ((order + 1) ** 2 * lam)
    return _MISC[key]


def sponge_array(order, **kw):
    key = ("sponge", order, kwkey(kw))
    if key not in _MISC:
        _, t, _, _, p, _ = V.inputs(order, **kw)
        _MISC[key] = onp.build_sponge_coeff(t, p["mapO"], 2e-3, 0.6)
        assert _MISC[key].max() > 0
    return _MISC[key]


def state(kind, order, **kw):
    return V.inputs(order, **kw)[3][:NF[kind]]


def advective(kind, order, **kw):
    """adv(q, time) -> the components of the reference advective right-hand side of a solver kind."""
    _, t, _, q0, p, _ = V.inputs(order, **kw)
    zero = np.zeros_like(t["x"])
    if kind == "A":
        return lambda q, time: onp.sw2d_rhs4(*q, q0[3], zero, zero, G, 0.0, 0.0, t)[:3]
    if kind == "D":
        zx, zy = slopes(order, **kw)
        return lambda q, time: onp.sw2d_rhs4(*q, zx, zy, G, D_F, D_CD, t)
    if kind == "B":
        return lambda q, time: tuple(onp.sw2d_rhs_b(*q, p["H"], p["Hx"], p["Hy"], G, p["f"], p["CD"], time, t, p["mapO"]))
    return lambda q, time: TB.rhsB4(*q, p["H"], p["Hx"], p["Hy"], G, p["f"], p["CD"], time, t, p["mapO"], p["tracer"])


VISC = {"scalar": lambda d: (d["nu"], 0.0), "field": lambda d: (d["nu_field"], 0.0),
        "smag": lambda d: (d["nu_field"], d["smagorinsky"])}


def model(kind, order, visc="smag", **kw):
    _, t, _, _, _, d = V.inputs(order, **kw)
    nu0, cs = VISC[visc](d)
    if kind == "B4":
        return V.Model(advective(kind, order, **kw), t, nu0, cs, d["kappa_field"], d["source"], d["decay"])
    return V.Model(advective(kind, order, **kw), t, nu0, cs)


def solver(kind, order, flags, visc="smag", sponge=False, diffusion=True, **kw):
    """visc: "scalar", "field", "smag" or None; B4 carries the tracer's diffusion unless diffusion=False."""
    nodes, t, ex, q, p, d = V.inputs(order, **kw)
    if kind == "D":
        zx, zy = slopes(order, **kw)
        s = sw2d.Sw2dSolver(nodes=nodes, g=G, flags=flags, fields=4, sources=dict(zx=zx, zy=zy, f=D_F, CD=D_CD))
    else:
        s = sw2d.Sw2dSolver(nodes=nodes, g=G, flags=flags, fields=NF[kind])
    if kind in ("B", "B4"):
        s.enableVariantB(p["H"], p["Hx"], p["Hy"], mapO=p["mapO"], CD=p["CD"], f=p["f"], tracer=p["tracer"] if kind == "B4" else None,
                         sponge=sponge_array(order, **kw) if sponge else None)
        s.time = ex["time"]
    if visc is not None and order % 2:                                      # either order of the two enable calls
        s.enableViscosity(*VISC[visc](d))
    if kind == "B4" and diffusion:
        s.enableTracerDiffusion(d["kappa_field"], source=d["source"], decay=d["decay"])
    if visc is not None and not order % 2:
        s.enableViscosity(*VISC[visc](d))
    assert s.usesAffineGeometry == (not flags & sw2d.NODAL_GEOMETRY)
    return s


def rhs_of(s, q, filt=False):
    return s.computeRHS4(*q, filter=filt) if len(q) == 4 else s.computeRHS(*q, filter=filt)


def set_state(s, q):
    s.setState4(*q) if len(q) == 4 else s.setState(*q)


def get_state(s, n):
    return s.getState4() if n == 4 else s.getState()


def reference(what, kind, order, visc="smag", **kw):
    key = (what, kind, order, visc, kwkey(kw))
    if key not in _REF:
        _, t, ex, _, _, d = V.inputs(order, **kw)
        q = state(kind, order, **kw)
        time, dt = ex["time"], step_size(order, **kw)
        m = model(kind, order, visc, **kw) if visc else None
        if what == "adv":
            adv = list(advective(kind, order, **kw)(q, time))
            _REF[key] = dict(adv=adv, adv_filtered=[t["Filter"] @ a for a in adv])
        elif what == "terms":
            out = dict(T=list(m.terms(q)), FT=list(m.terms(q, True)))
            if kind == "B4":
                out["T"].append(R.diffusion_term(q[0], q[3], d["kappa_field"], t, d["source"], d["decay"]))
                out["FT"].append(R.diffusion_term(q[0], q[3], d["kappa_field"], t, d["source"], d["decay"], True))
            _REF[key] = out
        elif what == "nu":
            _REF[key] = V.eddy_viscosity(*q[:3], *VISC[visc](d), t)
        elif what == "lserk":
            _REF[key] = V.lserk4_stages(m, q, dt, 7, time=time)
        elif what == "rk2":
            _REF[key] = V.rk2_steps(m, q, dt, 2, time=time, filt=True)
        else:
            sp = sponge_array(order, **kw) if kind in ("B", "B4") else SPONGE_SCALAR
            _REF[key] = V.heun_steps(m, q, dt, 3, time=time, sponge=sp)
    return _REF[key]


def check_terms(got, adv, want, what):
    """(right-hand side) - (reference advective part) on planes 1, 2 (and 3) against the terms, to RHS_TOL of max|T|."""
    errs = []
    for c, T in zip((1, 2, 3), want):
        err = np.abs((got[c] - adv[c]) - T).max() / np.abs(T).max()
        print(f"  {what} plane {c}: {err:.2e} of max|T| = {np.abs(T).max():.3e}")
        errs.append(err)
    assert max(errs) <= RHS_TOL, f"{what}: {max(errs):.2e} of max|T| > {RHS_TOL:.0e}"
    return errs


def rhs_checks(kind, order, flags, viscs, **kw):
    q = state(kind, order, **kw)
    adv = reference("adv", kind, order, None, **kw)
    plain = solver(kind, order, flags, visc=None, **kw)                       # B4: the diffusion-only solver
    base, base_f = rhs_of(plain, q), rhs_of(plain, q, True)
    lam0 = plain.globalSpeed if kind in ("B", "B4") else None
    plain.close()
    errs = []
    for visc in viscs:
        ref = reference("terms", kind, order, visc, **kw)
        assert all(np.abs(T).max() > 0 for T in ref["T"])
        s = solver(kind, order, flags, visc=visc, **kw)
        got = rhs_of(s, q)
        lam = s.globalSpeed if kind in ("B", "B4") else None
        got_f = rhs_of(s, q, True)
        s.close()
        errs += check_terms(got, adv["adv"], ref["T"], f"{kind} {visc}")
        errs += check_terms(got_f, adv["adv_filtered"], ref["FT"], f"{kind} {visc} filtered")
        for g_, b_ in ((got, base), (got_f, base_f)):
            assert np.array_equal(g_[0], b_[0])                                # mass never changes
            if len(q) == 4:
                assert np.array_equal(g_[3], b_[3])                            # nor the tracer (B4: equals the diffusion-only solver's)
        assert lam == lam0
    return errs


@cases
def test_rhs(order, form):
    d = V.inputs(order)[5]
    q = state("A", order)
    nu = reference("nu", "A", order, "smag")
    assert (nu - d["nu_field"]).max() >= d["nu_field"].max()                   # Smagorinsky shows on this input
    assert relmax(reference("terms", "A", order, "smag")["T"][0], reference("terms", "A", order, "field")["T"][0]) > 1e-2
    errs = rhs_checks("A", order, FORMS[form], ("scalar", "smag"))
    errs += rhs_checks("B", order, FORMS[form], ("field", "smag"))
    errs += rhs_checks("D", order, FORMS[form], ("smag",))
    errs += rhs_checks("B4", order, FORMS[form], ("smag",))
    print(f"N{order} {form}: largest {max(errs):.2e}")


@cases
def test_eddy_viscosity(order, form):
    errs = []
    for kind, visc in (("A", "smag"), ("B4", "smag"), ("B", "field")):
        q = state(kind, order)
        want = reference("nu", kind, order, visc)
        s = solver(kind, order, FORMS[form], visc=visc)
        set_state(s, q)
        got = s.eddyViscosity()
        s.close()
        errs.append(np.abs(got - want).max() / want.max())
    print(f"N{order} {form} nu: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= NU_TOL


def stepped(kind, order, flags, what, run, sponge=False, **kw):
    q = state(kind, order, **kw)
    ref, t_end = reference(what, kind, order, **kw)
    assert all(np.isfinite(a).all() for a in ref)
    s = solver(kind, order, flags, sponge=sponge, **kw)
    set_state(s, q)
    run(s)
    got = get_state(s, len(q))
    assert relmax(got[1], q[1]) > 1e-5 and relmax(got[2], q[2]) > 1e-5                  # the momentum moved
    print(f"  {kind} {what}: " + " ".join(f"{np.abs(a - b).max() / np.abs(b).max():.2e}" for a, b in zip(got, ref)))
    errs = assert_fields_close(got, ref, STATE_TOL, what=f"{kind} {what}")
    if kind in ("B", "B4"):
        assert abs(s.time - t_end) <= 1e-12 * t_end
    s.close()
    return errs


@cases
def test_lserk4_stages(order, form):
    dt = step_size(order)

    def run(s):
        s.lserk4Stages(dt, 4)
        s.lserk4Stages(dt, 3)

    errs = [e for kind in ("A", "B4") for e in stepped(kind, order, FORMS[form], "lserk", run)]
    print(f"N{order} {form} lserk: " + " ".join(f"{e:.2e}" for e in errs))


@cases
def test_rk2_filter_steps(order, form):
    dt = step_size(order)
    errs = [e for kind in ("B", "D") for e in stepped(kind, order, FORMS[form], "rk2", lambda s: s.stepRK2(dt, 2, filter=True))]
    print(f"N{order} {form} rk2: " + " ".join(f"{e:.2e}" for e in errs))


@cases
def test_heun_steps(order, form):
    """q1 = sponge(q + dt (R + T)): adding T behind a store that has divided already is off by about sponge dt T hu^2, far above
    STATE_TOL (asserted on the reference below)."""
    dt = step_size(order)

    def run(s):
        s.stepSSPRK2(dt, 1, sponge=SPONGE_SCALAR)
        s.stepSSPRK2(dt, 2, sponge=SPONGE_SCALAR)

    # what the wrong order would give after one stage, on A: sponge(q + dt R) + dt T against sponge(q + dt (R + T))
    q = state("A", order)
    m = model("A", order)
    time = V.inputs(order)[2]["time"]
    r_adv, r_all = advective("A", order)(q, time), m.evaluate(q, time)
    right = q[1] + dt * r_all[1]
    right = right / (1 + SPONGE_SCALAR * right * right)
    wrong = q[1] + dt * r_adv[1]
    wrong = wrong / (1 + SPONGE_SCALAR * wrong * wrong) + dt * (r_all[1] - r_adv[1])
    assert relmax(wrong, right) > 100 * STATE_TOL
    errs = [e for kind in ("B", "A") for e in stepped(kind, order, FORMS[form], "heun", run, sponge=True)]
    print(f"N{order} {form} heun: " + " ".join(f"{e:.2e}" for e in errs))


@pytest.mark.parametrize("order,form", [(1, "affine"), (3, "nodal"), (5, "affine"), (8, "nodal")])
def test_mesh_smaller_than_a_tile(order, form):
    """buildBoxMesh(2, 2): K = 8 < 64."""
    kw = dict(nx=2, ny=2)
    assert V.inputs(order, **kw)[1]["x"].shape[1] == 8
    rhs_checks("A", order, FORMS[form], ("scalar", "smag"), **kw)
    rhs_checks("B4", order, FORMS[form], ("smag",), **kw)
    dt = step_size(order, **kw)
    stepped("B4", order, FORMS[form], "lserk", lambda s: s.lserk4Stages(dt, 7), **kw)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", [2, 4, 6])
def test_renumbered_mesh(order, form):
    """A shuffled box, renumbered on the device: the nu0 plane, the nu output and the gather index go through the permutation."""
    kw = dict(seed=11)
    flags = FORMS[form] | sw2d.REORDER
    s = solver("A", order, flags, **kw)
    assert s.isRenumbered
    set_state(s, state("A", order, **kw))
    want = reference("nu", "A", order, "smag", **kw)
    assert np.abs(s.eddyViscosity() - want).max() <= NU_TOL * want.max()
    s.close()
    for kind in ("D", "B"):
        rhs_checks(kind, order, flags, ("smag",), **kw)
    dt = step_size(order, **kw)
    stepped("B4", order, flags, "lserk", lambda s: s.lserk4Stages(dt, 7), **kw)


def test_step_size():
    order = 4
    nodes, t, _, q4, _, d = V.inputs(order)
    q = q4[:3]
    cfl = 0.75
    plain = sw2d.Sw2dSolver(nodes=nodes, g=G)
    plain.setState(*q)
    advective_dt, eta = plain.computeDt(cfl)
    with pytest.raises(C.BdgError):
        plain.viscosityDt()                                                             # no viscosity: refused
    with pytest.raises(C.BdgError):
        plain.eddyViscosity()
    plain.close()
    for nu0, cs, bound in ((1e-6, 0.0, False), (5.0, 0.0, True), (5.0 * np.ones_like(q[0]), 0.0, True), (d["nu_field"], 2.0, None),
                           (0.0, 40.0, None)):
        s = sw2d.Sw2dSolver(nodes=nodes, g=G)
        s.enableViscosity(nu0, cs)
        s.setState(*q)
        want = V.viscosity_dt(V.eddy_viscosity(*q, nu0, cs, t).max(), order, t)
        got = s.viscosityDt()
        print(f"Cs {cs}: dt_visc {got:.6e} (reference {want:.6e}), advective {advective_dt:.3e}")
        assert abs(got - want) <= 1e-11 * want
        assert got == s.viscosityDt()                                                   # a fixed-order reduction
        dt, em = s.computeDt(cfl)
        assert em == eta
        if bound is not None:
            assert (cfl * want < advective_dt) == bound
        assert dt == min(advective_dt, cfl * got)                                       # bit for bit the advective value otherwise
        s.close()
    # ... and the three-way minimum with a diffusing tracer
    s = sw2d.Sw2dSolver(nodes=nodes, g=G, fields=4)
    s.enableTracerDiffusion(50.0)
    s.enableViscosity(5.0)
    s.setState4(*q4)
    assert s.computeDt(cfl)[0] == cfl * min(s.diffusionDt(), s.viscosityDt()) == cfl * s.diffusionDt()
    s.close()
    # 20 adaptive steps at CFL 0.75 where the Smagorinsky viscosity bounds the step: the state stays finite, the noise is smoothed
    s = sw2d.Sw2dSolver(nodes=nodes, g=G)
    s.enableViscosity(5.0, 2.0)
    s.setState(*q)
    first = cfl * s.viscosityDt()
    assert first < advective_dt
    tt, dt, steps = s.runAdaptive(cfl, 1e9, maxSteps=20, filter=True)
    got = s.getState()
    assert steps == 20 and dt == cfl * s.viscosityDt() and all(np.isfinite(a).all() for a in got)
    rough0, rough = np.std(q[1] / q[0]), np.std(got[1] / got[0])
    print(f"runAdaptive: dt {first:.3e} -> {dt:.3e} (advective {advective_dt:.3e}), std of u {rough0:.4f} -> {rough:.4f}")
    assert rough < 0.9 * rough0 and dt > first                                          # nu_max follows the state
    s.close()


def test_two_solves_give_the_same_bits_and_device_bytes_grow_by_the_planes():
    order = 4
    nodes, t, _, q4, _, d = V.inputs(order)
    Np, K = t["x"].shape
    ld = (K + 63) // 64 * 64
    dt = step_size(order)
    runs = []
    for _ in range(2):
        s = solver("B4", order, 0, sponge=True)
        s.setState4(*q4)
        s.lserk4Stages(dt, 5)
        s.stepSSPRK2(dt, 2, sponge=SPONGE_SCALAR)
        runs.append(list(s.getState4()) + [s.eddyViscosity()])
        s.close()
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    # four flux planes + the plane of nu (+ the plane of nu0 as a field; per-node geometry with a Filter: two planes more)
    for flags, field, planes in ((0, False, 5), (0, True, 6), (sw2d.NODAL_GEOMETRY, True, 8)):
        plain = solver("A", order, flags, visc=None)
        s = solver("A", order, flags, visc="smag" if field else "scalar")
        grown = s.deviceBytes - plain.deviceBytes
        ops = (2 * Np + 3 * (order + 1)) * Np * 8
        assert planes * Np * ld * 8 <= grown <= planes * Np * ld * 8 + 2 * ops + Np * Np * 8 + 257 * 8 + 4096, (flags, field, grown)
        # two more launches per evaluation, each taking the next direction of the alternating sweep
        q = q4[:3]
        for x in (plain, s):
            x.computeRHS(*q)
            x.computeRHS(*q)
        assert s.backwardLaunches - plain.backwardLaunches == 2
        plain.close()
        s.close()


def test_refusals_leave_the_solvers_usable():
    order = 2
    nodes, t, _, q4, _, d = V.inputs(order)
    q = q4[:3]
    E = C.BDG_ERR_ARGUMENT
    desc = lambda nu=0.1, field=None, cs=0.0: C.Sw2dViscosityDesc(nu, C.ptr(field), cs)
    enable = lambda s, dd: C.lib.bdg_sw2d_enable_viscosity(s._h, C.byref(dd))
    s3 = sw2d.Sw2dSolver(nodes=nodes, g=G)
    bad_field = d["nu_field"].copy()
    bad_field[1, 5] = -1e-3
    nan_field = d["nu_field"].copy()
    nan_field[0, 0] = np.nan
    zero_field = np.zeros_like(q[0])
    for dd in (desc(-0.1), desc(np.nan), desc(np.inf), desc(field=bad_field), desc(field=nan_field), desc(cs=-1.0), desc(cs=np.nan),
               desc(cs=np.inf), desc(0.0, None, 0.0), desc(0.0, zero_field, 0.0)):
        assert enable(s3, dd) == E and b"bdg_sw2d_enable_viscosity" in C.lib.bdg_last_error()
    assert C.lib.bdg_sw2d_enable_viscosity(s3._h, None) == E
    assert C.lib.bdg_sw2d_enable_viscosity(None, C.byref(desc())) == E
    for bad in (-0.1, np.nan):
        with pytest.raises(C.BdgError) as e:
            s3.enableViscosity(bad)
        assert e.value.code == E
    with pytest.raises(C.BdgError):
        s3.viscosityDt()                                                                # none of these enabled it
    plain = sw2d.Sw2dSolver(nodes=nodes, g=G)
    assert all(np.array_equal(a, b) for a, b in zip(plain.computeRHS(*q), s3.computeRHS(*q)))   # ... nor changed anything
    plain.close()
    s3.close()
    # the right call goes through, once
    s = sw2d.Sw2dSolver(nodes=nodes, g=G)
    s.enableViscosity(d["nu_field"], d["smagorinsky"])
    first = s.computeRHS(*q)
    check_terms(first, reference("adv", "A", order, None)["adv"], reference("terms", "A", order, "smag")["T"], "after the refusals")
    with pytest.raises(C.BdgError) as e:
        s.enableViscosity(0.2)                                                          # a second call
    assert e.value.code == E
    assert all(np.array_equal(a, b) for a, b in zip(first, s.computeRHS(*q)))
    # ... and a viscous solver takes no partition
    K = t["x"].shape[1]
    assert C.lib.bdg_sw2d_set_partition(s._h, K, K, None, 0) == E and b"viscosity" in C.lib.bdg_last_error()
    assert all(np.array_equal(a, b) for a, b in zip(first, s.computeRHS(*q)))
    s.close()
    # after the first evaluation
    s5 = sw2d.Sw2dSolver(nodes=nodes, g=G)
    before = s5.computeRHS(*q)
    with pytest.raises(C.BdgError) as e:
        s5.enableViscosity(0.1)
    assert e.value.code == E
    assert all(np.array_equal(a, b) for a, b in zip(before, s5.computeRHS(*q)))
    s5.close()
    # a solver with a partition set
    s6 = sw2d.Sw2dSolver(nodes=nodes, g=G, flags=sw2d.KEEP_ORDER)
    assert C.lib.bdg_sw2d_set_partition(s6._h, K, K, None, 0) == 0
    with pytest.raises(C.BdgError) as e:
        s6.enableViscosity(0.1)
    assert e.value.code == E and "partition" in str(e.value)
    assert all(np.array_equal(a, b) for a, b in zip(before, s6.computeRHS(*q)))
    s6.close()
    # the partitioned front end says so itself
    with pytest.raises(NotImplementedError, match="partitioned"):
        halo.NativeDistributedSw2d.enable_viscosity(None, 0.1)
