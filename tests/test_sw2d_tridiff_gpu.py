"""Diffusion, sources and decay of the tracer on the triangle solver (bdg_sw2d_enable_tracer_diffusion, the two passes of
csrc/hip/sw2d_diffusion_kernel.hpp behind every evaluation's own launches) against tests/tridiff_ref.py.

The inputs are tridiff_ref.inputs: conftest.variant_b_setup on buildBoxMesh(13, 11) -- K = 286: more than one 64-lane workgroup,
ragged against 64 and against 16 -- with a tracer that jumps at every face, kappa as an (Np, K) field or a scalar, a Gaussian
source and a decay rate. Orders 1 to 8 on straight-sided tables (flags = 0) and on per-node tables (NODAL_GEOMETRY), on three
kinds of four-field solver: "A4" (created without sources), "D" (created with bed slope, Coriolis and drag) and "B4" (variant B
with a tracer). Per (order, geometry):

  test_rhs              computeRHS4 with diffusion minus the REFERENCE advective right-hand side equals T, and Filter T, to
                        RHS_TOL of max|T|, on A4 (field kappa + S + k: the filter in two steps; scalar kappa alone: pre-filtered
                        rows on straight-sided elements), D and B4; components 1-3 (and B4's globalSpeed) are bit for bit those
                        of the same solver without diffusion
  test_lserk4_stages    7 stages as 4 + 3 on B4 and D                                          STATE_TOL
  test_rk2_filter_steps 2 midpoint-RK2 + filter steps on A4 and B4                             STATE_TOL
  test_heun_steps       3 Heun steps with the sponge (array on B4, scalar on D)                STATE_TOL

then a mesh smaller than a tile, a shuffled mesh renumbered on the device, tracer mass in a closed basin and under a source, the
step size, the sweep directions and device bytes, and the refusals. Tolerances are the project's: one RHS 1e-12, stepped states
1e-11 of max|field| (tests/test_tridiff_reference.py: the float64 definition is within 7.6e-16 of max|T| of its longdouble
evaluation at every order, far inside 2.5e-13, so no order needs a wider GPU tolerance). References are computed once per order
and shared by the geometry forms.

Measured on one MI355X: largest error of T 1.7e-13 of max|T| (N = 8, straight-sided, Filter T with the scalar kappa; 1.6e-13
unfiltered), per-node form at most 3.0e-15; largest state error 3.3e-14 (N = 8, straight-sided, three Heun steps), per-node form
at most 2.4e-15; drift of int hN in the closed basin 1.4e-16, deviation from the source's rate 3.2e-16 of int hN; 83 tests in
2.7 s."""
import numpy as np
import pytest

import trirefB4 as TB
import tridiff_ref as R
from blitzdg_amd import _capi as C
from blitzdg_amd import halo, sw2d
from conftest import relmax
from oracle import oracle_np as onp
from regimes import assert_fields_close

pytestmark = pytest.mark.gpu

RHS_TOL = 1e-12
STATE_TOL = 1e-11
G = 9.81
ORDERS = tuple(range(1, 9))
FORMS = {"affine": 0, "nodal": sw2d.NODAL_GEOMETRY}
SPONGE_SCALAR = 1e-3
D_F, D_CD = 0.07, 2.5e-3

cases = pytest.mark.parametrize("order,form", [pytest.param(n, f, id=f"N{n}-{f}") for n in ORDERS for f in FORMS])

_REF, _MISC = {}, {}


def slopes(order, **kw):
    """Bed slopes of variant D's sources."""
    key = ("slopes", order, tuple(sorted(kw.items())))
    if key not in _MISC:
        _, t, _, _, _, _ = R.inputs(order, **kw)
        _MISC[key] = onp.bed_slopes(0.3 * np.sin(2 * t["x"]) * np.cos(t["y"]), t)
    return _MISC[key]


def step_size(order, **kw):
    key = ("dt", order, tuple(sorted(kw.items())))
    if key not in _MISC:
        _, t, ex, q, p, _ = R.inputs(order, **kw)
        lam = TB.global_speed(*q[:3], p["H"], G, ex["time"], t, p["mapO"])
        _MISC[key] = 0.1 * (2.0 / max(kw.get("nx", 13), kw.get("ny", 11))) / ((order + 1) ** 2 * lam)
    return _MISC[key]


def sponge_array(order, **kw):
    key = ("sponge", order, tuple(sorted(kw.items())))
    if key not in _MISC:
        _, t, _, _, p, _ = R.inputs(order, **kw)
        _MISC[key] = onp.build_sponge_coeff(t, p["mapO"], 2e-3, 0.6)
        assert _MISC[key].max() > 0
    return _MISC[key]


def advective(kind, order, **kw):
    """adv(q, time) -> the four components of the reference advective right-hand side of a solver kind."""
    _, t, _, _, p, _ = R.inputs(order, **kw)
    if kind == "A4":
        zero = np.zeros_like(t["x"])
        return lambda q, time: onp.sw2d_rhs4(*q, zero, zero, G, 0.0, 0.0, t)
    if kind == "D":
        zx, zy = slopes(order, **kw)
        return lambda q, time: onp.sw2d_rhs4(*q, zx, zy, G, D_F, D_CD, t)
    return lambda q, time: TB.rhsB4(*q, p["H"], p["Hx"], p["Hy"], G, p["f"], p["CD"], time, t, p["mapO"], p["tracer"])


def model(kind, order, full=True, **kw):
    _, t, _, _, _, d = R.inputs(order, **kw)
    if full:
        return R.Model(advective(kind, order, **kw), t, d["kappa_field"], d["source"], d["decay"])
    return R.Model(advective(kind, order, **kw), t, d["kappa"])


def solver(kind, order, flags, diffusion="full", sponge=False, **kw):
    """diffusion: "full" (field kappa, S, k), "scalar" (scalar kappa alone), None."""
    nodes, t, ex, q, p, d = R.inputs(order, **kw)
    if kind == "D":
        zx, zy = slopes(order, **kw)
        s = sw2d.Sw2dSolver(nodes=nodes, g=G, flags=flags, fields=4, sources=dict(zx=zx, zy=zy, f=D_F, CD=D_CD))
    else:
        s = sw2d.Sw2dSolver(nodes=nodes, g=G, flags=flags, fields=4)
    if kind == "B4":
        s.enableVariantB(p["H"], p["Hx"], p["Hy"], mapO=p["mapO"], CD=p["CD"], f=p["f"], tracer=p["tracer"],
                         sponge=sponge_array(order, **kw) if sponge else None)
        s.time = ex["time"]
    if diffusion == "full":
        s.enableTracerDiffusion(d["kappa_field"], source=d["source"], decay=d["decay"])
    elif diffusion == "scalar":
        s.enableTracerDiffusion(d["kappa"])
    assert s.usesAffineGeometry == (not flags & sw2d.NODAL_GEOMETRY)
    return s


def reference(what, kind, order, **kw):
    key = (what, kind, order, tuple(sorted(kw.items())))
    if key not in _REF:
        _, t, ex, q, p, d = R.inputs(order, **kw)
        time, dt = ex["time"], step_size(order, **kw)
        if what == "rhs":
            adv = advective(kind, order, **kw)(q, time)
            full, scalar = model(kind, order, **kw), model(kind, order, False, **kw)
            _REF[key] = dict(adv=list(adv), adv_filtered=[t["Filter"] @ a for a in adv], T=full.term(q), FT=full.term(q, True),
                             Ts=scalar.term(q), FTs=scalar.term(q, True))
        elif what == "lserk":
            _REF[key] = R.lserk4_stages(model(kind, order, **kw), q, dt, 7, time=time)
        elif what == "rk2":
            _REF[key] = R.rk2_steps(model(kind, order, **kw), q, dt, 2, time=time, filt=True)
        else:
            sp = sponge_array(order, **kw) if kind == "B4" else SPONGE_SCALAR
            _REF[key] = R.heun_steps(model(kind, order, **kw), q, dt, 3, time=time, sponge=sp)
    return _REF[key]


def check_term(got4, adv4, want, what):
    """(computeRHS4's fourth component) - (reference advective component) against T, to RHS_TOL of max|T|."""
    err = np.abs((got4 - adv4) - want).max() / np.abs(want).max()
    assert err <= RHS_TOL, f"{what}: {err:.2e} of max|T| > {RHS_TOL:.0e}"
    return err


def rhs_checks(kind, order, flags, scalar_too, **kw):
    _, _, _, q, _, _ = R.inputs(order, **kw)
    ref = reference("rhs", kind, order, **kw)
    assert np.abs(ref["T"]).max() > 0 and relmax(ref["T"], ref["Ts"]) > 1e-3
    errs = []
    s = solver(kind, order, flags, **kw)
    got = s.computeRHS4(*q)
    lam = s.globalSpeed if kind == "B4" else None
    errs.append(check_term(got[3], ref["adv"][3], ref["T"], f"{kind} T"))
    got_f = s.computeRHS4(*q, filter=True)
    errs.append(check_term(got_f[3], ref["adv_filtered"][3], ref["FT"], f"{kind} Filter T"))
    s.close()
    plain = solver(kind, order, flags, diffusion=None, **kw)
    for a, b in zip(got[:3], plain.computeRHS4(*q)[:3]):
        assert np.array_equal(a, b)                                        # planes 0-2 are the solver's without diffusion
    if kind == "B4":
        assert lam == plain.globalSpeed
    for a, b in zip(got_f[:3], plain.computeRHS4(*q, filter=True)[:3]):
        assert np.array_equal(a, b)
    plain.close()
    if scalar_too:
        s = solver(kind, order, flags, diffusion="scalar", **kw)
        errs.append(check_term(s.computeRHS4(*q)[3], ref["adv"][3], ref["Ts"], f"{kind} T, scalar kappa"))
        errs.append(check_term(s.computeRHS4(*q, filter=True)[3], ref["adv_filtered"][3], ref["FTs"], f"{kind} Filter T, scalar kappa"))
        s.close()
    return errs


@cases
def test_rhs(order, form):
    errs = []
    for kind in ("A4", "D", "B4"):
        errs += rhs_checks(kind, order, FORMS[form], scalar_too=kind == "A4")
    print(f"N{order} {form}: " + " ".join(f"{e:.2e}" for e in errs))


def stepped(kind, order, flags, what, run, sponge=False, **kw):
    _, _, _, q, _, _ = R.inputs(order, **kw)
    ref, t_end = reference(what, kind, order, **kw)
    assert all(np.isfinite(a).all() for a in ref)
    s = solver(kind, order, flags, sponge=sponge, **kw)
    s.setState4(*q)
    run(s)
    got = s.getState4()
    assert relmax(got[1], q[1]) > 1e-5 and relmax(got[3], q[3]) > 1e-5                  # the state moved, the tracer too
    errs = assert_fields_close(got, ref, STATE_TOL, what=f"{kind} {what}")
    if kind == "B4":
        assert abs(s.time - t_end) <= 1e-12 * t_end
    s.close()
    return errs


@cases
def test_lserk4_stages(order, form):
    dt = step_size(order)

    def run(s):
        s.lserk4Stages(dt, 4)
        s.lserk4Stages(dt, 3)

    errs = [e for kind in ("B4", "D") for e in stepped(kind, order, FORMS[form], "lserk", run)]
    print(f"N{order} {form} lserk: " + " ".join(f"{e:.2e}" for e in errs))


@cases
def test_rk2_filter_steps(order, form):
    dt = step_size(order)
    errs = [e for kind in ("A4", "B4") for e in stepped(kind, order, FORMS[form], "rk2", lambda s: s.stepRK2(dt, 2, filter=True))]
    print(f"N{order} {form} rk2: " + " ".join(f"{e:.2e}" for e in errs))


@cases
def test_heun_steps(order, form):
    dt = step_size(order)

    def run(s):
        s.stepSSPRK2(dt, 1, sponge=SPONGE_SCALAR)
        s.stepSSPRK2(dt, 2, sponge=SPONGE_SCALAR)

    errs = [e for kind in ("B4", "D") for e in stepped(kind, order, FORMS[form], "heun", run, sponge=True)]
    print(f"N{order} {form} heun: " + " ".join(f"{e:.2e}" for e in errs))


@pytest.mark.parametrize("order,form", [(1, "affine"), (3, "nodal"), (5, "affine"), (8, "nodal")])
def test_mesh_smaller_than_a_tile(order, form):
    """buildBoxMesh(2, 2): K = 8 < 64 (and < 16)."""
    kw = dict(nx=2, ny=2)
    assert R.inputs(order, **kw)[1]["x"].shape[1] == 8
    for kind in ("A4", "B4"):
        rhs_checks(kind, order, FORMS[form], scalar_too=True, **kw)
    dt = step_size(order, **kw)
    stepped("B4", order, FORMS[form], "lserk", lambda s: s.lserk4Stages(dt, 7), **kw)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", [2, 4, 6])
def test_renumbered_mesh(order, form):
    """A shuffled box, renumbered on the device: the kappa and source planes and the gather index go through the permutation."""
    kw = dict(seed=11)
    s = solver("A4", order, FORMS[form] | sw2d.REORDER, **kw)
    assert s.isRenumbered
    s.close()
    for kind in ("D", "B4"):
        rhs_checks(kind, order, FORMS[form] | sw2d.REORDER, scalar_too=False, **kw)
    dt = step_size(order, **kw)
    stepped("B4", order, FORMS[form] | sw2d.REORDER, "lserk", lambda s: s.lserk4Stages(dt, 7), **kw)


def _monitored(order, form, source, steps, dt):
    nodes, t, _, q, _, d = R.inputs(order)
    s = sw2d.Sw2dSolver(nodes=nodes, g=G, flags=FORMS[form], fields=4)                  # walls on every side
    s.enableTracerDiffusion(d["kappa_field"], source=source)
    s.enableMonitor(nodes, stride=1, capacity=steps + 1)
    s.setState4(*q)
    s.sampleMonitor()
    s.stepRK2(dt, steps, filter=False)
    rec = s.monitorRecords()
    moved = relmax(s.getState4()[3], q[3])
    s.close()
    assert rec["tracer"].shape == (steps + 1,) and rec["nan"].max() == 0 and moved > 1e-6
    return rec["tracer"], np.asarray(nodes.quadratureWeights())


@pytest.mark.parametrize("order,form", [(2, "affine"), (4, "nodal"), (7, "affine")])
def test_tracer_mass_is_constant_in_a_closed_basin(order, form):
    """S = k = 0, walls on every side, 20 unfiltered RK2 steps: the monitor's int hN is constant to 1e-12 relative."""
    mass, _ = _monitored(order, form, None, 20, step_size(order))
    drift = np.abs(mass - mass[0]).max() / abs(mass[0])
    print(f"N{order} {form}: drift of int hN over 20 steps {drift:.2e}")
    assert drift <= 1e-12


@pytest.mark.parametrize("order,form", [(2, "nodal"), (4, "affine"), (7, "nodal")])
def test_a_source_feeds_tracer_mass_at_its_own_rate(order, form):
    """S != 0, k = 0: int hN grows by dt sum(w S) per step, to 1e-12 of int hN."""
    dt = step_size(order)
    S = 50.0 * R.inputs(order)[5]["source"]
    mass, w = _monitored(order, form, S, 20, dt)
    rate = dt * (w * S).sum()
    assert rate > 1e-9 * abs(mass[0])                                                   # far above the tolerance
    err = np.abs(np.diff(mass) - rate).max() / abs(mass[0])
    print(f"N{order} {form}: growth per step {rate:.3e}, largest deviation {err:.2e} of int hN")
    assert err <= 1e-12


def test_step_size():
    order = 4
    nodes, t, _, q, _, _ = R.inputs(order)
    cfl = 0.75
    plain = sw2d.Sw2dSolver(nodes=nodes, g=G, fields=4)
    plain.setState4(*q)
    advective_dt, eta = plain.computeDt(cfl)
    with pytest.raises(C.BdgError):
        plain.diffusionDt()                                                             # no diffusion: refused
    plain.close()
    fs = np.abs(t["Fscale"]).max()
    for kappa, bound in ((1e-6, False), (5.0, True), (5.0 * np.ones_like(q[0]), True), (0.0, False)):
        s = sw2d.Sw2dSolver(nodes=nodes, g=G, fields=4)
        s.enableTracerDiffusion(kappa)
        s.setState4(*q)
        kmax = float(np.max(kappa))
        want = R.DT_CONSTANT / (kmax * (order + 1) ** 4 * fs ** 2) if kmax > 0 else np.inf
        assert s.diffusionDt() == pytest.approx(want, rel=1e-14) and want == (R.diffusion_dt(R.DT_CONSTANT, kmax, order, t) if kmax else np.inf)
        dt, em = s.computeDt(cfl)
        assert em == eta
        assert (cfl * want < advective_dt) == bound
        assert dt == (cfl * s.diffusionDt() if bound else advective_dt)                 # bit for bit the advective value otherwise
        s.close()
    # 50 adaptive steps at CFL 0.75 where diffusion bounds the step: the state stays finite and the jumps of N are smoothed
    s = sw2d.Sw2dSolver(nodes=nodes, g=G, fields=4)
    s.enableTracerDiffusion(5.0)
    s.setState4(*q)
    tt, dt, steps = s.runAdaptive(cfl, 1e9, maxSteps=50, filter=True)
    got = s.getState4()
    assert steps == 50 and dt == cfl * s.diffusionDt() and all(np.isfinite(a).all() for a in got)
    spread0, spread = np.ptp(q[3] / q[0]), np.ptp(got[3] / got[0])
    print(f"runAdaptive: dt {dt:.3e} (advective {advective_dt:.3e}), spread of N {spread0:.3f} -> {spread:.3f}")
    assert spread < 0.9 * spread0
    s.close()


def test_sweep_directions_and_device_bytes():
    order = 4
    nodes, t, _, q, _, d = R.inputs(order)
    Np, K = t["x"].shape
    plain = solver("A4", order, 0, diffusion=None)
    s = solver("A4", order, 0, diffusion="scalar")
    for x in (plain, s):
        x.computeRHS4(*q)
        x.computeRHS4(*q)
    # two more launches per evaluation, each taking the next direction of the alternating sweep: four launches, two backward
    assert s.backwardLaunches - plain.backwardLaunches == 2
    ld = (K + 63) // 64 * 64
    assert s.deviceBytes - plain.deviceBytes >= 2 * Np * ld * 8                         # the two flux planes are counted
    plain.close()
    s.close()


def test_refusals_leave_the_solvers_usable():
    order = 2
    nodes, t, _, q, _, d = R.inputs(order)
    E = C.BDG_ERR_ARGUMENT
    desc = lambda kappa=0.1, field=None, source=None, decay=0.0: C.Sw2dDiffusionDesc(kappa, C.ptr(field), C.ptr(source), decay)
    enable = lambda s, dd: C.lib.bdg_sw2d_enable_tracer_diffusion(s._h, C.byref(dd))
    # three fields: ValueError from Python, BDG_ERR_ARGUMENT from the library; the solver goes on as it was
    s3 = sw2d.Sw2dSolver(nodes=nodes, g=G)
    before3 = s3.computeRHS(*q[:3])
    with pytest.raises(ValueError):
        s3.enableTracerDiffusion(0.1)
    assert enable(s3, desc()) == E and b"bdg_sw2d_enable_tracer_diffusion" in C.lib.bdg_last_error()
    assert all(np.array_equal(a, b) for a, b in zip(before3, s3.computeRHS(*q[:3])))
    s3.close()
    # bad numbers on a live four-field handle, then the right call goes through, once
    s4 = sw2d.Sw2dSolver(nodes=nodes, g=G, fields=4)
    bad_field = d["kappa_field"].copy()
    bad_field[1, 5] = -1e-3
    nan_field = d["kappa_field"].copy()
    nan_field[0, 0] = np.nan
    inf_source = d["source"].copy()
    inf_source[0, 3] = np.inf
    for dd in (desc(-0.1), desc(np.nan), desc(np.inf), desc(field=bad_field), desc(field=nan_field), desc(decay=-1.0),
               desc(decay=np.nan), desc(source=inf_source)):
        assert enable(s4, dd) == E
    assert C.lib.bdg_sw2d_enable_tracer_diffusion(s4._h, None) == E
    for bad in (-0.1, np.nan):
        with pytest.raises(C.BdgError) as e:
            s4.enableTracerDiffusion(bad)
        assert e.value.code == E
    with pytest.raises(C.BdgError):
        s4.diffusionDt()                                                                # none of these enabled it
    s4.enableTracerDiffusion(d["kappa_field"], source=d["source"], decay=d["decay"])
    ref = reference("rhs", "A4", order)
    first = s4.computeRHS4(*q)
    check_term(first[3], ref["adv"][3], ref["T"], "after the refusals")
    with pytest.raises(C.BdgError) as e:
        s4.enableTracerDiffusion(0.2)                                                   # a second call
    assert e.value.code == E
    assert all(np.array_equal(a, b) for a, b in zip(first, s4.computeRHS4(*q)))
    # ... and a diffusing solver takes no partition
    K = t["x"].shape[1]
    assert C.lib.bdg_sw2d_set_partition(s4._h, K, K, None, 0) == E and b"diffusion" in C.lib.bdg_last_error()
    assert all(np.array_equal(a, b) for a, b in zip(first, s4.computeRHS4(*q)))
    s4.close()
    # after the first evaluation
    s5 = sw2d.Sw2dSolver(nodes=nodes, g=G, fields=4)
    before = s5.computeRHS4(*q)
    with pytest.raises(C.BdgError) as e:
        s5.enableTracerDiffusion(0.1)
    assert e.value.code == E
    assert all(np.array_equal(a, b) for a, b in zip(before, s5.computeRHS4(*q)))
    s5.close()
    # a solver with a partition set
    s6 = sw2d.Sw2dSolver(nodes=nodes, g=G, fields=4, flags=sw2d.KEEP_ORDER)
    assert C.lib.bdg_sw2d_set_partition(s6._h, K, K, None, 0) == 0
    with pytest.raises(C.BdgError) as e:
        s6.enableTracerDiffusion(0.1)
    assert e.value.code == E and "partition" in str(e.value)
    assert all(np.array_equal(a, b) for a, b in zip(before, s6.computeRHS4(*q)))
    s6.close()
    # the partitioned front end says so itself
    with pytest.raises(NotImplementedError, match="partitioned"):
        halo.NativeDistributedSw2d.enable_tracer_diffusion(None, 0.1)
