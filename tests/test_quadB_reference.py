"""tests/quadrefB.py, the NumPy restatement of the tidal right-hand side (src/sw2d/main.cpp:279-484, "variant B"), held to what
the repository has from the reference, and measured; the host helpers of the quadrilateral tidal set-up. No GPU.

  * On triangle tables rhsB reproduces the sw2d_rhsB_{degenerate, bed, bed_drag}_* fixtures (output of the reference's Python
    RHS in the three constructions where variant B degenerates to it: tests/golden/make_golden.py:320-393) to RHS_TOL = 1e-12 of
    max|RHS| per field; on quadrilateral tables the sw2dq_rhsB_* fixtures of tests/golden/make_golden_quadsB.py, the same.
  * The float64 restatement stays within LD_TOL = 2.5e-13 per field of the np.longdouble one (the bound of
    tests/test_quad_reference_ld.py) in the four regimes of tests/regimes.py over a bed that jumps at every face, with an open
    boundary at a time where the tide is not zero, drag and Coriolis. Measured here: 2.1e-15 at most (N = 12, jitter).
  * Still water over the jumping bed is a steady state of the restatement, with walls and with an open side whose tide is zero.
  * bedSlopes and buildSpongeCoeff of QuadNodesProvisioner against NumPy.
  * NULL handles are refused without touching a GPU."""
import ctypes
import os

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
import quadref
import quadref_ld as Q
import quadrefB as B
from conftest import GOLDEN
from regimes import REGIMES, assert_fields_close, regime_fields

RHS_TOL = 1e-12
LD_TOL = 2.5e-13
TIDE = (3.0, 3600 * 12.42, 0.15 / 3600)

TRI_FIXTURES = [f"{kind}_{case}" for kind in ("degenerate", "bed", "bed_drag")
                for case in ("coarse_box_N3", "box6x5_shuffled_N6", "box3x2_N8")
                if os.path.exists(os.path.join(GOLDEN, f"sw2d_rhsB_{kind}_{case}.npz"))]
QUAD_FIXTURES = [f"{kind}_coarse_box_quads_N{n}" for kind in ("degenerate", "bed", "bed_drag") for n in (3, 6, 10)]


def fixture_vb(d):
    """The variant-B parameters of a fixture: no open boundary, so the tide does not enter."""
    zero = np.zeros_like(d["h"])
    return {"g": float(d["g"]), "H": d["H"], "Hx": d["Hx"] if "Hx" in d else zero, "Hy": d["Hy"] if "Hy" in d else zero,
            "mapO": [], "CD": float(d["CD"]) if "CD" in d else 0.0, "f": float(d["f"]), "tide": TIDE}


def quad_fixture(name):
    """(npz, tables) of a sw2dq_rhsB_* fixture, the tables rebuilt from its mesh."""
    d = np.load(os.path.join(GOLDEN, f"sw2dq_rhsB_{name}.npz"))
    mesh = dg.MeshManager()
    mesh.buildMesh(d["EToV"], d["Vert"])
    nodes = dg.QuadNodesProvisioner(int(d["order"]), mesh)
    nodes.buildFilter(0.99 * int(d["order"]), 4)
    return d, quadref.tables(nodes.dgContext()), nodes


def test_the_triangle_fixtures_are_all_there():
    assert len(TRI_FIXTURES) == 8


@pytest.mark.parametrize("name", TRI_FIXTURES)
def test_restatement_matches_the_reference_on_triangles(name):
    d = np.load(os.path.join(GOLDEN, f"sw2d_rhsB_{name}.npz"))
    t = {k: d[k] for k in ("Dr", "Ds", "Lift", "rx", "sx", "ry", "sy", "nx", "ny", "Fscale", "vmapM", "vmapP", "mapW")}
    assert t["nx"].shape[0] == 3 * (int(d["order"]) + 1)
    got = B.rhsB(d["h"], d["hu"], d["hv"], t, fixture_vb(d))
    errs = assert_fields_close(got, [d["rhs1"], d["rhs2"], d["rhs3"]], RHS_TOL, what=name)
    print(name, " ".join(f"{e:.2e}" for e in errs))


@pytest.mark.parametrize("name", QUAD_FIXTURES)
def test_restatement_matches_the_reference_on_quadrilaterals(name):
    d, t, _ = quad_fixture(name)
    assert t["nx"].shape[0] == 4 * (int(d["order"]) + 1)
    ref = [d["rhs1"], d["rhs2"], d["rhs3"]]
    vb = fixture_vb(d)
    got = B.rhsB(d["h"], d["hu"], d["hv"], t, vb)
    errs = assert_fields_close(got, ref, RHS_TOL, what=name)
    Q.require_extended_precision()
    got_ld = B.rhsB(*B.to_ld([d["h"], d["hu"], d["hv"]]), Q.to_ld(t), B.vb_ld(vb))
    assert all(a.dtype == B.LD for a in got_ld)
    errs += assert_fields_close(Q.f64(got_ld), ref, RHS_TOL, what=name + " (longdouble)")
    print(name, " ".join(f"{e:.2e}" for e in errs))


def regime_problem(nodes, t, regime, seed):
    """A regime state and a variant-B set-up scaled to it: the bed jumps by at most a fifth of the smallest depth at a face (no
    star depth reaches 0), the tide amplitude is a tenth of it."""
    q = list(regime_fields(t["x"], t["y"], regime, seed))
    hmin = q[0].min()
    H = B.jumping_bed(t, float(np.median(q[0])), 0.2 * hmin, seed=seed)
    Hx, Hy = nodes.bedSlopes(H)
    vb = {"g": B.G, "H": H, "Hx": Hx, "Hy": Hy, "mapO": t["mapO"], "CD": 2.5e-2, "f": 0.1, "tide": (0.1 * hmin, 40.0, 0.05)}
    return q, vb


def test_tide_is_not_zero_where_the_tests_evaluate_it():
    assert abs(B.tide_value(37.0, (1.0, 40.0, 0.05))) > 0.3


@pytest.mark.parametrize("order", [1, 4, 8, 12])
@pytest.mark.parametrize("mesh", Q.MESHES)
def test_float64_restatement_is_within_a_quarter_of_the_gpu_tolerance(mesh, order):
    Q.require_extended_precision()
    nodes, t = B.mesh_tables(mesh, order)
    tl = Q.to_ld(t)
    worst = 0.0
    for regime in REGIMES:
        q, vb = regime_problem(nodes, t, regime, seed=order)
        H = vb["H"].ravel("F")
        assert np.abs(H[t["vmapM"]] - H[t["vmapP"]]).max() > 0.01 * q[0].min()            # the bed does jump
        ref = B.rhsB(*B.to_ld(q), tl, B.vb_ld(vb), time=37.0, return_speed=True)
        got = B.rhsB(*q, t, vb, time=37.0, return_speed=True)
        assert all(np.all(np.isfinite(a)) for a in got[:3])
        errs = assert_fields_close(got[:3], Q.f64(ref[:3]), LD_TOL, what=f"{mesh} N{order} {regime}")
        assert abs(got[3] - float(ref[3])) <= LD_TOL * float(ref[3])
        worst = max(worst, *errs)
    print(f"{mesh} N{order}: float64 against longdouble, largest per-field error {worst:.2e}")


@pytest.mark.parametrize("open_side", [False, True])
@pytest.mark.parametrize("order", [1, 3, 6])
@pytest.mark.parametrize("mesh", Q.MESHES)
def test_still_water_over_a_jumping_bed_is_steady(mesh, order, open_side):
    nodes, t = B.mesh_tables(mesh, order)
    H = B.jumping_bed(t, 10.0, 2.0, flat=True)
    Hx, Hy = nodes.bedSlopes(H)
    period = 40.0
    vb = {"g": B.G, "H": H, "Hx": Hx, "Hy": Hy, "mapO": t["mapO"] if open_side else [], "CD": 2.5e-2, "f": 0.1,
          "tide": (3.0, period, 0.05)}
    time = period / 4                                                   # cos(2 pi t / T) = 0: the tide term vanishes
    assert abs(B.tide_value(time, vb["tide"])) < 1e-15
    r = B.rhsB(H.copy(), np.zeros_like(H), np.zeros_like(H), t, vb, time=time)
    bound = 1e-12 * B.G * H.max() ** 2 / B.min_edge(*Q.mesh_arrays(mesh))
    worst = max(np.abs(a).max() for a in r)
    print(f"{mesh} N{order} open={open_side}: max|RHS| {worst:.2e}, bound {bound:.2e}")
    assert worst <= bound


@pytest.mark.parametrize("order", [2, 5, 8, 12])
def test_bed_slopes_match_the_formula(order):
    """Against the formula evaluated by NumPy in np.longdouble: at N = 12 NumPy's own float64 evaluation of it is 3.7e-13 away
    from that (the mean of H cancels in Dr H), so it cannot serve as the reference of a 1e-13 bound."""
    Q.require_extended_precision()
    nodes, t = B.mesh_tables("jitter", order)
    x, y = t["x"], t["y"]
    H = 10.0 + 1.5 * x - 0.8 * y * y + 0.3 * np.sin(3 * x) * np.cos(2 * y)
    Hx, Hy = nodes.bedSlopes(H)
    tl, Hl = Q.to_ld(t), np.asarray(H, dtype=B.LD)
    wx = tl["Filter"] @ (tl["rx"] * (tl["Dr"] @ Hl) + tl["sx"] * (tl["Ds"] @ Hl))
    wy = tl["Filter"] @ (tl["ry"] * (tl["Dr"] @ Hl) + tl["sy"] * (tl["Ds"] @ Hl))
    assert np.abs(wx).max() > 0.5 and np.abs(wy).max() > 0.5
    ex, ey = float(np.abs(Hx - wx).max() / np.abs(wx).max()), float(np.abs(Hy - wy).max() / np.abs(wy).max())
    print(f"N{order}: bedSlopes against the longdouble formula {ex:.2e} {ey:.2e}")
    assert ex <= 1e-13 and ey <= 1e-13


def test_sponge_coefficient_is_the_transcription():
    nodes, t = B.mesh_tables("shear", 3)
    x, y, mapO = t["x"], t["y"], t["mapO"]
    strength, radius = 100.0, 0.6
    got = nodes.buildSpongeCoeff(mapO, strength, radius)
    xo, yo = x.ravel("F")[t["vmapM"][mapO]], y.ravel("F")[t["vmapM"][mapO]]
    want = np.zeros_like(x)
    for n in range(x.shape[0]):                                          # main.cpp:535-551
        for k in range(x.shape[1]):
            dist = np.hypot(x[n, k] - xo, y[n, k] - yo)
            dist = dist[dist < radius]
            if dist.size:
                want[n, k] = strength * (1.0 - dist.min() / radius)
    assert 0 < (want > 0).sum() < want.size and want.max() == strength
    assert np.array_equal(got, want)
    assert not nodes.buildSpongeCoeff([], strength, radius).any()


def test_null_handles_are_refused():
    from blitzdg_amd import _capi as C
    lib, ARG = C.lib, C.BDG_ERR_ARGUMENT
    a = np.zeros((4, 1))
    d = C.Sw2dVbDesc(C.ptr(a), C.ptr(a), C.ptr(a), None, 0, 0.0, 0.0, 3.0, 100.0, 0.0, None)
    assert lib.bdg_sw2dq_enable_variant_b(None, ctypes.byref(d)) == ARG
    assert lib.bdg_sw2dq_enable_variant_b(None, None) == ARG
    v, ms = ctypes.c_double(), ctypes.c_float()
    assert lib.bdg_sw2dq_set_time(None, 1.0) == ARG
    assert lib.bdg_sw2dq_get_time(None, ctypes.byref(v)) == ARG
    assert lib.bdg_sw2dq_global_speed(None, ctypes.byref(v)) == ARG
    assert lib.bdg_sw2dq_step_ssprk2(None, 0.1, 1, 0, 0.0) == ARG
    assert lib.bdg_sw2dq_step_ssprk2_exchanged(None, 0.1, 1, 0, 0.0) == ARG
    assert lib.bdg_sw2dq_time_speed(None, 1, ctypes.byref(ms)) == ARG
    assert lib.bdg_quadnodes_bed_slopes(None, C.ptr(a), C.ptr(a), C.ptr(a)) == ARG
    assert lib.bdg_quadnodes_sponge_coeff(None, None, 0, 1.0, 1.0, C.ptr(a)) == ARG
    nodes, _ = B.mesh_tables("shear", 1)
    assert lib.bdg_quadnodes_bed_slopes(nodes._h, None, None, None) == ARG
    assert lib.bdg_quadnodes_sponge_coeff(nodes._h, None, 3, 1.0, 1.0, None) == ARG
