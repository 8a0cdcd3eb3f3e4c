"""CPU side of tests/quadref_ld.py, the np.longdouble reference of the quadrilateral stage-kernel instances.

  * It reproduces every sw2dq_rhs_* and sw2dq_rhs4_* fixture (the reference's own functions on this repository's tables) to
    the 1e-12 per field that test_quad_setup.py and test_quad4_setup.py ask of the float64 restatements.
  * The float64 restatement stays within LD_TOL = 2.5e-13 per field of the longdouble one (a quarter of the 1e-12 the GPU is
    held to) on both 13 x 11 meshes, orders 1 to 8, all four regimes, three and four fields (with and without sources),
    plain and filtered. Measured maxima of that sweep, per regime (the test prints them): jumpy 1.27e-15, supercritical
    9.52e-16, deep 1.05e-14, contrast 1.22e-15, so the reference itself spends about 1 % of the GPU's tolerance.
  * The shear mesh is what the GPU test needs: oblique parallelograms (every metric term non-zero, no axis-aligned normal)
    that the solver's 1e-10 parallelogram test accepts at every order, while the jitter mesh is refused by it.
  * Both meshes are ragged at every tile size: K % 64, K % 32, K % 16 != 0 and at least 3 tiles.
"""
import numpy as np
import pytest

import quadref
import quadref4
import quadref_ld as Q
from regimes import REGIMES, assert_fields_close

LD_TOL = 2.5e-13


def test_longdouble_is_wider_than_float64():
    Q.require_extended_precision()
    assert np.finfo(Q.LD).eps < 1e-18 and np.finfo(Q.LD).nmant >= 63


@pytest.mark.parametrize("name", quadref.FIXTURES)
def test_longdouble_reference_matches_three_field_fixture(name):
    d, _, _, ctx = quadref.load_fixture(name)
    tl = Q.to_ld(quadref.tables(ctx))
    got = Q.rhs_ld([d["h"], d["hu"], d["hv"]], float(d["g"]), tl)
    assert all(a.dtype == Q.LD for a in got)
    assert_fields_close(Q.f64(got), [d[f"rhs{i}"] for i in (1, 2, 3)], 1e-12, what=name)


@pytest.mark.parametrize("name", quadref4.FIXTURES4)
def test_longdouble_reference_matches_four_field_fixture(name):
    d, _, _, ctx = quadref4.load_fixture4(name)
    tl = Q.to_ld(quadref.tables(ctx))
    got = Q.rhs_ld(quadref4.state(d), float(d["g"]), tl, quadref4.sources(d))
    assert all(a.dtype == Q.LD for a in got)
    assert_fields_close(Q.f64(got), quadref4.reference(d), 1e-12, what=name)


@pytest.mark.parametrize("order", range(1, 9))
@pytest.mark.parametrize("mesh", Q.MESHES)
def test_float64_restatement_is_within_a_quarter_of_the_gpu_tolerance(mesh, order):
    _, t = Q.mesh_tables(mesh, order)
    tl = Q.to_ld(t)
    F = t["Filter"]
    worst = {}
    for regime in REGIMES:
        for fs in Q.FIELD_SETS:
            fields, src = Q.field_set(t, fs)
            q = Q.state(t, fields, regime, seed=order)
            r64 = quadref.rhs(*q, Q.G, t) if fields == 3 else quadref4.rhs4(*q, Q.G, t, **(src or {}))
            assert all(a.dtype == np.float64 for a in r64)
            for filt in (False, True):
                ref = Q.f64(Q.rhs_ld(q, Q.G, tl, src, filt))
                got = [F @ a for a in r64] if filt else r64
                errs = assert_fields_close(got, ref, LD_TOL, what=f"{mesh} N{order} {regime} fields {fs} filter {filt}")
                worst[regime] = max(worst.get(regime, 0.0), max(errs))
    print(f"float64 against longdouble, {mesh} N={order}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_scalar_coriolis_is_the_array_of_that_value():
    _, t = Q.mesh_tables("jitter", 3)
    tl = Q.to_ld(t)
    q = Q.state(t, 4, "jumpy", seed=3)
    src = Q.sources(t, scalar_f=True)
    a = Q.rhs_ld(q, Q.G, tl, src)
    b = Q.rhs_ld(q, Q.G, tl, {**src, "f": np.full_like(t["x"], 0.1)})
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = Q.rhs_ld(q, Q.G, tl, Q.sources(t))
    assert np.abs(Q.f64(a)[1] - Q.f64(c)[1]).max() > 1e-6


def test_tracer_jumps_at_faces_and_sources_act():
    _, t = Q.mesh_tables("shear", 4)
    q = Q.state(t, 4, "smooth", seed=4)
    hN = q[3].ravel("F")
    inner = t["vmapM"] != t["vmapP"]
    assert np.abs(hN[t["vmapM"]] - hN[t["vmapP"]])[inner].min() > 0
    tl = Q.to_ld(t)
    a, b = Q.f64(Q.rhs_ld(q, Q.G, tl, Q.sources(t))), Q.f64(Q.rhs_ld(q, Q.G, tl))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3])
    assert np.abs(a[1] - b[1]).max() > 1e-2 and np.abs(a[2] - b[2]).max() > 1e-2


def _spreads(t):
    """The quantities of the solver's parallelogram test (sw2d_quad_device.hip): the largest |value - mean| of a metric term
    inside an element over the element's largest metric term, and of nx, ny (absolute) and Fscale (over the face's largest)
    along a face."""
    Nq = t["order"] + 1
    met = np.stack([t[k] for k in ("rx", "sx", "ry", "sy")])                      # (4, Np, K)
    scale = np.abs(met).max(axis=(0, 1))
    metric = (np.abs(met - met.mean(axis=1, keepdims=True)).max(axis=1) / scale).max()
    face = 0.0
    for k in ("nx", "ny", "Fscale"):
        a = t[k].reshape(4, Nq, -1)
        sc = np.abs(a).max(axis=1) if k == "Fscale" else 1.0
        face = max(face, (np.abs(a - a.mean(axis=1, keepdims=True)).max(axis=1) / sc).max())
    return metric, face


@pytest.mark.parametrize("order", range(1, 9))
def test_shear_mesh_is_oblique_and_a_parallelogram_mesh_to_the_solver(order):
    _, t = Q.mesh_tables("shear", order)
    # the inverse Jacobian of x = SHEAR diag(1/13, 1/11) (r, s) (up to the rotation of the local order, which permutes and
    # signs its entries) has the entries 13 * (0.8, -0.35) / 0.87 and 11 * (0.2, 1) / 0.87: the smallest is 11 * 0.2 / 0.87
    smallest = min(np.abs(t[k]).min() for k in ("rx", "sx", "ry", "sy"))
    assert abs(smallest - 11 * 0.2 / 0.87) < 1e-9, smallest
    # the normals are +-(0.2, 1) / |.| and +-(0.8, -0.35) / |.|: no component below 0.2 / sqrt(1.04)
    assert min(np.abs(t["nx"]).min(), np.abs(t["ny"]).min()) > 0.19
    metric, face = _spreads(t)
    print(f"shear N={order}: metric spread {metric:.2e}, face spread {face:.2e}")
    assert metric < 1e-11 and face < 1e-11
    # the rotated local order reaches the tables: rx takes the four values of the four rotations
    assert len(set(np.round(t["rx"][0], 6))) == 4


@pytest.mark.parametrize("order", range(1, 9))
def test_jitter_mesh_is_refused_by_the_parallelogram_test(order):
    _, t = Q.mesh_tables("jitter", order)
    metric, face = _spreads(t)
    assert metric > 1e-3 and face > 1e-3            # far beyond the solver's 1e-10


@pytest.mark.parametrize("mesh", Q.MESHES)
def test_meshes_are_ragged_at_every_tile_size(mesh):
    E, V = Q.mesh_arrays(mesh)
    K = len(E)
    assert K == 143 and V.shape == (14 * 12, 2)
    for tile in (64, 32, 16):
        assert K % tile == 15 and -(-K // tile) >= 3
    _, t = Q.mesh_tables(mesh, 2)
    # walls on the whole boundary: 2 (13 + 11) faces of 3 nodes
    assert len(t["mapW"]) == 2 * (13 + 11) * 3 and (t["vmapM"] == t["vmapP"]).sum() == len(t["mapW"])
    # shuffled: neighbours are not consecutive elements
    assert np.abs(t["vmapP"] // 9 - t["vmapM"] // 9).max() > 64


def test_steppers_reduce_to_their_definitions():
    """One RK2 step and two LSERK4 stages written out by hand, and the split of a stage run."""
    import blitzdg_amd.pyblitzdg as dg
    _, t = Q.mesh_tables("jitter", 2)
    tl = Q.to_ld(t)
    q = Q.state(t, 3, "smooth", seed=2)
    dt = Q.LD(1e-3)
    k1 = Q.rhs_ld(q, Q.G, tl, filt=True)
    k2 = Q.rhs_ld([a + dt / 2 * b for a, b in zip(q, k1)], Q.G, tl, filt=True)
    want = [a + dt * b for a, b in zip(q, k2)]
    got = Q.rk2_steps(q, Q.G, tl, 1e-3, 1, True)
    assert all(np.abs(a - b).max() < 1e-17 * 11 for a, b in zip(got, want))
    a0, b0, a1, b1 = (Q.LD(x) for x in (dg.LSERK4.rk4a[0], dg.LSERK4.rk4b[0], dg.LSERK4.rk4a[1], dg.LSERK4.rk4b[1]))
    assert a0 == 0
    res = [dt * r for r in Q.rhs_ld(q, Q.G, tl)]
    qa = [x + b0 * r for x, r in zip(q, res)]
    res = [a1 * x + dt * r for x, r in zip(res, Q.rhs_ld(qa, Q.G, tl))]
    want = [x + b1 * r for x, r in zip(qa, res)]
    got = Q.lserk4_stages(q, Q.G, tl, 1e-3, 2)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert all(a.dtype == Q.LD for a in got)
