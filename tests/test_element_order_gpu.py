"""The patch numbering of the sw2d solver on the device: per-element arithmetic does not depend on the slot, so a
renumbered solver reproduces the caller-order solver bit for bit, whatever the patch size (BDG_SW2D_ORDER_PATCH; 0 is
the breadth-first order). Meshes: the 61x39-cell box (K = 4758: a ragged last wave, patches of 7 and 64 that straddle
waves) and its seed-9 shuffle. Both the default kernel choice of that size and the unrolled N <= 4 kernel of large
meshes (BDG_SW2D_AFFINE_VARIANT=0) are run."""
import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
from blitzdg_amd import sw2d
from conftest import seeded_fields

pytestmark = pytest.mark.gpu

PATCHES = (0, 7, 64)
_NODES = {}


def nodes_of(order, seed):
    if (order, seed) not in _NODES:
        mesh = dg.MeshManager()
        mesh.buildBoxMesh(61, 39, shuffleSeed=seed)
        nodes = dg.TriangleNodesProvisioner(order, mesh)
        ctx = nodes.dgContext()
        _NODES[order, seed] = nodes, seeded_fields(ctx.x, ctx.y, seed=order)
    return _NODES[order, seed]


def ten_stages(solver, q0):
    solver.setState(*q0)
    dt, eta = solver.computeDt(0.5)
    solver.lserk4Stages(dt, 10)  # two steps: FIRST, MID x3 and LAST twice
    return solver.getState(), dt, eta, solver.computeDt(0.5)


@pytest.mark.parametrize("variant", [None, "0"], ids=["default_kernel", "unrolled_kernel"])
@pytest.mark.parametrize("seed", [0, 9], ids=["natural", "shuffled"])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_renumbered_solver_matches_caller_order_bit_for_bit(order, seed, variant, monkeypatch):
    if variant is not None:
        monkeypatch.setenv("BDG_SW2D_AFFINE_VARIANT", variant)
    nodes, q0 = nodes_of(order, seed)
    keep = sw2d.Sw2dSolver(nodes=nodes, flags=sw2d.KEEP_ORDER)
    assert not keep.isRenumbered
    ref, dt_ref, eta_ref, after_ref = ten_stages(keep, q0)
    assert all(np.isfinite(f).all() for f in ref) and not np.array_equal(ref[0], q0[0])
    for patch in PATCHES:
        monkeypatch.setenv("BDG_SW2D_ORDER_PATCH", str(patch))
        s = sw2d.Sw2dSolver(nodes=nodes, flags=sw2d.REORDER)
        assert s.isRenumbered
        got, dt, eta, after = ten_stages(s, q0)
        assert (dt, eta) == (dt_ref, eta_ref) and after == after_ref, patch
        for name, a, b in zip(("h", "hu", "hv"), got, ref):
            assert np.array_equal(a, b), f"patch {patch}: {name} differs in {np.count_nonzero(a != b)} entries"


@pytest.mark.parametrize("seed", [0, 9], ids=["natural", "shuffled"])
def test_state_round_trips_under_the_patch_order(seed, monkeypatch):
    nodes, _ = nodes_of(3, seed)
    rng = np.random.default_rng(5)
    f = [rng.standard_normal((10, 4758)) for _ in range(3)]
    for patch in PATCHES + (None,):  # None: the default patch size
        if patch is None:
            monkeypatch.delenv("BDG_SW2D_ORDER_PATCH")
        else:
            monkeypatch.setenv("BDG_SW2D_ORDER_PATCH", str(patch))
        s = sw2d.Sw2dSolver(nodes=nodes, flags=sw2d.REORDER)
        s.setState(*f)
        assert all(np.array_equal(a, b) for a, b in zip(f, s.getState())), patch


def test_is_renumbered_for_forced_and_natural_solvers():
    nat = dg.MeshManager()
    nat.buildBoxMesh(60, 40)
    nodes = dg.TriangleNodesProvisioner(2, nat)
    assert not sw2d.Sw2dSolver(nodes=nodes).isRenumbered
    assert sw2d.Sw2dSolver(nodes=nodes, flags=sw2d.REORDER).isRenumbered
    # the 61x39 box at N = 4 moves more than one L2 per stage, but no neighbour is further than 121 slots away
    assert not sw2d.Sw2dSolver(nodes=nodes_of(4, 0)[0]).isRenumbered
    assert sw2d.Sw2dSolver(nodes=nodes_of(4, 9)[0]).isRenumbered  # shuffled: the mean-distance rule
