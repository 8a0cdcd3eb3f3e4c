"""The halo plan (blitzdg_amd.halo.build_plan / build_local_mesh) on quadrangle meshes, and unchanged on triangles.

Quadrangle meshes -- a shuffled 12 x 9 box and tests/golden/coarse_box_quads_fine.msh -- split 2-, 3- and 4-way by
MeshManager.partitionMesh: ownership, ghosts, send / receive pairing, the interior range, and the rank-local meshes.
Triangle plans built from flat or 2-D tables equal the plan recorded before quadrangles were supported
(tests/golden/halo_plan_tri_box6x5.npz). CPU only."""
import os

import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
from blitzdg_amd.halo import build_local_mesh, build_plan
from quadref import GOLDEN, quad_box


def shuffled_box():
    E, V = quad_box(12, 9)
    rng = np.random.default_rng(7)
    return E[rng.permutation(len(E))], V


def quad_mesh(name):
    mesh = dg.MeshManager()
    if name == "box12x9_shuffled":
        mesh.buildMesh(*shuffled_box())
    else:
        mesh.readMesh(os.path.join(GOLDEN, name + ".msh"))
    return mesh


def plans_of(mesh, world):
    mesh.partitionMesh(world)
    tabs = mesh.elements, mesh.vertices, mesh.EToE, mesh.elementPartitionMap
    return [build_plan(*tabs, r, world, bctype=mesh.bcType) for r in range(world)]


@pytest.mark.parametrize("name", ["box12x9_shuffled", "coarse_box_quads_fine"])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_quad_plan_partitions_and_pairs(name, world):
    mesh = quad_mesh(name)
    assert mesh.numFaces == 4
    plans = plans_of(mesh, world)
    EToE = np.asarray(mesh.EToE).reshape(-1, 4)
    epart = np.asarray(mesh.elementPartitionMap).reshape(-1)
    K = mesh.numElements
    owned = np.zeros(K, dtype=int)
    for p in plans:
        owned[p.own_global] += 1
    assert (owned == 1).all()
    for r, p in enumerate(plans):
        own = p.own_global
        assert (epart[own] == r).all()
        nb = EToE[own]
        remote = epart[nb] != r
        ghosts = np.unique(nb[remote])                     # the remote face neighbours, grouped by owner
        assert np.array_equal(p.halo_global, ghosts[np.lexsort((ghosts, epart[ghosts]))])
        # [interior | partition boundary]: no interior element has a remote neighbour, every boundary element has one
        assert not remote[:p.num_interior].any()
        assert remote[p.num_interior:].any(axis=1).all()
        assert 0 < p.num_interior < p.num_owned
        # ghosts grouped by owner, one contiguous receive range per peer
        start = 0
        for peer, s, c in p.recv_slices:
            assert s == start and (epart[p.halo_global[s:s + c]] == peer).all()
            start += c
        assert start == p.num_halo
        # what r sends to a peer is, record for record, what the peer receives from r
        for peer, s, c in p.send_slices:
            sent = own[p.send_local[s:s + c]]
            q = plans[peer]
            (qs, qc), = [(s2, c2) for src, s2, c2 in q.recv_slices if src == r]
            assert c == qc and np.array_equal(sent, q.halo_global[qs:qs + qc])
            assert (p.send_local[s:s + c] >= p.num_interior).all()
        assert {pr for pr, _, _ in p.send_slices} == {pr for pr, _, _ in p.recv_slices}


@pytest.mark.parametrize("name", ["box12x9_shuffled", "coarse_box_quads_fine"])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_quad_local_mesh(name, world):
    mesh = quad_mesh(name)
    gE = np.asarray(mesh.elements).reshape(-1, 4)
    gV = np.asarray(mesh.vertices)
    gbc = np.asarray(mesh.bcType).reshape(-1, 4)
    for p in plans_of(mesh, world):
        assert p.local_EToV.shape == (p.num_owned + p.num_halo, 4) and p.local_bctype.shape[1] == 4
        local = build_local_mesh(p)
        assert local.numFaces == 4 and local.numElements == p.num_owned + p.num_halo
        le = np.asarray(local.elements)
        assert np.array_equal(le, p.local_EToV)  # vertex order unchanged
        lv = np.asarray(local.vertices)
        ids = p.local_to_global
        assert np.array_equal(lv[le][..., :2], gV[gE[ids]][..., :2])  # the same corners, in the same order
        bc = np.asarray(local.bcType).reshape(-1, 4)
        assert np.array_equal(bc[:p.num_owned], gbc[p.own_global])


def _tri_plans(flat):
    mesh = dg.MeshManager()
    mesh.buildBoxMesh(6, 5, shuffleSeed=3)
    mesh.partitionMesh(3)
    E, V, EToE, ep, bc = mesh.elements, mesh.vertices, mesh.EToE, mesh.elementPartitionMap, mesh.bcType
    if flat:
        E, EToE, bc = (np.asarray(a).reshape(-1) for a in (E, EToE, bc))
    return [build_plan(E, V, EToE, ep, r, 3, bctype=bc) for r in range(3)]


@pytest.mark.parametrize("flat", [True, False])
def test_triangle_plan_is_unchanged(flat):
    want = np.load(os.path.join(GOLDEN, "halo_plan_tri_box6x5.npz"))
    for r, p in enumerate(_tri_plans(flat)):
        for key in ("own_global", "halo_global", "send_local", "local_EToV", "local_verts", "local_bctype"):
            got = getattr(p, key)
            assert got.dtype == want[f"{key}{r}"].dtype and np.array_equal(got, want[f"{key}{r}"]), (r, key)
        assert p.num_interior == int(want[f"num_interior{r}"])
        assert np.array_equal(np.asarray(p.send_slices).reshape(-1, 3), want[f"send_slices{r}"].reshape(-1, 3))
        assert np.array_equal(np.asarray(p.recv_slices).reshape(-1, 3), want[f"recv_slices{r}"].reshape(-1, 3))


def test_bad_face_count_is_refused():
    E, V = quad_box(2)
    with pytest.raises(ValueError, match="3 or 4 columns"):
        build_plan(np.zeros((4, 5), dtype=int), V, np.zeros((4, 5), dtype=int), np.zeros(4, dtype=int), 0, 1)
