"""The element numbering of the sw2d solvers (csrc/host/element_order.cpp) through bdg_element_order and
bdg_element_order_wanted: graph only, no GPU. Natural order of a box mesh is row by row, two triangles per cell,
so a third of the interior faces have their neighbour 2*nx - 1 slots away.

Locality bounds (200x100-cell box, patch 256): the share of interior faces with the neighbour more than 185 slots
away is at most half the natural order's 0.332, and the share with both elements in one 64-slot block at least
the natural order's 0.658."""
import numpy as np
import pytest

import blitzdg_amd.pyblitzdg as dg
from blitzdg_amd._capi import check, lib, ptr

_ETOE = {}


def box_etoe(nx, ny, seed=0):
    if (nx, ny, seed) not in _ETOE:
        mesh = dg.MeshManager()
        mesh.buildBoxMesh(nx, ny, shuffleSeed=seed)
        e = np.ascontiguousarray(mesh.EToE, dtype=np.int32)
        assert e.shape == (2 * nx * ny, 3)
        e.setflags(write=False)
        _ETOE[nx, ny, seed] = e
    return _ETOE[nx, ny, seed]


def two_boxes():
    a, b = box_etoe(61, 39), box_etoe(7, 5)
    return np.ascontiguousarray(np.concatenate([a, b + a.shape[0]]), dtype=np.int32)


MESHES = {"box61x39": lambda: box_etoe(61, 39), "box61x39_shuffled": lambda: box_etoe(61, 39, seed=9),
          "two_boxes": two_boxes}


def element_order(etoe, patch):
    perm = np.full(etoe.shape[0], -1, dtype=np.int32)
    check(lib.bdg_element_order(ptr(etoe), etoe.shape[0], int(patch), ptr(perm)))
    return perm


def wanted(etoe, order):
    return lib.bdg_element_order_wanted(ptr(etoe), etoe.shape[0], int(order))


def locality(etoe, perm, far=185, block=64):
    """(share of interior faces whose neighbour is more than `far` slots away, share with both elements in one block)."""
    k = np.arange(etoe.shape[0])[:, None]
    interior = etoe != k
    a, b = perm[k] + 0 * etoe, perm[etoe]
    n = interior.sum()
    return ((np.abs(a - b) > far) & interior).sum() / n, ((a // block == b // block) & interior).sum() / n


@pytest.mark.parametrize("mesh", MESHES)
def test_every_patch_size_gives_a_bijection(mesh):
    etoe = MESHES[mesh]()
    K = etoe.shape[0]
    for patch in (1, 7, 64, 256, K, K + 5, 0):  # 0: the breadth-first order
        perm = element_order(etoe, patch)
        assert np.array_equal(np.sort(perm), np.arange(K)), (mesh, patch)


def test_a_patch_as_large_as_a_connected_mesh_is_the_identity():
    for etoe in (box_etoe(61, 39), box_etoe(61, 39, seed=9)):
        K = etoe.shape[0]
        for patch in (K, K + 5):
            assert np.array_equal(element_order(etoe, patch), np.arange(K))
    # one element per patch: the order in which the patches start, so not the identity on a shuffled mesh
    assert not np.array_equal(element_order(box_etoe(61, 39, seed=9), 1), np.arange(4758))


def test_first_patch_grows_from_element_zero_and_is_sorted_by_caller_index():
    perm = element_order(box_etoe(61, 39, seed=9), 64)
    first = np.argsort(perm)[:64]  # slot -> caller element
    assert first[0] == 0 and np.all(np.diff(first) > 0)


def test_disconnected_components_continue_in_caller_order():
    etoe = two_boxes()
    perm = element_order(etoe, 256)
    n0 = 4758
    assert np.array_equal(np.sort(perm[:n0]), np.arange(n0))  # the first box fills the first slots, the second the rest
    assert np.array_equal(np.sort(perm[n0:]), np.arange(n0, etoe.shape[0]))


@pytest.mark.parametrize("mesh", MESHES)
def test_result_does_not_depend_on_the_worker_count(mesh, monkeypatch):
    etoe = MESHES[mesh]()
    got = {}
    for threads in ("1", "8"):
        monkeypatch.setenv("OMP_NUM_THREADS", threads)
        monkeypatch.delenv("BDG_NUM_THREADS", raising=False)
        got[threads] = [element_order(etoe, p) for p in (0, 7, 64, 256)] + [wanted(etoe, n) for n in (2, 4, 8)]
    assert all(np.array_equal(a, b) for a, b in zip(got["1"], got["8"]))


def test_locality_of_the_patch_order_on_a_structured_box():
    etoe = box_etoe(200, 100)
    K = etoe.shape[0]
    far_nat, same_nat = locality(etoe, np.arange(K))
    assert abs(far_nat - 0.332) < 0.002 and abs(same_nat - 0.658) < 0.002  # the measure itself
    far, same = locality(etoe, element_order(etoe, 256))
    print(f"patch 256: far {far:.4f} (natural {far_nat:.4f}), same block {same:.4f} (natural {same_nat:.4f})")
    assert far <= 0.5 * far_nat
    assert same >= same_nat


def test_decision_rule():
    assert wanted(box_etoe(60, 40), 2) == 0              # 3 MB of stage traffic: fits one L2
    assert wanted(box_etoe(60, 40, seed=9), 2) == 1      # shuffled: the mean-distance rule
    assert wanted(box_etoe(61, 39), 4) == 0              # larger than L2, but every neighbour within 121 slots
    # a box wide enough that a third of the faces lie 799 > 742 slots (1 MiB at N = 4) apart, 11 MB per stage
    assert wanted(box_etoe(400, 10), 4) == 1
    assert wanted(box_etoe(400, 10), 1) == 0             # 3 MB per stage at N = 1
    assert lib.bdg_element_order_wanted(None, 10, 4) == -1


def test_decision_rule_fires_on_the_headline_mesh():
    """The 1000x500-cell box in natural order at N = 4: a third of its faces lie 1999 slots apart, 742 make 1 MiB."""
    etoe = box_etoe(1000, 500)
    far, _ = locality(etoe, np.arange(etoe.shape[0]), far=742)
    assert abs(far - 1 / 3) < 0.01
    assert wanted(etoe, 4) == 1
    assert wanted(etoe, 4) == wanted(etoe, 3) == 1 and wanted(box_etoe(60, 40), 4) == 0
    assert wanted(etoe, 5) == wanted(etoe, 8) == 0  # the far-neighbour rule is for the N <= 4 kernels only
