"""The assumption the face-link gather of the unrolled LSERK kernel rests on (FaceLink, sw2d_kernels.hpp): every face of
every straight-element table is either a boundary face (vmapP == vmapM) or a neighbour element's face f' whose Fmask
row pairs node for node, forward or reversed, so that one (k', f', reversed) entry reproduces the face's Nfp gather
offsets. Wall flags (mapW) cover whole faces. The solver checks every face again when it is created and keeps the
vmapP gather if one does not fit; these fixtures are meshes it must accept. Runs without a GPU."""
import glob
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fmask(order):
    """Face-node table of the warp & blend lattice (Elem<N>::fmask): face 0 s = -1, face 1 r + s = 0, face 2 r = -1."""
    row = lambda j: j * (order + 1) - j * (j - 1) // 2  # noqa: E731
    n = np.arange(order + 1)
    return np.stack([n, np.array([row(i) + order - i for i in n]), np.array([row(i) for i in n])])


def face_links(vmapP, order):
    """(K, 3) link codes f' | reversed << 2 (first fitting code; -1 where none fits) and the (K, 3) neighbour elements."""
    nfp, np_ = order + 1, (order + 1) * (order + 2) // 2
    faces = np.asarray(vmapP).reshape(-1, 3, nfp)
    k2 = faces[:, :, 0] // np_
    fm = fmask(order)
    code = np.full(k2.shape, -1)
    for rev in (0, 1):
        for f2 in range(3):
            nodes = fm[f2][::-1] if rev else fm[f2]
            fits = np.all(faces == nodes[None, None, :] + np_ * k2[:, :, None], axis=2)
            code = np.where((code < 0) & fits, f2 | (rev << 2), code)
    return code, k2


def fixtures():
    out = []
    for f in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        with np.load(f) as d:
            if "vmapP" in d.files and "order" in d.files and "vmapM" in d.files:
                order = int(d["order"])
                if d["vmapP"].size % (3 * (order + 1)) == 0:
                    out.append(os.path.basename(f))
    return out


CASES = [c for c in fixtures() if not c.startswith("advec1d")]   # (1-D: two end points per element, no faces to link)


def test_every_two_dimensional_fixture_with_vmapP_is_covered():
    assert len(CASES) >= 30
    assert "curved_helpers_channel32x6_N4.npz" in CASES and "sw2d_rhs_box6x5_shuffled_N4.npz" in CASES


@pytest.mark.parametrize("case", CASES)
def test_every_face_is_a_boundary_face_or_a_neighbour_face_in_fmask_order(case):
    d = np.load(os.path.join(GOLDEN, case))
    order = int(d["order"])
    nfp = order + 1
    if "Fmask" in d.files:   # the lattice's own table, where the fixture carries it
        assert np.array_equal(np.asarray(d["Fmask"]).reshape(nfp, 3).T, fmask(order))
    code, k2 = face_links(d["vmapP"], order)
    assert (code >= 0).all(), f"faces that fit no link: {np.argwhere(code < 0)[:5].tolist()}"
    # a face that links to its own element and face is exactly a boundary face (vmapP == vmapM there)
    K = code.shape[0]
    own = (k2 == np.arange(K)[:, None]) & (code == np.arange(3)[None, :])
    boundary = np.all(np.asarray(d["vmapP"]).reshape(K, 3, nfp) == np.asarray(d["vmapM"]).reshape(K, 3, nfp), axis=2)
    assert np.array_equal(own, boundary)
    assert boundary.any() and (~boundary).any()
    if "mapW" in d.files and d["mapW"].size:
        wall = np.zeros(3 * nfp * K, bool)
        wall[np.asarray(d["mapW"])] = True
        per_face = wall.reshape(K, 3, nfp)
        assert np.array_equal(per_face.all(axis=2), per_face.any(axis=2)), "a wall flag covers part of a face"
        assert not (per_face.any(axis=2) & ~boundary).any(), "a wall face with a neighbour"


def test_a_periodic_map_is_what_the_solver_must_refuse():
    """The curved helper channel's periodic map pairs the two ends of the channel, whose nodes do not meet in Fmask
    order: the rule does not hold there, and the solver's check at creation keeps such a mesh on the vmapP gather."""
    d = np.load(os.path.join(GOLDEN, "curved_helpers_channel32x6_N4.npz"))
    code, _ = face_links(d["vmapP_periodic"], int(d["order"]))
    assert (code < 0).any()
    code, _ = face_links(d["vmapP"], int(d["order"]))
    assert (code >= 0).all()
