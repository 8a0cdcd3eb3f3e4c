#!/usr/bin/env python3
"""Generates the high-order quadrilateral fixtures under tests/golden/. Run in the BUILD container only (needs the
reference checkout, as make_golden_quads.py and make_golden_quads4.py, whose case builders it calls); what it writes is
plain data.

  python tests/golden/make_golden_quads_high_order.py

Writes, on coarse_box_quads.msh (the smallest quadrangle mesh here) at N = 10, with this repository's tables,
  sw2dq_rhs_coarse_box_quads_N10.npz    the reference script's sw2dComputeRHS (sw2dquads.py:24-133), three fields
  sw2dq_rhs4_coarse_box_quads_N10.npz   the reference's swhelpers.rhs.sw2dComputeRHS (rhs.py:178-311), four fields with
                                        tracer, Coriolis array, drag and bed slope
in the format of the other sw2dq_rhs_* / sw2dq_rhs4_* fixtures: mesh, order, state, parameters and RHS; the tables are
rebuilt by QuadNodesProvisioner when a test loads them.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden_quads  # noqa: E402
import make_golden_quads4  # noqa: E402

ORDER = 10


def main():
    _, E, V = make_golden_quads.mesh_tables(path=os.path.join(HERE, "coarse_box_quads.msh"))
    make_golden_quads.case(f"coarse_box_quads_N{ORDER}", ORDER, E, V, seed=ORDER)
    make_golden_quads4.case(f"coarse_box_quads_N{ORDER}", ORDER, E, V, seed=ORDER)


if __name__ == "__main__":
    main()
