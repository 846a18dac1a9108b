"""Point-block Jacobi (smoother="pbjacobi") on the CPU oracle: the portable forms of the four CEED_EXTERN_OPTIONAL entry points -- the
3 x 3 nodal blocks from the element matrices of AssembledLevel, NumPy for the block algebra -- the solver option, its refusals, and the
header / export check of the new names."""
import os
import re
import sys

import numpy as np
import pytest

from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mesh import box_mesh, hollow_cylinder_mesh
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG
from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _newton_tolerance import straddling_snes_rtol  # noqa: E402
from _pointblock_common import blocks_of_dense, check_block_algebra, dense_jacobian, jittered_box, problem_with_state  # noqa: E402

PHYSICS = ["linElas", "hyperSS", "hyperFS"]
CLAMP = {998: dict(translate=(0.0, -0.05, 0.1)), 999: dict()}
NAMES = ["CeedOperatorLinearAssemblePointBlockDiagonal", "CeedXVectorPointBlockInvert", "CeedXVectorPointBlockMult",
         "CeedXVectorChebyshevStepPointBlock"]


# ---------------------------------------------------------------- 1. the portable blocks
@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("model", PHYSICS)
def test_portable_blocks_on_the_oracle(oracle, oracle_lib, model, degree):
    assert not oracle_lib.has("CeedOperatorLinearAssemblePointBlockDiagonal")
    p = problem_with_state(oracle, jittered_box(), degree, model)
    lv, n = p.fine, p.lsize()
    B, D = oracle.vector(3 * n).set_value(3.0), oracle.vector(n)
    p.get_pointblock_diag(lv, B)
    p.get_diag(lv, D)
    blocks, diag = B.to_numpy().reshape(-1, 3, 3), D.to_numpy().reshape(-1, 3)
    scale = np.abs(blocks).max()
    d_err = np.abs(blocks[:, [0, 1, 2], [0, 1, 2]] - diag).max() / scale
    want = blocks_of_dense(dense_jacobian(p, lv))
    b_err = np.abs(blocks - want).max() / scale
    print(f"{model} p={degree}: block diagonal vs get_diag {d_err:.2e}; blocks vs dense Jacobian {b_err:.2e}; "
          f"asymmetry {np.abs(blocks - blocks.transpose(0, 2, 1)).max() / scale:.2e}")
    assert d_err <= 1e-12
    assert b_err <= 1e-12
    m = p.levels[lv].mask.reshape(-1, 3) != 0
    assert m.any() and not m.all()
    dead = m[:, :, None] | m[:, None, :]
    assert np.all(blocks[dead] == 0.0) and not np.any(B.to_numpy() == 3.0)      # overwritten everywhere (prefilled with 3)
    assert np.all(blocks[:, [0, 1, 2], [0, 1, 2]][~m] > 0.0)
    p.destroy()


def test_portable_blocks_follow_the_context_of_the_level(oracle):
    """The smoother-nu swap of GetDiag_Ceed: the blocks are built with the context the level's Jacobian has at the call."""
    p = problem_with_state(oracle, jittered_box(), 1, "linElas", nu=0.3)
    q = problem_with_state(oracle, jittered_box(), 1, "linElas", nu=0.45)
    n = p.lsize()
    B, Bq = oracle.vector(3 * n), oracle.vector(3 * n)
    p.levels[p.fine].qfJacob.set_context(np.array([0.45, 1.0]), reported_size=8)
    p.get_pointblock_diag(p.fine, B)
    q.get_pointblock_diag(q.fine, Bq)
    assert np.abs(B.to_numpy() - Bq.to_numpy()).max() <= 1e-14 * np.abs(Bq.to_numpy()).max()
    p.levels[p.fine].qfJacob.set_context(p.phys, reported_size=8)
    p.get_pointblock_diag(p.fine, B)
    assert np.abs(B.to_numpy() - Bq.to_numpy()).max() > 1e-3 * np.abs(Bq.to_numpy()).max()
    p.destroy(); q.destroy()


# ---------------------------------------------------------------- 2. invert, multiply, step
@pytest.mark.parametrize("nnodes", [1, 8, 65])
def test_portable_invert_multiply_and_step(oracle, oracle_lib, nnodes):
    assert not any(oracle_lib.has(s) for s in NAMES)
    check_block_algebra(oracle, nnodes, 1e-13)


# ---------------------------------------------------------------- 3. the solver
def test_pbjacobi_solve_reaches_the_jacobi_solution_on_the_oracle(oracle):
    """Only the smoother differs: the converged displacement is the same to what the Newton tolerance leaves open -- the distance of two
    "jacobi" solves at snes_rtol and snes_rtol / 10 (x 10), snes_rtol straddling one residual of the recorded history."""
    mesh = hollow_cylinder_mesh(1, 6, 2, z0=-1.0, z1=1.0)

    def solve(smoother, snes_rtol):
        p = SolidProblem(oracle, mesh, 2, "hyperFS", nu=0.3, E=10.0, bc_sides=[998, 999])
        s = NewtonPMG(p, clamp=CLAMP, snes_rtol=snes_rtol, smoother=smoother)
        assert s.smoother == smoother and ("pb" in s.w[0]) == (smoother == "pbjacobi")
        st = s.solve(2)
        u = s.U.to_numpy()
        p.destroy()
        return st, u
    rtol = straddling_snes_rtol(solve("jacobi", 1e-8)[0])
    st_j, u_j = solve("jacobi", rtol)
    st_t, u_t = solve("jacobi", rtol / 10)
    st_b, u_b = solve("pbjacobi", rtol)
    assert st_j.converged and st_t.converged and st_b.converged and st_b.increments == 2
    allowed = 10.0 * np.linalg.norm(u_j - u_t)
    assert st_t.newton_its > st_j.newton_its and allowed > 0.0
    diff = np.linalg.norm(u_b - u_j)
    print(f"snes_rtol {rtol:.2e}; Newton jacobi {st_j.newton_its} pbjacobi {st_b.newton_its}; Krylov jacobi {st_j.ksp_its} pbjacobi {st_b.ksp_its}; "
          f"|u_pb - u_j| = {diff:.3e}, allowed {allowed:.3e} (|u| = {np.linalg.norm(u_j):.3e})")
    assert diff <= allowed
    assert st_b.newton_its == st_j.newton_its


def test_smoother_refusals(oracle):
    p = SolidProblem(oracle, box_mesh(2, 1, 1), 2, "linElas", nu=0.3, E=1.0, bc_sides=[6])

    class TwoRanks:
        world = 2
    with pytest.raises(ValueError, match="halo"):
        NewtonPMG(p, halo=[TwoRanks()] * len(p.levels), smoother="pbjacobi")
    with pytest.raises(ValueError, match="halo"):
        NewtonPMG(p, halo=TwoRanks(), smoother="pbjacobi")
    with pytest.raises(ValueError, match="smoother"):
        NewtonPMG(p, smoother="sor")
    assert NewtonPMG(p).smoother == "jacobi"
    p.destroy()


# ---------------------------------------------------------------- 4. header and exports
def test_header_declares_the_entry_points_optional_and_the_product_exports_them(oracle_lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ceed.h")).read(), flags=re.S)
    optional = re.findall(r"CEED_EXTERN_OPTIONAL\s+int\s+(Ceed[A-Za-z0-9_]+)\s*\(", txt)
    required = re.findall(r"CEED_EXTERN\s+int\s+(Ceed[A-Za-z0-9_]+)\s*\(", txt)
    for s in NAMES:
        assert s in optional and s not in required and s in cd.CeedLib.OPTIONAL and s not in cd.CeedLib.FUNCTIONS
    assert not oracle_lib.missing_symbols(optional=False)          # the oracle needs none of them
    if not os.path.exists(cd.PRODUCT_LIB):
        pytest.fail("product library not built: run __graft_entry__.build()")
    lib = cd.CeedLib(cd.PRODUCT_LIB)
    assert not [s for s in NAMES if not lib.has(s)]
    assert not lib.missing_symbols()
