"""Point-block Jacobi on the device: k_pbdiag_sf against the oracle's blocks (the 3 x 3 diagonal blocks of the element matrices that
AssembledLevel builds from the ORACLE's Jacobian applies), the block kernels against NumPy, a smoothing sweep against the same
recurrence in NumPy on the oracle's dense matrix, and config 3 with smoother="pbjacobi"."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.krylov import chebyshev_coefficients
from ceedpetscsolid_amd.mesh import load_mesh_npz
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG
from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _newton_tolerance import straddling_snes_rtol  # noqa: E402
from _plain_kernels import STREAM_ITEMS, lap_sizes  # noqa: E402
from _pointblock_common import check_block_algebra, dense_jacobian, embedded_inverse, blocks_of_dense, jittered_box, level_problem, problem_with_state  # noqa: E402

pytestmark = pytest.mark.gpu

CLAMP = {998: dict(translate=(0.0, -0.05, 0.1)), 999: dict()}
KERNEL_QF = {"linElas": "LinElas", "hyperSS": "HyperSSdF", "hyperFS": "HyperFSdF"}
# (P, Q): plain, P < Q, qextra, and the full LDS slab of Q = 8 (147 KB: the dynamic-shared-memory attribute)
PQ = [(2, 2), (3, 3), (2, 5), (3, 5), (5, 5), (4, 6), (7, 7), (2, 8), (8, 8)]


def oracle_blocks(oracle, mesh, P, Q, model, nu=0.3, bc_sides=(6,)):
    p, lv = level_problem(oracle, mesh, P, Q, model, nu=nu, bc_sides=bc_sides)
    B = oracle.vector(3 * p.lsize(lv))
    assert not oracle.L.has("CeedOperatorLinearAssemblePointBlockDiagonal")     # the portable form: AssembledLevel on the oracle
    p.get_pointblock_diag(lv, B)
    out = B.to_numpy().reshape(-1, 3, 3)
    B.destroy(); p.destroy()
    return out


def device_blocks_match(oracle, gpu, mesh, P, Q, model, bc_sides=(6,)):
    want = oracle_blocks(oracle, mesh, P, Q, model, bc_sides=bc_sides)
    p, lv = level_problem(gpu, mesh, P, Q, model, bc_sides=bc_sides)
    n = p.lsize(lv)
    B, D = gpu.vector(3 * n).set_value(3.0), gpu.vector(n)          # prefilled: overwrite semantics
    p.get_pointblock_diag(lv, B)
    assert p.levels[lv].opJacob.kernel_name == f"pbdiag<P={P},Q={Q},{KERNEL_QF[model]}>"
    p.get_diag(lv, D)
    got, diag = B.to_numpy().reshape(-1, 3, 3), D.to_numpy().reshape(-1, 3)
    scale = np.abs(want).max()
    err = np.abs(got - want).max() / scale
    d_err = np.abs(got[:, [0, 1, 2], [0, 1, 2]] - diag).max() / scale
    print(f"{model} (P,Q)=({P},{Q}) {mesh.nelem} elements: pbdiag vs oracle blocks {err:.2e}; its diagonal vs the device diagonal {d_err:.2e}; "
          f"asymmetry {np.abs(got - got.transpose(0, 2, 1)).max() / scale:.2e}")
    assert err <= 1e-10
    assert d_err <= 1e-12
    m = p.levels[lv].mask.reshape(-1, 3) != 0
    assert m.any() and np.all(got[m[:, :, None] | m[:, None, :]] == 0.0)     # constrained rows and columns: exactly zero
    p.destroy()


# the unstructured 672-hex cylinder at degree 2: rows of 3 and 6 contributors beside 1, 2, 4 and 8 (the boxes have only those)
CYL672 = os.path.join(GOLDEN, "mesh_cylinder8_672e_4ss_us.npz")


@pytest.mark.parametrize("model", ["linElas", "hyperSS", "hyperFS"])
@pytest.mark.parametrize("P,Q,fixture", [(P, Q, None) for P, Q in PQ] + [(3, 3, CYL672)], ids=[f"{P}-{Q}" for P, Q in PQ] + ["cyl672-3-3"])
def test_pbdiag_matches_the_oracle_blocks(oracle, gpu, P, Q, fixture, model):
    if fixture:
        device_blocks_match(oracle, gpu, load_mesh_npz(fixture), P, Q, model, bc_sides=(998,))
    else:
        device_blocks_match(oracle, gpu, jittered_box(2), P, Q, model)


@pytest.mark.parametrize("model", ["linElas", "hyperFS"])
def test_pbdiag_on_a_single_element(oracle, gpu, model):
    """Fewer elements than anything packs together: one workgroup, every node with one contributor."""
    device_blocks_match(oracle, gpu, jittered_box(1), 3, 4, model)


def test_pbdiag_overwrites_a_longer_vector(gpu):
    p = problem_with_state(gpu, jittered_box(2), 2, "linElas")
    n = p.lsize()
    B, B2 = gpu.vector(3 * n + 18).set_value(3.0), gpu.vector(3 * n).set_value(0.0)
    p.get_pointblock_diag(p.fine, B); p.get_pointblock_diag(p.fine, B2)
    b = B.to_numpy()
    assert np.array_equal(b[:3 * n], B2.to_numpy()) and not b[3 * n:].any() and np.abs(b).max() > 0
    p.get_pointblock_diag(p.fine, B)                                         # and again over its own output: the same bits
    assert np.array_equal(B.to_numpy(), b)
    p.destroy()


def test_pbdiag_reads_the_context_at_call_time(oracle, gpu):
    """The -nu_smoother swap of GetDiag_Ceed (matops.c:215-232): after set_context to another nu the blocks are the oracle's for that nu."""
    mesh = jittered_box(2)
    want = oracle_blocks(oracle, mesh, 3, 3, "hyperFS", nu=0.45)
    other = oracle_blocks(oracle, mesh, 3, 3, "hyperFS", nu=0.3)
    p = problem_with_state(gpu, mesh, 2, "hyperFS", nu=0.3)
    B = gpu.vector(3 * p.lsize())
    # the stored state does not depend on the material; the oracle problem above stored the same one
    p.levels[p.fine].qfJacob.set_context(np.array([0.45, 1.0]), reported_size=8)
    p.get_pointblock_diag(p.fine, B)
    got = B.to_numpy().reshape(-1, 3, 3)
    scale = np.abs(want).max()
    print(f"smoother nu: {np.abs(got - want).max() / scale:.2e} (the nu = 0.3 blocks are {np.abs(other - want).max() / scale:.2e} away)")
    assert np.abs(got - want).max() <= 1e-10 * scale and np.abs(other - want).max() > 1e-2 * scale
    p.levels[p.fine].qfJacob.set_context(p.phys, reported_size=8)
    p.get_pointblock_diag(p.fine, B)
    assert np.abs(B.to_numpy().reshape(-1, 3, 3) - other).max() <= 1e-10 * scale
    p.destroy()


def test_pbdiag_refusals(gpu):
    p = problem_with_state(gpu, jittered_box(2), 2, "hyperSS")
    n, L = p.lsize(), gpu.L
    B = gpu.vector(3 * n)
    with pytest.raises(cd.CeedError, match="Jacobian"):
        p.opApply.assemble_pointblock_diagonal(B)                            # the residual operator
    with pytest.raises(cd.CeedError, match="too short"):
        p.levels[p.fine].opJacob.assemble_pointblock_diagonal(gpu.vector(3 * n - 1))
    with pytest.raises(cd.CeedError, match="too short"):
        p.get_pointblock_diag(p.fine, gpu.vector(n))
    comp = C.c_void_p()
    L.chk(L.lib.CeedCompositeOperatorCreate(gpu.h, C.byref(comp)))
    L.chk(L.lib.CeedCompositeOperatorAddSub(comp, p.levels[p.fine].opJacob.h))
    rc = L.lib.CeedOperatorLinearAssemblePointBlockDiagonal(comp, B.h, C.c_void_p(L.REQUEST_IMMEDIATE))
    assert rc != 0 and b"composite" in L.lib.CeedXLastError()
    L.lib.CeedOperatorDestroy(C.byref(comp))
    p.destroy()


# the last four: around one grid of the lane-per-node kernels (launch_stream: 2048 x 256 nodes) and two laps and three nodes
BLOCK_NODES = [1, 63, 64, 65, 257] + lap_sizes(STREAM_ITEMS)


def bad_block_sets(nnodes, G=STREAM_ITEMS):
    """Where the blocks that are not positive definite are planted: the first and the last node; past one grid also nodes of the SECOND
    lap alone, and nodes n, n + G (, n + 2 G) of ONE lane, whose count k_pb_invert carries from lap to lap into one atomic per wave."""
    sets = [sorted({0, nnodes - 1})]
    if nnodes > G:
        sets.append(sorted({G, nnodes - 1, G + (nnodes - G) // 2}))
        sets.append([n for n in (0, G, 2 * G, 70, 70 + G) if n < nnodes])
    return sets


@pytest.mark.parametrize("nnodes", BLOCK_NODES)
def test_block_kernels_against_numpy(gpu, product_lib, nnodes):
    assert all(product_lib.has(s) for s in ("CeedXVectorPointBlockInvert", "CeedXVectorPointBlockMult", "CeedXVectorChebyshevStepPointBlock"))
    check_block_algebra(gpu, nnodes, 1e-13, bad_sets=bad_block_sets(nnodes))


def sweep_setup(ceed, graph=False):
    """A p = 2 hyperFS problem on the two-element mesh at a smooth state, its solver with the block smoother, preconditioner set up."""
    p = SolidProblem(ceed, jittered_box(2), 2, "hyperFS", nu=0.3, E=1.0, bc_sides=[6])
    s = NewtonPMG(p, clamp={6: dict()}, smoother="pbjacobi", coarse="chebyshev", coarse_cheb_its=8, coarse_cheb_ratio=20.0, graph=graph)
    free = p.levels[p.fine].mask == 0
    s._set(s.U, p.smooth_state(0.1) * free); s._set(s.bcv, np.zeros(p.lsize())); s.residual(s.U, s.R)
    return p, s, free


def test_chebyshev_sweep_with_blocks_against_numpy(oracle, gpu):
    po, so, free = sweep_setup(oracle)
    top = so.nlev - 1
    A = dense_jacobian(po, top)                                               # the oracle's masked Jacobian at the stored state
    Binv = embedded_inverse(blocks_of_dense(A))
    po.destroy()
    p, s, free = sweep_setup(gpu)
    s.setup_preconditioner()
    n = p.lsize()
    b = np.random.default_rng(11).uniform(-1, 1, n) * free
    bv, xv = s.w[top]["b"], s.w[top]["x"]
    s._set(bv, b)
    s.chebyshev(top, bv, xv, 3, True)
    got = xv.to_numpy()
    # the same recurrence (solver.py::chebyshev) with the oracle's matrix, NumPy block inverses and the solver's own emax
    mult = lambda r: np.einsum("nij,nj->ni", Binv, r.reshape(-1, 3)).reshape(-1)
    x = d = np.zeros(n)
    for c1, c2 in chebyshev_coefficients(s.emax[top], 0.1, 3):
        d = c1 * mult(b - A @ x) + c2 * d
        x = x + d
    err = np.abs(got - x).max() / np.abs(x).max()
    print(f"3 Chebyshev steps with blocks, emax {s.emax[top]:.4f}: device vs NumPy recurrence {err:.2e}")
    assert err <= 1e-9 and np.abs(x).max() > 0
    p.destroy()


def test_recorded_vcycle_with_blocks_replays_the_eager_bits(gpu):
    p, s, free = sweep_setup(gpu, graph=True)
    s.setup_preconditioner()
    top = s.nlev - 1
    r, z, z2 = s.w[top]["b"], s.kz, s._vec(p.lsize(), top)
    s._set(r, np.random.default_rng(4).uniform(-1, 1, p.lsize()) * free)
    # the sweep alone, eager
    s.chebyshev(top, r, z2, 3, True)
    sweep = z2.to_numpy().copy()
    s.vcycle(top, r, z2)
    want = z2.to_numpy().copy()
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    s.record_preconditioner(r, z)
    assert s._pc_graph is not None
    z.set_value(3.0); s.precondition(r, z)
    assert np.array_equal(z.to_numpy(), want)
    # and the sweep recorded on its own
    g = gpu.capture(lambda: s.chebyshev(top, r, z2, 3, True))
    z2.set_value(3.0); g.launch()
    assert np.array_equal(z2.to_numpy(), sweep)
    g.destroy()
    p.destroy()


def test_config3_solve_with_pbjacobi(gpu):
    """BASELINE config 3 (hyperSS, the reference's 5 580-hex cylinder, p = 4, 10 load increments) with the block smoother: converges in
    the Newton steps of the "jacobi" run to the same displacement, as far as the Newton tolerance decides it.  Krylov counts and times
    are printed, not asserted: nobody has measured a ratio."""
    mesh = load_mesh_npz(os.path.join(GOLDEN, "mesh_cylinder8_5580e_4ss_us.npz"))

    def solve(smoother, snes_rtol):
        p = SolidProblem(gpu, mesh, 4, "hyperSS", nu=0.3, E=1e3, bc_sides=[998, 999])
        s = NewtonPMG(p, clamp=CLAMP, coarse="amg", graph=True, snes_rtol=snes_rtol, smoother=smoother)
        st = s.solve(10)
        u = s.U.to_numpy()
        p.destroy()
        return st, u, np.abs(u.reshape(-1, 3)).max(axis=0)
    rtol = straddling_snes_rtol(solve("jacobi", 1e-8)[0])
    st_j, u_j, m_j = solve("jacobi", rtol)
    st_t, u_t, m_t = solve("jacobi", rtol / 10)
    st_b, u_b, m_b = solve("pbjacobi", rtol)
    print(f"config 3: snes_rtol {rtol:.2e}; Newton jacobi {st_j.newton_its} (tight {st_t.newton_its}) pbjacobi {st_b.newton_its}; "
          f"Krylov jacobi {st_j.ksp_its} pbjacobi {st_b.ksp_its}; solve seconds jacobi {st_j.seconds:.2f} pbjacobi {st_b.seconds:.2f}")
    print(f"max |u| jacobi {m_j} pbjacobi {m_b}; |max_pb - max_j| {np.abs(m_b - m_j)} allowed {10 * np.abs(m_j - m_t)}; "
          f"|u_pb - u_j| {np.linalg.norm(u_b - u_j):.3e} allowed {10 * np.linalg.norm(u_j - u_t):.3e}")
    assert st_j.converged and st_t.converged and st_b.converged and st_b.increments == 10
    assert st_t.newton_its > st_j.newton_its                       # the tolerance is what ends the solves (straddling_snes_rtol)
    assert st_b.newton_its == st_j.newton_its
    assert np.linalg.norm(m_b - m_j) <= 10.0 * np.linalg.norm(m_j - m_t)
    assert np.linalg.norm(u_b - u_j) <= 10.0 * np.linalg.norm(u_j - u_t)
