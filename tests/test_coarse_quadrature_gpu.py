"""coarse_quadrature="own" on the MI355X: the state kernel (CeedXOperatorApplyState, k_state_at_points) against the oracle's portable
form, the own-quadrature level operators against the oracle, and config 3 solved with the option."""
import os

import numpy as np
import pytest

from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.assembly import AssembledLevel
from ceedpetscsolid_amd.mesh import box_mesh, hollow_cylinder_mesh, load_mesh_npz, scramble_mesh
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG
from conftest import GOLDEN, rel_err
from _newton_tolerance import straddling_snes_rtol

pytestmark = pytest.mark.gpu

PAIRS = [(5, 2), (5, 3), (4, 2), (4, 3), (7, 3), (7, 5), (5, 4)]
CLAMP = {998: dict(translate=(0.0, -0.05, 0.1)), 999: dict()}


def meshes(name):
    if name == "cylinder":
        return hollow_cylinder_mesh(2, 8, 3, z0=-1.0, z1=1.0), [998]
    if name == "scrambled box":
        m = box_mesh(3, 3, 2)
        m.coords += 0.04 / 3 * np.random.default_rng(1).uniform(-1, 1, m.coords.shape)
        return scramble_mesh(m, seed=3, order=True, orient=True), [1]
    nx = {"one element": 1, "three elements": 3}[name]          # fewer elements than a workgroup packs / not a multiple of the pack
    return box_mesh(nx, 1, 1), []


def state_operator(p, Qc):
    """The residual operator of `p` (built with multigrid="none": its one level is the fine one) once more on the basis (P_fine, Qc),
    with q-data and a state vector of its own on those points -- what SolidProblem builds for an own-quadrature level."""
    c, ne, nq, fine = p.ceed, p.mesh.nelem, Qc ** 3, p.levels[p.fine]
    rq, rg = c.strided_restriction(ne, nq, 10, 10 * ne * nq), c.strided_restriction(ne, nq, 9, 9 * ne * nq)
    qd, gu = c.vector(10 * ne * nq), c.vector(9 * ne * nq)
    gu.set_value(-7.0)
    p._setup_geo(c.basis_lagrange(3, 3, 2, Qc, cd.GAUSS), rq, qd)
    bs = c.basis_lagrange(3, 3, fine.degree + 1, Qc, cd.GAUSS)
    op = c.operator(p.qfApply)
    op.set_field("du", fine.Erestrictu, bs, "active")
    op.set_field("qdata", rq, None, qd)
    op.set_field("dv", fine.Erestrictu, bs, "active")
    op.set_field("gradu", rg, bs, gu)
    p._set_mask(op, fine.mask, mode=2)
    return op, gu


def state_both(oracle, gpu, mesh, bc, problem, Pf, Qc):
    out = []
    for c in (oracle, gpu):
        p = SolidProblem(c, mesh, Pf - 1, problem, nu=0.3, E=1.0, bc_sides=bc, multigrid="none")
        op, gu = state_operator(p, Qc)
        n = p.lsize()
        X = c.vector(n).set_array(p.smooth_state(0.1))
        if c is gpu:
            op.apply_state(X)
            assert op.kernel_name == f"state<Pf={Pf},Qc={Qc}>", op.kernel_name
        else:
            op.apply(X, c.vector(n))          # the portable form: the whole operator, its active output discarded
        out.append(gu.to_numpy())
    return out


@pytest.mark.parametrize("Pf,Qc", PAIRS)
@pytest.mark.parametrize("problem", ["hyperSS", "hyperFS"])
@pytest.mark.parametrize("meshname", ["cylinder", "scrambled box"])
def test_state_kernel_matches_the_oracles_portable_form(oracle, gpu, meshname, problem, Pf, Qc):
    mesh, bc = meshes(meshname)
    want, got = state_both(oracle, gpu, mesh, bc, problem, Pf, Qc)
    err = rel_err(got, want)
    print(f"{meshname} {problem} state<Pf={Pf},Qc={Qc}>: {err:.2e}")
    assert err <= 1e-10


@pytest.mark.parametrize("Pf,Qc", [(5, 2), (5, 3), (7, 5), (4, 3), (5, 6), (3, 4)])      # the last two: Q_c > P_f (qextra)
@pytest.mark.parametrize("meshname", ["one element", "three elements"])
def test_state_kernel_at_its_edge_shapes(oracle, gpu, meshname, Pf, Qc):
    mesh, bc = meshes(meshname)
    want, got = state_both(oracle, gpu, mesh, bc, "hyperFS", Pf, Qc)
    assert got.size == 9 * mesh.nelem * Qc ** 3 and not np.any(got == -7.0)         # every entry written
    err = rel_err(got, want)
    print(f"{meshname} state<Pf={Pf},Qc={Qc}>: {err:.2e}")
    assert err <= 1e-10


def test_state_kernel_refuses_what_it_is_not_for(gpu):
    p = SolidProblem(gpu, box_mesh(2, 2, 2), 4, "hyperFS", nu=0.3, E=1.0, bc_sides=[1], coarse_quadrature="own")
    X = gpu.vector(p.lsize()).set_array(p.smooth_state(0.1))
    with pytest.raises(cd.CeedError, match="residual operators"):
        p.levels[0].opJacob.apply_state(X)
    short = gpu.vector(10).set_value(0.0)
    with pytest.raises(cd.CeedError, match="shorter"):
        p.levels[0].opState.apply_state(short)
    with pytest.raises(cd.CeedError, match="more nodes than points"):     # the whole residual on (P_f, Q_c < P_f): refused, no fallback
        p.levels[0].opState.apply(X, gpu.vector(p.lsize()))
    p.destroy()


def test_state_kernel_touches_nothing_but_the_level_state(gpu):
    mesh, bc = meshes("cylinder")
    p = SolidProblem(gpu, mesh, 4, "hyperFS", nu=0.3, E=1.0, bc_sides=bc, coarse_quadrature="own")
    n = p.lsize()
    X, Y = gpu.vector(n).set_array(p.smooth_state(0.1)), gpu.vector(n)
    p.form_residual(X, Y)
    y0, g0, x0 = Y.to_numpy(), p.gradu.to_numpy(), X.to_numpy()
    lv0 = [lv.gradu.to_numpy() for lv in p.levels[:-1]]
    X2 = gpu.vector(n).set_array(p.smooth_state(0.05))
    for lv in p.levels[:-1]:
        lv.opState.apply_state(X2)
    assert np.array_equal(Y.to_numpy(), y0) and np.array_equal(p.gradu.to_numpy(), g0) and np.array_equal(X.to_numpy(), x0)
    for lv, old in zip(p.levels[:-1], lv0):
        new = lv.gradu.to_numpy()
        assert not np.array_equal(new, old) and rel_err(new, 0.5 * old) < 0.2        # half the amplitude: about half the gradient
    p.destroy()


@pytest.mark.parametrize("problem", ["hyperSS", "hyperFS"])
@pytest.mark.parametrize("meshname,qextra", [("cylinder", 0), ("scrambled box", 0), ("cylinder", 1)])
def test_own_quadrature_levels_match_the_oracle(oracle, gpu, meshname, qextra, problem):
    mesh, bc = meshes(meshname)
    res = []
    for c in (oracle, gpu):
        p = SolidProblem(c, mesh, 4, problem, nu=0.3, E=2.0, bc_sides=bc, qextra=qextra, coarse_quadrature="own")
        assert [lv.Q for lv in p.levels] == [2 + qextra, 3 + qextra, 5 + qextra]
        n = p.lsize()
        X, R = c.vector(n).set_array(p.smooth_state(0.1)), c.vector(n)
        p.form_residual(X, R)
        out = {"residual": R.to_numpy()}
        for lv in range(len(p.levels)):
            nl = p.lsize(lv)
            x = np.random.default_rng(lv).uniform(-1, 1, nl)
            Xl, Yl, D = c.vector(nl).set_array(x), c.vector(nl), c.vector(nl)
            p.apply_jacobian(lv, Xl, Yl); p.get_diag(lv, D)
            out[f"state{lv}"], out[f"jacobian{lv}"], out[f"diag{lv}"] = p.levels[lv].gradu.to_numpy(), Yl.to_numpy(), D.to_numpy()
            if lv < p.fine:
                A = AssembledLevel(p, lv); A.assemble()
                Ya = c.vector(nl); A.apply(Xl, Ya)
                out[f"assembled{lv}"] = Ya.to_numpy()
                free = p.levels[lv].mask == 0
                assert rel_err(Ya.to_numpy()[free], Yl.to_numpy()[free]) < 1e-12
                A.destroy()
        if c is gpu:
            assert [p.levels[lv].opJacob.kernel_name.split("/")[0] for lv in (0, 1)] == \
                [f"fused_grad<P=2,Q={2 + qextra},{p.info['jacob']}>", f"fused_grad<P=3,Q={3 + qextra},{p.info['jacob']}>"]
            assert [lv.opState.kernel_name for lv in p.levels[:-1]] == [f"state<Pf=5,Qc={2 + qextra}>", f"state<Pf=5,Qc={3 + qextra}>"]
        res.append(out)
        p.destroy()
    for k in res[0]:
        err = rel_err(res[1][k], res[0][k])
        print(f"{meshname} qextra={qextra} {problem} {k}: {err:.2e}")
        assert err <= 1e-10, (k, err)


# snes_rtol of the comparison: derived from the fine-quadrature run's own Newton history, as in test_coarse_quadrature.py
# (_newton_tolerance.py): at the default 1e-8 both fine solves stop at the same iterate and the yardstick is zero.


def test_config3_solve_with_own_quadrature(gpu):
    """BASELINE config 3 (hyperSS, the reference's 5 580-hex cylinder, p = 4, 10 load increments) with the option: converges in the Newton
    steps of the fine-quadrature run to the same displacement, as far as the Newton tolerance decides it."""
    mesh = load_mesh_npz(os.path.join(GOLDEN, "mesh_cylinder8_5580e_4ss_us.npz"))

    def solve(mode, snes_rtol):
        p = SolidProblem(gpu, mesh, 4, "hyperSS", nu=0.3, E=1e3, bc_sides=[998, 999], coarse_quadrature=mode)
        s = NewtonPMG(p, clamp=CLAMP, coarse="amg", graph=True, snes_rtol=snes_rtol)
        st = s.solve(10)
        u = s.U.to_numpy()
        p.destroy()
        return st, u, np.abs(u.reshape(-1, 3)).max(axis=0)
    rtol = straddling_snes_rtol(solve("fine", 1e-8)[0])
    st_f, u_f, m_f = solve("fine", rtol)
    st_t, u_t, m_t = solve("fine", rtol / 10)
    st_o, u_o, m_o = solve("own", rtol)
    print(f"config 3: snes_rtol {rtol:.2e}; Newton fine {st_f.newton_its} (tight {st_t.newton_its}) own {st_o.newton_its}; Krylov fine {st_f.ksp_its} own {st_o.ksp_its}; "
          f"solve seconds fine {st_f.seconds:.2f} own {st_o.seconds:.2f}")
    print(f"max |u| fine {m_f} own {m_o}; |max_own - max_fine| {np.abs(m_o - m_f)} allowed {10 * np.abs(m_f - m_t)}; "
          f"|u_own - u_fine| {np.linalg.norm(u_o - u_f):.3e} allowed {10 * np.linalg.norm(u_f - u_t):.3e}")
    assert st_f.converged and st_t.converged and st_o.converged and st_o.increments == 10
    assert st_t.newton_its > st_f.newton_its                       # the tolerance is what ends the solves (straddling_snes_rtol)
    assert st_o.newton_its == st_f.newton_its
    assert np.linalg.norm(m_o - m_f) <= 10.0 * np.linalg.norm(m_f - m_t)
    assert np.linalg.norm(u_o - u_f) <= 10.0 * np.linalg.norm(u_f - u_t)


def test_config3_own_quadrature_vcycle_graph_replays_the_eager_bits(gpu):
    """The recorded V-cycle over own-quadrature levels: the same bits as the eager one; and after ANOTHER residual evaluation -- the state
    kernel is then the new writer of the levels' gradu -- the recording is not stale (it reads the arrays, no provenance buffer) and
    replays the eager V-cycle on the NEW state, as today's rule demands of a graph recorded before a residual evaluation."""
    mesh = load_mesh_npz(os.path.join(GOLDEN, "mesh_cylinder8_5580e_4ss_us.npz"))
    p = SolidProblem(gpu, mesh, 4, "hyperSS", nu=0.3, E=1e3, bc_sides=[998, 999], coarse_quadrature="own")
    s = NewtonPMG(p, clamp=CLAMP, coarse="amg", graph=True)
    s.U.set_value(0.0); s._set(s.bcv, s.bc_values(0.1)); s.residual(s.U, s.R)
    s.setup_preconditioner()
    top = s.nlev - 1
    r, z, z2 = s.w[top]["b"], s.kz, s._vec(p.lsize(), top)
    rng = np.random.default_rng(4)
    s._set(r, rng.uniform(-1, 1, p.lsize()) * (p.levels[top].mask == 0))
    s.vcycle(top, r, z2)
    want = z2.to_numpy().copy()
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    s.record_preconditioner(r, z)
    assert s._pc_graph is not None
    z.set_value(3.0); s.precondition(r, z)
    assert np.array_equal(z.to_numpy(), want)
    # a residual evaluation at another state: fine gradu by the residual kernel, the levels' by the state kernel
    before = [lv.gradu.to_numpy() for lv in p.levels]
    s._set(s.U, 0.5 * p.smooth_state(0.02) * (p.levels[top].mask == 0)); s.residual(s.U, s.R)
    assert all(not np.array_equal(lv.gradu.to_numpy(), b) for lv, b in zip(p.levels, before))
    assert s._pc_graph.stale() == 0
    s.vcycle(top, r, z2)
    want2 = z2.to_numpy().copy()
    assert not np.array_equal(want2, want)
    z.set_value(3.0); s.precondition(r, z)
    assert s._pc_graph is not None                                   # not dropped: replayed
    assert np.array_equal(z.to_numpy(), want2)
    p.destroy()
