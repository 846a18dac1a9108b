"""Spring and dashpot supports on the device (CeedXSupport*, the support modes of k_contact in csrc/kernels_contact.hip) against the
portable NumPy form of support.py.

Bound: 1e-12 relative to the result's max norm -- contact's bound with the same derivation (test_contact_gpu.py: both sides sum O(P^2)
products of O(1) table entries per pass in float64, from two independent table generators that agree to a few ulp); contact measured
1.7e-14 at the most.  The state is compared entry by entry against its largest entry.  The worst value per (P, Q) is printed.

Face counts: 1, FPW - 1, FPW and FPW + 1 with FPW = max(1, 64 / Q^2) the faces of a wave, on a planar side set (the bottom of a row of
elements) and on a curved one (the first faces of a cylinder's inner wall), without a mask and with the mask of a clamped neighbouring
side set, whose rim nodes carry values the force must read and the tangent must not."""
import numpy as np
import pytest

import _numbering as nb
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mesh import box_mesh, build_dofmap, dirichlet_mask, hollow_cylinder_mesh, side_set_nodes
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.support import NSTATE, SupportSurface

pytestmark = pytest.mark.gpu

PQ = [(P, Q) for P in range(2, 9) for Q in range(P, 9)]
TOL = 1e-12
KN, KT = 3.0, 0.75


def test_the_instantiated_pairs():
    assert len(PQ) == 28


def face_counts(Q):
    fpw = max(1, 64 // (Q * Q))
    return sorted({1, fpw - 1, fpw, fpw + 1} - {0})


def side_sets(nf):
    """(name, mesh, side set id, the side set whose clamp masks a rim of it) with nf faces each."""
    cyl = hollow_cylinder_mesh(1, 6, 3)
    assert len(cyl.side_sets[996]) == 18 >= nf
    cyl.side_sets[7] = cyl.side_sets[996][:nf].copy()                  # the first faces of the inner wall: they touch the end z = z0
    return [("planar", box_mesh(nf, 1, 1), 1, 6), ("curved", cyl, 7, 998)]


def both(gpu, mesh, dm, sides, Q, mask=None):
    return SupportSurface(gpu, mesh, dm, sides, Q, mask=mask), SupportSurface(gpu, mesh, dm, sides, Q, mask=mask, portable=True)


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def device_results(gpu, dev, x, n, P, Q):
    """(state, force, tangent, diagonal) from the device, each L-vector result added into a zeroed vector; the kernel name after each."""
    S, X = dev.new_state(), gpu.vector(n).set_array(x)
    S.set_value(-7.0)
    dev.form_state(KN, KT, S)
    assert dev.kernel_name == f"contact<P={P},Q={Q},support_state>"
    out = [S.to_numpy()[:dev.state_size].reshape(dev.nface, NSTATE, -1).copy()]
    for mode, call in (("support_force", lambda y: dev.force_add(1.0, S, X, y)), ("tangent", lambda y: dev.tangent_add(1.0, S, X, y)),
                       ("diagonal", lambda y: dev.diagonal_add(1.0, S, y))):
        Y = gpu.vector(n).set_value(0.0)
        call(Y)
        assert dev.kernel_name == f"contact<P={P},Q={Q},{mode}>", (dev.kernel_name, mode)
        out.append(Y.to_numpy().copy())
        Y.destroy()
    S.destroy(); X.destroy()
    return out


@pytest.mark.parametrize("P,Q", PQ)
def test_every_instantiation_against_the_portable_form(gpu, P, Q):
    worst = 0.0
    for nf in face_counts(Q):
        for name, mesh, sid, clamped in side_sets(nf):
            dm = build_dofmap(mesh, P - 1)
            n = dm.lsize
            x = np.random.default_rng(100 * P + Q).uniform(-1, 1, n)
            for masked in (False, True):
                mask = dirichlet_mask(dm, side_set_nodes(mesh, dm, [clamped])).copy() if masked else None
                dev, ref = both(gpu, mesh, dm, [sid], Q, mask=mask)
                assert not dev.portable and ref.portable and dev.nface == nf
                where = (name, nf, masked)
                state = ref.state_host(KN, KT)
                want = [state, ref.force_host(state, x), ref.tangent_host(state, x), ref.diagonal_host(state)]
                if masked:
                    m = mask != 0
                    rim = m & np.repeat(np.isin(np.arange(dm.nnodes), np.unique(ref.faces)), 3)
                    assert rim.any() and np.abs(x[rim]).min() > 0 and rel(want[1], want[2]) > 1e-3, where     # the rim's values matter
                got = device_results(gpu, dev, x, n, P, Q)
                for kind, a, b in zip(("state", "force", "tangent", "diagonal"), got, want):
                    err = rel(a, b)
                    worst = max(worst, err)
                    assert err <= TOL, (where, kind, err)
                    if masked and kind != "state":
                        assert np.all(a[m] == 0.0), (where, kind)                  # masked rows are never written
                assert abs(dev.area(got[0].reshape(-1)) - ref.area(state)) <= 1e-13 * ref.area(state), where
                dev.destroy()
    print(f"support<P={P},Q={Q}>: worst device-vs-portable error {worst:.2e}")


@pytest.mark.parametrize("Pc,Q", [(2, 5), (3, 6)])
def test_coarse_handle_on_a_combined_fine_state(gpu, Pc, Q):
    """A coarse level's handle (its own P, the fine Q) on K_s + a1 C_d formed from two fine states with the vector waxpby."""
    mesh = box_mesh(2, 2, 1)
    sides = [1, 2, 3, 4, 5, 6]
    dmf, dmc = build_dofmap(mesh, 3), build_dofmap(mesh, Pc - 1)
    fine, ref = both(gpu, mesh, dmf, sides, Q)
    coarse, cref = both(gpu, mesh, dmc, sides, Q)
    Ss, Sd, Sc = fine.new_state(), fine.new_state(), fine.new_state()
    fine.form_state(KN, KT, Ss); fine.form_state(0.5, 0.0, Sd)
    Sc.waxpby(1.0, Ss, 20.0, Sd)
    state = ref.state_host(KN, KT) + 20.0 * ref.state_host(0.5, 0.0)
    v = np.random.default_rng(Pc).uniform(-1, 1, dmc.lsize)
    V, T, D = gpu.vector(dmc.lsize).set_array(v), gpu.vector(dmc.lsize).set_value(0.0), gpu.vector(dmc.lsize).set_value(0.0)
    coarse.tangent_add(1.0, Sc, V, T)
    assert coarse.kernel_name == f"contact<P={Pc},Q={Q},tangent>"
    coarse.diagonal_add(1.0, Sc, D)
    assert coarse.kernel_name == f"contact<P={Pc},Q={Q},diagonal>"
    for got, want in ((T.to_numpy(), cref.tangent_host(state, v)), (D.to_numpy(), cref.diagonal_host(state))):
        assert rel(got, want) <= TOL
    for o in (fine, coarse):
        o.destroy()


def test_refusals_before_any_launch(gpu):
    mesh = box_mesh(1, 1, 1)
    dm = build_dofmap(mesh, 1)
    n = dm.lsize
    assert n == 24
    for P, Q in ((3, 2), (9, 9), (1, 1), (8, 9)):
        with pytest.raises(cd.CeedError, match=f"no support kernel for P={P} Q={Q}"):
            cd.SupportHandle(gpu, P, Q, np.zeros((1, P * P), dtype=np.int32), n)
    with pytest.raises(cd.CeedError, match="lies past the L-size"):
        cd.SupportHandle(gpu, 2, 2, [[0, 3, 6, 24]], n)
    dev = SupportSurface(gpu, mesh, dm, [1], 3)
    H = dev.handle
    X = gpu.vector(n).set_array(dev.Xh)
    short, ok, ok2 = gpu.vector(n - 1).set_value(0.0), gpu.vector(n).set_value(0.0), gpu.vector(n).set_value(0.0)
    S, Sshort, big = dev.new_state(), gpu.vector(dev.state_size - 1).set_value(0.0), gpu.vector(dev.state_size).set_value(0.0)
    assert dev.state_size == 1 * 7 * 9
    for kn, kt in ((-1.0, 1.0), (1.0, -1.0), (float("nan"), 1.0), (1.0, float("inf"))):
        with pytest.raises(cd.CeedError, match="not finite and non-negative"):
            H.form_state(kn, kt, X, S)
    for call in (lambda: H.form_state(1.0, 1.0, short, S), lambda: H.apply_force_add(1.0, S, short, ok), lambda: H.apply_force_add(1.0, S, ok, short),
                 lambda: H.apply_tangent_add(1.0, S, short, ok), lambda: H.apply_tangent_add(1.0, S, ok, short), lambda: H.diagonal_add(1.0, S, short)):
        with pytest.raises(cd.CeedError, match="shorter than the L-size 24"):
            call()
    for call in (lambda: H.form_state(1.0, 1.0, X, Sshort), lambda: H.apply_force_add(1.0, Sshort, ok, ok2), lambda: H.apply_tangent_add(1.0, Sshort, ok, ok2),
                 lambda: H.diagonal_add(1.0, Sshort, ok)):
        with pytest.raises(cd.CeedError, match="state vector shorter than 63 = nface x 7 x Q\\^2"):
            call()
    for call in (lambda: H.form_state(1.0, 1.0, big, big), lambda: H.apply_force_add(1.0, S, ok, ok), lambda: H.apply_tangent_add(1.0, S, ok, ok),
                 lambda: H.apply_force_add(1.0, big, ok, big), lambda: H.apply_tangent_add(1.0, big, ok, big), lambda: H.diagonal_add(1.0, big, big)):
        with pytest.raises(cd.CeedError, match="aliases an input"):
            call()
    assert dev.kernel_name == ""                                     # nothing was launched
    with pytest.raises(cd.CeedError, match="shorter than the L-vector"):
        H.set_dirichlet_mask(np.zeros(n - 1, dtype=np.uint8))
    dev.destroy()


def test_first_use_during_capture_is_refused_and_a_warm_sequence_replays(product_lib):
    ceed = cd.Ceed(product_lib, "/gpu/hip/mi355x")                   # a Ceed of its own: nothing of it is warm
    mesh = nb.distorted_box(2, 2, 1)
    prob = SolidProblem(ceed, mesh, 2, "hyperFS", nu=0.3, E=1.0, bc_sides=[1], multigrid="none")
    lv = prob.levels[prob.fine]
    n = prob.lsize()
    dev = SupportSurface(ceed, mesh, lv.dofmap, [5], prob.Q, mask=lv.mask)          # side 5 shares an edge with the clamped side 1
    ref = SupportSurface(ceed, mesh, lv.dofmap, [5], prob.Q, mask=lv.mask, portable=True)
    u = prob.smooth_state(0.1) + 0.01
    U, R, Rg, S = ceed.vector(n).set_array(u), ceed.vector(n).set_value(0.0), ceed.vector(n).set_value(0.0), dev.new_state()
    dev.form_state(KN, KT, S)                                        # (the state kernel needs no map: it is not the first apply)
    prob.form_residual(U, R); prob.form_residual(U, Rg)              # the operator is warm, the vectors are on the device
    S.device_pointer()
    with pytest.raises(cd.CeedError, match="apply once before recording"):
        ceed.capture(lambda: dev.force_add(1.0, S, U, Rg))

    def sequence(out):
        prob.form_residual(U, out)
        dev.force_add(0.5, S, U, out)
        dev.tangent_add(2.0, S, U, out)
    sequence(R)                                                      # one eager apply
    eager = R.to_numpy().copy()
    R.device_pointer()
    plain = ceed.vector(n).set_value(0.0)
    prob.form_residual(U, plain)
    state = ref.state_host(KN, KT)
    want = plain.to_numpy() + 0.5 * ref.force_host(state, u) + 2.0 * ref.tangent_host(state, u)
    assert not np.array_equal(eager, plain.to_numpy()) and np.abs(eager - want).max() <= 1e-12 * np.abs(want).max()
    g = ceed.capture(lambda: sequence(Rg))
    for _ in range(2):
        Rg.set_value(-3.0)
        g.launch()
        assert np.array_equal(Rg.to_numpy(), eager)
    dev.set_mask(lv.mask)                                            # a new mask drops the row flags: the next first use is refused again
    with pytest.raises(cd.CeedError, match="apply once before recording"):
        ceed.capture(lambda: dev.tangent_add(1.0, S, R, Rg))
    g.destroy()
    dev.destroy(); prob.destroy()


def test_area_of_a_box_side(gpu):
    mesh = box_mesh(3, 2, 1, hi=(1.5, 0.7, 1.0))
    for P, Q in ((2, 2), (4, 5)):
        dm = build_dofmap(mesh, P - 1)
        dev = SupportSurface(gpu, mesh, dm, [1], Q)
        S = dev.new_state()
        dev.form_state(KN, KT, S)
        assert abs(dev.area(S) - 1.5 * 0.7) <= 1e-13 * 1.5 * 0.7
        S.destroy(); dev.destroy()


def test_no_faces_no_launch(gpu):
    mesh = box_mesh(1, 1, 1)
    dm = build_dofmap(mesh, 2)
    dev = SupportSurface(gpu, mesh, dm, [], 4)
    assert dev.nface == 0 and not dev.portable and dev.state_size == 0
    y0 = np.random.default_rng(1).uniform(-1, 1, dm.lsize)
    Y, U, S = gpu.vector(dm.lsize).set_array(y0), gpu.vector(dm.lsize).set_array(y0), dev.new_state()
    dev.form_state(1.0, 1.0, S); dev.force_add(1.0, S, U, Y); dev.tangent_add(1.0, S, U, Y); dev.diagonal_add(1.0, S, Y)
    assert np.array_equal(Y.to_numpy(), y0) and dev.kernel_name == "" and dev.area(S) == 0.0
    dev.destroy()
