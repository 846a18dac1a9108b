"""Penalty contact on the device (CeedXContact*, csrc/kernels_contact.hip) against the portable NumPy form of contact.py.

Inputs and their input condition (min |g| >= 1e-6, 10 % .. 90 % of the points active, asserted first on the portable form):
``_contact_inputs``.  With that margin both sides agree on which points are active: their gaps differ by roundings of O(1e-13).

Bound: 1e-12 relative to the result's max norm -- the surface loads' bound with the same derivation.  Both sides sum O(P^2) products of
O(1) table entries per pass in float64; the tables come from two independent generators (Fornberg's recurrence on Newton-iterated points
in the library, product formulas on numpy's leggauss points here) that agree to a few ulp, so the difference is a few hundred roundings of
1.1e-16 at most.  The state is compared entry by entry: the six entries of K against the largest of them, the gaps against the largest
|x - x0| (resp. |x - c|) of the points, the size of the numbers the gap is the difference of.  The worst value per (P, Q) is printed."""
import ctypes as C

import numpy as np
import pytest

import _contact_inputs as ci
import _numbering as nb
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.contact import NSTATE, ContactSurface
from ceedpetscsolid_amd.mesh import box_mesh, build_dofmap, dirichlet_mask, hollow_cylinder_mesh, side_set_nodes
from ceedpetscsolid_amd.solid import SolidProblem

pytestmark = pytest.mark.gpu

PQ = [(P, Q) for P in range(2, 9) for Q in range(P, 9)]
TOL = 1e-12


def test_the_instantiated_pairs():
    assert len(PQ) == 28


def shapes(P):
    """(name, mesh, side sets): the smallest shapes at which the kernels can go wrong."""
    out = [("one face", box_mesh(1, 1, 1), [1]),                               # fewer rows than a wave
           ("side 1", box_mesh(2, 2, 1), [1]),
           ("six sides", box_mesh(2, 2, 1), [1, 2, 3, 4, 5, 6]),              # rows of valence 1, 2, 3, 4 with contributors from different local faces
           ("curved wall", hollow_cylinder_mesh(1, 5, 2), [996])]
    if P <= 3:
        out.append(("three faces", box_mesh(3, 1, 1), [1]))                    # nface no multiple of the faces of a wave (16, 7, 4, 2)
    return out


def both(gpu, mesh, dm, sides, Q, mask=None):
    return ContactSurface(gpu, mesh, dm, sides, Q, mask=mask), ContactSurface(gpu, mesh, dm, sides, Q, mask=mask, portable=True)


def scale_of_gap(ref, u):
    x = np.einsum("ai,bj,fjic->fbac", ref.B, ref.B, ref._gather(ref.Xh) + ref._gather(u))
    return float(np.linalg.norm(x - ref.par[:3], axis=-1).max())


def device_results(gpu, dev, u, du, n, name=None):
    """(residual, state, tangent, diagonal) from the device, each into a zeroed vector; the kernel name is checked after each call."""
    U, DU, S = gpu.vector(n).set_array(u), gpu.vector(n).set_array(du), dev.new_state()
    out = []
    for mode, call in (("residual", lambda y: dev.residual_add(1.0, U, y, S)), ("tangent", lambda y: dev.tangent_add(1.0, S, DU, y)),
                       ("diagonal", lambda y: dev.diagonal_add(1.0, S, y))):
        Y = gpu.vector(n).set_value(0.0)
        call(Y)
        if name is not None:
            assert dev.kernel_name == name.format(mode), (dev.kernel_name, mode)
        out.append(Y.to_numpy().copy())
        Y.destroy()
    state = S.to_numpy()[:dev.state_size].reshape(dev.nface, NSTATE, -1).copy()
    U.destroy(); DU.destroy(); S.destroy()
    return out[0], state, out[1], out[2]


def compare(got, ref, u, du, where):
    """The device's (residual, state, tangent, diagonal) against the portable form's; returns the worst relative error."""
    r, state = ref.residual_host(u)
    want = {"residual": r, "tangent": ref.tangent_host(state, du), "diagonal": ref.diagonal_host(state)}
    worst = 0.0
    for kind, a in zip(("residual", "tangent", "diagonal"), (got[0], got[2], got[3])):
        b = want[kind]
        err = np.abs(a - b).max() / np.abs(b).max()
        worst = max(worst, err)
        assert err <= TOL, (where, kind, err)
    ek = np.abs(got[1][:, :6] - state[:, :6]).max() / np.abs(state[:, :6]).max()
    eg = np.abs(got[1][:, 6] - state[:, 6]).max() / scale_of_gap(ref, u)
    assert ek <= TOL and eg <= TOL, (where, "state", ek, eg)
    assert np.array_equal(got[1][:, 6] < 0, state[:, 6] < 0), where            # the same active set
    return max(worst, ek, eg)


@pytest.mark.parametrize("P,Q", PQ)
def test_every_instantiation_against_the_portable_form(gpu, P, Q):
    worst = 0.0
    for name, mesh, sides in shapes(P):
        dm = build_dofmap(mesh, P - 1)
        dev, ref = both(gpu, mesh, dm, sides, Q)
        assert not dev.portable and ref.portable
        u, du = ci.displacement(dm, P, Q)
        for which in ci.OBSTACLES:
            dev.set_obstacle(**ci.set_obstacle(ref, which, u))
            ci.input_condition(ref, u)
            got = device_results(gpu, dev, u, du, dm.lsize, name=f"contact<P={P},Q={Q},{{}}>")
            worst = max(worst, compare(got, ref, u, du, (name, which)))
        dev.destroy()
    print(f"contact<P={P},Q={Q}>: worst device-vs-portable error {worst:.2e}")


@pytest.mark.parametrize("Pc,Q", [(2, 5), (3, 6)])
def test_coarse_handle_on_the_fine_state(gpu, Pc, Q):
    mesh = box_mesh(2, 2, 1)
    sides = [1, 2, 3, 4, 5, 6]
    dmf, dmc = build_dofmap(mesh, 3), build_dofmap(mesh, Pc - 1)
    fine, ref = both(gpu, mesh, dmf, sides, Q)
    coarse, cref = both(gpu, mesh, dmc, sides, Q)
    u, _ = ci.displacement(dmf, 4, Q)
    fine.set_obstacle(**ci.set_obstacle(ref, "ball", u))
    ci.input_condition(ref, u)
    U, S, Y = gpu.vector(dmf.lsize).set_array(u), fine.new_state(), gpu.vector(dmf.lsize).set_value(0.0)
    fine.residual_add(1.0, U, Y, S)
    assert fine.kernel_name == f"contact<P=4,Q={Q},residual>"
    _, state = ref.residual_host(u)
    v = np.random.default_rng(Pc).uniform(-1, 1, dmc.lsize)
    V, T, D = gpu.vector(dmc.lsize).set_array(v), gpu.vector(dmc.lsize).set_value(0.0), gpu.vector(dmc.lsize).set_value(0.0)
    coarse.tangent_add(1.0, S, V, T)                          # no obstacle was ever set on the coarse handle
    assert coarse.kernel_name == f"contact<P={Pc},Q={Q},tangent>"
    coarse.diagonal_add(1.0, S, D)
    assert coarse.kernel_name == f"contact<P={Pc},Q={Q},diagonal>"
    for got, want in ((T.to_numpy(), cref.tangent_host(state, v)), (D.to_numpy(), cref.diagonal_host(state))):
        assert np.abs(got - want).max() <= TOL * np.abs(want).max()
    for o in (fine, coarse):
        o.destroy()


@pytest.mark.parametrize("P,Q", [(2, 2), (3, 5), (5, 5), (8, 8)])
def test_apply_add_semantics(gpu, P, Q):
    mesh = box_mesh(2, 2, 1)
    dm = build_dofmap(mesh, P - 1)
    n = dm.lsize
    on = np.zeros(dm.nnodes, dtype=bool); on[side_set_nodes(mesh, dm, [1, 5])] = True
    mask = dirichlet_mask(dm, side_set_nodes(mesh, dm, [6])).copy()         # the edge side 1 shares with side 6 is masked ...
    mask[3 * side_set_nodes(mesh, dm, [5])[1] + 2] = 1                       # ... and one component of one more node
    m = mask != 0
    dev, ref = both(gpu, mesh, dm, [1, 5], Q, mask=mask)
    u, du = ci.displacement(dm, P, Q)
    dev.set_obstacle(**ci.set_obstacle(ref, "cavity", u))
    ci.input_condition(ref, u)
    y0 = np.random.default_rng(7).uniform(-1, 1, n)
    U, DU, S = gpu.vector(n).set_array(u), gpu.vector(n).set_array(du), dev.new_state()
    junk = du.copy(); junk[m] = 1e30
    JUNK = gpu.vector(n).set_array(junk)
    r, state = ref.residual_host(u)

    def run(call, s=1.0, start=y0):
        Y = gpu.vector(n).set_array(start)
        call(Y, s)
        return Y.to_numpy().copy()
    calls = {"residual": (lambda y, s: dev.residual_add(s, U, y, S), r),                  # (first: it writes the state the others read)
             "tangent": (lambda y, s: dev.tangent_add(s, S, DU, y), ref.tangent_host(state, du)),
             "diagonal": (lambda y, s: dev.diagonal_add(s, S, y), ref.diagonal_host(state))}
    for kind, (call, want) in calls.items():
        y = run(call)
        changed = y != y0
        assert changed.any() and not changed[m].any() and not changed[~np.repeat(on, 3)].any(), kind      # off the surface and masked rows: same bits
        assert np.array_equal(y, run(call)), kind                                                           # bit-reproducible
        scale = np.abs(want).max()
        assert np.abs(y - y0 - want).max() <= 1e-12 * scale + 4 * np.finfo(float).eps * np.abs(y0).max(), kind  # (y0 + g - y0 rounds at |y0|)
        zero = np.zeros(n)
        g1 = run(call, 1.0, zero)
        assert np.array_equal(run(call, 0.5, zero), 0.5 * g1) and np.array_equal(run(call, -4.0, zero), -4.0 * g1), kind   # powers of two: exact
        # any other factor enters at the quadrature points: one rounding per term of a nodal sum, at most 2 Q + 4 terms -- 64 eps of the
        # largest nodal value covers Q = 8 (the surface loads' bound)
        assert np.abs(run(call, 0.3, zero) - 0.3 * g1).max() <= 64 * np.finfo(float).eps * scale, kind
    s1 = S.to_numpy().copy()
    dev.residual_add(0.25, U, gpu.vector(n).set_value(0.0), S)
    assert np.array_equal(S.to_numpy(), s1)                                                                 # the state is never scaled
    assert np.array_equal(run(lambda y, s: dev.tangent_add(s, S, JUNK, y)), run(calls["tangent"][0]))       # masked du is never read as it is
    dev.destroy()


@pytest.mark.parametrize("numbering", ["permuted", "gaps"])
def test_caller_chosen_numbering(gpu, numbering):
    mesh = nb.distorted_box(2, 2, 1)
    dm = nb.NUMBERINGS[numbering](mesh, 2)
    n = dm.lsize
    dev, ref = both(gpu, mesh, dm, [2, 4, 5], 4)
    u, du = ci.displacement(dm, 3, 4)
    kw = ci.set_obstacle(ref, "ball", u)
    dev.set_obstacle(**kw)
    ci.input_condition(ref, u)
    got = device_results(gpu, dev, u, du, n)
    compare(got, ref, u, du, numbering)
    for a in (got[0], got[2], got[3]):
        assert np.all(a[~nb.referenced(dm)] == 0.0)                 # nodes no element holds are never written
    # the same field under the default numbering: the nodal vectors agree after carrying them over
    d0 = nb.default(mesh, 2)
    ref0 = ContactSurface(gpu, mesh, d0, [2, 4, 5], 4, portable=True)
    ref0.set_obstacle(**kw)
    r0, _ = ref0.residual_host(nb.to_default(u, dm))
    assert np.abs(nb.to_default(got[0], dm) - r0).max() <= TOL * np.abs(r0).max()
    dev.destroy()


def test_refusals(gpu, product_lib):
    mesh = box_mesh(1, 1, 1)
    dm = build_dofmap(mesh, 1)
    n = dm.lsize
    assert n == 24
    with pytest.raises(cd.CeedError, match="lies past the L-size"):
        cd.ContactHandle(gpu, 2, 2, [[0, 3, 6, 24]], n)
    with pytest.raises(cd.CeedError, match="lies past the L-size"):
        cd.ContactHandle(gpu, 2, 2, [[0, 3, 6, 22]], n)              # offset + 2 == lsize
    with pytest.raises(cd.CeedError, match="lies past the L-size"):
        cd.ContactHandle(gpu, 2, 2, [[0, 3, -3, 9]], n)
    with pytest.raises(cd.CeedError, match="no multiple of 3"):
        cd.ContactHandle(gpu, 2, 2, [[0, 3, 6, 10]], n)
    for P, Q in ((3, 2), (9, 9), (1, 1), (8, 9), (1, 4)):
        with pytest.raises(cd.CeedError, match=f"no contact kernel for P={P} Q={Q}"):
            cd.ContactHandle(gpu, P, Q, np.zeros((1, P * P), dtype=np.int32), n)
    L = gpu.L
    h = C.c_void_p()
    with pytest.raises(cd.CeedError, match="nface = -1 is negative"):
        L.chk(L.lib.CeedXContactCreate(gpu.h, -1, 2, 2, None, n, C.byref(h)))
    dev = ContactSurface(gpu, mesh, dm, [1], 3)
    H = dev.handle
    X = gpu.vector(n).set_array(dev.Xh)
    short, ok, ok2 = gpu.vector(n - 1).set_value(0.0), gpu.vector(n).set_value(0.0), gpu.vector(n).set_value(0.0)
    S, Sshort, big = dev.new_state(), gpu.vector(dev.state_size - 1).set_value(0.0), gpu.vector(dev.state_size).set_value(0.0)
    assert dev.state_size == 1 * 7 * 9
    with pytest.raises(cd.CeedError, match="no obstacle set"):
        H.apply_residual_add(1.0, X, ok, ok2, S)
    for kind, par, pen, msg in ((0, (0, 0, 0, 0, 0, 1), 0.0, "penalty 0 is not positive"), (0, (0, 0, 0, 0, 0, 1), -2.0, "penalty -2 is not positive"),
                                (0, (0, 0, 0, 0, 0, 1.5), 1.0, "plane normal has length 1.5, not 1"), (0, (0, 0, 0, 0, 0, 0), 1.0, "plane normal has length 0, not 1"),
                                (1, (0, 0, 0, 0.0, 1), 1.0, "sphere radius 0 is not positive"), (1, (0, 0, 0, -1.0, 1), 1.0, "sphere radius -1 is not positive"),
                                (1, (0, 0, 0, 1.0, 0.5), 1.0, "neither \\+1"), (2, (0, 0, 0, 0, 0, 1), 1.0, "kind 2 is neither plane nor sphere")):
        with pytest.raises(cd.CeedError, match=msg):
            H.set_obstacle(kind, par, pen)
    with pytest.raises(cd.CeedError, match="no obstacle set"):      # a refused obstacle sets nothing
        H.apply_residual_add(1.0, X, ok, ok2, S)
    dev.set_obstacle(plane=((0, 0, 0.1), (0, 0, 1.0)), penalty=2.0)
    for call in (lambda: H.apply_residual_add(1.0, short, ok, ok2, S), lambda: H.apply_residual_add(1.0, X, short, ok2, S),
                 lambda: H.apply_residual_add(1.0, X, ok, short, S), lambda: H.apply_tangent_add(1.0, S, short, ok), lambda: H.apply_tangent_add(1.0, S, ok, short),
                 lambda: H.diagonal_add(1.0, S, short)):
        with pytest.raises(cd.CeedError, match="shorter than the L-size 24"):
            call()
    for call in (lambda: H.apply_residual_add(1.0, X, ok, ok2, Sshort), lambda: H.apply_tangent_add(1.0, Sshort, ok, ok2), lambda: H.diagonal_add(1.0, Sshort, ok)):
        with pytest.raises(cd.CeedError, match="state vector shorter than 63 = nface x 7 x Q\\^2"):
            call()
    for call in (lambda: H.apply_residual_add(1.0, X, ok, ok, S), lambda: H.apply_residual_add(1.0, X, ok, X, S), lambda: H.apply_tangent_add(1.0, S, ok, ok),
                 lambda: H.apply_residual_add(1.0, X, big, ok2, big), lambda: H.diagonal_add(1.0, big, big)):
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
    dev = ContactSurface(ceed, mesh, lv.dofmap, [2], prob.Q, mask=lv.mask)
    ref = ContactSurface(ceed, mesh, lv.dofmap, [2], prob.Q, mask=lv.mask, portable=True)
    u = prob.smooth_state(0.1)
    dev.set_obstacle(**ci.set_obstacle(ref, "ball", u))
    ci.input_condition(ref, u)
    U, R, Rg, S = ceed.vector(n).set_array(u), ceed.vector(n).set_value(0.0), ceed.vector(n).set_value(0.0), dev.new_state()
    prob.form_residual(U, R); prob.form_residual(U, Rg)              # the operator is warm, the vectors are on the device
    dev.X = ceed.vector(n).set_array(dev.Xh)
    dev.X.device_pointer(); S.device_pointer()
    with pytest.raises(cd.CeedError, match="apply once before recording"):
        ceed.capture(lambda: dev.residual_add(1.0, U, Rg, S))

    def sequence(out):
        prob.form_residual(U, out)
        dev.residual_add(0.5, U, out, S)
        dev.tangent_add(2.0, S, U, out)
        dev.diagonal_add(1.0, S, out)
    sequence(R)                                                      # one eager apply
    eager, eager_state = R.to_numpy().copy(), S.to_numpy().copy()
    R.device_pointer(); S.device_pointer()
    plain = ceed.vector(n).set_value(0.0)
    prob.form_residual(U, plain)
    assert not np.array_equal(eager, plain.to_numpy())               # the contact terms are in it
    g = ceed.capture(lambda: sequence(Rg))
    for _ in range(2):
        Rg.set_value(-3.0); S.set_value(-1.0)
        g.launch()
        assert np.array_equal(Rg.to_numpy(), eager) and np.array_equal(S.to_numpy(), eager_state)
    # a new mask drops the row flags: the next first use is refused again
    dev.set_mask(lv.mask)
    with pytest.raises(cd.CeedError, match="apply once before recording"):
        ceed.capture(lambda: dev.tangent_add(1.0, S, R, Rg))
    g.destroy()
    dev.destroy(); prob.destroy()


def test_no_faces_no_launch(gpu):
    mesh = box_mesh(1, 1, 1)
    dm = build_dofmap(mesh, 2)
    dev = ContactSurface(gpu, mesh, dm, [], 4)
    assert dev.nface == 0 and not dev.portable and dev.state_size == 0
    dev.set_obstacle(plane=((0, 0, 0.5), (0, 0, 1.0)), penalty=1.0)
    y0 = np.random.default_rng(1).uniform(-1, 1, dm.lsize)
    Y, U, S = gpu.vector(dm.lsize).set_array(y0), gpu.vector(dm.lsize).set_array(y0), dev.new_state()
    dev.residual_add(1.0, U, Y, S); dev.tangent_add(1.0, S, U, Y); dev.diagonal_add(1.0, S, Y)
    assert np.array_equal(Y.to_numpy(), y0) and dev.kernel_name == ""
    assert dev.min_gap(S) == float("inf") and dev.active_fraction(S) == 0.0
    dev.destroy()
