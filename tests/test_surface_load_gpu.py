"""Surface loads on the device (CeedXSurfaceLoad*, csrc/kernels_surface.hip) against the portable NumPy form of surface.py.

Bound: 1e-12 relative to the result's max norm.  Both sides sum O(P^2) products of O(1) table entries per pass in float64; the
tables come from two independent generators (Fornberg's recurrence on Newton-iterated points in the library, product formulas on
numpy's leggauss points here) that agree to a few ulp, so the difference is a few hundred roundings of 1.1e-16 at most.  The worst
value per (P, Q) is printed (profiles/surface_load.txt keeps a record)."""
import ctypes as C

import numpy as np
import pytest

import _numbering as nb
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mesh import box_mesh, build_dofmap, dirichlet_mask, hollow_cylinder_mesh, side_set_nodes
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.surface import SurfaceLoad

pytestmark = pytest.mark.gpu

PQ = [(P, Q) for P in range(2, 9) for Q in range(P, min(P + 2, 8) + 1)]
TOL = 1e-12
T = (0.3, -1.1, 0.7)


def test_the_instantiated_pairs():
    assert len(PQ) == 18


def shapes(P):
    """(name, mesh, side sets): the smallest shapes at which the kernels can go wrong."""
    out = [("one face", box_mesh(1, 1, 1), [2]),                              # fewer rows than a wave
           ("six sides", box_mesh(2, 2, 1), [1, 2, 3, 4, 5, 6]),             # rows of valence 1, 2, 3, 4 with contributors from different local faces
           ("curved wall", hollow_cylinder_mesh(1, 5, 2), [996])]
    if P <= 3:
        out.append(("three faces", box_mesh(3, 1, 1), [1]))                   # nface no multiple of the faces of a wave (16, 7, 4, 2)
    return out


def both(gpu, mesh, dm, sides, Q, mask=None):
    return SurfaceLoad(gpu, mesh, dm, sides, Q=Q, mask=mask), SurfaceLoad(gpu, mesh, dm, sides, Q=Q, mask=mask, portable=True)


def device_results(gpu, dev, u, du, n):
    """(traction, pressure at u, pressure at the reference configuration, tangent) from the device, each into a zeroed vector."""
    U, DU = gpu.vector(n).set_array(u), gpu.vector(n).set_array(du)
    out = []
    for call in (lambda y: dev.traction_add(T, 1.0, y), lambda y: dev.pressure_add(1.0, 1.0, U, y), lambda y: dev.pressure_add(1.0, 1.0, None, y),
                 lambda y: dev.tangent_add(1.0, 1.0, U, DU, y)):
        Y = gpu.vector(n).set_value(0.0)
        call(Y)
        out.append(Y.to_numpy().copy())
        Y.destroy()
    U.destroy(); DU.destroy()
    return out


@pytest.mark.parametrize("P,Q", PQ)
def test_every_instantiation_against_the_portable_form(gpu, P, Q):
    worst = 0.0
    for name, mesh, sides in shapes(P):
        dm = build_dofmap(mesh, P - 1)
        dev, ref = both(gpu, mesh, dm, sides, Q)
        assert not dev.portable and ref.portable
        rng = np.random.default_rng(100 * P + Q)
        u, du = 0.1 * rng.uniform(-1, 1, dm.lsize), rng.uniform(-1, 1, dm.lsize)
        got = device_results(gpu, dev, u, du, dm.lsize)
        want = [ref.traction_host(T), ref.pressure_host(u), ref.pressure_host(), ref.tangent_host(u, du)]
        assert dev.kernel_name == f"surface<P={P},Q={Q}>"
        for kind, a, b in zip(("traction", "pressure", "pressure(u=0)", "tangent"), got, want):
            err = np.abs(a - b).max() / np.abs(b).max()
            worst = max(worst, err)
            assert err <= TOL, (name, kind, err)
        dev.destroy()
    print(f"surface<P={P},Q={Q}>: worst device-vs-portable error {worst:.2e}")


@pytest.mark.parametrize("P,Q", [(2, 2), (3, 4), (5, 5), (8, 8)])
def test_apply_add_semantics(gpu, P, Q):
    mesh = box_mesh(2, 2, 1)
    dm = build_dofmap(mesh, P - 1)
    n = dm.lsize
    on = np.zeros(dm.nnodes, dtype=bool); on[side_set_nodes(mesh, dm, [2, 5])] = True
    mask = dirichlet_mask(dm, side_set_nodes(mesh, dm, [6])).copy()         # the edge side 2 shares with side 6 is masked ...
    mask[3 * side_set_nodes(mesh, dm, [5])[1] + 2] = 1                       # ... and one component of one more node
    m = mask != 0
    dev, ref = both(gpu, mesh, dm, [2, 5], Q, mask=mask)
    rng = np.random.default_rng(7)
    u, du, y0 = 0.1 * rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    U, DU = gpu.vector(n).set_array(u), gpu.vector(n).set_array(du)
    junk = du.copy(); junk[m] = 1e30
    JUNK = gpu.vector(n).set_array(junk)

    def run(call):
        Y = gpu.vector(n).set_array(y0)
        call(Y)
        return Y.to_numpy().copy()
    calls = {"traction": (lambda y, s=1.0, c=1.0: dev.traction_add(tuple(c * t for t in T), s, y), ref.traction_host(T)),
             "pressure": (lambda y, s=1.0, c=1.0: dev.pressure_add(c, s, U, y), ref.pressure_host(u)),
             "tangent": (lambda y, s=1.0, c=1.0: dev.tangent_add(c, s, U, DU, y), ref.tangent_host(u, du))}
    for kind, (call, want) in calls.items():
        y = run(call)
        changed = y != y0
        assert changed.any() and not changed[m].any() and not changed[~np.repeat(on, 3)].any(), kind      # off the surface and masked rows: same bits
        assert np.array_equal(y, run(call)), kind                                                           # bit-reproducible
        g = y - y0
        scale = np.abs(want).max()
        assert np.abs(g - want).max() <= 1e-12 * scale + 4 * np.finfo(float).eps * np.abs(y0).max(), kind  # (y0 + g - y0 rounds at |y0|)
        # linear in scale and in coef, into zeroed vectors.  The factor enters at the quadrature points, so a nodal value differs from
        # the scaled one by one rounding per term of its sum: at most 2 Q + 4 (the two passes, four faces) of them, each below the
        # largest nodal value times the tables' O(1) entries -- 64 eps covers Q = 8 with a factor of three to spare
        def z(s, c):
            Y = gpu.vector(n).set_value(0.0)
            call(Y, s, c)
            return Y.to_numpy().copy()
        g1, lin = z(1.0, 1.0), 64 * np.finfo(float).eps * scale
        assert np.abs(z(0.3, 1.0) - 0.3 * g1).max() <= lin, kind
        assert np.abs(z(1.0, -2.5) + 2.5 * g1).max() <= 2.5 * lin, kind
        assert np.array_equal(z(0.5, 4.0), 2.0 * g1), kind            # powers of two: exact
    assert np.array_equal(run(lambda y: dev.tangent_add(1.0, 1.0, U, JUNK, y)), run(lambda y: dev.tangent_add(1.0, 1.0, U, DU, y)))   # masked du is never read as it is
    dev.destroy()


@pytest.mark.parametrize("numbering", ["permuted", "gaps"])
def test_caller_chosen_numbering(gpu, numbering):
    mesh = nb.distorted_box(2, 2, 1)
    dm = nb.NUMBERINGS[numbering](mesh, 2)
    n = dm.lsize
    dev, ref = both(gpu, mesh, dm, [2, 4, 5], 4)
    rng = np.random.default_rng(3)
    u, du = 0.1 * rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    got = device_results(gpu, dev, u, du, n)
    want = [ref.traction_host(T), ref.pressure_host(u), ref.pressure_host(), ref.tangent_host(u, du)]
    for a, b in zip(got, want):
        assert np.abs(a - b).max() <= TOL * np.abs(b).max()
        assert np.all(a[~nb.referenced(dm)] == 0.0)                 # nodes no element holds are never written
    # the same field under the default numbering: the nodal vectors agree after carrying them over
    d0 = nb.default(mesh, 2)
    ref0 = SurfaceLoad(gpu, mesh, d0, [2, 4, 5], Q=4, portable=True)
    assert np.abs(nb.to_default(got[1], dm) - ref0.pressure_host(nb.to_default(u, dm))).max() <= TOL * np.abs(want[1]).max()
    dev.destroy()


def test_refusals(gpu, product_lib):
    mesh = box_mesh(1, 1, 1)
    dm = build_dofmap(mesh, 1)
    n = dm.lsize
    assert n == 24
    with pytest.raises(cd.CeedError, match="lies past the L-size"):
        cd.SurfaceLoadHandle(gpu, 2, 2, [[0, 3, 6, 24]], n)
    with pytest.raises(cd.CeedError, match="lies past the L-size"):
        cd.SurfaceLoadHandle(gpu, 2, 2, [[0, 3, 6, 22]], n)          # offset + 2 == lsize
    with pytest.raises(cd.CeedError, match="lies past the L-size"):
        cd.SurfaceLoadHandle(gpu, 2, 2, [[0, 3, -3, 9]], n)
    with pytest.raises(cd.CeedError, match="no multiple of 3"):
        cd.SurfaceLoadHandle(gpu, 2, 2, [[0, 3, 6, 10]], n)
    for P, Q in ((2, 5), (3, 2), (9, 9), (1, 1), (8, 9)):
        with pytest.raises(cd.CeedError, match="no surface kernel for P="):
            cd.SurfaceLoadHandle(gpu, P, Q, np.zeros((1, P * P), dtype=np.int32), n)
    L = gpu.L
    h = C.c_void_p()
    with pytest.raises(cd.CeedError, match="nface = -1 is negative"):
        L.chk(L.lib.CeedXSurfaceLoadCreate(gpu.h, -1, 2, 2, None, n, C.byref(h)))
    dev = SurfaceLoad(gpu, mesh, dm, [2])
    short, ok = gpu.vector(n - 1).set_value(0.0), gpu.vector(n).set_value(0.0)
    ok2 = gpu.vector(n).set_value(0.0)
    for call in (lambda: dev.pressure_add(1.0, 1.0, ok, short), lambda: dev.pressure_add(1.0, 1.0, short, ok), lambda: dev.traction_add(T, 1.0, short),
                 lambda: dev.tangent_add(1.0, 1.0, ok, short, ok2), lambda: dev.tangent_add(1.0, 1.0, short, ok, ok2), lambda: dev.tangent_add(1.0, 1.0, ok, ok2, short)):
        with pytest.raises(cd.CeedError, match="shorter than the L-size 24"):
            call()
    assert dev.kernel_name == ""                                     # nothing was launched
    with pytest.raises(cd.CeedError, match="aliases an input"):
        dev.pressure_add(1.0, 1.0, ok, ok)
    with pytest.raises(cd.CeedError, match="neither traction nor pressure"):
        dev.handle.apply_add(2, T, 1.0, dev.X, None, ok)
    with pytest.raises(cd.CeedError, match="shorter than the L-vector"):
        dev.handle.set_dirichlet_mask(np.zeros(n - 1, dtype=np.uint8))
    dev.destroy()


def test_first_use_during_capture_is_refused_and_a_warm_sequence_replays(product_lib):
    ceed = cd.Ceed(product_lib, "/gpu/hip/mi355x")                   # a Ceed of its own: nothing of it is warm
    mesh = nb.distorted_box(2, 2, 1)
    prob = SolidProblem(ceed, mesh, 2, "hyperFS", nu=0.3, E=1.0, bc_sides=[1], multigrid="none")
    lv = prob.levels[prob.fine]
    n = prob.lsize()
    dev = SurfaceLoad(ceed, mesh, lv.dofmap, [2], Q=prob.Q, mask=lv.mask)
    U, R, Rg = ceed.vector(n).set_array(prob.smooth_state(0.1)), ceed.vector(n).set_value(0.0), ceed.vector(n).set_value(0.0)
    prob.form_residual(U, R); prob.form_residual(U, Rg)              # the operator is warm, the vectors are on the device
    dev.X.device_pointer()
    with pytest.raises(cd.CeedError, match="apply once before recording"):
        ceed.capture(lambda: dev.pressure_add(0.02, 1.0, U, Rg))

    def sequence(out):
        prob.form_residual(U, out)
        dev.pressure_add(0.02, 0.5, U, out)
    sequence(R)                                                      # one eager apply
    eager = R.to_numpy().copy()
    R.device_pointer()
    plain = ceed.vector(n).set_value(0.0)
    prob.form_residual(U, plain)
    assert not np.array_equal(eager, plain.to_numpy())               # the pressure is in it
    g = ceed.capture(lambda: sequence(Rg))
    for _ in range(2):
        Rg.set_value(-3.0)
        g.launch()
        assert np.array_equal(Rg.to_numpy(), eager)
    # a new mask drops the row flags: the next first use is refused again, and an eager apply makes it recordable
    dev.set_mask(lv.mask)
    with pytest.raises(cd.CeedError, match="apply once before recording"):
        ceed.capture(lambda: dev.tangent_add(0.02, 1.0, U, R, Rg))
    g.destroy()
    dev.destroy(); prob.destroy()


def test_no_faces_no_launch(gpu):
    mesh = box_mesh(1, 1, 1)
    dm = build_dofmap(mesh, 2)
    dev = SurfaceLoad(gpu, mesh, dm, [])
    assert dev.nface == 0 and not dev.portable
    y0 = np.random.default_rng(1).uniform(-1, 1, dm.lsize)
    Y, U = gpu.vector(dm.lsize).set_array(y0), gpu.vector(dm.lsize).set_array(y0)
    dev.traction_add(T, 1.0, Y); dev.pressure_add(1.0, 1.0, U, Y); dev.tangent_add(1.0, 1.0, U, U, Y)
    assert np.array_equal(Y.to_numpy(), y0) and dev.kernel_name == ""
    dev.destroy()
