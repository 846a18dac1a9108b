"""A surface load and a contact surface on the SAME faces of one Ceed, their calls interleaved: the two handles share the Ceed's
E-vector scratch, the face-set layer of the host (csrc/face_set.hpp) and the face passes of the device (csrc/kernel_face_pass.hpp), and
nothing of one may show in the other.  box_mesh(2, 2, 1), side set 1, P = 3, Q = 4 (four faces, the four a wave holds at Q = 4), the
edge shared with side 6 masked.

Every result of the interleaved sequence is compared BIT FOR BIT with the same call made alone on fresh handles: the kernels and the
node sum are deterministic (no atomics, sums in face order), so equality is what the code promises, and no tolerance is involved."""
import numpy as np
import pytest

import _contact_inputs as ci
from ceedpetscsolid_amd.contact import ContactSurface
from ceedpetscsolid_amd.mesh import box_mesh, build_dofmap, dirichlet_mask, side_set_nodes
from ceedpetscsolid_amd.surface import SurfaceLoad

pytestmark = pytest.mark.gpu

P, Q, SIDES = 3, 4, [1]
SURFACE, CONTACT = f"surface<P={P},Q={Q}>", f"contact<P={P},Q={Q},{{}}>"


def test_interleaved_calls_of_two_handles_equal_the_calls_made_alone(gpu):
    mesh = box_mesh(2, 2, 1)
    dm = build_dofmap(mesh, P - 1)
    n = dm.lsize
    mask = dirichlet_mask(dm, side_set_nodes(mesh, dm, [6]))
    m = mask != 0
    on = np.zeros(dm.nnodes, dtype=bool); on[side_set_nodes(mesh, dm, SIDES)] = True
    on = np.repeat(on, 3)
    assert (m & on).any() and (~m & on).any()                        # the masked edge lies on the surface, and not all of it does
    ref = ContactSurface(gpu, mesh, dm, SIDES, Q, mask=mask, portable=True)
    u, du = ci.displacement(dm, P, Q)
    kw = ci.set_obstacle(ref, "ball", u)
    ci.input_condition(ref, u)
    y0 = np.random.default_rng(5).uniform(-1, 1, n)
    U, DU = gpu.vector(n).set_array(u), gpu.vector(n).set_array(du)

    def handles():
        sl, ct = SurfaceLoad(gpu, mesh, dm, SIDES, Q=Q, mask=mask), ContactSurface(gpu, mesh, dm, SIDES, Q, mask=mask)
        assert not sl.portable and not ct.portable and sl.nface == ct.nface == 4
        ct.set_obstacle(**kw)
        return sl, ct

    def calls(sl, ct, S):
        return {"pressure": lambda y: sl.pressure_add(0.7, 1.0, U, y), "residual": lambda y: ct.residual_add(1.0, U, y, S),
                "surface tangent": lambda y: sl.tangent_add(0.7, 1.0, U, DU, y), "contact tangent": lambda y: ct.tangent_add(1.0, S, DU, y),
                "diagonal": lambda y: ct.diagonal_add(1.0, S, y)}

    def run(call):
        Y = gpu.vector(n).set_array(y0)
        call(Y)
        out = Y.to_numpy().copy()
        Y.destroy()
        return out

    # the interleaved sequence on one pair of handles; after each call each handle names the last kernel of its OWN
    sl, ct = handles()
    S = ct.new_state()
    last = {"sl": "", "ct": ""}
    together = {}
    for name, call in calls(sl, ct, S).items():
        together[name] = run(call)
        if name in ("pressure", "surface tangent"):
            last["sl"] = SURFACE
        else:
            last["ct"] = CONTACT.format(name.split()[-1])
        assert (sl.kernel_name, ct.kernel_name) == (last["sl"], last["ct"]), name
        changed = together[name] != y0
        assert changed.any() and not changed[m].any() and not changed[~on].any(), name
    state = S.to_numpy().copy()

    # each call alone on fresh handles (the tangent and the diagonal on a copy of the state, as a coarse level takes it)
    for name in together:
        sl1, ct1 = handles()
        S1 = ct1.new_state() if name == "residual" else gpu.vector(state.size).set_array(state)
        assert np.array_equal(run(calls(sl1, ct1, S1)[name]), together[name]), name
        if name == "residual":
            assert np.array_equal(S1.to_numpy(), state)
        sl1.destroy(); ct1.destroy(); S1.destroy()

    # the mask is a handle's own: without the load's, the contact's masked rows stay unwritten while the load's are written
    sl.set_mask(None)
    for name in ("contact tangent", "diagonal", "residual"):
        y = run(calls(sl, ct, S)[name])
        assert np.array_equal(y, together[name]), name
    y = run(calls(sl, ct, S)["pressure"])
    assert ((y != y0) & m & on).any() and np.array_equal(y[~m], together["pressure"][~m])
    assert not (run(calls(sl, ct, S)["contact tangent"]) != y0)[m].any()
    sl.destroy(); ct.destroy(); S.destroy(); U.destroy(); DU.destroy()
