"""Explicit elastodynamics on the device: CeedXVectorLeapfrogStep (csrc/kernels_explicit.hip, ceed_explicit.cpp) against its portable form
bit for bit, the lumped mass, and dynamics.ExplicitDynamics against the same runs on the CPU oracle and against dense references.
Measured figures: profiles/explicit.txt."""
import itertools
import math
import os
import re

import numpy as np
import pytest

import _explicit_common as ec
from _mass_common import RHO
from conftest import ROOT
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.dynamics import ExplicitDynamics
from ceedpetscsolid_amd.mass import MassOperator
from ceedpetscsolid_amd.solver import NewtonPMG

pytestmark = pytest.mark.gpu

TOL = 1e-10                                   # the project's parity bound (tests/test_mass_gpu.py)
PAD = 5
COMBOS = list(itertools.product([True, False], [True, False], [0.0, 0.3]))          # f, tally, alpha


def stream_grid_cap():
    """The largest grid of the streaming kernels, read from the source (stream_grid in kernels_common.hpp)."""
    txt = open(os.path.join(ROOT, "ceedpetscsolid_amd", "csrc", "kernels_common.hpp")).read()
    m = re.search(r"b > (\d+) \? \1 : b", txt)
    assert m, "stream_grid's cap was not found in kernels_common.hpp"
    return int(m[1])


SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, 256 * stream_grid_cap() + 301]          # the last: a lane takes two rows


def test_entry_point_is_exported(gpu):
    assert gpu.L.has("CeedXVectorLeapfrogStep")


@pytest.mark.parametrize("n", SIZES)
def test_entry_point_against_the_portable_form(gpu, n):
    dt, load = 0.037, 0.8
    for k, (with_f, tally, alpha) in enumerate(COMBOS):
        c1, c2 = ec.coefficients(alpha, dt)
        a = ec.step_inputs(n, PAD, 100 + k, with_f)
        fa = None if a["f"] is None else a["f"][:n]
        x, vh = a["x"].copy(), a["vh"].copy()
        act = a["m"][:n] > 0.0
        cd.leapfrog_step_host(x[:n], vh[:n], a["r"][:n], fa, a["m"][:n], load, c1, c2, dt, False)
        vm = 0.5 * (a["vh"][:n][act] + vh[:n][act])
        terms = a["m"][:n][act] * (vm * vm)                    # the portable terms of the tally
        V = {key: gpu.vector(n + PAD).set_array(v) for key, v in a.items() if v is not None}
        S = gpu.vector(3).set_array(np.array([11.0, 12.0, 13.0]))
        got = []
        for _ in range(2):                                     # two calls from the same start: the same bits
            V["x"].set_array(a["x"]); V["vh"].set_array(a["vh"])
            V["x"].leapfrog_step(V["vh"], V["r"], V.get("f"), V["m"], load, c1, c2, dt, n, S if tally else None, 1)
            got.append((V["x"].to_numpy(), V["vh"].to_numpy(), S.to_numpy()))
        gx, gv, gs = got[0]
        assert gx.tobytes() == x.tobytes(), (n, with_f, tally, alpha)          # rows with m = 0, NaN rows and canaries included
        assert gv.tobytes() == vh.tobytes(), (n, with_f, tally, alpha)
        for key in ("r", "m") + (("f",) if with_f else ()):
            assert V[key].to_numpy().tobytes() == a[key].tobytes()
        assert all(g[i].tobytes() == got[0][i].tobytes() for g in got for i in range(3))
        assert (gs[0], gs[2]) == (11.0, 13.0)
        if tally:
            want = 0.5 * math.fsum(terms)
            bound = n * 2.0 ** -52 * 0.5 * math.fsum(np.abs(terms))
            assert np.isfinite(gs[1]) and abs(gs[1] - want) <= bound, (n, gs[1], want, bound)
            if act.any():
                assert gs[1] > 0.0
        else:
            assert gs[1] == 12.0
        for v in list(V.values()) + [S]:
            v.destroy()


def test_every_refusal_leaves_the_state_alone(gpu):
    n = 12
    V = {k: gpu.vector(n).set_value(1.0) for k in ("x", "vh", "r", "f", "m")}
    S, short = gpu.vector(2).set_value(0.0), gpu.vector(n - 1).set_value(1.0)
    L = gpu.L

    def call(**kw):
        a = {**V, **kw}
        h = lambda v: v.h if v is not None else None
        return L.lib.CeedXVectorLeapfrogStep(h(a["x"]), h(a["vh"]), h(a["r"]), h(a["f"]), h(a["m"]), cd.C.c_double(1.0), cd.C.c_double(1.0),
                                             cd.C.c_double(0.1), cd.C.c_double(0.1), cd.c_int(a.get("n", n)), h(a.get("scalars")),
                                             cd.c_int(a.get("slot", 0)))

    cases = [dict(x=None), dict(vh=None), dict(r=None), dict(m=None), dict(n=0), dict(n=-3), dict(n=n + 1), dict(r=short), dict(m=short),
             dict(f=short), dict(x=short, n=n), dict(vh=V["x"]), dict(r=V["x"]), dict(m=V["vh"]), dict(f=V["m"]), dict(f=V["r"]), dict(r=V["vh"]),
             dict(scalars=S, slot=2), dict(scalars=S, slot=-1), dict(scalars=V["r"]), dict(scalars=V["x"]), dict(scalars=V["f"])]
    for kw in cases:
        assert call(**kw) != 0, kw
        assert L.lib.CeedXLastError()
        for key in ("x", "vh"):
            if kw.get(key, V[key]) is V[key]:
                assert np.all(V[key].to_numpy() == 1.0), kw
    assert call(scalars=S, slot=1) == 0
    assert np.all(V["x"].to_numpy() == 1.0 + 0.1 * 1.0) and np.all(V["vh"].to_numpy() == 1.0)
    assert np.array_equal(S.to_numpy(), [0.0, 0.5 * n])
    for v in list(V.values()) + [S, short]:
        v.destroy()


@pytest.mark.parametrize("mesh,degree", [("box", 2), ("box", 4), ("cylinder", 2)])
def test_lumped_mass_against_the_portable_form(gpu, mesh, degree):
    prob = ec.box_problem(gpu, degree, "linElas") if mesh == "box" else ec.cylinder_problem(gpu, degree)
    n = prob.lsize()
    mask = prob.levels[prob.fine].mask != 0
    want = MassOperator(prob, prob.fine, RHO, portable=True, mask_mode=2).lumped_host()
    for mode in (2, 3):
        dev = MassOperator(prob, prob.fine, RHO, mask_mode=mode)
        assert not dev.portable
        D = gpu.vector(n + 4).set_value(7.0)
        dev.lumped(D)
        d = D.to_numpy()
        assert dev.kernel_name == f"mass<{degree + 1},{degree + 1}>"
        err = float(np.abs(d[:n] - want).max() / np.abs(want).max())
        print(f"lumped mass {mesh} p = {degree}, mask mode {mode}: device against portable {err:.2e}")
        assert err <= TOL
        assert np.all(d[:n][mask] == 0.0) and np.all(d[n:] == 0.0) and np.all(d[:n][~mask] > 0.0)
        if mode == 3:                                                   # the operator reads masked entries as zero again afterwards
            x = np.random.default_rng(3).uniform(-1, 1, n)
            X, Y = gpu.vector(n).set_array(x), gpu.vector(n)
            dev.apply(X, Y)
            ref3 = MassOperator(prob, prob.fine, RHO, portable=True, mask_mode=3)
            assert np.abs(Y.to_numpy() - np.where(mask, 0.0, ref3.apply_host(x))).max() <= TOL * np.abs(want).max()
            X.destroy(); Y.destroy()
        dev.destroy(); D.destroy()
    prob.destroy()


@pytest.mark.parametrize("degree", [2, 4])
def test_solver_against_the_same_run_on_the_oracle(gpu, oracle, degree):
    """hyperFS, 50 steps from rest under m (.) g, both with the oracle's dt.  A perturbation of the start grows by at most 8 over these steps,
    so rounding differences of 1e-15 per step stay far below the bound."""
    xo, moved_o, dt = ec.loaded_run(oracle, degree)
    xg, moved_g, dtg = ec.loaded_run(gpu, degree, dt=dt)
    assert dtg == dt
    err = float(np.abs(xg - xo).max() / moved_o)
    print(f"ExplicitDynamics p = {degree}: 50 steps at dt = {dt:.5f}, max |x - x_0| = {moved_o:.4f}, device against oracle {err:.2e}")
    assert 0.1 < moved_o < 0.6
    assert err <= TOL


def test_leapfrog_invariant_on_the_device(gpu, oracle):
    rprob = ec.box_problem(oracle, 2, "linElas")
    drift = ec.invariant_run(gpu, rprob, 2, 0.9)
    rprob.destroy()
    print(f"leapfrog invariant on the device, p = 2, 400 steps at 0.9 dt_crit: worst relative drift {drift:.2e}")
    assert drift <= TOL


def test_relaxation_on_the_device_reaches_the_oracles_static_solution(gpu, oracle):
    x, free, _ = ec.relaxation_run(gpu, 2)
    prob = ec.box_problem(oracle, 2, "hyperFS")
    probe = ExplicitDynamics(prob, RHO)
    st = NewtonPMG(prob, forcing=ec.body_load(probe.m.to_numpy()), snes_rtol=1e-12)
    assert st.solve(4).converged
    u = st.U.to_numpy()
    err = float(np.abs(x - u)[free].max())
    print(f"relaxation on the device p = 2: max |u| = {np.abs(u).max():.4f}, |x - static (oracle)| = {err:.2e}")
    assert err <= TOL * np.abs(u).max()
    probe.destroy(); prob.destroy()


@pytest.mark.parametrize("sample_every", [0, 5])
def test_replayed_steps_give_the_bits_of_eager_steps(gpu, sample_every):
    prob = ec.box_problem(gpu, 2, "hyperFS")
    probe = ExplicitDynamics(prob, RHO)
    f = ec.body_load(probe.m.to_numpy())
    out = []
    for graph in (False, True):
        sol = ExplicitDynamics(prob, RHO, damping=0.1, forcing=f)
        sol.set_initial()
        h = sol.run(11, sample_every=sample_every, graph=graph)              # graph: one eager step, ten replayed
        assert h["steps"] == 11 and sol.nsteps_done == 11 and abs(sol.t - 11 * sol.dt) < 1e-14
        out.append((sol.x.to_numpy(), sol.vh.to_numpy(), h["kinetic"], h["max_disp"]))
        sol.destroy()
    assert np.abs(out[0][0]).max() > 1e-3
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    assert out[0][2] == out[1][2] and out[0][3] == out[1][3] and len(out[0][2]) == (2 if sample_every else 0)
    sol = ExplicitDynamics(prob, RHO, forcing=f)
    sol.set_initial(load=lambda t: min(1.0, t))
    with pytest.raises(ValueError, match="constant load"):
        sol.run(3, graph=True)
    sol.destroy(); probe.destroy(); prob.destroy()
