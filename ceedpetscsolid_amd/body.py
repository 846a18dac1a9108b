"""A body and its loads: what the quasi-static solve (solver.NewtonPMG) and the implicit and explicit time steppers (dynamics.py) share,
and nothing of how a system is solved.  ``LoadedBody`` holds the problem, its element partition over several ranks (halo.py: interface
sums, owner-weighted dots), the boundary values (src/boundary.c), the load vector, the follower pressures (surface.py), the contact
surfaces with their stored state (contact.py), the spring and dashpot supports with their states (support.py), the static
residual and the tangent apply ``A`` in its plain form.  It owns every vector made through ``_vec``, its surface loads and its contact surfaces: ``destroy()``
releases them, and what it was handed (the problem, the halos, a caller's RcclHalo list) stays the caller's."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, Optional

import numpy as np

from .solid import SolidProblem


# ---- boundary functions (src/boundary.c) -------------------------------------------------------
def bc_mms(X: np.ndarray, load: float) -> np.ndarray:
    """BCMMS, boundary.c:31-50."""
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    return np.stack([np.exp(2 * x) * np.sin(3 * y) * np.cos(4 * z), np.exp(3 * y) * np.sin(4 * z) * np.cos(2 * x),
                     np.exp(4 * z) * np.sin(2 * x) * np.cos(3 * y)], axis=1) / 1e8 * load


def bc_clamp(X: np.ndarray, load: float, translate=(0., 0., 0.), axis=(0., 0., 1.), angle_over_pi: float = 0.0) -> np.ndarray:
    """BCClamp, boundary.c:53-74: translation + rotation about `axis` by angle_over_pi*pi, scaled by the load
    fraction.  The x-component's (1-c) term is reproduced AS WRITTEN at boundary.c:69
    (`-ky*ky + kz*kz*x + ...`)."""
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    lx, ly, lz = (t * load for t in translate)
    kx, ky, kz = axis
    th = angle_over_pi * np.pi * load
    c, s = np.cos(th), np.sin(th)
    u0 = lx + s * (-kz * y + ky * z) + (1 - c) * (-ky * ky + kz * kz * x + kx * ky * y + kx * kz * z)
    u1 = ly + s * (kz * x + -kx * z) + (1 - c) * (kx * ky * x - (kx * kx + kz * kz) * y + ky * kz * z)
    u2 = lz + s * (-ky * x + kx * y) + (1 - c) * (kx * kz * x + ky * kz * y - (kx * kx + ky * ky) * z)
    return np.stack([u0, u1, u2], axis=1)


@dataclass
class SolveStats:
    newton_its: int = 0
    ksp_its: int = 0
    coarse_its: int = 0
    jacobian_applies: int = 0
    coarse_spmv: int = 0
    residual_evals: int = 0
    seconds: float = 0.0
    increments: int = 0
    converged: bool = True
    history: list = field(default_factory=list)
    initial_residuals: list = field(default_factory=list)   # |R| at the start of every load increment (what snes_rtol is relative to)


class LoadedBody:
    def __init__(self, prob: SolidProblem, clamp: Optional[Dict[int, dict]] = None, mms: bool = False, forcing=None, halo=None,
                 rccl="auto", traction: Optional[Dict[int, tuple]] = None, pressure: Optional[Dict[int, float]] = None,
                 pressure_tangent: str = "full", verbose: bool = False, contact: Optional[Dict[int, dict]] = None,
                 contact_tangent: str = "levels", support: Optional[Dict[int, dict]] = None,
                 traction_field: Optional[Dict[int, object]] = None, pressure_field: Optional[Dict[int, object]] = None,
                 hydrostatic: Optional[Dict[int, dict]] = None, density=None, gravity=None, acceleration_field=None,
                 spin: Optional[dict] = None, thermal: Optional[dict] = None):
        """Thermal load (thermal.py; one rank): ``thermal`` = dict(alpha=, theta=, tangent="full") -- a nodal temperature change theta
        from the stress-free state (a float, an array (nnodes,) of the fine level, or a callable of its node coordinates) with the
        linearised coefficient of expansion alpha; theta scales with the load fraction, like ``forcing``.  linElas, hyperSS: the dead
        load +int beta theta_h div v is folded once into the load vector.  hyperFS: the term follows the body -- ``has_followers()`` is
        true, every residual adds load R_theta(x) (``follower_add``), and with tangent "full" its exact, symmetric tangent
        load T_theta(x) goes to ``A_outer`` only: the multigrid levels and smoothers do not see it, as with ``pressure_tangent``
        ("none" omits it).  No stiffness is added on the levels, so ``ExplicitDynamics.stable_dt`` is what it was.
        Body loads (mass.py; one rank): ``density`` -- a positive float or a ``mass.DensityField`` -- is required by the three below.
        ``gravity``: (gx, gy, gz), an acceleration; the load int rho N g = M_rho (tile g), through the mass apply with mask mode 2, is
        folded once into the load vector and scaled by the load fraction like ``forcing``.
        ``acceleration_field``: array (nnodes, 3) | callable(X) -> (n, 3), a nodal acceleration b_h; the load M_rho b_h likewise
        (inertia relief: a rigid-body acceleration field is linear in X and lies in the space).
        ``spin``: dict(omega=, axis=(0, 0, 1), origin=(0, 0, 0), follow=True, tangent="full") -- the centrifugal load
        rho Omega^2 P (X + u - c), P = I - a a^T.  The part at X is dead and folded in once; with ``follow`` the part in u is added in
        every residual (``follower_add``, scaled by the load fraction), and with tangent "full" its tangent -load Omega^2 M_rho P --
        symmetric, negative semi-definite: the spin softening -- goes to ``A_outer`` only: the multigrid levels and smoothers do not
        see it, as with ``pressure_tangent``.
        ``clamp``: {side_set_id: dict(translate=(..), axis=(..), angle_over_pi=..)} as
        -bc_clamp_<id>_translate / _rotate (cloptions.c:86-131); ids present in the problem's Dirichlet
        set but absent here are held at zero.
        Surface loads (surface.py; one rank, and never on a clamped side set):
        ``traction``: {side_set_id: (tx, ty, tz)} -- a dead load per unit REFERENCE area acting on the body in the direction t, scaled by
        the load fraction like the body force; evaluated once and folded into the load vector.
        ``pressure``: {side_set_id: p} -- a pressure on the CURRENT surface, p > 0 pushing on the body, scaled by the load fraction;
        evaluated in every residual, R = F_int(u) - load (f + sum_s g_s^traction) + load sum_s p_s g_s^pressure(u).
        ``pressure_tangent``: "full" adds load sum_s p_s T_s(u) to ``A_outer`` (the Jacobian of an outer Krylov iteration; ``A``, and
        with it a V-cycle, its smoothers, diagonals and eigenvalue estimates, do not see it); "none" omits it (modified Newton).
        T(u) is symmetric only on the variations that vanish on the rim of the loaded surface: a closed surface, or
        a patch whose rim is clamped (a tube with clamped ends).  A CG iteration assumes a symmetric operator; a follower pressure on a
        patch with a free rim is the caller's responsibility, as with any non-conservative load.
        Loads that vary over a side set (surface.py, "Fields"; the rules, the load scaling and the symmetry caveat of the two above):
        ``traction_field``: {side_set_id: array (nnodes, 3) | callable(X) -> (n, 3)} -- a dead traction per unit reference area given
        at the fine level's nodes and interpolated over the faces; folded once into the load vector, like ``traction``.
        ``pressure_field``: {side_set_id: array (nnodes,) | callable(X) -> (n,)} -- a pressure given at the nodes (it rides with the
        material points) on the CURRENT surface; added in every residual like ``pressure``.
        ``hydrostatic``: {side_set_id: dict(gamma=, level=, up=(0, 0, 1))} -- the pressure gamma <level - e . x> of a fluid of weight
        gamma per unit volume at rest up to ``level`` along the unit vector e = up / |up|, the depth taken at the CURRENT position of
        every point; added in every residual.  A callable is evaluated once, on the fine level's ``node_coords``.  With
        ``pressure_tangent="full"`` the exact tangents of the two followers go to ``A_outer`` beside the constant pressure's.
        ``contact``: {side_set_id: dict(plane=(x0, n) | sphere=(c, R, s), penalty=eps, travel=(0, 0, 0))} -- frictionless penalty
        contact of the side set with a rigid obstacle (contact.py: g > 0 separated, n the unit normal from the obstacle to the body,
        s = +1 a ball, -1 a cavity, eps per unit reference area).  The contact term is NOT scaled by the load fraction; only the
        obstacle moves with it: x0 or c at load l is x0 + l travel.  Every residual adds r(u) and refreshes the contact state, which the
        tangent reads: ``contact_tangent`` "levels" (solver.NewtonPMG: C in every matrix-free level's operator and diagonal) or "outer"
        (C in ``A_outer`` only, the follower pressure's form).  One rank, and never on a clamped side set.
        ``support``: {side_set_id: dict(kn=0., kt=0., cn=0., ct=0.)} -- linear supports of the side set (support.py): springs kn (normal)
        and kt (tangential) and dashpots cn, ct, all per unit REFERENCE area and fixed in the reference configuration.  NOT scaled by the
        load fraction.  The residual adds the spring force K_s x (x with its boundary values) and ``A`` the spring tangent K_s on every
        level it is asked for; the dashpot force C_d v is the time steppers' (dynamics.py).  One rank, and never on a clamped side set."""
        self.p, self.ceed, self.L = prob, prob.ceed, prob.ceed.L
        self.verbose = verbose
        self.nlev = len(prob.levels)
        # Several ranks (one element partition per rank, halo.py): `halo` is one HaloExchange per multigrid level (a single one stands
        # for a one-level list).  Every vector then aliases a torch tensor (host memory for the CPU oracle, device memory otherwise;
        # the Ceed's stream must be torch's current stream, as in bench.py), so the interface sums of halo.add() act on the operators'
        # outputs in place: the L -> G sum of matops.c:57 after each Jacobian / residual / transfer / diagonal.  Dots are owner-weighted.
        single = halo is not None and not isinstance(halo, (list, tuple))
        halo = [halo] if single else halo
        many = self._several_ranks(halo)
        if traction or pressure or traction_field or pressure_field or hydrostatic:
            # partial face sums at the interface nodes would need the exchange between the add and its consumer
            self._refuse_several_ranks(halo, "surface loads (traction=, pressure=, traction_field=, pressure_field=, hydrostatic=) are"
                                       if (traction_field or pressure_field or hydrostatic) else "surface loads (traction=, pressure=) are",
                                       "the face sums of the interface nodes are not summed over the ranks")
        if contact:
            self._refuse_several_ranks(halo, "contact surfaces (contact=) are", "the face sums of the interface nodes are not summed over the ranks")
        if support:
            self._refuse_several_ranks(halo, "supports (support=) are", "the face sums of the interface nodes are not summed over the ranks")
        if thermal is not None:
            self._refuse_several_ranks(halo, "thermal loads (thermal=) are",
                                       "the element sums at the interface nodes have not been run over several ranks")
        if many and single and self.nlev > 1:
            raise ValueError("a multi-rank multigrid solve needs one HaloExchange per level")
        if many and len(halo) != self.nlev:
            raise ValueError("one HaloExchange per multigrid level expected")
        self.halos = list(halo) if many else None
        self.halo = self.halos[-1] if self.halos else None
        self.clamp, self.mms = clamp or {}, mms
        # the library's exchange per level (halo.RcclHalo), or None: torch.distributed point-to-point + index ops
        self.rhalos, self._own_rhalos = None, []
        if self.halos:
            if isinstance(rccl, (list, tuple)):
                self.rhalos = list(rccl)
            elif rccl == "auto":
                import torch.distributed as dist
                if dist.is_initialized() and dist.get_backend(self.halos[-1].group) == "nccl" and self.halos[-1].device.type == "cuda":
                    from .halo import RcclHalo
                    self.rhalos = self._own_rhalos = [RcclHalo(self.ceed, h) for h in self.halos]
            if self.rhalos is not None and len(self.rhalos) != self.nlev:
                raise ValueError("one RcclHalo per multigrid level expected")
        self._vectors = []                           # every vector made by _vec: what destroy() releases
        self._x0 = {}
        n, top = prob.lsize(), self.nlev - 1
        self.R, self.Xloc, self.bcv = (self._vec(n, top) for _ in range(3))
        self.free = prob.levels[prob.fine].mask == 0
        self.weights = [None] * self.nlev
        if self.halos:
            for lv in range(self.nlev):
                wv = self._vec(prob.lsize(lv), lv)
                self._set(wv, self.halos[lv].owner_weight * (prob.levels[lv].mask == 0))
                self.weights[lv] = wv
                self._refresh_multiplicity(lv)
        # body force vector (opSetupForce output, setuplibceed.c:555-583): SNESSolve(snes, F, U) solves
        # residual(U) = load * F on the unconstrained dofs (elasticity.c:645-654)
        self.fv = None
        if forcing is not None:
            self.fv = self._vec(n, top)
            self._set(self.fv, np.asarray(forcing, dtype=np.float64) * self.free)
            self._halo_sum(top, self.fv)
        self.load = 1.0
        self.stats = SolveStats()
        self._bc_nodes = self._collect_bc_nodes()
        self._setup_surface_loads(traction, pressure, pressure_tangent)
        self._setup_surface_fields(traction_field, pressure_field, hydrostatic)
        self._setup_contact(contact, contact_tangent)
        self._setup_support(support)
        self._setup_body_loads(density, gravity, acceleration_field, spin, halo)
        self._setup_thermal(thermal, halo)

    # ---- thermal load (thermal.py) ------------------------------------------------------------
    def _setup_thermal(self, thermal, halo):
        """With no thermal= given nothing here runs and no thermal operator is made."""
        self.thermal = None                          # the ThermalLoad of the fine level
        self.thermal_follows = False                 # hyperFS: added in every residual
        self.thermal_tangent = "full"
        if thermal is None:
            return
        if not isinstance(thermal, dict) or set(thermal) - {"alpha", "theta", "tangent"} or not {"alpha", "theta"} <= set(thermal):
            raise ValueError("thermal: dict(alpha=, theta=, tangent='full') expected")
        tangent = thermal.get("tangent", "full")
        if tangent not in ("full", "none"):
            raise ValueError(f"thermal: tangent must be 'full' or 'none', not {tangent!r}")
        from .thermal import ThermalLoad
        prob = self.p
        n, top = prob.lsize(), self.nlev - 1
        self.thermal = ThermalLoad(prob, prob.fine, thermal["alpha"], thermal["theta"], prob.problem)
        self.thermal_tangent = tangent
        if prob.problem == "hyperFS":
            self.thermal_follows = True
            return
        out = self._vec(n, top)
        self.thermal.force(None, out)                # masked rows are stored as zeros: fv stays zero on the constrained dofs
        if self.fv is None:
            self.fv = self._vec(n, top)
        self.axpby(self.fv, -1.0, out, 1.0)          # R = F_int - load fv: the share R_theta of the residual is -fv's

    # ---- body loads (mass.py) -----------------------------------------------------------------
    def _setup_body_loads(self, density, gravity, acceleration_field, spin, halo):
        """With none of gravity=, acceleration_field=, spin= given nothing here runs and no mass operator is made."""
        self.body_mass = None                        # M_rho of the fine level, mask mode 2: the loads read the vectors as they are
        self.spin = None                             # dict(omega2, follow, tangent, blocks, px, mp) of a spinning body
        if gravity is None and acceleration_field is None and spin is None:
            return
        if density is None:
            raise ValueError("gravity=, acceleration_field= and spin= need density= (a positive float or a mass.DensityField)")
        self._refuse_several_ranks(halo, "body loads (gravity=, acceleration_field=, spin=) are",
                                   "the mass operator's sums at the interface nodes have not been run over several ranks")
        from .mass import DensityField, MassOperator
        prob, lv = self.p, self.p.levels[self.p.fine]
        n, top, nn = prob.lsize(), self.nlev - 1, lv.dofmap.nnodes
        X = np.asarray(lv.dofmap.node_coords, dtype=np.float64)
        field = density if isinstance(density, DensityField) else None
        if field is None and not (isinstance(density, (int, float, np.integer, np.floating)) and np.isfinite(density) and density > 0.0):
            raise ValueError(f"density must be a positive float or a mass.DensityField, not {density!r}")
        b = np.zeros((nn, 3))
        if gravity is not None:
            g = np.asarray(gravity, dtype=np.float64).reshape(-1)
            if g.size != 3 or not np.all(np.isfinite(g)):
                raise ValueError("gravity: three finite components (gx, gy, gz) expected")
            b += g
        if acceleration_field is not None:
            a = np.asarray(acceleration_field(X) if callable(acceleration_field) else acceleration_field, dtype=np.float64)
            if a.shape != (nn, 3) or not np.all(np.isfinite(a)):
                raise ValueError(f"acceleration_field: a finite array of shape {(nn, 3)} expected (one row per node of the fine level), "
                                 f"not {a.shape}")
            b += a
        if spin is not None:
            if not isinstance(spin, dict) or set(spin) - {"omega", "axis", "origin", "follow", "tangent"} or "omega" not in spin:
                raise ValueError("spin: dict(omega=, axis=(0, 0, 1), origin=(0, 0, 0), follow=True, tangent='full') expected")
            ax = np.asarray(spin.get("axis", (0.0, 0.0, 1.0)), dtype=np.float64).reshape(-1)
            c0 = np.asarray(spin.get("origin", (0.0, 0.0, 0.0)), dtype=np.float64).reshape(-1)
            om, tangent = float(spin["omega"]), spin.get("tangent", "full")
            if ax.size != 3 or c0.size != 3 or not np.isfinite(om) or not np.all(np.isfinite(ax)) or not np.all(np.isfinite(c0)) or not ax @ ax > 0.0:
                raise ValueError("spin: a finite omega, a non-zero axis and an origin of three components each expected")
            if tangent not in ("full", "none"):
                raise ValueError(f"spin: tangent must be 'full' or 'none', not {tangent!r}")
            ax = ax / np.sqrt(ax @ ax)
            Pm = np.eye(3) - np.outer(ax, ax)
            b += om * om * (X - c0) @ Pm                 # (P is symmetric) the dead part, at the reference position
        self.body_mass = MassOperator(prob, prob.fine, 1.0 if field is not None else float(density), mask_mode=2, density=field)
        full = np.zeros(n)                               # (an L-vector may be longer than 3 nnodes: a caller's numbering)
        full[:3 * nn] = b.reshape(-1)
        bv, out = self._vec(n, top), self._vec(n, top)
        self._set(bv, full)
        self.body_mass.apply(bv, out)                    # masked rows are stored as zeros: fv stays zero on the constrained dofs
        if self.fv is None:
            self.fv = out
        else:
            self.axpby(self.fv, 1.0, out, 1.0)
        if spin is not None and spin.get("follow", True):
            blocks = self._vec(3 * n, top)               # P on every node: the point-block multiply forms P u nodewise
            self._set(blocks, np.tile(Pm.reshape(-1), n // 3))
            self.spin = dict(omega2=om * om, tangent=tangent, blocks=blocks, px=bv, mp=self._vec(n, top))

    def _spin_add(self, x, y):
        """y -= load Omega^2 M_rho P x on the free rows (x read as it is).  The sign: the residual is R = F_int - load f + followers,
        and the centrifugal force +rho Omega^2 P u acts ON the body, so its share of R (``follower_add``'s "R += load g(x)" with
        g = -Omega^2 M_rho P x) and of the tangent is negative.  ``px`` is the scratch vector the load was set up in, free since."""
        from .ceed import pointblock_mult
        s = self.spin
        pointblock_mult(s["px"], s["blocks"], x)
        self.body_mass.apply(s["px"], s["mp"])           # masked rows are zeros: y keeps its own there
        self.axpby(y, -self.load * s["omega2"], s["mp"], 1.0)

    # ---- several ranks ------------------------------------------------------------------------
    @staticmethod
    def _several_ranks(halo) -> bool:
        hl = halo if halo is None or isinstance(halo, (list, tuple)) else [halo]
        return bool(hl) and hl[-1].world > 1

    @classmethod
    def _refuse_several_ranks(cls, halo, who: str, why: str):
        if cls._several_ranks(halo):
            raise ValueError(f"{who} not provided with a halo (several ranks): {why}")

    @staticmethod
    def _load_function(load) -> Callable[[float], float]:
        """The load fraction as a function of time: ``load`` itself, or the constant it states."""
        return load if callable(load) else (lambda t, v=float(load): v)

    # ---- surface loads (surface.py) -----------------------------------------------------------
    def _setup_surface_loads(self, traction, pressure, pressure_tangent):
        """With no surface load given nothing here runs beyond the argument checks, and no solve takes a new path."""
        if pressure_tangent not in ("full", "none"):
            raise ValueError(f"pressure_tangent must be 'full' or 'none', not {pressure_tangent!r}")
        self.pressure_tangent = pressure_tangent
        self.pressure_loads = []                     # (SurfaceLoad, p) per loaded side set
        self.surface_loads = []                      # every SurfaceLoad made here (destroy_surface_loads)
        if not traction and not pressure:
            return
        from .mesh import side_set_nodes
        from .surface import SurfaceLoad
        prob, lv = self.p, self.p.levels[self.p.fine]
        for sid in list(traction or {}) + list(pressure or {}):
            if sid not in prob.mesh.side_sets:
                raise ValueError(f"surface load on side set {sid}: the mesh has no such side set")
            nodes = side_set_nodes(prob.mesh, lv.dofmap, [sid])
            if sid in prob.bc_sides or (nodes.size and lv.mask.reshape(-1, 3)[nodes].all()):
                raise ValueError(f"surface load on side set {sid}, which is one of the problem's Dirichlet side sets")
        n, top = prob.lsize(), self.nlev - 1
        make = lambda sid: SurfaceLoad(self.ceed, prob.mesh, lv.dofmap, [sid], Q=prob.Q, mask=lv.mask)
        for sid, t in (traction or {}).items():
            t = np.asarray(t, dtype=np.float64).reshape(-1)
            if t.size != 3:
                raise ValueError(f"traction on side set {sid}: three components expected")
            if self.fv is None:
                self.fv = self._vec(n, top)
            sl = make(sid)
            sl.traction_add(t, 1.0, self.fv)         # masked rows are never written: fv stays zero on the constrained dofs
            self.surface_loads.append(sl)
        for sid, pval in (pressure or {}).items():
            sl = make(sid)
            self.pressure_loads.append((sl, float(pval)))
            self.surface_loads.append(sl)

    def _setup_surface_fields(self, traction_field, pressure_field, hydrostatic):
        """The loads that vary over a side set.  With none of them given nothing here runs, and no solve takes a new path."""
        self.field_loads = []                        # the followers: ("pressure_field", SurfaceLoad, Vector) | ("hydrostatic", SurfaceLoad, (gamma, level, up))
        if not traction_field and not pressure_field and not hydrostatic:
            return
        from .mesh import side_set_nodes
        from .surface import SurfaceLoad, check_hydrostatic
        prob, lv = self.p, self.p.levels[self.p.fine]
        for sid in list(traction_field or {}) + list(pressure_field or {}) + list(hydrostatic or {}):
            if sid not in prob.mesh.side_sets:
                raise ValueError(f"surface load on side set {sid}: the mesh has no such side set")
            nodes = side_set_nodes(prob.mesh, lv.dofmap, [sid])
            if sid in prob.bc_sides or (nodes.size and lv.mask.reshape(-1, 3)[nodes].all()):
                raise ValueError(f"surface load on side set {sid}, which is one of the problem's Dirichlet side sets")
        n, top, nn = prob.lsize(), self.nlev - 1, lv.dofmap.nnodes

        def nodal(what, sid, f, shape):
            """The field as a flat array over the fine level's nodes: an array of ``shape``, or a callable of the node coordinates."""
            f = np.asarray(f(lv.dofmap.node_coords) if callable(f) else f, dtype=np.float64)
            if f.shape != shape:
                raise ValueError(f"{what} on side set {sid}: an array of shape {shape} expected (one entry per node of the fine level), "
                                 f"not {f.shape}")
            if not np.all(np.isfinite(f)):
                raise ValueError(f"{what} on side set {sid}: the field is not finite")
            full = np.zeros(n if len(shape) == 2 else n // 3)       # (an L-vector may be longer than 3 nnodes: a caller's numbering)
            full[:f.size] = f.reshape(-1)
            return full
        make = lambda sid: SurfaceLoad(self.ceed, prob.mesh, lv.dofmap, [sid], Q=prob.Q, mask=lv.mask)
        # every argument is checked before the first object is made
        tfields = {sid: nodal("traction_field", sid, f, (nn, 3)) for sid, f in (traction_field or {}).items()}
        pfields = {sid: nodal("pressure_field", sid, f, (nn,)) for sid, f in (pressure_field or {}).items()}
        hydro = {}
        for sid, spec in (hydrostatic or {}).items():
            if not isinstance(spec, dict) or set(spec) - {"gamma", "level", "up"} or "gamma" not in spec or "level" not in spec:
                raise ValueError(f"hydrostatic on side set {sid}: dict(gamma=, level=, up=(0, 0, 1)) expected")
            up = tuple(float(v) for v in np.asarray(spec.get("up", (0.0, 0.0, 1.0)), dtype=np.float64).reshape(-1))
            check_hydrostatic(spec["gamma"], spec["level"], up)
            hydro[sid] = (float(spec["gamma"]), float(spec["level"]), up)
        for sid, t in tfields.items():
            if self.fv is None:
                self.fv = self._vec(n, top)
            sl, tv = make(sid), self._vec(n, top)
            self._set(tv, t)
            sl.traction_field_add(tv, 1.0, self.fv)  # masked rows are never written: fv stays zero on the constrained dofs
            self.surface_loads.append(sl)
        for sid, pf in pfields.items():
            sl, pv = make(sid), self._vec(n // 3, top)
            self._set(pv, pf)
            self.field_loads.append(("pressure_field", sl, pv))
            self.surface_loads.append(sl)
        for sid, par in hydro.items():
            sl = make(sid)
            self.field_loads.append(("hydrostatic", sl, par))
            self.surface_loads.append(sl)

    def has_followers(self) -> bool:
        """Whether a load follows the body: a constant pressure, a pressure field, a hydrostatic pressure, a spin with follow=True or a
        thermal load in the finite-strain model."""
        return bool(self.pressure_loads or self.field_loads or self.spin or self.thermal_follows)

    def follower_add(self, x, R):
        """R += load sum_s g_s(x) over every load that follows the surface, x the position's displacement WITH its boundary values.
        The one place the static, the Newmark and the explicit residual add them (constrained rows are not written)."""
        for sl, pval in self.pressure_loads:
            sl.pressure_add(pval, self.load, x, R)
        for kind, sl, par in self.field_loads:
            if kind == "pressure_field":
                sl.pressure_field_add(par, self.load, x, R)
            else:
                sl.hydrostatic_add(par[0], par[1], par[2], self.load, x, R)
        if self.spin:                                  # the centrifugal load grows with the radius the points have moved to
            self._spin_add(x, R)
        if self.thermal_follows:                       # theta scales with the load fraction
            self.thermal.set_scale(self.load)
            self.thermal.force(x, R, add=True)

    def follower_tangent_add(self, x, dx, y):
        """y += load sum_s T_s(x) dx, the exact tangents of ``follower_add``."""
        for sl, pval in self.pressure_loads:
            sl.tangent_add(pval, self.load, x, dx, y)
        for kind, sl, par in self.field_loads:
            if kind == "pressure_field":
                sl.pressure_field_tangent_add(par, self.load, x, dx, y)
            else:
                sl.hydrostatic_tangent_add(par[0], par[1], par[2], self.load, x, dx, y)

    def spin_tangent_add(self, dx, y):
        """y -= load Omega^2 M_rho P dx: the spin softening, linear in dx and independent of the state (masked entries of dx are zero
        in a Krylov vector; masked rows are not written)."""
        if self.spin and self.spin["tangent"] == "full":
            self._spin_add(dx, y)

    def thermal_tangent_add(self, x, dx, y):
        """y += load T_theta(x) dx, the exact tangent of the finite-strain thermal term (masked entries of dx read as zero, masked rows
        are not written)."""
        if self.thermal_follows and self.thermal_tangent == "full":
            self.thermal.set_scale(self.load)
            self.thermal.tangent(x, dx, y, add=True)

    # ---- contact with a rigid obstacle (contact.py) -------------------------------------------
    def _setup_contact(self, contact, contact_tangent):
        """With no contact given nothing here runs beyond the argument check, and no solve takes a new path."""
        if contact_tangent not in ("levels", "outer"):
            raise ValueError(f"contact_tangent must be 'levels' or 'outer', not {contact_tangent!r}")
        self.contact_tangent = contact_tangent
        self.contacts = []          # per side set: dict(sid, kind, at, rest, travel, penalty, state, levels={level: ContactSurface})
        if not contact:
            return
        from .contact import ContactSurface, obstacle_parameters
        from .mesh import side_set_nodes
        prob, top = self.p, self.nlev - 1
        lv = prob.levels[prob.fine]
        for sid, spec in contact.items():
            if sid not in prob.mesh.side_sets:
                raise ValueError(f"contact on side set {sid}: the mesh has no such side set")
            nodes = side_set_nodes(prob.mesh, lv.dofmap, [sid])
            if sid in prob.bc_sides or (nodes.size and lv.mask.reshape(-1, 3)[nodes].all()):
                raise ValueError(f"contact on side set {sid}, which is one of the problem's Dirichlet side sets")
            unknown = set(spec) - {"plane", "sphere", "penalty", "travel"}
            if unknown or "penalty" not in spec:
                raise ValueError(f"contact on side set {sid}: dict(plane=(x0, n) | sphere=(c, R, s), penalty=eps, travel=(0, 0, 0)) expected")
            obstacle_parameters(spec.get("plane"), spec.get("sphere"))          # (refuses what the library would)
            if not float(spec["penalty"]) > 0.0:
                raise ValueError(f"contact on side set {sid}: the penalty {float(spec['penalty']):g} is not positive")
            travel = np.asarray(spec.get("travel", (0.0, 0.0, 0.0)), dtype=np.float64).reshape(-1)
            if travel.size != 3:
                raise ValueError(f"contact on side set {sid}: travel has three components")
            kind = "plane" if spec.get("plane") is not None else "sphere"
            at, rest = np.asarray(spec[kind][0], dtype=np.float64).reshape(3), tuple(spec[kind][1:])
            fine = ContactSurface(self.ceed, prob.mesh, lv.dofmap, [sid], prob.Q, mask=lv.mask)
            self.contacts.append(dict(sid=sid, kind=kind, at=at, rest=rest, travel=travel, penalty=float(spec["penalty"]),
                                      state=fine.new_state(), levels={top: fine}, placed=None))

    def _place_obstacles(self):
        """The obstacles at the current load fraction: x0 + load travel."""
        for c in self.contacts:
            if c["placed"] != self.load:
                c["levels"][self.nlev - 1].set_obstacle(penalty=c["penalty"], **{c["kind"]: (c["at"] + self.load * c["travel"],) + c["rest"]})
                c["placed"] = self.load

    def contact_tangent_add(self, lv, x, y):
        """y += sum_s C_s x with level lv's tables on the state of the last residual evaluation."""
        for c in self.contacts:
            c["levels"][lv].tangent_add(1.0, c["state"], x, y)

    def _contact_gaps(self) -> np.ndarray:
        return np.concatenate([c["levels"][self.nlev - 1]._gaps(c["state"]).reshape(-1) for c in self.contacts]) if self.contacts else np.zeros(0)

    def min_gap(self) -> float:
        """The smallest gap over all contact points at the last residual evaluation (negative: the largest penetration)."""
        g = self._contact_gaps()
        return float(g.min()) if g.size else float("inf")

    def active_fraction(self) -> float:
        """The share of the contact points in contact (g < 0) at the last residual evaluation."""
        g = self._contact_gaps()
        return float((g < 0.0).mean()) if g.size else 0.0

    def destroy_contacts(self):
        for c in self.contacts:
            for cs in c["levels"].values():
                cs.destroy()
            c["state"].destroy()
        self.contacts = []

    # ---- spring and dashpot supports (support.py) ---------------------------------------------
    def _setup_support(self, support):
        """With no support given nothing here runs, and no solve takes a new path."""
        self.supports = []          # per side set: dict(sid, kn, kt, cn, ct, spring=state | None, dashpot=state | None, levels={level: SupportSurface})
        if not support:
            return
        from .mesh import side_set_nodes
        from .support import SupportSurface
        prob, top = self.p, self.nlev - 1
        lv = prob.levels[prob.fine]
        for sid, spec in support.items():
            if sid not in prob.mesh.side_sets:
                raise ValueError(f"support on side set {sid}: the mesh has no such side set")
            nodes = side_set_nodes(prob.mesh, lv.dofmap, [sid])
            if sid in prob.bc_sides or (nodes.size and lv.mask.reshape(-1, 3)[nodes].all()):
                raise ValueError(f"support on side set {sid}, which is one of the problem's Dirichlet side sets")
            if not isinstance(spec, dict) or set(spec) - {"kn", "kt", "cn", "ct"}:
                raise ValueError(f"support on side set {sid}: dict(kn=0., kt=0., cn=0., ct=0.) expected")
            co = {k: float(spec.get(k, 0.0)) for k in ("kn", "kt", "cn", "ct")}
            if not all(v >= 0.0 and np.isfinite(v) for v in co.values()):
                raise ValueError(f"support on side set {sid}: the coefficients {co} are not finite and non-negative")
            if not any(v > 0.0 for v in co.values()):
                raise ValueError(f"support on side set {sid}: all four coefficients are zero")
            fine = SupportSurface(self.ceed, prob.mesh, lv.dofmap, [sid], prob.Q, mask=lv.mask)
            s = dict(sid=sid, spring=None, dashpot=None, levels={top: fine}, **co)
            for name, a, b in (("spring", co["kn"], co["kt"]), ("dashpot", co["cn"], co["ct"])):
                if a > 0.0 or b > 0.0:
                    s[name] = fine.new_state()
                    fine.form_state(a, b, s[name])
            self.supports.append(s)

    def _support_surface(self, s, lv):
        """The support's surface on level lv (that level's dofmap and mask, the fine Q), made when first asked for."""
        if lv not in s["levels"]:
            from .support import SupportSurface
            level = self.p.levels[lv]
            s["levels"][lv] = SupportSurface(self.ceed, self.p.mesh, level.dofmap, [s["sid"]], self.p.Q, mask=level.mask)
        return s["levels"][lv]

    def _support_tangent_state(self, s):
        """The state whose B^T K_q B is the support's share of the tangent: the springs' (dynamics.NewmarkPMG: K_s + a1 C_d); or None."""
        return s["spring"]

    def support_tangent_add(self, lv, x, y):
        """y += the supports' tangent on level lv applied to x."""
        for s in self.supports:
            st = self._support_tangent_state(s)
            if st is not None:
                self._support_surface(s, lv).tangent_add(1.0, st, x, y)

    def support_diagonal_add(self, lv, d):
        """d += the diagonal of the supports' tangent on level lv."""
        for s in self.supports:
            st = self._support_tangent_state(s)
            if st is not None:
                self._support_surface(s, lv).diagonal_add(1.0, st, d)

    def support_force_add(self, which, x, y):
        """y += K_s x (``which`` "spring") or C_d x ("dashpot") on the fine level; x is read as it is."""
        for s in self.supports:
            if s[which] is not None:
                s["levels"][self.nlev - 1].force_add(1.0, s[which], x, y)

    def has_dashpots(self) -> bool:
        return any(s["dashpot"] is not None for s in self.supports)

    def destroy_supports(self):
        for s in self.supports:
            for sf in s["levels"].values():
                sf.destroy()
            for k in ("spring", "dashpot", "combined"):
                if s.get(k) is not None:
                    s[k].destroy()
        self.supports = []

    def destroy_surface_loads(self):
        for sl in self.surface_loads:
            sl.destroy()
        self.surface_loads, self.pressure_loads, self.field_loads = [], [], []

    def destroy(self):
        """Release what this object made: its vectors, its surface loads and the RcclHalos of rccl="auto".  Idempotent; a subclass
        releases its own first and ends with super().destroy()."""
        self.destroy_surface_loads()
        self.destroy_contacts()
        self.destroy_supports()
        if self.body_mass is not None:
            self.body_mass.destroy()
        self.body_mass = self.spin = None
        if self.thermal is not None:
            self.thermal.destroy()
        self.thermal, self.thermal_follows = None, False
        for o in self._vectors + self._own_rhalos:
            o.destroy()
        self._vectors, self._own_rhalos, self._x0 = [], [], {}

    # ---- vector helpers ---------------------------------------------------------------------
    def axpby(self, y, a, x, b):
        y.axpby(a, x, b)

    def copy(self, dst, src):
        dst.axpby(1.0, src, 0.0)

    def dot(self, x, y, fine_weight=False, lv=None) -> float:
        """x . y; on several ranks each dof counts once (owner weights of level `lv`, default the fine level)."""
        lv = self.nlev - 1 if lv is None else lv
        if self.rhalos:      # the sum over the ranks on the device (ncclAllReduce on the Ceed's stream), ONE read at the end
            sc = self.ceed.scalars
            x.dot_to(y, sc, 7, self.weights[lv])
            self.ceed.all_reduce(sc, 7, 1)
            return float(sc.to_numpy()[7])
        v = x.dot(y, self.weights[lv])
        if self.halos:
            import torch, torch.distributed as dist
            t = torch.tensor([v], dtype=torch.float64, device="cpu" if self.halos[lv].device.type == "cpu" or self.halos[lv].stage_host else self.halos[lv].device)
            dist.all_reduce(t, group=self.halos[lv].group)
            v = float(t.item())
        return v

    def _vec(self, n, lv):
        """A zeroed vector of this object's (several ranks: one that aliases a torch tensor)."""
        v = self.ceed.tensor_vector(n, self.halos[lv].device) if self.halos else self.ceed.vector(n).set_value(0.0)
        self._vectors.append(v)
        return v

    def _set(self, vec, arr):
        """vec := arr (host array), keeping the torch alias intact."""
        vec.fill(arr)

    def _halo_sum(self, lv, vec):
        """Interface sum of an operator output at level lv (the DMLocalToGlobal(ADD_VALUES) of matops.c:57)."""
        if self.rhalos:               # the library's exchange, on the Ceed's stream: nothing to synchronise, nothing to re-wrap
            self.rhalos[lv].add(vec)
        elif self.halos:
            if vec.t.device.type == "cuda":
                self.ceed.synchronize()
            self.halos[lv].add(vec.t)
            vec.touched()

    def _refresh_multiplicity(self, lv):
        """multVec of misc.c:115-143 counted over ALL ranks: 1 / (halo-summed element multiplicity)."""
        level = self.p.levels[lv]
        m = self._vec(self.p.lsize(lv), lv)
        level.Erestrictu.multiplicity(m)
        self._halo_sum(lv, m)
        self._set(level.multinv, 1.0 / m.to_numpy())

    def _start_vector(self, lv):
        """The start vector of an eigenvalue estimate on level lv (free dofs only, norm 1), drawn once per level; no BLAS on the host
        (a threaded BLAS call leaves its worker pool spinning, which starves a CPU-quota'd process for ~0.1 s a call)."""
        if lv not in self._x0:
            free = self.p.levels[lv].mask == 0
            if self.halos:   # shared nodes must get the same value on every rank: a hash of the coordinates
                X = self.p.levels[lv].dofmap.node_coords
                k = np.array([[12.9898, 78.233, 37.719], [93.989, 67.345, 24.113], [45.164, 11.135, 83.951]])
                v = np.sin(X @ k.T) * 437.5453
                x = (2.0 * (v - np.floor(v)) - 1.0).reshape(-1) * free
            else:
                x = np.random.default_rng(1234 + lv).uniform(-1, 1, free.size) * free
            x0 = self._vec(free.size, lv)
            self._set(x0, x / np.sqrt(np.square(x).sum()))     # (any positive scale: the iteration renormalises)
            self._x0[lv] = x0
        return self._x0[lv]

    # ---- operators ---------------------------------------------------------------------------
    def A(self, lv, x, y):
        """y = the tangent of level lv at the stored state applied to x, summed over the interfaces."""
        self.p.apply_jacobian(lv, x, y)
        self.stats.jacobian_applies += 1
        self._halo_sum(lv, y)
        if self.supports:
            self.support_tangent_add(lv, x, y)

    def A_outer(self, lv, x, y):
        """The Jacobian of the outer Krylov iteration: the level's operator plus load sum_s p_s T_s(u) x, the tangents of the pressure
        fields and the hydrostatic pressures likewise (and, with
        contact_tangent="outer", the contact tangent sum_s C_s x), u the state of the last
        residual evaluation (Xloc: free part + boundary values).  Masked entries of x read as zero and masked rows are not written,
        as in the volume operator."""
        self.A(lv, x, y)
        if self.pressure_tangent == "full":
            self.follower_tangent_add(self.Xloc, x, y)
        self.spin_tangent_add(x, y)
        self.thermal_tangent_add(self.Xloc, x, y)
        if self.contacts and self.contact_tangent == "outer":
            self.contact_tangent_add(lv, x, y)

    def _collect_bc_nodes(self):
        from .mesh import side_set_nodes
        lv = self.p.levels[self.p.fine]
        return {sid: side_set_nodes(self.p.mesh, lv.dofmap, [sid]) for sid in self.clamp}

    def bc_values(self, load: float) -> np.ndarray:
        """DMPlexInsertBoundaryValues at `time = loadIncrement` (matops.c:70-72)."""
        lv = self.p.levels[self.p.fine]
        v = np.zeros((lv.dofmap.nnodes, 3))
        if self.mms:
            nodes = np.nonzero(lv.mask.reshape(-1, 3)[:, 0])[0]
            v[nodes] = bc_mms(lv.dofmap.node_coords[nodes], load)
        for sid, par in self.clamp.items():
            nodes = self._bc_nodes[sid]
            v[nodes] = bc_clamp(lv.dofmap.node_coords[nodes], load, **par)
        return (v.reshape(-1) * (lv.mask != 0))

    def residual(self, U, R):
        """FormResidual_Ceed: Xloc = free part of U + boundary values; R = F(Xloc), constrained rows dropped."""
        self.copy(self.Xloc, U)
        self.axpby(self.Xloc, 1.0, self.bcv, 1.0)
        self.p.form_residual(self.Xloc, R)
        self._halo_sum(self.nlev - 1, R)
        if self.fv is not None:
            self.axpby(R, -self.load, self.fv, 1.0)
        self.follower_add(self.Xloc, R)                # follower loads on the current surface (constrained rows are not written)
        if self.contacts:                              # contact is not scaled by the load: only the obstacle travels with it
            self._place_obstacles()
            for c in self.contacts:
                c["levels"][self.nlev - 1].residual_add(1.0, self.Xloc, R, c["state"])
        if self.supports:                              # the spring force reads the boundary values too; not scaled by the load
            self.support_force_add("spring", self.Xloc, R)
        self.stats.residual_evals += 1
