"""The contact inputs the contact tests share, and their input condition.

Obstacles are placed from the geometry alone (the positions of the Gauss points under the tables of ``surface.lagrange_tables``), never
from what the code under test returns:

  plane   normal ∝ (0.2, -0.1, 1) through the centroid of the surface's nodes, shifted 0.013 along the normal (NOT through the centroid:
          that put a Gauss point at |g| ~ 1e-17);
  sphere  centre at that centroid moved 0.6 of the surface's largest extent along the same direction, so that the ball dents the middle
          of a flat patch; the radius in the middle of the widest empty interval of the points' distances from the centre between the
          30 % and the 60 % quantile.  s = +1 (ball) then has that share of the points active, s = -1 (cavity) the rest.

Input condition (asserted by every test that uses these inputs, before anything else): for the portable form min |g| >= 1e-6 over all
Gauss points and between 10 % and 90 % of them active.
"""
import numpy as np

DIRECTION = np.array([0.2, -0.1, 1.0]) / np.linalg.norm([0.2, -0.1, 1.0])
OBSTACLES = ("plane", "ball", "cavity")
PENALTY = 7.0


def displacement(dm, P, Q):
    """u = 0.1 uniform(-1, 1) with seed 100 P + Q, and a variation |du| <= 1 from the same generator."""
    rng = np.random.default_rng(100 * P + Q)
    return 0.1 * rng.uniform(-1, 1, dm.lsize), rng.uniform(-1, 1, dm.lsize)


def _surface_nodes(cs):
    return cs.Xh.reshape(-1, 3)[np.unique(cs.faces)]


def plane_for(cs):
    return _surface_nodes(cs).mean(axis=0) + 0.013 * DIRECTION, DIRECTION


def sphere_for(cs, u, s):
    X = _surface_nodes(cs)
    c = X.mean(axis=0) + 0.6 * np.ptp(X, axis=0).max() * DIRECTION
    x = np.einsum("ai,bj,fjic->fbac", cs.B, cs.B, cs._gather(cs.Xh) + cs._gather(u))
    r = np.sort(np.linalg.norm(x - c, axis=-1).reshape(-1))
    lo, hi = int(0.3 * r.size), max(int(0.6 * r.size), int(0.3 * r.size) + 1)
    k = lo + int(np.argmax(np.diff(r)[lo:hi]))                    # r[k] < R < r[k + 1]
    return c, 0.5 * (r[k] + r[k + 1]), float(s)


def set_obstacle(cs, which, u, penalty=PENALTY):
    """Give ``cs`` the obstacle ``which`` of OBSTACLES for the displacement ``u``; returns the keywords, for a second surface."""
    kw = {"plane": plane_for(cs)} if which == "plane" else {"sphere": sphere_for(cs, u, +1 if which == "ball" else -1)}
    cs.set_obstacle(penalty=penalty, **kw)
    return dict(kw, penalty=penalty)


def input_condition(ref, u):
    """(min |g|, active share) of the portable surface ``ref`` at ``u``, asserted to meet the input condition."""
    g = ref.gap_host(u)
    gmin, share = float(np.abs(g).min()), float((g < 0).mean())
    assert gmin >= 1e-6 and 0.1 <= share <= 0.9, (gmin, share)
    return gmin, share
