"""The snes_rtol pair of the own- vs fine-quadrature solve comparisons (test_coarse_quadrature*.py), derived from the recorded Newton
history of a FINE-quadrature solve at the solver's default tolerance.

The comparisons measure "what the Newton tolerance leaves open" as the distance between two fine-quadrature solves at snes_rtol and
snes_rtol / 10.  Newton converges quadratically here, so at the default 1e-8 both stop at the same iterate and that distance is exactly
zero.  The pair is therefore put where it straddles one residual of the fine history: the looser solve stops at the last-but-one iterate
of every load increment, the tighter one goes on to the last."""
import numpy as np


def straddling_snes_rtol(stats):
    """snes_rtol such that, in EVERY load increment of the recorded solve, the last-but-one Newton iterate meets snes_rtol (and the one
    before it does not) but misses snes_rtol / 10.  `stats`: SolveStats of a converged solve with at least two steps per increment."""
    hi, lo, before = 0.0, np.inf, np.inf
    for inc, r0 in enumerate(stats.initial_residuals, start=1):
        rel = [h[4] / r0 for h in stats.history if h[0] == inc]
        assert len(rel) >= 2, "the comparison needs at least two Newton steps per load increment"
        hi, lo = max(hi, rel[-2]), min(lo, rel[-2])
        before = min(before, rel[-3] if len(rel) >= 3 else 1.0)
    rtol = float(np.sqrt(hi * 10.0 * lo))              # the middle (in the exponent) of [hi, 10 lo)
    assert hi <= rtol < 10.0 * lo and rtol < before, (hi, lo, before)
    return rtol
