"""The p-multigrid V-cycle of solver.NewtonPMG and the flexible PCG around it on the device against dense references formed on the CPU
oracle (tests/_vcycle_dense.py; the same checks run on the oracle alone, with the controls, in tests/test_vcycle_dense.py): per case
the V-cycle as ONE matrix in the default form (fused consumers, eager) against its closed form within 1e-10, its symmetry and
definiteness, the eigenvalue estimates of the smoothers, fcg against a dense PCG; and the device's forms -- fused consumers or two
passes, each eager or replayed from a recording -- bitwise on 32 columns.

Measured on an MI355X (default form; |B - B_ref| / max|B_ref|, |B - B^T| / max|B|, emax / lambda_max over the smoothing levels, fcg
against dense PCG iterations, cond(A)):

  case  free dofs  |B - B_ref|  asymmetry  emax / lambda_max  fcg / dense  cond(A)
  a     252        3.0e-15      3.5e-16    0.9958 .. 1.0000   16 / 16      2.8e3
  b     540        4.6e-15      5.1e-16    0.9726 .. 1.0000   19 / 19      5.5e3
  c     420        1.4e-15      3.5e-16    0.9900 .. 1.0000   14 / 14      1.6e3
  d1    420        2.2e-15      6.0e-16    0.9454 .. 0.9998   -            7.1e2
  d2    420        2.1e-15      8.7e-16    0.9454 .. 0.9998   -            7.1e2
  e     252        2.2e-15      5.4e-16    0.9949 .. 1.0000   15 / 15      2.8e3
  f     441        2.6e-15      4.1e-16    0.9962 .. 0.9999   19 / 19      2.6e3
  g     90         3.3e-15      4.3e-16    0.9939 .. 1.0000   19 / 19      1.6e3
  h     252        2.0e-15      1.7e-16    0.9874 .. 1.0000   11 / 11      4.1e2
  a40   252        3.0e-15      4.1e-16    0.9958 .. 1.0000   16 / 16      2.8e3

The solutions of fcg lie within 6.5e-13 of the refined A^-1 b; the one-level preconditioners within 6.1e-16 of M^-1; the factors of
case a (sweep, residual, restriction, prolongation per level) within 2.9e-15 of theirs.  Every form of every case gave the bits of
the default form on its 32 columns.  The bounds are five orders wider than the device needs: they are the project's, and still seven
orders under the smallest seeded fault of the controls (2.5e-3)."""
import pytest

import _vcycle_dense as vd

pytestmark = pytest.mark.gpu

FORM_CASES = [name for name in vd.CASES if name not in ("d1", "a40")]


@pytest.mark.parametrize("degree,multigrid", [(3, "uniform"), (4, "logarithmic")])
def test_prolongation_reproduces_affine_fields(gpu, degree, multigrid):
    vd.affine_prolongation_check(gpu, degree, multigrid, "device")


@pytest.mark.parametrize("name", list(vd.CASES))
def test_vcycle_and_pcg_against_the_dense_references(gpu, oracle, name):
    vd.vcycle_check(gpu, oracle, name, "device")


@pytest.mark.parametrize("smoother", ["jacobi", "pbjacobi"])
def test_one_level_preconditioner_is_the_inverted_smoother_matrix(gpu, oracle, smoother):
    vd.one_level_check(gpu, oracle, smoother, "device")


def test_factors_of_the_recursion_one_by_one(gpu, oracle):
    out = vd.factors_check(gpu, oracle, "a", "device")
    assert len(out) == 8


@pytest.mark.parametrize("name", FORM_CASES)
def test_forms_of_the_vcycle_give_the_same_bits(gpu, name):
    same = vd.forms_check(gpu, name)
    assert len(same) == (1 if vd.CASES[name]["opts"]["coarse"] == "cg" or vd.CASES[name].get("level0") else 3)
