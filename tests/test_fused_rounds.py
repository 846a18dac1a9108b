"""The launch arithmetic of the fused kernel as tests/_fused_rounds.py restates it: the work list covers every group once whatever the
grid, and the meshes of tests/test_fused_rounds_gpu.py run the persistent group loop for several rounds on a 256-CU device with one
wave per CU -- and for one round with the default grid, which is why that file needs CEED_MI355X_PENCIL_WAVES."""
import os
import re
from itertools import chain

import numpy as np
import pytest

import _fused_rounds as fr

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ceedpetscsolid_amd", "csrc")
NCU = 256


def test_the_work_list_visits_every_group_exactly_once():
    for ngroups in range(1, 3001):
        for grid in (ngroups, 256, 512, 1024, 1536, 2048, 250):
            # every workgroup's walk expanded at once: its k-th group is lo + k step while that is < hi
            lo, hi, step = fr.walk_bounds(ngroups, grid)
            assert lo.size == grid
            n = np.maximum(0, (hi - lo + step - 1) // step)
            seen = np.repeat(lo, n) + step * (np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n))
            assert seen.size == ngroups and np.array_equal(np.bincount(seen, minlength=ngroups), np.ones(ngroups, dtype=np.int64)), (ngroups, grid)
            if ngroups % 250 == 0 or ngroups < 20:      # (the expansion above against the lists rounds() hands out)
                lists = fr.walk(ngroups, grid)
                assert len(lists) == grid and np.array_equal(seen, np.fromiter(chain.from_iterable(lists), dtype=np.int64))
            if grid % 8 == 0:           # a workgroup stays inside its XCD chunk
                chunk = (ngroups + 7) // 8
                c = np.arange(grid) % 8
                assert np.all((hi <= lo) | ((lo >= c * chunk) & (hi <= (c + 1) * chunk))), (ngroups, grid)


def test_a_launch_worked_by_hand():
    """20 elements at Q = 6 (one per group) on 16 CUs with one wave each: 16 workgroups, eight chunks of 3 groups, two wave ranks."""
    lists = fr.rounds(20, 6, 16, 1)
    assert len(lists) == 16
    assert lists[0] == [0, 2] and lists[8] == [1] and lists[1] == [3, 5] and lists[9] == [4]
    assert lists[6] == [18] and lists[14] == [19] and lists[7] == [] and lists[15] == []     # the last chunk begins behind the last group
    assert fr.rounds(20, 6, 16) == [[g] for g in range(20)]                                # 6 waves per CU: the grid capped at the groups
    assert fr.rounds(21, 5, 1, 3) == [[0, 3, 6, 9], [1, 4, 7, 10], [2, 5, 8]]              # 11 groups of 2, a grid of 3: one chunk


def test_waves_per_cu_and_group_sizes():
    assert [fr.pencil_waves_per_cu(Q) for Q in range(2, 9)] == [8, 8, 8, 8, 8, 6, 4]
    assert [fr.pencil_group_elems(Q) for Q in range(2, 9)] == [8, 4, 4, 2, 1, 1, 1]
    assert all(fr.pencil_lds_bytes(Q) <= fr.LDS_PER_CU for Q in range(2, 9))


def test_the_restated_constants_are_those_of_the_kernels_header():
    """The expressions of kernels.hpp this module restates, held as text: whoever changes one there is sent here."""
    with open(os.path.join(CSRC, "kernels.hpp")) as f:
        src = f.read()
    assert "constexpr int pencil_group_elems(int Q) { return Q <= 2 ? 8 : (Q <= 4 ? 4 : (Q == 5 ? 2 : 1)); }" in src
    assert "constexpr int pencil_lds_bytes(int Q) { return (pencil_group_elems(Q) * (9 * Q * Q * Q + (Q == 5 ? 5 : 1) + GEO_NCOEF) + 2 * Q) * 8; }" in src
    assert "const int by_lds = (160 * 1024) / pencil_lds_bytes(Q); return by_lds < 1 ? 1 : (by_lds > 4 * PENCIL_MINW ? 4 * PENCIL_MINW : by_lds);" in src
    assert int(re.search(r"constexpr int GEO_NCOEF = (\d+);", src)[1]) == fr.GEO_NCOEF
    assert int(re.search(r"constexpr int PENCIL_MINW = (\d+);", src)[1]) == fr.PENCIL_MINW
    with open(os.path.join(CSRC, "kernel_fused_pencil.hpp")) as f:
        launcher = f.read()
    assert "ncu * (l.waves_per_cu > 0 ? l.waves_per_cu : pencil_waves_per_cu(Q));" in launcher and "if (grid > ngroups) grid = ngroups;" in launcher
    with open(os.path.join(CSRC, "kernel_fused_pencil_body.hpp")) as f:
        body = f.read()
    for line in ("const int nxcd = gridDim.x % 8 == 0 ? 8 : 1;", "const int wrank = (int)blockIdx.x / nxcd, wper = (int)gridDim.x / nxcd;",
                 "const int gend = min(ngroups, (int)(blockIdx.x % nxcd + 1) * ((ngroups + nxcd - 1) / nxcd));",
                 "int grp = (int)(blockIdx.x % nxcd) * ((ngroups + nxcd - 1) / nxcd) + wrank;", "const int grp_nx = grp + wper;"):
        assert line in body, line


# size class -> (elements, groups, chunk of the first seven XCDs, the last chunk) with one wave per CU on 256 CUs
FIGURES = {"Q2": (4335, 542, 68, 66), "Q3-4": (2197, 550, 69, 67), "Q5": (1089, 545, 69, 62), "Q6-8": (567, 567, 71, 70)}


@pytest.mark.parametrize("cls", list(fr.SIZE_CLASSES))
@pytest.mark.parametrize("meshname", fr.MESHES)
def test_the_meshes_run_the_loop_with_one_wave_per_cu_and_not_by_default(cls, meshname):
    Q = fr.SIZE_CLASSES[cls]
    nelem, ngroups, chunk, last = FIGURES[cls]
    for Qc in (q for q in fr.SIZES if fr.SIZES[q] == fr.SIZES[Q]):      # every Q of the class: the same figures
        one = fr.describe(Qc, NCU, 1, meshname)
        assert (one["nelem"], one["ngroups"], one["grid"], one["nxcd"]) == (nelem, ngroups, 256, 8)
        assert one["chunks"] == [chunk] * 7 + [last]
        assert all(one["conditions"].values()), one
        assert set(one["hist"]) <= {1, 2, 3} and one["hist"][3] == 7 * (chunk - 64) + max(0, last - 64) and sum(k * v for k, v in one["hist"].items()) == ngroups
        ok, msg = fr.loop_runs(NCU, Qc, meshname)
        assert ok, msg
        dflt = fr.describe(Qc, NCU, 0, meshname)
        assert dflt["grid"] == ngroups and dflt["nxcd"] == 1 and dflt["hist"] == {1: ngroups} and ngroups % 8 != 0
        assert NCU * fr.pencil_waves_per_cu(Qc) >= 1024
        missed = {k for k, v in dflt["conditions"].items() if not v}
        # one round each: nothing of the loop-carried path runs (what remains true is that the sides own elements of round 0)
        assert missed == {k for k in dflt["conditions"] if not k.endswith("of round 0")}, dflt


def test_the_side_elements_are_those_of_the_meshes():
    for Q in (2, 5):
        for meshname in ("general", "swept1"):
            mesh, sides = fr.rounds_mesh(meshname, Q)
            want = fr.side_elements(meshname, Q)
            assert sides == sorted(want)
            for s in sides:
                assert np.array_equal(np.sort(np.asarray(mesh.side_sets[s])[:, 0]), want[s])


def test_a_device_that_runs_one_round_is_reported():
    ok, msg = fr.loop_runs(1024, 5)            # more CUs than groups per chunk allow: no third round
    assert not ok and "not met" in msg and "three rounds" in msg
