"""bench.py --dump-outputs DIR: y of the last timed step as float64 .npy files -- a fixed seeded sample of a large vector with its
positions, and a summary of the whole vector -- so that two builds can be compared output for output.  The writer is checked here on
a CPU tensor; the device run calls the same function on the device's y."""
import numpy as np
import torch

import bench


def test_small_vectors_are_dumped_whole(tmp_path):
    y = torch.linspace(-1.0, 2.0, 1000, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "out"), y, 0, 1)
    vals, idx, summ = (np.load(tmp_path / "out" / f) for f in ("y.npy", "y_index.npy", "y_summary.npy"))
    assert vals.dtype == idx.dtype == summ.dtype == np.float64
    assert np.array_equal(idx, np.arange(1000)) and np.array_equal(vals, y.numpy())
    assert summ[0] == 1000 and np.isclose(summ[1], np.linalg.norm(y.numpy())) and np.isclose(summ[2], y.numpy().sum()) and summ[3] == 2.0


def test_large_vectors_are_sampled_the_same_way_every_run():
    n, k = 20_000_000, bench.DUMP_ENTRIES
    a, b = bench.dump_sample_index(n, k), bench.dump_sample_index(n, k)
    assert np.array_equal(a, b) and len(a) == k and len(np.unique(a)) == k and a[0] >= 0 and a[-1] < n
    assert np.all(np.diff(a) > 0)
    assert 2 * 8 * k <= 64 * 2 ** 20            # values + positions stay within 64 MB


def test_ranks_write_their_own_share(tmp_path):
    y = torch.arange(10, dtype=torch.float64)
    for r in (0, 1):
        bench.dump_outputs(str(tmp_path), y + r, r, 2)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f"{s}_rank{r}.npy" for s in ("y", "y_index", "y_summary") for r in (0, 1))
    assert np.array_equal(np.load(tmp_path / "y_rank1.npy"), np.arange(10) + 1.0)
