"""What the CPU and the device tests of the block-vector operations share: blocks with a poisoned padding, the references in extended
precision (np.longdouble: products and sums carry 64 bits, so the reference's own error n 2^-64 is far below the bounds), and the
bounds, which are derived and not measured (u = 2^-53):

    Gram:     |G_ij - ref| <= (n + 4) u sum_r |w a b|        recursive summation in ANY order, plus the weight and product roundings
    combine:  |Y - ref|    <= (ka + 3) u (sum_i |a_i c_ij| + |beta y|)   per entry
"""
import numpy as np

U_ROUND = 2.0 ** -53


def make_block(ceed, n, k, ld, seed, poison=True):
    """(BlockVector, its columns [k][n] as a host array): uniform(-1, 1) entries, the padding rows n <= r < ld filled with NaN."""
    b = ceed.block(n, k, ld)
    rng = np.random.default_rng(seed)
    cols = rng.uniform(-1.0, 1.0, (k, n))
    if poison and ld > n:
        import torch
        full = np.full((k, ld), np.nan)
        full[:, :n] = cols
        b.t.copy_(torch.from_numpy(full.reshape(-1)))
        if b.on_device:
            torch.cuda.current_stream().synchronize()
        b.touched()
    else:
        b.fill(cols)
    return b, cols


def padding_bits(b):
    """The bit patterns of the padding rows, [k][ld - n] as uint64."""
    if b.on_device:
        b.ceed.synchronize()
    return b.t.cpu().numpy().reshape(b.k, b.ld)[:, b.n:].copy().view(np.uint64)


def gram_reference(A, B, w=None):
    """(ref, bound) of G = A diag(w) B' for host arrays [ka][n], [kb][n]"""
    n = A.shape[1]
    wl = np.ones(n, dtype=np.longdouble) if w is None else w.astype(np.longdouble)
    Al, Bl = A.astype(np.longdouble), B.astype(np.longdouble)
    ref = (Al * wl[None, :]) @ Bl.T
    mag = (np.abs(A) * (np.ones(n) if w is None else np.abs(w))[None, :]) @ np.abs(B).T
    return ref, (n + 4) * U_ROUND * mag


def combine_reference(Y, A, Cm, beta):
    """(ref, bound) of Y_j = sum_i A_i Cm[i][j] + beta Y_j for host arrays [ky][n], [ka][n], [ka][ky]; beta == 0 ignores Y"""
    ka = A.shape[0]
    ref = Cm.astype(np.longdouble).T @ A.astype(np.longdouble)
    mag = np.abs(Cm).T @ np.abs(A)
    if beta != 0.0:
        ref = ref + np.longdouble(beta) * Y.astype(np.longdouble)
        mag = mag + abs(beta) * np.abs(Y)
    return ref, (ka + 3) * U_ROUND * mag


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the entries (0 where the bound is 0 and the entry exact)"""
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    assert np.all(np.isfinite(got))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))
    return float(ratio.max())
