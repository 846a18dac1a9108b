"""Rates of the block-vector kernels (k_block_gram, k_block_combine) beside the same Gram matrix formed by a loop of CeedXVectorDotTo
calls (the reduction the library had before), in one process: what profiles/modal.txt records.  Each figure is the median of
``--blocks`` timed blocks of ``--reps`` calls, each block between two synchronisations of the Ceed's stream.

    python tools/block_rates.py                       # n = 19 537 320 and 1 100 000; ka = kb = 8, 24, 48; combine 24 -> 8, 48 -> 16
    python tools/block_rates.py --n 1100000 --once gram --k 24    # one Gram matrix and nothing else (for a counter run)
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ceedpetscsolid_amd import ceed as cd

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="*", default=[19537320, 1100000]); ap.add_argument("--k", type=int, nargs="*", default=[8, 24, 48])
ap.add_argument("--blocks", type=int, default=5); ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--once", default=None, choices=["gram", "combine"], help="launch one call of this kind and exit")
ap.add_argument("--no-dots", action="store_true")
a = ap.parse_args()
c = cd.Ceed(cd.CeedLib(cd.PRODUCT_LIB), "/gpu/hip/mi355x")


def timed(fn, reps):
    fn(); c.synchronize()
    out = []
    for _ in range(a.blocks):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        c.synchronize()
        out.append((time.perf_counter() - t0) / reps)
    return float(np.median(out))


for n in a.n:
    kmax = max(a.k)
    A, B = c.block(n, kmax), c.block(n, kmax)
    for blk in (A, B):
        blk.t.uniform_(-1.0, 1.0)
        blk.touched()
    import torch
    torch.cuda.synchronize()
    G = c.vector(kmax * kmax).set_value(0.0)
    sc = c.vector(kmax * kmax).set_value(0.0)
    if a.once:
        k = a.k[0]
        if a.once == "gram":
            A.gram(B, G, ka=k, kb=k)
        else:
            A.combine(B, np.ones((k, max(k // 3, 1))), y0=0, ky=max(k // 3, 1), a0=0, ka=k)
        c.synchronize()
        sys.exit(0)
    for k in a.k:
        t = timed(lambda: A.gram(B, G, ka=k, kb=k), a.reps)
        gb = 2 * k * 8 * n / 1e9
        line = f"gram    n={n:9d} ka=kb={k:2d}: {1e3 * t:9.3f} ms  {gb / t / 1e3:6.3f} TB/s on (ka+kb) 8 n = {gb:7.3f} GB"
        if not a.no_dots:
            def dots():
                for i in range(k):
                    for j in range(k):
                        A[i].dot_to(B[j], sc, i * k + j)
            td = timed(dots, 1)
            line += f";  loop of {k * k:4d} CeedXVectorDotTo: {1e3 * td:9.3f} ms  ratio {td / t:6.1f}"
            err = np.abs(G.to_numpy()[:k * k] - sc.to_numpy()[:k * k]).max()
            line += f"  (max |block - dots| = {err:.2e})"
        print(line, flush=True)
    for ka, ky in ((24, 8), (48, 16)):
        if ka > kmax:
            continue
        Cm = c.vector(ka * ky).set_array(np.random.default_rng(0).uniform(-1, 1, ka * ky))
        for beta in (0.0, 1.0):
            t = timed(lambda: A.combine(B, Cm, y0=0, ky=ky, a0=0, ka=ka, beta=beta), a.reps)
            gb = (ka + ky + (ky if beta else 0)) * 8 * n / 1e9
            print(f"combine n={n:9d} {ka:2d}->{ky:2d} beta={beta:g}: {1e3 * t:9.3f} ms  {gb / t / 1e3:6.3f} TB/s on {gb:7.3f} GB", flush=True)
        Cm.destroy()
    A.destroy(); B.destroy(); G.destroy(); sc.destroy()
    del A, B
    torch.cuda.empty_cache()
