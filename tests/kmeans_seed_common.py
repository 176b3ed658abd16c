"""Shared by test_gpu_kmeans_seed.py and test_kmeans_seed_cpu.py: the numpy float64 restatement of the greedy k-means++ step rule of
include/sgl_kmeans_seed.h, and the inputs of the float-row tests."""
import numpy as np

from kmeans_common import BLOBS

FLOAT_CASES = tuple((BLOBS[b], trials, seed) for b, trials, seed in ((0, 1, 11), (0, 3, 12), (1, 3, 13), (1, 5, 14), (3, 2, 15), (3, 8, 16)))
MARGIN = 1e-9            # relative room the float-row inputs must leave at every draw and between the two lowest potentials


def draws_table(k, trials, seed):
    """the table kmeans(init="greedy-k-means++", seed=seed) draws for its first run"""
    import torch
    return torch.rand((k, trials), generator=torch.Generator().manual_seed(seed), dtype=torch.float64).numpy()


def seed_reference(distance_to, n, k, trials, draws):
    """(centre_ids, near float32 [n], pot float64 [k], margin): distance_to(row) -> float32 [n] squared distances of all rows to one.
    margin: the smallest |cum - t| / pot over the draws and the smallest relative gap between the two lowest potentials of a step"""
    near, cand = np.full(n, np.inf, dtype=np.float32), [min(int(draws[0, 0] * n), n - 1)]
    ids, pots, margin = [], [], np.inf
    finite64 = lambda v: np.where(np.isfinite(v), v, 0).astype(np.float64)
    for j in range(k):
        trial = [np.minimum(near, distance_to(c)) for c in cand]              # NaN where either is NaN
        pot = np.array([finite64(t).sum() for t in trial])
        best = int(np.argmin(pot))                                            # the lowest on a tie
        if len(pot) > 1 and pot[best] > 0:
            margin = min(margin, (np.sort(pot)[1] - pot[best]) / pot[best])
        near = trial[best]
        ids.append(cand[best]), pots.append(pot[best])
        if j + 1 < k:
            cum, t = np.cumsum(finite64(near)), draws[j + 1, :trials] * pot[best]
            cand = [int(c) for c in np.minimum(np.searchsorted(cum, t, side="right"), n - 1)]   # the first row with cum > t
            if pot[best] > 0:
                margin = min(margin, np.abs(cum[:, None] - t[None, :]).min() / pot[best])
    return np.array(ids, dtype=np.int64), near, np.array(pots), margin
