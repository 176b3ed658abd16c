"""Shared by test_gpu_kmeans.py and test_kmeans_cpu.py (importable without a GPU), and by golden/make_g16_node_clustering.py: the
inputs of the k-means tests and their float64 references -- computed once per (d, k) and left unchanged.

Tolerances (none is chosen from what the kernel returns).  A distance is a d-term fmaf sum of squared ROUNDED differences: one
rounding of the difference (2 relative roundings of its square), at most d roundings of the running sum of non-negative terms,
one more for the final lane sums' order: (d + 3) 2^-24 relative, first order.  Two distances of a row can therefore change order
only when, in float64, (d2 - d1) <= tau d2 with tau = 2 x 2 x (d + 3) 2^-24 = (d + 3) 2^-22 -- twice the sum of the two bounds; such
rows are `near a tie` and left out of the label comparison, at most 1 % of a case.  mindist is held to (d + 3) 2^-23 relative."""
import numpy as np
import torch

from inputs import hash_matrix

N_ROWS = 1031
WIDTHS = (1, 3, 4, 7, 12, 16, 31, 32, 33, 64, 100, 128, 147, 256, 257, 500, 600, 1030)
KS = (1, 2, 7, 47, 64)
# k * d beyond one 64 KiB tile (16384 floats), beyond two; an odd width in several tiles; the two register capacities the widths above
# leave out (4 and 8 vectors per lane); rows beyond the register layouts (d > 2048)
BIG = ((600, 64), (1030, 64), (257, 130), (1000, 3), (1800, 3), (2500, 9))
LAYOUTS = ("padded", "odd_view", "last_row")
MAX_LEFT_OUT = 0.01
POISONS = (float("nan"), 1e30)


def tau(d):
    return (d + 3) * 2.0 ** -22


def dist_tol(d):
    return (d + 3) * 2.0 ** -23


_X, _REF = {}, {}


def host_x(d, n=N_ROWS):
    """[n, d] float32 normal data; beyond 8 columns the first 8 have a standard deviation of 2 sqrt(d / 8), the rest 1.  Why: the
    squared distances of ISOTROPIC normal rows to k centres concentrate at 2 d +- sqrt(8 d) while tau grows with d, so from d = 600
    on more than 1 % of such rows sit near a tie in the float64 reference itself (11 of 1031 at d = 600, k = 7; 14 at d = 1030).
    With four fifths of the energy in 8 directions the distances of a row spread over about half their mean, at every d, and a
    plain column still carries 1 / (5 d) of a distance: more than the tolerance of mindist up to d = 1030"""
    if (d, n) not in _X:
        x = np.random.default_rng(1000 + d).standard_normal((n, d))
        if d > 8:
            x[:, :8] *= 2.0 * np.sqrt(d / 8.0)
        _X[(d, n)] = x.astype(np.float32)
    return _X[(d, n)]


def host_centres(d, k, n=N_ROWS):
    """k rows of host_x(d) plus 0.01 noise"""
    rng = np.random.default_rng(7000 + 131 * d + k)
    rows = rng.choice(n, k, replace=k > n)
    return (host_x(d, n)[rows] + 0.01 * rng.standard_normal((k, d))).astype(np.float32)


def distances64(x, c):
    """[n, k] float64 squared distances, centre by centre (no [n, k, d] temporary)"""
    x64 = np.asarray(x, dtype=np.float64)
    return np.stack([((x64 - np.asarray(cj, dtype=np.float64)) ** 2).sum(1) for cj in c], axis=1) if x64.shape[1] else np.zeros((len(x), len(c)))


def reference(d, k):
    """(labels, mindist, near_tie) of host_x(d) against host_centres(d, k) in float64"""
    if (d, k) not in _REF:
        dist = distances64(host_x(d), host_centres(d, k))
        labels = dist.argmin(1)
        d1 = dist[np.arange(len(dist)), labels]
        if k > 1:
            d2 = np.partition(dist, 1, axis=1)[:, 1]
            near = (d2 - d1) <= tau(d) * d2
        else:
            near = np.zeros(len(dist), dtype=bool)
        _REF[(d, k)] = (labels.astype(np.int64), d1, near)
    return _REF[(d, k)]


def cases():
    return [(d, k) for d in WIDTHS for k in KS] + list(BIG)


def in_layout(host, layout, device):
    """the [n, d] matrix on the device as a view of a buffer whose pad holds NaN and 1e30:
    padded    rows on a pitch of round_up(d, 4) + 4 floats from an aligned base (16-byte lanes);
    odd_view  columns 1 .. d of a [n, d + 3] buffer (4-byte lanes);
    last_row  a pitch of round_up(d, 4) whose storage ends with column d of the last row (16-byte lanes; the last row's straddling
              vector must be read element by element)"""
    n, d = host.shape
    src = torch.from_numpy(host).to(device)
    if layout == "odd_view":
        buf = torch.empty((n, d + 3), dtype=torch.float32, device=device)
        buf[:, 0::2], buf[:, 1::2] = POISONS[0], POISONS[1]
        view = buf[:, 1:d + 1]
    elif layout == "padded":
        pitch = (d + 3) // 4 * 4 + 4
        buf = torch.empty((n, pitch), dtype=torch.float32, device=device)
        buf[:, 0::2], buf[:, 1::2] = POISONS[0], POISONS[1]
        view = buf[:, :d]
    elif layout == "last_row":
        pitch = (d + 3) // 4 * 4
        flat = torch.empty(max(n - 1, 0) * pitch + d, dtype=torch.float32, device=device)
        flat[0::2], flat[1::2] = POISONS[0], POISONS[1]
        view = torch.as_strided(flat, (n, d), (pitch, 1))
    else:
        raise ValueError(layout)
    view.copy_(src)
    return view


# ---- the blob sets of fixture (a): regenerated, not stored (integer hash and IEEE + and x only: the same bits on every machine) ----
BLOBS = ((600, 16, 3, 3.0), (1500, 100, 7, 1.0), (3000, 100, 47, 1.0), (1200, 24, 5, 0.6))
BLOB_SEEDS = {(600, 16, 3): 160, (1500, 100, 7): 171, (3000, 100, 47): 162, (1200, 24, 5): 163}


def _unit_noise(n, d, seed):
    """sum of three uniform [-1, 1) hash matrices: mean 0, variance 1, bell-shaped"""
    return sum(hash_matrix(n, d, seed=seed + s).astype(np.float64) for s in (0, 1, 2))


def blob_set(n, d, k, spread):
    """(x float32 [n, d], generating labels int64 [n], c0 float32 [k, d]): centres spread * unit noise, points centre + unit noise,
    c0 = k distinct seeded rows of x"""
    seed = BLOB_SEEDS[(n, d, k)] * 1000
    centres = spread * _unit_noise(k, d, seed)
    y = np.minimum(((hash_matrix(n, 1, seed=seed + 10)[:, 0].astype(np.float64) + 1.0) * 0.5 * k).astype(np.int64), k - 1)
    x = (centres[y] + _unit_noise(n, d, seed + 20)).astype(np.float32)
    rows = np.argsort(hash_matrix(n, 1, seed=seed + 30)[:, 0], kind="stable")[:k]
    return x, y, x[rows].copy()
