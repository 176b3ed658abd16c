"""The one-pass per-cluster sums (csrc/sgl_cluster_sums.hip, include/sgl_cluster_sums.h; device.cluster_sums, kmeans update="sums") on a
real MI355X: run with `-m gpu`.  The reference is numpy float64, the membership matrix times x.  Integer rows in [-8, 8] keep every
partial sum below 2^24: any order is exact and the sums must EQUAL it.  Float rows: the header's bound, (R + B) 2^-24 sum |x|."""
import ctypes

import numpy as np
import pytest
import torch

from kmeans_common import BLOBS, LAYOUTS, N_ROWS, blob_set, dist_tol, distances64, host_x, in_layout, tau
from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.tricks import kmeans

pytestmark = pytest.mark.gpu
WIDTHS = (1, 3, 4, 7, 33, 100, 128, 147, 600, 1030, 2500)
KS = (1, 2, 7, 47, 64, 130)
PREFIXES = (1, 63, 64, 65, 257)
_REF = {}


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def rule(n, d, k):
    out = (ctypes.c_int64 * 5)()
    _lib.check(_lib.lib().sgl_cluster_sums_rule(n, d, k, 1, out), "sgl_cluster_sums_rule")
    return tuple(out)                                                   # B, R, slab, S, LDS bytes


def hash_labels(n, k, variant="hash"):
    """a seeded hash mod k; "empty": cluster k - 1 (k >= 2) gets no row; "last": every row sits in cluster k - 1"""
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) >> np.uint64(7)) % np.uint64(1 << 20)
    return {"hash": h % k, "empty": h % max(k - 1, 1), "last": np.full(n, k - 1)}[variant].astype(np.int64)


def sums64(x, labels, k):
    keep = (labels >= 0) & (labels < k)
    member = np.zeros((k, len(x)))
    member[labels[keep], np.flatnonzero(keep)] = 1.0
    return member @ x.astype(np.float64), member.sum(1).astype(np.int64), member @ np.abs(x.astype(np.float64))


def integer_case(d, k, variant, n):
    """(x, labels, sums, counts) -- once per case, left unchanged"""
    if (d, k, variant, n) not in _REF:
        if ("x", d) not in _REF:
            _REF[("x", d)] = np.random.default_rng(500 + d).integers(-8, 9, (N_ROWS, d)).astype(np.float32)
        x, labels = _REF[("x", d)][:n], hash_labels(n, k, variant)
        _REF[(d, k, variant, n)] = (x, labels) + sums64(x, labels, k)[:2]
    return _REF[(d, k, variant, n)]


def same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", WIDTHS)
def test_exact_on_integer_rows(cuda, d, layout):
    if d == 2500:
        assert rule(N_ROWS, d, 130)[3] > 1 and rule(N_ROWS, d, 64)[3] > 1, "no case with more than one column slab is left"
    bad = []
    for k in KS:
        runs = [(v, N_ROWS, 0) for v in ("hash", "empty", "last")] + [("hash", n, 0) for n in PREFIXES] + [("hash", N_ROWS, 1), ("hash", N_ROWS, 3)]
        for variant, n, blocks in runs:
            x, labels, want, counts = integer_case(d, k, variant, n)
            try:                                                        # 1: one block over all rows; 3: the multi-block fold
                _lib.set_tuning("loss_blocks", blocks)
                if blocks:
                    assert rule(n, d, k)[0] == blocks
                got, got_counts = dev.cluster_sums(in_layout(x, layout, cuda), torch.from_numpy(labels).to(cuda), k)
            finally:
                _lib.set_tuning("loss_blocks", 0)
            if not (np.array_equal(got.cpu().numpy().astype(np.float64), want) and np.array_equal(got_counts.cpu().numpy(), counts)):
                bad.append((k, variant, n, blocks, int((got.cpu().numpy() != want).sum())))
    assert not bad, bad


@pytest.mark.parametrize("d,k", ((100, 47), (147, 7), (600, 64)))
def test_bound_and_invariants_on_float_rows(cuda, d, k):
    x, labels = host_x(d), hash_labels(N_ROWS, k)
    want, counts, mass = sums64(x, labels, k)
    blocks, rows = rule(N_ROWS, d, k)[:2]
    lab = torch.from_numpy(labels).to(cuda)
    got, got_counts = dev.cluster_sums(torch.from_numpy(x).to(cuda), lab, k)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    assert (err <= (rows + blocks) * 2.0 ** -24 * mass).all() and np.array_equal(got_counts.cpu().numpy(), counts)
    assert same(dev.cluster_sums(torch.from_numpy(x).to(cuda), lab, k)[0], got), "two runs differ"
    for layout in LAYOUTS:
        assert same(dev.cluster_sums(in_layout(x, layout, cuda), lab, k)[0], got), ("the layout shows", layout)

    holed = torch.from_numpy(x).to(cuda)
    holed[40, d // 2] = float("nan")                                    # reaches sums[labels[40], d // 2] and no other bit
    nan_sums = dev.cluster_sums(holed, lab, k)[0]
    hit = torch.zeros((k, d), dtype=torch.bool, device=cuda)
    hit[int(labels[40]), d // 2] = True
    assert bool(torch.isnan(nan_sums[hit]).all()) and same(nan_sums[~hit], got[~hit])

    try:                                                                # one block: the rows of a cluster in one chain, so skipping a row
        _lib.set_tuning("loss_blocks", 1)                               # and not having it are the same sum
        out_of_range = labels.copy()
        out_of_range[5], out_of_range[N_ROWS - 1] = -1, k
        skipped = dev.cluster_sums(torch.from_numpy(x).to(cuda), torch.from_numpy(out_of_range).to(cuda), k, check=False)
        keep = np.setdiff1d(np.arange(N_ROWS), (5, N_ROWS - 1))
        without = dev.cluster_sums(torch.from_numpy(x[keep]).to(cuda), torch.from_numpy(labels[keep]).to(cuda), k)
    finally:
        _lib.set_tuning("loss_blocks", 0)
    assert same(skipped[0], without[0]) and torch.equal(skipped[1], without[1])
    with pytest.raises(ValueError, match="outside"):
        dev.cluster_sums(torch.from_numpy(x).to(cuda), torch.from_numpy(out_of_range).to(cuda), k)

    buf = torch.full((k + 2, d + 3), -7.0, dtype=torch.float32, device=cuda)      # canaries around the outputs and in the pads of `sums`
    cbuf, xd = torch.full((k + 2,), -7, dtype=torch.int64, device=cuda), torch.from_numpy(x).to(cuda)
    scratch = torch.empty(int(dev._call(None, "sgl_cluster_sums_scratch", N_ROWS, d, k, raw=True)) // 4 + 1, dtype=torch.float32, device=cuda)
    dev._call(cuda, "sgl_cluster_sums_f32", _lib.ptr(xd), d, N_ROWS, d, _lib.ptr(lab), k, _lib.ptr(buf[1:]), d + 3, _lib.ptr(cbuf[1:]), _lib.ptr(scratch))
    assert same(buf[1:-1, :d].contiguous(), got) and torch.equal(cbuf[1:-1], got_counts)
    assert bool((buf[[0, -1]] == -7).all()) and bool((buf[:, d:] == -7).all()) and cbuf[0] == -7 and cbuf[-1] == -7


def rows_inside_the_perturbation(x, c0, k, max_iter=300):
    """a float64 Lloyd loop on the CPU: the rows, summed over the iterations, whose two nearest centres are closer than the float32
    assignment's rounding (tau) plus twice the centre perturbation e_j = (n_j + 1) 2^-24 |mean |x| of cluster j|_2 -- the longer of the
    two updates' chains -- can move them: (sqrt(d1) + sqrt(d2)) 2 max e"""
    x64, c = x.astype(np.float64), c0.astype(np.float64)
    inside, old = 0, None
    for _ in range(max_iter):
        dist = np.sort(distances64(x64, c), axis=1)
        labels = distances64(x64, c).argmin(1)
        counts = np.maximum(np.bincount(labels, minlength=k), 1)
        e = max((counts[j] + 1) * 2.0 ** -24 * np.linalg.norm(np.abs(x64[labels == j]).sum(0) / counts[j]) for j in range(k))
        inside += int((dist[:, 1] - dist[:, 0] <= tau(x.shape[1]) * dist[:, 1] + 2 * e * (np.sqrt(dist[:, 0]) + np.sqrt(dist[:, 1]))).sum())
        if old is not None and np.array_equal(labels, old):
            break
        old, c = labels, np.stack([x64[labels == j].sum(0) / counts[j] for j in range(k)])
    return inside


@pytest.mark.parametrize("n,d,k,spread", (BLOBS[0], BLOBS[3]))
def test_kmeans_with_the_new_update(cuda, n, d, k, spread):
    """equal labels are a claim only where no row comes closer to a tie than the centres' perturbation: checked here in float64.  The
    blob sets (1500, 100, 7) and (3000, 100, 47) have 2 and 4 such rows (summed over their iterations) and are left out"""
    x, _, c0 = blob_set(n, d, k, spread)
    assert rows_inside_the_perturbation(x, c0, k) == 0
    xd = torch.from_numpy(x).to(cuda)
    want, got = kmeans(xd, k, init=c0), kmeans(xd, k, init=c0, update="sums")
    assert got.n_iter == want.n_iter and torch.equal(got.labels, want.labels)
    labels = want.labels.cpu().numpy()
    _, counts, mass = sums64(x, labels, k)
    blocks, rows = rule(n, d, k)[:2]                                    # either update: its sum's bound over the count, and the division
    bound = ((rows + blocks) + counts[:, None]) * 2.0 ** -24 * mass / counts[:, None] + 2.0 ** -23 * np.abs(want.centres.cpu().numpy())
    assert (np.abs(got.centres.cpu().numpy().astype(np.float64) - want.centres.cpu().numpy()) <= bound).all()
    assert abs(got.inertia - want.inertia) <= dist_tol(d) * want.inertia, (got.inertia, want.inertia)


def test_an_empty_start_and_the_refusals(cuda):
    n, d, k, spread = BLOBS[0]
    x, _, c0 = blob_set(n, d, k, spread)
    c0[1] = c0[0]                                                       # cluster 1 starts empty: the lowest index wins the tie
    xd = torch.from_numpy(x).to(cuda)
    want, got = kmeans(xd, k, init=c0), kmeans(xd, k, init=c0, update="sums")
    assert got.n_iter == want.n_iter and torch.equal(got.labels, want.labels)
    with pytest.raises(ValueError, match="update"):
        kmeans(xd, k, update="atomic")
    with pytest.raises(ValueError, match=str(dev.CLUSTER_SUMS_MAX_K)):
        kmeans(xd, dev.CLUSTER_SUMS_MAX_K + 1, update="sums")
