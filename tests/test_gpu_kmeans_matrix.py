"""The matrix-core k-means assignment (csrc/sgl_kmeans_mfma.hip; device.kmeans_assign form="matrix", kmeans assign="matrix") on a real
MI355X: run with `-m gpu`.

Every row is compared.  With float64 distances D, float64 argmin b, x' = x - shift and c' = c - shift, the returned label L must satisfy
D[i, L] - D[i, b] <= 2 (E_L + E_b),  E_j = (d + 3) 2^-23 (|c'_j|^2 + 2 |x'_i| |c'_j|) + 2^-23 sqrt(D[i, j]) (|x'_i| + |c'_j|):
a d-term dot product and norm at one unit per operation (2^-23 covers an instruction that rounds or truncates), then the rounding of
the two centring subtractions.  The bound is derived, nothing is fitted to the kernel.  It is sharp enough only while few rows have
their float64 SECOND-best centre inside it (a wrong label could hide there): the test asserts at most 1 % per case (worst on these
inputs, from float64 alone: 8 of 1031 rows at d = 600 / 640, k = 64 / 65).  mindist is the direct form for L: dist_tol(d), as K9."""
import numpy as np
import pytest
import torch

from kmeans_common import BLOBS, LAYOUTS, N_ROWS, blob_set, dist_tol, distances64, host_centres, host_x, in_layout
from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.tricks import kmeans

pytestmark = pytest.mark.gpu
WIDTHS = (1, 3, 7, 8, 9, 33, 100, 128, 147, 600, 640)
KS = (1, 2, 7, 33, 47, 64, 65)
OFFSETS = (0.0, 100.0)
_REF = {}


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def reference(d, k, offset):
    """(x, c, shift in float32; D [n, k] and the bound E [n, k] in float64) -- once per case, left unchanged"""
    if (d, k, offset) not in _REF:
        x, c = host_x(d) + np.float32(offset), host_centres(d, k) + np.float32(offset)
        shift = c.mean(0, dtype=np.float32)
        dist = distances64(x, c)
        xn, cn = np.linalg.norm(x.astype(np.float64) - shift, axis=1)[:, None], np.linalg.norm(c.astype(np.float64) - shift, axis=1)[None, :]
        bound = (d + 3) * 2.0 ** -23 * (cn ** 2 + 2 * xn * cn) + 2.0 ** -23 * np.sqrt(dist) * (xn + cn)
        _REF[(d, k, offset)] = (x, c, shift, dist, bound)
    return _REF[(d, k, offset)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", WIDTHS)
def test_values_on_every_row(cuda, d, layout):
    bad, rows = [], np.arange(N_ROWS)
    for k in KS:
        for offset in OFFSETS:
            x, c, shift, dist, bound = reference(d, k, offset)
            labels, mindist = dev.kmeans_assign(in_layout(x, layout, cuda), in_layout(c, layout, cuda), form="matrix", shift=torch.from_numpy(shift).to(cuda))
            assert labels.dtype == torch.int64 and labels.shape == (N_ROWS,) and mindist.shape == (N_ROWS,)
            got, mindist = labels.cpu().numpy(), mindist.cpu().numpy().astype(np.float64)
            order = np.argsort(dist, axis=1, kind="stable")
            b = order[:, 0]
            if k > 1:                                                  # sharpness: a condition on the inputs, asserted
                s = order[:, 1]
                hidden = dist[rows, s] - dist[rows, b] <= 2 * (bound[rows, s] + bound[rows, b])
                if hidden.mean() > 0.01:
                    bad.append((d, k, offset, "second best inside the bound", int(hidden.sum())))
            if got.min() < 0 or got.max() >= k:
                bad.append((d, k, offset, "label range", int(got.min()), int(got.max())))
                continue
            excess = (dist[rows, got] - dist[rows, b]) - 2 * (bound[rows, got] + bound[rows, b])
            err = np.abs(mindist - dist[rows, got]) / np.maximum(dist[rows, got], np.finfo(np.float64).tiny)
            print(d, k, offset, layout, "labels off the argmin", int((got != b).sum()), "largest excess", float(excess.max()), "mindist", float(np.nanmax(err)))
            if not excess.max() <= 0:
                bad.append((d, k, offset, "labels", int((excess > 0).sum()), np.flatnonzero(excess > 0)[:5].tolist()))
            if not (np.isfinite(mindist).all() and err.max() <= dist_tol(d)):
                bad.append((d, k, offset, "mindist", float(np.nanmax(err)), dist_tol(d)))
    assert not bad, bad


@pytest.mark.parametrize("d,k", ((100, 47), (147, 7), (600, 64)))
def test_edges_and_invariants(cuda, d, k):
    x, c = torch.from_numpy(host_x(d)).to(cuda), torch.from_numpy(host_centres(d, k)).to(cuda)
    labels, mindist = dev.kmeans_assign(x, c, form="matrix")
    again = dev.kmeans_assign(x, c, form="matrix")
    assert same(labels, again[0]) and same(mindist, again[1]), "two runs differ"
    only, none = dev.kmeans_assign(x, c, want_dist=False, form="matrix")
    assert none is None and same(only, labels)
    for n in (1, 31, 32, 33, 63, 64, 65, 255, 256, 257):
        lp, mp = dev.kmeans_assign(x[:n].clone(), c, form="matrix")
        assert same(lp, labels[:n]) and same(mp, mindist[:n]), ("n shows", n)
    perm = torch.randperm(N_ROWS, generator=torch.Generator().manual_seed(d + k)).to(cuda)
    l2, m2 = dev.kmeans_assign(x[perm].contiguous(), c, form="matrix")
    assert same(l2, labels[perm]) and same(m2, mindist[perm]), "the row's position shows"
    try:                                                               # the strided form: one workgroup, then three
        for cap in (1, 3):
            _lib.set_tuning("loss_blocks", cap)
            ls, ms = dev.kmeans_assign(x, c, form="matrix")
            assert same(ls, labels) and same(ms, mindist), ("loss_blocks", cap)
    finally:
        _lib.set_tuning("loss_blocks", 0)
    shift = c.mean(0)
    out_l = torch.full((N_ROWS + 2,), -7, dtype=torch.int64, device=cuda)        # stale outputs; nothing before or after them is written
    out_m = torch.full((N_ROWS + 2,), float("nan"), dtype=torch.float32, device=cuda)
    dev._call(cuda, "sgl_kmeans_assign_matrix_f32", _lib.ptr(x), d, N_ROWS, d, _lib.ptr(c), d, k, _lib.ptr(shift), _lib.ptr(out_l[1:]), _lib.ptr(out_m[1:]))
    assert same(out_l[1:-1], labels) and same(out_m[1:-1], mindist)
    assert out_l[0] == -7 and out_l[-1] == -7 and bool(torch.isnan(out_m[[0, -1]]).all())
    holed = x.clone()
    holed[40, d // 2] = float("nan")                                   # rows 32 .. 63 share its tile
    ln, mn = dev.kmeans_assign(holed, c, form="matrix")
    keep = torch.arange(N_ROWS, device=cuda) != 40
    assert int(ln[40]) == 0 and bool(torch.isnan(mn[40])) and same(ln[keep], labels[keep]) and same(mn[keep], mindist[keep])


@pytest.mark.parametrize("n,d,k,spread", (BLOBS[0], BLOBS[3]))
def test_lloyd_takes_the_steps_of_the_direct_form(cuda, n, d, k, spread):
    """equal labels are a claim only where no row comes inside the bound above during the iterations; a float64 Lloyd loop on the CPU
    finds none in these two sets and 2 / 5 such rows (summed over 9 / 7 iterations) in (1500, 100, 7) / (3000, 100, 47): left out"""
    x, _, c0 = blob_set(n, d, k, spread)
    x = torch.from_numpy(x).to(cuda)
    want, got = kmeans(x, k, init=c0), kmeans(x, k, init=c0, assign="matrix")
    assert got.n_iter == want.n_iter and same(got.labels, want.labels)
    assert abs(got.inertia - want.inertia) <= dist_tol(d) * want.inertia, (got.inertia, want.inertia)
