"""The k-means assignment kernel (csrc/sgl_kmeans.hip), the Lloyd loop, the seeding and the clustering task on a real MI355X: run with
`-m gpu`.

Labels are compared with the float64 argmin on every row that is not near a tie, mindist with the float64 minimum; both tolerances
are derived in kmeans_common from the arithmetic.  Lloyd parity with sklearn is asserted where it is defined -- from the same
initial centres (fixture (a) of g16_node_clustering.npz), labels and iteration count exactly, centres and inertia through
oracle.truth_report -- and scores where sklearn itself reaches one partition from five seedings (fixture (c)).  Bit-for-bit claims
use torch.equal."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import oracle
from kmeans_common import BIG, BLOBS, KS, LAYOUTS, MAX_LEFT_OUT, N_ROWS, WIDTHS, blob_set, dist_tol, host_centres, host_x, in_layout, reference
from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.tricks import clustering_scores, kmeans, nafs_node_clustering

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def check_case(d, k, layout, cuda):
    """one launch against the float64 reference; returns the problems found"""
    x, c = in_layout(host_x(d), layout, cuda), in_layout(host_centres(d, k), layout, cuda)
    labels, mindist = dev.kmeans_assign(x, c)
    want, d1, near = reference(d, k)
    labels, mindist = labels.cpu().numpy(), mindist.cpu().numpy().astype(np.float64)
    bad = []
    if labels.dtype != np.int64 or labels.shape != (N_ROWS,) or mindist.shape != (N_ROWS,):
        return [(d, k, layout, "shapes", labels.dtype, labels.shape, mindist.shape)]
    if near.mean() > MAX_LEFT_OUT:
        bad.append((d, k, layout, "left out", float(near.mean())))
    wrong = np.flatnonzero((labels != want) & ~near)
    if wrong.size:
        bad.append((d, k, layout, "labels", wrong.size, wrong[:5].tolist()))
    err = np.abs(mindist - d1) / np.maximum(d1, np.finfo(np.float64).tiny)
    if not (np.isfinite(mindist).all() and err.max() <= dist_tol(d)):
        bad.append((d, k, layout, "mindist", float(np.nanmax(err)), dist_tol(d)))
    return bad


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", WIDTHS)
def test_values_in_every_instance(cuda, d, layout):
    bad = []
    for k in KS:
        bad += check_case(d, k, layout, cuda)
    assert not bad, bad


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d,k", BIG)
def test_values_across_tiles_and_beyond_the_register_layouts(cuda, d, k, layout):
    bad = check_case(d, k, layout, cuda)
    assert not bad, bad


def test_labels_only_and_contiguous_inputs(cuda):
    for d, k in ((100, 47), (600, 64), (7, 2)):
        x, c = torch.from_numpy(host_x(d)).to(cuda), torch.from_numpy(host_centres(d, k)).to(cuda)
        labels, mindist = dev.kmeans_assign(x, c)
        only, none = dev.kmeans_assign(x, c, want_dist=False)
        assert none is None and same(labels, only)
        want, d1, near = reference(d, k)
        assert np.array_equal(labels.cpu().numpy()[~near], want[~near])


# ---- determinism ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,k", ((100, 47), (147, 7), (600, 64), (1030, 64), (33, 64)))
def test_bits_do_not_depend_on_rows_centres_or_tiles(cuda, d, k):
    x, c = torch.from_numpy(host_x(d)).to(cuda), torch.from_numpy(host_centres(d, k)).to(cuda)
    labels, mindist = dev.kmeans_assign(x, c)
    again = dev.kmeans_assign(x, c)
    assert same(labels, again[0]) and same(mindist, again[1]), "two runs differ"
    g = torch.Generator().manual_seed(d * 100 + k)
    rows = torch.randperm(N_ROWS, generator=g).to(cuda)
    l2, m2 = dev.kmeans_assign(x[rows].contiguous(), c)
    assert same(l2, labels[rows]) and same(m2, mindist[rows]), "the row's position shows"
    cen = torch.randperm(k, generator=g).to(cuda)
    l3, m3 = dev.kmeans_assign(x, c[cen].contiguous())                 # centres move between tiles; no exact ties in this data
    assert same(m3, mindist) and same(cen[l3], labels), "the centre's position shows"
    for lo, hi in ((0, 500), (500, N_ROWS), (N_ROWS - 1, N_ROWS), (0, 255)):      # n = 531, n = 1 and n = 255 among them
        lp, mp = dev.kmeans_assign(x[lo:hi].clone(), c)
        assert same(lp, labels[lo:hi]) and same(mp, mindist[lo:hi]), ("n shows", lo, hi)
    lk, mk = dev.kmeans_assign(x, c[:1].clone())                       # k = 1: every label 0, the distance to that centre
    assert int(lk.abs().max()) == 0
    hit = labels == 0
    assert same(mk[hit], mindist[hit]), "k shows"


def test_stale_output_buffers_do_not_show_through(cuda):
    d, k = 100, 47
    x, c = torch.from_numpy(host_x(d)).to(cuda), torch.from_numpy(host_centres(d, k)).to(cuda)
    want_l, want_m = dev.kmeans_assign(x, c)
    labels = torch.full((N_ROWS,), -7, dtype=torch.int64, device=cuda)
    mindist = torch.full((N_ROWS,), float("nan"), dtype=torch.float32, device=cuda)
    dev._call(cuda, "sgl_kmeans_assign_f32", _lib.ptr(x), d, N_ROWS, d, _lib.ptr(c), d, k, _lib.ptr(labels), _lib.ptr(mindist))
    assert same(labels, want_l) and same(mindist, want_m)
    guard_l = torch.full((N_ROWS + 2,), -7, dtype=torch.int64, device=cuda)       # nothing before or after the n outputs is written
    guard_m = torch.full((N_ROWS + 2,), -7.0, dtype=torch.float32, device=cuda)
    dev._call(cuda, "sgl_kmeans_assign_f32", _lib.ptr(x), d, N_ROWS, d, _lib.ptr(c), d, k, _lib.ptr(guard_l[1:]), _lib.ptr(guard_m[1:]))
    assert same(guard_l[1:-1], want_l) and same(guard_m[1:-1], want_m)
    assert guard_l[0] == -7 and guard_l[-1] == -7 and guard_m[0] == -7 and guard_m[-1] == -7


def test_nan_rows_and_empty_shapes(cuda):
    d, k = 100, 7
    hx = host_x(d).copy()
    hx[5, 3] = hx[700, 99] = hx[N_ROWS - 1, 0] = np.nan
    x, c = torch.from_numpy(hx).to(cuda), torch.from_numpy(host_centres(d, k)).to(cuda)
    labels, mindist = dev.kmeans_assign(x, c)
    clean = dev.kmeans_assign(torch.from_numpy(host_x(d)).to(cuda), c)
    holed = torch.zeros(N_ROWS, dtype=torch.bool, device=cuda)
    holed[[5, 700, N_ROWS - 1]] = True
    assert int(labels[holed].abs().max()) == 0 and bool(torch.isnan(mindist[holed]).all())
    assert same(labels[~holed], clean[0][~holed]) and same(mindist[~holed], clean[1][~holed]), "a NaN row touched its neighbours"
    # d = 0: labels 0 and distances 0, no kernel; n = 0: nothing
    labels, mindist = dev.kmeans_assign(torch.empty((9, 0), device=cuda), torch.empty((3, 0), device=cuda))
    assert labels.shape == (9,) and int(labels.abs().max()) == 0 and float(mindist.abs().max()) == 0.0
    labels, mindist = dev.kmeans_assign(torch.empty((0, 12), device=cuda), c[:, :12])
    assert labels.shape == (0,) and mindist.shape == (0,)
    with pytest.raises(ValueError):
        dev.kmeans_assign(x, torch.empty((0, d), device=cuda))
    with pytest.raises(ValueError):
        dev.kmeans_assign(x, c[:, :50])


def test_bfloat16_hops_raise(cuda):
    x = torch.zeros((8, 16), dtype=torch.bfloat16, device=cuda)
    c = torch.zeros((2, 16), dtype=torch.float32, device=cuda)
    with pytest.raises(TypeError):
        dev.kmeans_assign(x, c)
    with pytest.raises(TypeError):
        dev.kmeans_assign(c, x)
    with pytest.raises(TypeError):
        kmeans(x, 2, n_init=1, seed=0)


# ---- Lloyd parity with sklearn from the same initial centres ----------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k,spread", BLOBS)
def test_lloyd_from_fixed_centres_equals_sklearn(cuda, goldens, n, d, k, spread):
    g = goldens.npz("g16_node_clustering")
    key = f"lloyd|{n}x{d}x{k}"
    x, _, c0 = blob_set(n, d, k, spread)
    got = kmeans(torch.from_numpy(x).to(cuda), k, init=c0)
    again = kmeans(torch.from_numpy(x).to(cuda), k, init=torch.from_numpy(c0), n_init=7)      # an init forces one run
    assert same(got.labels, again.labels) and same(got.centres, again.centres) and got.inertia == again.inertia
    assert got.n_iter == int(g[key + "|n_iter"][0]), (got.n_iter, g[key + "|n_iter"])
    assert np.array_equal(got.labels.cpu().numpy(), g[key + "|labels"])
    assert got.labels.dtype == torch.int64 and got.centres.dtype == torch.float32 and got.centres.shape == (k, d)
    rep = oracle.truth_report(got.centres.cpu().numpy(), g[key + "|centres"], g[key + "|truth_centres"])
    print(key, "centres", rep)
    assert rep["ok"], rep
    rep = oracle.truth_report([got.inertia], g[key + "|inertia"], g[key + "|truth_inertia"])
    print(key, "inertia", got.inertia, rep)
    assert rep["ok"], rep


# ---- properties of kmeans -----------------------------------------------------------------------------------------------------------------
def test_same_seed_same_bits_and_best_of_n_init(cuda):
    n, d, k, spread = BLOBS[3]                                         # the set whose clusters overlap: runs differ
    x = torch.from_numpy(blob_set(n, d, k, spread)[0]).to(cuda)
    a, b = kmeans(x, k, n_init=4, seed=11), kmeans(x, k, n_init=4, seed=11)
    assert same(a.labels, b.labels) and same(a.centres, b.centres) and a.inertia == b.inertia and a.n_iter == b.n_iter
    first = kmeans(x, k, n_init=1, seed=11)                            # the first of the four runs: same generator, same first draws
    assert a.inertia <= first.inertia
    check = dev.kmeans_assign(x, a.centres)
    assert same(check[0], a.labels) and float(check[1].sum(dtype=torch.float64)) == a.inertia
    assert sorted(torch.bincount(a.labels, minlength=k).tolist())[0] > 0


def test_a_far_centre_does_not_leave_a_cluster_empty(cuda):
    n, d, k, spread = BLOBS[0]
    x, _, c0 = blob_set(n, d, k, spread)
    c0 = c0.copy()
    c0[1] = 1e4                                                        # no row is nearest to it
    got = kmeans(torch.from_numpy(x).to(cuda), k, init=c0)
    counts = torch.bincount(got.labels, minlength=k)
    assert int(counts.min()) > 0 and int(counts.sum()) == n, counts
    assert bool(torch.isfinite(got.centres).all())


@pytest.mark.parametrize("n,d,k,spread", BLOBS[:2])
def test_separated_blobs_are_recovered(cuda, n, d, k, spread):
    x, y, _ = blob_set(n, d, k, spread)
    got = kmeans(torch.from_numpy(x).to(cuda), k, n_init=5, seed=0)
    acc, nmi, adjscore = clustering_scores(torch.from_numpy(y).to(cuda), got.labels)
    assert adjscore == 1.0 and acc == 1.0, (acc, nmi, adjscore)
    assert clustering_scores(y, got.labels.cpu())[2] == 1.0            # the table does not depend on the device it is counted on


# ---- the task ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ("mean", "max", "concat", "simple"))
def test_nafs_node_clustering_reproduces_the_reference_task(cuda, goldens, method):
    g = goldens.npz("g16_node_clustering")
    n = len(g["task|y"])
    adj = sp.csr_matrix((np.ones(len(g["task|row"]), np.float32), (g["task|row"], g["task|col"])), shape=(n, n))
    hops = [int(h) for h in g["task|hops"]]
    res = nafs_node_clustering(adj, g["task|x"], g["task|y"], hops, r_list=[float(r) for r in g["task|r_list"]], method=method, n_init=5,
                               seed=42, device=cuda)
    for h in hops:
        want = g[f"task|{method}|hops{h}"]
        print(method, h, res.metrics[h], want)
        assert np.abs(np.array(res.metrics[h]) - want).max() <= 1e-9, (method, h, res.metrics[h], want)
    best = g[f"task|{method}|best"]
    assert (res.best_hop_acc, res.best_hop_nmi, res.best_hop_adjscore) == tuple(int(v) for v in best[:3])
    assert np.abs(np.array([res.acc, res.nmi, res.adjscore]) - best[3:]).max() <= 1e-9
