"""The fused clustering loss (csrc/sgl_cluster_loss.hip), its wrappers and the trainable clustering task on a real MI355X: run with
`-m gpu`.

Loss and dX are compared with the reference's own expression (cluster_loss, sgl/tasks/utils.py:101-113) under CPU autograd, in float32
and in float64 (the truth), through oracle.truth_report -- at most twice as far from the truth as the reference's float32 result, with
the condition-aware floor; no tolerance is chosen in this file, and test_cluster_loss_cpu.py pins that a plain float32 evaluation
passes the rule on these inputs.  Bit-for-bit claims use torch.equal.  The value tests run under torch.profiler: the kernel instances
seen must be the ones the restated selection rule (cluster_loss_common) announces, and all of them together exactly the compiled ones."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import oracle
from cluster_loss_common import (KS, SHIFT, WIDTHS, compiled_instances, expected_instance, inputs, parse_kernel_name, references,
                                 step_references)
from far_common import FILL32, GIB, TIERS, FarTable, pick_tier, table_elems
from kmeans_common import BIG, LAYOUTS, N_ROWS, POISONS, in_layout
from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.tricks import cluster_loss, clustering_train, kmeans, node_clustering

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


class Trace:
    """Runs launches under torch.profiler and checks, at exit, that the cluster-loss kernel instances that really ran are, in order,
    the ones `expect()` announced; every other kernel is ignored.  A profiler that reports no kernel names fails the comparison."""

    def __init__(self):
        self.expected, self.seen = [], set()

    def expect(self, label, x, c, dx):
        self.expected.append((label, expected_instance(x, c, dx)))

    def __enter__(self):
        from torch.profiler import ProfilerActivity, profile
        self.prof = profile(activities=[ProfilerActivity.CUDA])
        self.prof.__enter__()
        return self

    def __exit__(self, et, ev, tb):
        torch.cuda.synchronize()
        self.prof.__exit__(et, ev, tb)
        if et is not None:
            return False
        from torch.autograd import DeviceType
        evs = sorted((e for e in self.prof.events() if e.device_type == DeviceType.CUDA), key=lambda e: e.time_range.start)
        got = [p for p in (parse_kernel_name(e.name) for e in evs) if p is not None]
        assert len(got) == len(self.expected), (len(got), len(self.expected), len(evs), got[:3], self.expected[:3])
        wrong = [(i, lab, g, w) for i, (g, (lab, w)) in enumerate(zip(got, self.expected)) if g != w]
        assert not wrong, (len(wrong), wrong[:8])
        self.seen |= set(got)
        return False


def same(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def step(x, c, y, layout="padded", w=None, tr=None, label=None):
    """one launch of the low-level call into NaN-filled outputs of the given layout: (loss, dX, row_loss)"""
    n, d = x.shape
    w = 1.0 / n if w is None else w
    dx = in_layout(np.full((n, d), np.nan, dtype=np.float32), layout, x.device)
    rows = torch.full((n,), float("nan"), device=x.device)
    if tr is not None:
        tr.expect(label, x, c, dx)
    out = dev.cluster_loss_grad(x, c, y, w, dx=dx, row_loss=rows)
    assert out[0] is dx and out[1] is rows
    return float(rows.double().sum() * w), dx, rows


def check_truth(bad, label, loss, dx, refs):
    dx = dx.cpu().numpy()
    if not (np.isfinite(dx).all() and np.isfinite(loss)):
        bad.append((label, "not finite"))
        return
    for what, got, i in (("loss", loss, 0), ("dX", dx, 1)):
        rep = oracle.truth_report(got, refs["ref32"][i], refs["truth"][i], cond=refs["cond"][i])
        if not rep["ok"]:
            bad.append((label, what, rep))


def on_device(d, k, layout, cuda, shift=0.0):
    x, c, y = inputs(d, k, shift)
    return in_layout(x, layout, cuda), in_layout(c, layout, cuda), torch.from_numpy(y).to(cuda)


# ---- values, in every compiled instance -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d", WIDTHS)
def test_values_in_every_instance(cuda, d, layout):
    bad = []
    with Trace() as tr:
        for k in KS:
            x, c, y = on_device(d, k, layout, cuda)
            if k > 1:                                                 # (a single centre row is passed with pitch d)
                assert expected_instance(x, c)[1] == (1 if layout == "odd_view" else 4)
            loss, dx, _ = step(x, c, y, layout, tr=tr, label=(d, k, layout))
            check_truth(bad, (d, k, layout), loss, dx, references(d, k))
    assert not bad, bad


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("d,k", BIG)
def test_values_across_tiles_and_beyond_the_register_layouts(cuda, d, k, layout):
    bad = []
    with Trace() as tr:
        x, c, y = on_device(d, k, layout, cuda)
        loss, dx, _ = step(x, c, y, layout, tr=tr, label=(d, k, layout))
        check_truth(bad, (d, k, layout), loss, dx, references(d, k))
    assert not bad, bad


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_widths_launch_exactly_the_compiled_instances(cuda, layout):
    """the widths of the two value tests above reach every compiled instance of the layout's lane size, and nothing else runs"""
    with Trace() as tr:
        for d, k in [(d, 2) for d in WIDTHS] + list(BIG):
            x, c, y = on_device(d, k, layout, cuda)
            step(x, c, y, layout, tr=tr, label=(d, k, layout))
    vec = 1 if layout == "odd_view" else 4
    want = {i for i in compiled_instances() if i[1] == vec}
    print(f"\n[cluster_loss {layout}] instances seen: {sorted(tr.seen)}")
    assert tr.seen == want, sorted(want ^ tr.seen)


def test_pad_columns_never_reach_the_output(cuda):
    """in_layout fills the pads with NaN and 1e30 alternately; the same values from buffers whose pads hold zeros have the same bits"""
    assert any(p != p for p in POISONS)
    for d, k in ((7, 2), (100, 47), (147, 7), (257, 64)):
        x_h, c_h, y_h = inputs(d, k)
        y = torch.from_numpy(y_h).to(cuda)
        x, c = in_layout(x_h, "padded", cuda), in_layout(c_h, "padded", cuda)
        x0, c0 = dev.alloc_rows(N_ROWS, d, cuda), dev.alloc_rows(k, d, cuda)
        x0.copy_(torch.from_numpy(x_h))
        c0.copy_(torch.from_numpy(c_h))
        assert expected_instance(x, c) == expected_instance(x0, c0)
        a, b = step(x, c, y, "padded"), step(x0, c0, y, "padded")
        assert a[0] == b[0] and same(a[1], b[1]) and same(a[2], b[2]), (d, k)


# ---- translation invariance --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,k", ((7, 2), (100, 47), (147, 7), (600, 64)))
def test_translation_invariance(cuda, d, k):
    """x and the centres both shifted by +100 per column; the references are recomputed from the shifted float32 inputs and the
    result is held to the same rule -- the expanded form x sum a - sum a c fails it"""
    bad = []
    for layout in LAYOUTS:
        x, c, y = on_device(d, k, layout, cuda, SHIFT)
        loss, dx, _ = step(x, c, y, layout)
        check_truth(bad, (d, k, layout), loss, dx, references(d, k, SHIFT))
    assert not bad, bad


# ---- bits -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,k", ((100, 47), (147, 7), (600, 64), (1030, 64), (33, 64), (2500, 9)))
def test_bits_do_not_depend_on_rows_or_outputs(cuda, d, k):
    x_h, c_h, y_h = inputs(d, k)
    x, c, y = torch.from_numpy(x_h).to(cuda), torch.from_numpy(c_h).to(cuda), torch.from_numpy(y_h).to(cuda)
    w = 1.0 / N_ROWS

    def run(xx, yy, want_dx=True, want_loss=True):
        return dev.cluster_loss_grad(xx, c, yy, w, dx=torch.full_like(xx, float("nan")) if want_dx else None,
                                     row_loss=torch.full((len(xx),), float("nan"), device=cuda) if want_loss else None)

    dx, rows = run(x, y)
    again = run(x, y)
    assert same(dx, again[0]) and same(rows, again[1]), "two runs differ"
    perm = torch.randperm(N_ROWS, generator=torch.Generator().manual_seed(d * 100 + k)).to(cuda)
    dx2, rows2 = run(x[perm].contiguous(), y[perm].contiguous())
    assert same(dx2, dx[perm]) and same(rows2, rows[perm]), "the row's position shows"
    for lo, hi in ((0, 500), (500, N_ROWS), (N_ROWS - 1, N_ROWS), (0, 255)):      # the row set split in two calls; n = 1 and n = 255
        dxp, rowsp = run(x[lo:hi].clone(), y[lo:hi].clone())
        assert same(dxp, dx[lo:hi]) and same(rowsp, rows[lo:hi]), ("n shows", lo, hi)
    only_dx, none = run(x, y, want_loss=False)
    assert none is None and same(only_dx, dx), "dX alone differs"
    none, only_rows = run(x, y, want_dx=False)
    assert none is None and same(only_rows, rows), "row_loss alone differs"


# ---- edge cases --------------------------------------------------------------------------------------------------------------------------
def test_zero_distance_gives_a_finite_gradient_and_contributes_nothing(cuda):
    """rows that coincide with a centre: the gradient is finite and, under the acceptance rule, the reference's -- whose term for that
    centre is 0 (torch.norm's subgradient); a row that coincides with its ONLY centre has l_i = 0 and dX_i = 0 exactly"""
    d, k = 100, 7
    x_h, c_h, y_h = inputs(d, k)
    rows_hit = np.flatnonzero((x_h[:, None, :] == c_h[None, :3, :]).all(-1).any(1))
    assert len(rows_hit) == 3
    bad = []
    for layout in LAYOUTS:
        x, c, y = on_device(d, k, layout, cuda)
        loss, dx, rows = step(x, c, y, layout)
        assert bool(torch.isfinite(dx[rows_hit]).all()) and bool(torch.isfinite(rows[rows_hit]).all())
        refs = references(d, k)
        rep = oracle.truth_report(dx[rows_hit].cpu().numpy(), refs["ref32"][1][rows_hit], refs["truth"][1][rows_hit], cond=refs["cond"][1][rows_hit])
        if not rep["ok"]:
            bad.append((layout, rep))
        dx1, rows1 = dev.cluster_loss_grad(x[5:6], x[5:6].clone(), torch.zeros(1, dtype=torch.int64, device=cuda), 1.0, dx=True, row_loss=True)
        assert float(rows1[0]) == 0.0 and bool((dx1 == 0).all())
    assert not bad, bad


def test_out_of_range_labels_read_nothing_out_of_bounds(cuda):
    """a label outside [0, k) means `no assigned centre`: l_i = -(1 / k) sum_j D_ij and the 2 D term's gradient is absent; the guard
    rows around every buffer keep their fill"""
    d, k = 100, 7
    x_h, c_h, y_h = inputs(d, k)
    y_bad = y_h.copy()
    y_bad[::5] = k
    y_bad[1::5] = -1
    y_bad[2::5] = 2 ** 40
    fill = -7.0
    xg = torch.full((N_ROWS + 2, d), fill, device=cuda)
    cg = torch.full((k + 2, d), fill, device=cuda)
    dxg = torch.full((N_ROWS + 2, d), fill, device=cuda)
    rg = torch.full((N_ROWS + 2,), fill, device=cuda)
    yg = torch.full((N_ROWS + 2,), 3, dtype=torch.int64, device=cuda)
    xg[1:-1] = torch.from_numpy(x_h).to(cuda)
    cg[1:-1] = torch.from_numpy(c_h).to(cuda)
    yg[1:-1] = torch.from_numpy(y_bad).to(cuda)
    w = 1.0 / N_ROWS
    dev.cluster_loss_grad(xg[1:-1], cg[1:-1], yg[1:-1], w, dx=dxg[1:-1], row_loss=rg[1:-1])
    for t in (dxg, rg):
        assert bool((t[0] == fill).all()) and bool((t[-1] == fill).all())
    assert bool(torch.isfinite(dxg).all()) and bool(torch.isfinite(rg).all())
    # against float64: the rows with a bad label have no assigned centre
    x64, c64 = x_h.astype(np.float64), c_h.astype(np.float64)
    dist = np.sqrt(((x64[:, None, :] - c64[None]) ** 2).sum(-1))
    ok = (y_bad >= 0) & (y_bad < k)
    assigned = np.where(ok, dist[np.arange(N_ROWS), np.where(ok, y_bad, 0)], 0.0)
    want = 2.0 * assigned - dist.mean(1)
    got = rg[1:-1].cpu().numpy().astype(np.float64)
    # a distance is within ((d + 3) / 2 + 1) roundings (the sum of squares of kmeans_common.dist_tol, halved by the root, and the root),
    # the k-term sum, the product with 1 / k, 2 D and the difference add k + 3: relative to the sum of the absolute terms
    tol = ((d + 3) / 2 + 1 + k + 3) * 2.0 ** -24
    assert (np.abs(got - want) <= tol * (2.0 * assigned + dist.mean(1))).all()
    good = torch.from_numpy(np.where(ok, y_bad, 0)).to(cuda)
    dx_good, rows_good = dev.cluster_loss_grad(xg[1:-1], cg[1:-1], good, w, dx=True, row_loss=True)
    keep = torch.from_numpy(ok).to(cuda)
    assert same(dx_good[keep], dxg[1:-1][keep]) and same(rows_good[keep], rg[1:-1][keep]), "a bad label touched another row"
    # the public function: check=True refuses them, check=False takes them
    with pytest.raises(IndexError):
        cluster_loss(xg[1:-1], yg[1:-1], cg[1:-1])
    loss = cluster_loss(xg[1:-1], yg[1:-1], cg[1:-1], check=False)
    assert abs(float(loss) - want.mean()) <= (tol + 2.0 ** -24) * (2.0 * assigned + dist.mean(1)).mean()
    wrapped = y_h - k                                                 # all negative: numpy's wrap
    assert float(cluster_loss(xg[1:-1], wrapped, cg[1:-1])) == float(cluster_loss(xg[1:-1], torch.from_numpy(y_h), cg[1:-1]))


def test_nan_rows_poison_only_themselves_and_empty_shapes(cuda):
    d, k = 100, 7
    x_h, c_h, y_h = inputs(d, k)
    hx = x_h.copy()
    hx[5, 3] = hx[700, 99] = np.nan
    hx[N_ROWS - 1, 0] = np.inf
    c, y = torch.from_numpy(c_h).to(cuda), torch.from_numpy(y_h).to(cuda)
    _, dx, rows = step(torch.from_numpy(hx).to(cuda), c, y)
    _, dx0, rows0 = step(torch.from_numpy(x_h).to(cuda), c, y)
    holed = torch.zeros(N_ROWS, dtype=torch.bool, device=cuda)
    holed[[5, 700, N_ROWS - 1]] = True
    assert not bool(torch.isfinite(rows[holed]).any()) and not bool(torch.isfinite(dx[holed]).all(1).any())
    assert same(dx[~holed], dx0[~holed]) and same(rows[~holed], rows0[~holed]), "a non-finite row touched its neighbours"
    # d = 0: zeros and no kernel; n = 0: nothing
    with Trace():
        dx, rows = dev.cluster_loss_grad(torch.empty((9, 0), device=cuda), torch.empty((3, 0), device=cuda), torch.zeros(9, dtype=torch.int64, device=cuda),
                                         1.0, dx=True, row_loss=torch.full((9,), float("nan"), device=cuda))
        assert dx.shape == (9, 0) and float(rows.abs().max()) == 0.0
        dx, rows = dev.cluster_loss_grad(torch.empty((0, 12), device=cuda), c[:, :12], torch.zeros(0, dtype=torch.int64, device=cuda), 1.0,
                                         dx=True, row_loss=True)
        assert dx.shape == (0, 12) and rows.shape == (0,)
        out = torch.empty((0, 12), device=cuda, requires_grad=True)
        loss = cluster_loss(out, np.zeros(0, dtype=np.int64), c[:, :12])
        loss.backward()
        assert float(loss.detach()) == 0.0 and out.grad.shape == (0, 12)
    x = torch.from_numpy(x_h).to(cuda)
    with pytest.raises(ValueError):
        dev.cluster_loss_grad(x, torch.empty((0, d), device=cuda), y, 1.0, dx=True)
    with pytest.raises(ValueError):
        dev.cluster_loss_grad(x, c[:, :50], y, 1.0, dx=True)
    with pytest.raises(ValueError):
        dev.cluster_loss_grad(x, c, y, 1.0)
    with pytest.raises(ValueError):
        dev.cluster_loss_grad(x, c, y.to(torch.int32), 1.0, dx=True)
    with pytest.raises(TypeError):
        dev.cluster_loss_grad(x.to(torch.bfloat16), c, y, 1.0, dx=True)
    with pytest.raises(TypeError):
        cluster_loss(x.to(torch.bfloat16), y, c)


def test_one_centre(cuda):
    """k = 1: every label is 0, l_i = D_i and dX_i = w (x_i - c) / D_i"""
    for d in (7, 147):
        x_h, c_h, y_h = inputs(d, 1)
        x, c, y = torch.from_numpy(x_h).to(cuda), torch.from_numpy(c_h).to(cuda), torch.from_numpy(y_h).to(cuda)
        _, dx, rows = step(x, c, y, w=1.0)
        diff = x_h.astype(np.float64) - c_h[0].astype(np.float64)
        dist = np.sqrt((diff ** 2).sum(1))
        assert np.abs(rows.cpu().numpy() - dist).max() <= (d + 4) * 2.0 ** -24 * dist.max()
        unit = np.divide(diff, dist[:, None], out=np.zeros_like(diff), where=dist[:, None] > 0)
        assert np.abs(dx.cpu().numpy() - unit).max() <= (d + 8) * 2.0 ** -24


# ---- autograd -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,k", ((100, 47), (147, 7)))
def test_autograd_returns_the_kernels_gradient(cuda, d, k):
    x_h, c_h, y_h = inputs(d, k)
    x, c, y = torch.from_numpy(x_h).to(cuda), torch.from_numpy(c_h).to(cuda), torch.from_numpy(y_h).to(cuda)
    want_dx, want_rows = dev.cluster_loss_grad(x, c, y, 1.0 / N_ROWS, dx=True, row_loss=True)
    want_loss = (want_rows.double().sum() / N_ROWS).float()
    out = x.clone().requires_grad_(True)
    cg = c.clone().requires_grad_(True)
    loss = cluster_loss(out, y, cg)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and float(loss.detach()) == float(want_loss)
    loss.backward()
    assert same(out.grad.contiguous(), want_dx.contiguous()) and cg.grad is None and y.grad is None
    out2 = x.clone().requires_grad_(True)
    (cluster_loss(out2, y_h, c_h) * 3.0).backward()                   # ndarray labels and centres; an upstream factor of 3
    assert same(out2.grad.contiguous(), (want_dx * 3.0).contiguous())
    with torch.no_grad():
        assert float(cluster_loss(out, y, c)) == float(want_loss)
    bad = []
    out3 = x.clone().requires_grad_(True)
    total = cluster_loss(out3, y, c, reduction="sum")
    total.backward()
    check_truth(bad, "sum", float(total.detach()), out3.grad, step_references(x_h, c_h, y_h, reduction="sum"))
    assert not bad, bad
    # through a model: the gradient reaches the parameters
    lin = torch.nn.Linear(d, 16).to(cuda)
    z = lin(x)
    km_c = z.detach()[:k].clone()
    cluster_loss(z, y, km_c).backward()
    assert lin.weight.grad is not None and bool(torch.isfinite(lin.weight.grad).all()) and float(lin.weight.grad.abs().max()) > 0


# ---- offsets beyond 2^32 elements -----------------------------------------------------------------------------------------------------------
def test_far_offsets(cuda):
    """X, dX and the k = 64 centres as column ranges of rows of one table whose last rows start beyond 2^32 elements (2^31 at the
    smaller tier); the same acceptance rule, and the table is swept for words off its fill afterwards"""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    tier = pick_tier(free)
    if tier is None:
        pytest.skip(f"the far-offset case needs {TIERS['B'][0] / GIB:.0f} GiB of free device memory, {free / GIB:.1f} GiB are free")
    flat = torch.empty(table_elems(tier), dtype=torch.float32, device=cuda)
    words = flat.view(torch.int32)
    words.fill_(FILL32)
    table = FarTable(flat, TIERS[tier][1])
    n, k = N_ROWS, 64
    s = (n - 1) // (k - 1)
    lay = table.layout(n, pitch_rows=(k - 1) * s + 1)
    bad = []
    for d in (147, 600):                                              # one float per lane never: the table's views are 32-byte aligned
        x_h, c_h, y_h = inputs(d, k)
        x, c, dx = lay.take(d), lay.take(d, rows=k, step=s), lay.take(d)
        assert x.far_rows(table.threshold) > 0 and c.far_rows(table.threshold) > 0 and dx.far_rows(table.threshold) > 0
        x.t.copy_(torch.from_numpy(x_h))
        c.t.copy_(torch.from_numpy(c_h))
        y = torch.from_numpy(y_h).to(cuda)
        rows = torch.full((n,), float("nan"), device=cuda)
        dev.cluster_loss_grad(x.t, c.t, y, 1.0 / n, dx=dx.t, row_loss=rows)
        check_truth(bad, ("far", d), float(rows.double().sum() / n), dx.t, references(d, k))
        xn, cn = dev.alloc_rows(n, d, cuda), dev.alloc_rows(k, d, cuda)          # the same call on ordinary buffers: the same bits
        xn.copy_(torch.from_numpy(x_h))
        cn.copy_(torch.from_numpy(c_h))
        near = dev.cluster_loss_grad(xn, cn, y, 1.0 / n, dx=True, row_loss=True)
        assert expected_instance(x.t, c.t, dx.t) == expected_instance(xn, cn, near[0])
        if not (same(dx.t.contiguous(), near[0].contiguous()) and same(rows, near[1])):
            bad.append(("far and near buffers give different bits", d))
        lay.refill()
    stray = 0
    for lo in range(0, words.numel(), 1 << 28):
        stray += int(torch.count_nonzero(words[lo:lo + (1 << 28)] != FILL32))
    print(f"\n[far cluster_loss] tier {tier}, pitch {lay.ld}: words off the fill afterwards: {stray}")
    del table, lay, x, c, dx, words, flat
    torch.cuda.empty_cache()
    assert not bad, bad
    assert stray == 0


# ---- the reference fixture ------------------------------------------------------------------------------------------------------------------
class SGCLike(torch.nn.Module):
    """one Linear layer on pre-propagated features, with the reference's model interface"""

    def __init__(self, f_in, hidden):
        super().__init__()
        self._base_model = torch.nn.Linear(f_in, hidden)
        self.x = None

    def preprocess(self, adj, x):
        self.x = x

    def model_forward(self, idx, device):
        return self._base_model(self.x[idx])


def test_step_on_the_reference_fixture(cuda, goldens):
    g = goldens.npz("g19_node_clustering_train")
    z, c, y = g["step|z"], g["step|centres"], g["step|labels"]
    cond = step_references(z, c, y)["cond"]
    out = torch.from_numpy(z).to(cuda).requires_grad_(True)
    loss = cluster_loss(out, y, c)
    loss.backward()
    reps = (oracle.truth_report(float(loss.detach()), g["step|loss"], g["step|loss64"], cond=cond[0]),
            oracle.truth_report(out.grad.cpu().numpy(), g["step|grad"], g["step|grad64"], cond=cond[1]))
    print("loss", float(loss.detach()), reps[0], "\ngrad", reps[1])
    assert reps[0]["ok"] and reps[1]["ok"], reps
    assert bool(torch.isfinite(out.grad).all())                       # row 7 coincides with centre 0


def test_three_epochs_of_the_task_on_the_reference_fixture(cuda, goldens):
    g = goldens.npz("g19_node_clustering_train")
    x = torch.from_numpy(g["task|x"]).to(cuda)
    n = x.shape[0]
    adj = sp.csr_matrix((np.ones(len(g["task|row"]), np.float32), (g["task|row"], g["task|col"])), shape=(n, n))
    model = SGCLike(x.shape[1], g["task|state|_base_model.bias"].shape[0])
    model.load_state_dict({key[len("task|state|"):]: torch.from_numpy(v) for key, v in g.items() if key.startswith("task|state|")})
    res = node_clustering(model, adj, x, g["task|y"], epochs=int(g["task|epochs"]), lr=float(g["task|lr"]), weight_decay=0.0, n_init=5, seed=42,
                          device=cuda)
    losses = np.array([h["loss"] for h in res.history[:-1]])
    assert len(losses) == 3 and res.history[-1]["epoch"] == "post"
    rep = oracle.truth_report(losses, g["task|loss"], g["task|loss64"], cond=g["task|loss_cond"])
    print("loss", losses, g["task|loss"], rep)
    assert rep["ok"], rep
    for e, h in enumerate(res.history[:-1]):                          # the same partition: the same scores
        assert np.abs(np.array([h["acc"], h["nmi"], h["adjscore"]]) - g["task|scores"][e]).max() <= 1e-12, (e, h, g["task|scores"][e])
    last = res.history[-1]                                            # (float64 evaluations of the same expressions of one integer table)
    assert np.abs(np.array([last["acc"], last["nmi"], last["adjscore"]]) - g["task|final"]).max() <= 1e-12
    assert np.abs(np.array([res.acc, res.nmi, res.adjscore]) - g["task|best"]).max() <= 1e-12
    # one more step without an optimizer: nothing is updated, the loss and scores come back
    before = {key: v.clone() for key, v in model.state_dict().items()}
    nodes = torch.arange(n, device=cuda)
    got = clustering_train(model, nodes, g["task|y"], None, 3, n_init=5, seed=1, device=cuda)
    assert all(torch.equal(v, before[key]) for key, v in model.state_dict().items()) and np.isfinite(got[0])
    labels = kmeans(model.model_forward(nodes, cuda).detach(), 3, n_init=5, seed=1).labels.cpu().numpy()
    assert len(np.unique(labels * 3 + g["task|block"])) == 3          # the planted partition up to renaming
