"""The fused classification loss (csrc/sgl_class_loss.hip), its wrappers and the node-classification task on a real MI355X: run with
`-m gpu`.

Loss and dZ are compared with F.cross_entropy under CPU autograd, in float32 and in float64 (the truth), through oracle.truth_report --
at most twice as far from the truth as the reference's float32 result, with the condition-aware floor; no tolerance is chosen in this
file, and test_class_loss_cpu.py pins that a plain float32 evaluation passes the rule on these inputs.  The predicted classes must be
torch's CPU arg-max exactly.  Bit-for-bit claims use torch.equal.  The value tests run under torch.profiler: the kernel instances seen
must be the ones the restated selection rule (class_loss_common) announces, and all of them together exactly the compiled ones."""
import itertools
import math

import numpy as np
import pytest
import torch

import oracle
from class_loss_common import (IGNORE, N_ROWS, WIDTHS, argmax_cases, compiled_instances, expected_instance, inputs, parse_kernel_name,
                               reference_pred, references, step_references, unique_maximum, weight)
from far_common import FILL32, GIB, TIERS, FarTable, pick_tier, table_elems
from kmeans_common import LAYOUTS, POISONS, in_layout
from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.tricks import (accuracy, cross_entropy, evaluate, loge_cross_entropy, mini_batch_evaluate, mini_batch_train,
                            node_classification, predict, train)

pytestmark = pytest.mark.gpu
GUARD = 4                                          # guard rows in front of and behind every output


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


class Trace:
    """Runs launches under torch.profiler and checks, at exit, that the class-loss kernel instances that really ran are, in order,
    the ones `expect()` announced; every other kernel is ignored.  A profiler that reports no kernel names fails the comparison."""

    def __init__(self):
        self.expected, self.seen = [], set()

    def expect(self, label, z, dz):
        self.expected.append((label, expected_instance(z, dz)))

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
    if a.dtype == torch.int64:
        return torch.equal(a, b)
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def guarded(n, layout, device, c=None):
    """an output of n rows inside GUARD rows of fill on either side: ([n, c] float32 in the given layout | float32 [n] | int64 [n]
    when c is None and layout names the dtype, the whole buffer, the fill)"""
    if c is None:
        dtype = layout
        fill = -7 if dtype == torch.int64 else -7.0
        whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=device)
        whole[GUARD:GUARD + n] = -1 if dtype == torch.int64 else float("nan")
        return whole[GUARD:GUARD + n], whole, fill
    whole = in_layout(np.full((n + 2 * GUARD, c), -7.0, dtype=np.float32), layout, device)
    view = whole[GUARD:GUARD + n]
    view.fill_(float("nan"))
    return view, whole, -7.0


class Outside:
    """the words of a float32 view's storage that lie outside the view -- pad columns, guard rows, the buffer's ends: unchanged()
    says whether they still hold what they held"""

    def __init__(self, view):
        words = view.untyped_storage().nbytes() // 4
        self.flat = torch.as_strided(view.view(torch.int32), (words,), (1,), 0)
        self.mask = torch.ones(words, dtype=torch.bool, device=view.device)
        torch.as_strided(self.mask, view.shape, view.stride(), view.storage_offset()).fill_(False)
        self.before = self.flat[self.mask].clone()

    def unchanged(self):
        return torch.equal(self.flat[self.mask], self.before)


def guards_kept(whole, fill, n):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + n:] == fill).all())


def step(z, y, layout="padded", w=None, tr=None, label=None):
    """one launch of the low-level call into NaN-filled outputs of the given layout between guard rows: (loss, dZ, row_loss, pred)"""
    n, c = z.shape
    w = weight(y.cpu().numpy(), c) if w is None else w
    dz, dz_all, f1 = guarded(n, layout, z.device, c)
    rows, rows_all, f2 = guarded(n, torch.float32, z.device)
    pred, pred_all, f3 = guarded(n, torch.int64, z.device)
    if tr is not None:
        tr.expect(label, z, dz)
    outside = Outside(dz)
    out = dev.class_loss_grad(z, y, w, dz=dz, row_loss=rows, pred=pred)
    assert out[0] is dz and out[1] is rows and out[2] is pred
    assert outside.unchanged(), "a word of dZ's buffer outside its n x c entries was written"
    assert guards_kept(dz_all, f1, n) and guards_kept(rows_all, f2, n) and guards_kept(pred_all, f3, n), "a guard row was written"
    return float(rows.double().sum() * w), dz, rows, pred


def check_truth(bad, label, loss, dz, refs):
    dz = dz.cpu().numpy()
    if not (np.isfinite(dz).all() and np.isfinite(loss)):
        bad.append((label, "not finite"))
        return
    for what, got, i in (("loss", loss, 0), ("dZ", dz, 1)):
        rep = oracle.truth_report(got, refs["ref32"][i], refs["truth"][i], cond=refs["cond"][i])
        if not rep["ok"]:
            bad.append((label, what, rep))


def on_device(c, layout, cuda):
    z, y = inputs(c)
    return in_layout(z, layout, cuda), torch.from_numpy(y).to(cuda)


# ---- values, in every compiled instance -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_values_in_every_instance(cuda, layout):
    """every width through the C ABI: loss and dZ under the rule, pred equal to torch's CPU arg-max, the pads of z holding NaN and
    1e30 (kmeans_common.in_layout), guard rows around the three outputs; the instances that ran are the announced ones and, together,
    exactly the compiled ones of the layout's lane size"""
    assert any(p != p for p in POISONS)
    bad = []
    with Trace() as tr:
        for c in WIDTHS:
            z, y = on_device(c, layout, cuda)
            if c > 1:
                assert expected_instance(z)[1] == (1 if layout == "odd_view" else 4)
            loss, dz, rows, pred = step(z, y, layout, tr=tr, label=(c, layout))
            check_truth(bad, (c, layout), loss, dz, references(c))
            z_h, y_h = inputs(c)
            if not np.array_equal(pred.cpu().numpy(), reference_pred(z_h)):
                bad.append((c, layout, "pred"))
            ignored = torch.from_numpy(y_h == IGNORE).to(cuda)
            if not (bool((dz[ignored] == 0).all()) and bool((rows[ignored] == 0).all())):
                bad.append((c, layout, "an ignored row is not zero"))
    vec = 1 if layout == "odd_view" else 4
    want = {i for i in compiled_instances() if i[1] == vec}
    print(f"\n[class_loss {layout}] instances seen: {sorted(tr.seen)}")
    assert not bad, bad
    assert tr.seen == want, sorted(want ^ tr.seen)


@pytest.mark.parametrize("c", (3, 7, 47, 172, 1030, 2500))
def test_argmax_ties_and_nans(cuda, c):
    z_h = argmax_cases(c)
    want = reference_pred(z_h)
    assert unique_maximum(z_h[4:8]).all()
    for layout in LAYOUTS:
        z = in_layout(z_h, layout, cuda)
        assert np.array_equal(predict(z).cpu().numpy(), want), (c, layout)
        y = torch.zeros(len(z_h), dtype=torch.int64, device=cuda)
        assert np.array_equal(step(z, y, layout)[3].cpu().numpy(), want), (c, layout, "with the other outputs")
    assert accuracy(torch.from_numpy(z_h).to(cuda), want) == 1.0
    assert accuracy(torch.from_numpy(z_h).to(cuda), (want + 1) % c) == 0.0


# ---- bits -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", (7, 47, 172, 600, 1030))
def test_bits_do_not_depend_on_rows_or_outputs(cuda, c):
    z_h, y_h = inputs(c)
    z, y = torch.from_numpy(z_h).to(cuda), torch.from_numpy(y_h).to(cuda)
    w = weight(y_h, c)

    def run(zz, yy, want=(True, True, True)):
        n = len(zz)
        return dev.class_loss_grad(zz, yy, w, dz=torch.full_like(zz, float("nan")) if want[0] else None,
                                   row_loss=torch.full((n,), float("nan"), device=cuda) if want[1] else None,
                                   pred=torch.full((n,), -1, dtype=torch.int64, device=cuda) if want[2] else None)

    full = run(z, y)
    again = run(z, y)
    assert all(same(a, b) for a, b in zip(full, again)), "two runs differ"
    for want in itertools.product((True, False), repeat=3):           # each of the seven output subsets: the bits of the full launch
        if not any(want):
            continue
        part = run(z, y if (want[0] or want[1]) else None, want)
        for got, ref, asked in zip(part, full, want):
            assert (got is None) == (not asked) and (got is None or same(got, ref)), want
    perm = torch.randperm(N_ROWS, generator=torch.Generator().manual_seed(c)).to(cuda)
    moved = run(z[perm].contiguous(), y[perm].contiguous())
    assert all(same(a, b[perm]) for a, b in zip(moved, full)), "the row's position shows"
    for lo, hi in ((0, 500), (500, N_ROWS), (N_ROWS - 1, N_ROWS), (0, 255)):      # the row set split in two calls; n = 1 and n = 255
        piece = run(z[lo:hi].clone(), y[lo:hi].clone())
        assert all(same(a, b[lo:hi]) for a, b in zip(piece, full)), ("n shows", lo, hi)


def test_pad_columns_never_reach_the_output(cuda):
    """in_layout fills the pads with NaN and 1e30 alternately; the same values from buffers whose pads hold zeros have the same bits"""
    for c in (7, 47, 172, 257, 1030):
        z_h, y_h = inputs(c)
        y = torch.from_numpy(y_h).to(cuda)
        z = in_layout(z_h, "padded", cuda)
        z0 = dev.alloc_rows(N_ROWS, c, cuda)
        z0.copy_(torch.from_numpy(z_h))
        assert expected_instance(z) == expected_instance(z0)
        a, b = step(z, y, "padded"), step(z0, y, "padded")
        assert a[0] == b[0] and all(same(p, q) for p, q in zip(a[1:], b[1:])), c


# ---- edge cases --------------------------------------------------------------------------------------------------------------------------
def test_labels_outside_the_classes_mean_no_label(cuda):
    """labels of c, -1, 2^40 and -100: rows of zeros, nothing read out of bounds, the other rows untouched; all labels ignored: zeros"""
    c = 47
    z_h, y_h = inputs(c)
    y_bad = y_h.copy()
    y_bad[::5], y_bad[1::5], y_bad[2::5] = c, -1, 2 ** 40
    z = torch.from_numpy(z_h).to(cuda)
    _, dz, rows, pred = step(z, torch.from_numpy(y_bad).to(cuda), w=1.0)
    _, dz0, rows0, pred0 = step(z, torch.from_numpy(y_h).to(cuda), w=1.0)
    live = torch.from_numpy((y_bad >= 0) & (y_bad < c)).to(cuda)
    assert bool((dz[~live] == 0).all()) and bool((rows[~live] == 0).all()) and same(pred, pred0)
    assert same(dz[live], dz0[live]) and same(rows[live], rows0[live]), "a bad label touched another row"
    _, dz, rows, pred = step(z, torch.full((N_ROWS,), IGNORE, dtype=torch.int64, device=cuda), w=float("nan"))
    assert bool((dz == 0).all()) and bool((rows == 0).all()) and same(pred, pred0)
    # the public function: check=True refuses them, check=False takes them as ignored; all ignored: NaN mean and zero gradient, as torch
    with pytest.raises(IndexError):
        cross_entropy(z, y_bad, fused=True)
    a = cross_entropy(z, y_bad, fused=True, check=False)
    b = cross_entropy(z, np.where((y_bad >= 0) & (y_bad < c), y_bad, IGNORE), fused=True)
    assert abs(float(a) - float(b)) <= 2.0 ** -22 * abs(float(b))     # (the divisor applied on the device in float64, or folded into w on the host)
    leaf = z.clone().requires_grad_(True)
    loss = cross_entropy(leaf, np.full(N_ROWS, IGNORE), fused=True)
    loss.backward()
    assert math.isnan(float(loss.detach())) and bool((leaf.grad == 0).all())
    assert float(cross_entropy(z, np.full(N_ROWS, IGNORE), fused=True, reduction="sum")) == 0.0


def test_one_class_no_rows_and_a_side_stream(cuda):
    z = torch.from_numpy(inputs(1)[0]).to(cuda)
    y = torch.zeros(N_ROWS, dtype=torch.int64, device=cuda)
    _, dz, rows, pred = step(z, y, w=1.0)                             # C = 1: the loss and the gradient are exactly 0
    assert bool((dz == 0).all()) and bool((rows == 0).all()) and bool((pred == 0).all())
    with Trace():                                                     # n = 0: nothing is launched
        out = dev.class_loss_grad(torch.empty((0, 12), device=cuda), torch.zeros(0, dtype=torch.int64, device=cuda), 1.0, dz=True, row_loss=True,
                                  pred=True)
        assert out[0].shape == (0, 12) and out[1].shape == (0,) and out[2].shape == (0,)
        assert predict(torch.empty((0, 3), device=cuda)).shape == (0,)
    z_h, y_h = inputs(47)
    z, y = torch.from_numpy(z_h).to(cuda), torch.from_numpy(y_h).to(cuda)
    want = step(z, y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = step(z, y)
    side.synchronize()
    assert got[0] == want[0] and all(same(a, b) for a, b in zip(got[1:], want[1:]))
    with pytest.raises(ValueError):
        dev.class_loss_grad(z, y, 1.0)
    with pytest.raises(ValueError):
        dev.class_loss_grad(z, None, 1.0, dz=True)
    with pytest.raises(ValueError):
        dev.class_loss_grad(z, y.to(torch.int32), 1.0, dz=True)
    with pytest.raises(ValueError):
        dev.class_loss_grad(z, y, 1.0, dz=torch.empty((N_ROWS, 48), device=cuda))
    with pytest.raises(TypeError):
        dev.class_loss_grad(z.to(torch.bfloat16), y, 1.0, dz=True)
    with pytest.raises(TypeError):
        cross_entropy(z.to(torch.bfloat16), y, fused=True)


@pytest.mark.parametrize("c", (47, 172, 1030))
def test_large_and_non_finite_rows(cuda, c):
    """rows of magnitude 1e4 stay finite (they are in every case of inputs()); rows holding -inf, +inf or NaN give torch-CPU's
    pattern of non-finite values, in that row alone"""
    z_h, y_h = inputs(c)
    y_h = np.where(y_h == IGNORE, 0, y_h)
    big = np.abs(z_h).max(1) > 9e3
    assert big.sum() > 100
    hz = z_h.copy()
    hz[5, 3] = hz[700, c - 1] = np.nan
    hz[N_ROWS - 1, 0] = np.inf
    free = (y_h[9] + 1) % c
    hz[9, free] = -np.inf                                             # a class of probability 0 ...
    hz[11, y_h[11]] = -np.inf                                         # ... which is the row's label: an infinite loss, a finite gradient
    hz[13, :] = -np.inf
    holed = np.zeros(N_ROWS, dtype=bool)
    holed[[5, 700, N_ROWS - 1, 9, 11, 13]] = True
    zt = torch.from_numpy(hz).requires_grad_(True)
    per_row = torch.nn.functional.cross_entropy(zt, torch.from_numpy(y_h), reduction="none")
    per_row.sum().backward()
    for layout in LAYOUTS:
        y = torch.from_numpy(y_h).to(cuda)
        _, dz, rows, pred = step(in_layout(hz, layout, cuda), y, layout, w=1.0)
        _, dz0, rows0, pred0 = step(in_layout(z_h, layout, cuda), y, layout, w=1.0)
        assert bool(torch.isfinite(dz0).all()) and bool(torch.isfinite(rows0).all())
        keep = torch.from_numpy(~holed).to(cuda)
        assert same(dz[keep], dz0[keep]) and same(rows[keep], rows0[keep]) and same(pred[keep], pred0[keep]), "a non-finite row touched its neighbours"
        got_rows, got_dz = rows.cpu().numpy(), dz.cpu().numpy()
        assert np.array_equal(np.isnan(got_rows), np.isnan(per_row.detach().numpy())), layout
        assert np.array_equal(np.isposinf(got_rows), np.isposinf(per_row.detach().numpy())), layout
        assert np.array_equal(np.isnan(got_dz), np.isnan(zt.grad.numpy())), layout
        assert np.isnan(got_dz[[5, 700, N_ROWS - 1, 13]]).all() and np.isfinite(got_dz[[9, 11]]).all() and got_rows[11] == np.inf
        assert got_dz[9, free] == 0.0 and got_dz[11, y_h[11]] == -1.0
        assert np.array_equal(pred.cpu().numpy(), reference_pred(hz))


# ---- autograd -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", (7, 47))
def test_autograd(cuda, c):
    z_h, y_h = inputs(c)
    refs = references(c)
    z, y = torch.from_numpy(z_h).to(cuda), torch.from_numpy(y_h).to(cuda)
    w = weight(y_h, c)
    want_dz, want_rows, want_pred = dev.class_loss_grad(z, torch.where(y < 0, -1, y), w, dz=True, row_loss=True, pred=True)
    want_loss = (want_rows.double().sum() * w).float()
    out = z.clone().requires_grad_(True)
    loss, pred = cross_entropy(out, y, fused=True, return_pred=True)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and float(loss.detach()) == float(want_loss) and same(pred, want_pred)
    assert not pred.requires_grad
    loss.backward()
    assert same(out.grad.contiguous(), want_dz.contiguous())
    with pytest.raises(RuntimeError):                                 # the buffer was handed out
        out2 = z.clone().requires_grad_(True)
        twice = cross_entropy(out2, y, fused=True)
        twice.backward(retain_graph=True)
        twice.backward()
    out3 = z.clone().requires_grad_(True)
    (cross_entropy(out3, y_h, fused=True) * 3.0).backward()           # ndarray labels; an upstream factor of 3
    assert same(out3.grad.contiguous(), (want_dz * 3.0).contiguous())
    with torch.no_grad():
        assert float(cross_entropy(out, y, fused=True)) == float(want_loss)
    bad = []
    for fused in (True, False):                                       # both routes under the rule, mean and sum, with and without the host read
        for reduction, check in (("mean", True), ("mean", False), ("sum", True)):
            leaf = z.clone().requires_grad_(True)
            got = cross_entropy(leaf, y, reduction=reduction, check=check, fused=fused)
            got.backward()
            check_truth(bad, (fused, reduction, check), float(got.detach()), leaf.grad,
                        refs if reduction == "mean" else step_references(z_h, y_h, reduction="sum"))
    assert not bad, bad
    # LogeCrossEntropy: the scalar transform's factor reaches dZ through the backward
    eps = 1.0 - math.log(2)
    chain = 1.0 / (eps + refs["truth"][0])
    for fused in (True, False):
        leaf = z.clone().requires_grad_(True)
        got = loge_cross_entropy(leaf, y, fused=fused)
        got.backward()
        zz = torch.from_numpy(z_h).double().requires_grad_(True)
        truth = torch.log(eps + torch.nn.functional.cross_entropy(zz, torch.from_numpy(y_h))) - math.log(eps)
        truth.backward()
        z32 = torch.from_numpy(z_h).requires_grad_(True)
        ref32 = torch.log(eps + torch.nn.functional.cross_entropy(z32, torch.from_numpy(y_h))) - math.log(eps)
        ref32.backward()
        check_truth(bad, ("loge", fused), float(got.detach()), leaf.grad,
                    {"ref32": (float(ref32.detach()), z32.grad.numpy()), "truth": (float(truth.detach()), zz.grad.numpy()),
                     "cond": (refs["cond"][0] * chain, refs["cond"][1] * chain)})
    assert not bad, bad


def test_gradients_reach_a_linear_layer(cuda):
    """cross_entropy and loge_cross_entropy behind a Linear layer, fused and unfused, against CPU autograd in float32 and float64; cond
    of a weight gradient = sum over the rows of |dZ| |x| (a sum of cancelling terms, as in K12's Linear case)"""
    c, f = 47, 24
    rng = np.random.default_rng(72000)
    x_h = rng.standard_normal((N_ROWS, f)).astype(np.float32)
    y_h = inputs(c)[1]
    torch.manual_seed(3)
    lin = torch.nn.Linear(f, c)
    state = {k: v.clone() for k, v in lin.state_dict().items()}
    eps = 1.0 - math.log(2)
    fns = {"ce": lambda out, y: torch.nn.functional.cross_entropy(out, y),
           "loge": lambda out, y: torch.log(eps + torch.nn.functional.cross_entropy(out, y)) - math.log(eps)}
    ours = {"ce": cross_entropy, "loge": loge_cross_entropy}
    bad = []
    for name, fn in fns.items():
        cpu = {}
        for tag, dt in (("ref32", torch.float32), ("truth", torch.float64)):
            m = torch.nn.Linear(f, c).to(dt)
            m.load_state_dict({k: v.to(dt) for k, v in state.items()})
            out = m(torch.from_numpy(x_h).to(dt))
            out.retain_grad()
            loss = fn(out, torch.from_numpy(y_h))
            loss.backward()
            cpu[tag] = (float(loss.detach()), m.weight.grad.numpy(), out.grad.numpy())
        cond = np.abs(cpu["truth"][2]).T @ np.abs(x_h.astype(np.float64))
        for fused in (True, False):
            m = torch.nn.Linear(f, c)
            m.load_state_dict(state)
            m = m.to(cuda)
            loss = ours[name](m(torch.from_numpy(x_h).to(cuda)), y_h, fused=fused)
            loss.backward()
            rep = oracle.truth_report(m.weight.grad.cpu().numpy(), cpu["ref32"][1], cpu["truth"][1], cond=cond)
            rep_loss = oracle.truth_report(float(loss.detach()), cpu["ref32"][0], cpu["truth"][0])
            print(name, fused, rep, rep_loss)
            if not (rep["ok"] and rep_loss["ok"]):
                bad.append((name, fused, rep, rep_loss))
    assert not bad, bad


# ---- the reference fixture ------------------------------------------------------------------------------------------------------------------
class Stub(torch.nn.Module):
    """G21's stub model: model_forward = a Linear layer over the rows of a fixed feature matrix, postprocess = a fixed matrix applied
    to the output"""

    def __init__(self, g, device, post=False):
        super().__init__()
        self.lin = torch.nn.Linear(g["loop|x"].shape[1], g["loop|state|lin.bias"].shape[0])
        self.load_state_dict({key[len("loop|state|"):]: torch.from_numpy(v) for key, v in g.items() if key.startswith("loop|state|")})
        self.x = torch.from_numpy(g["loop|x"]).to(device)
        self.post = torch.from_numpy(g["task|post"]).to(device) if post else None

    def preprocess(self, adj, x):
        pass

    def model_forward(self, idx, device):
        if isinstance(idx, range):
            idx = list(idx)
        return self.lin(self.x[torch.as_tensor(np.asarray(idx) if not torch.is_tensor(idx) else idx, dtype=torch.long, device=self.x.device)])

    def postprocess(self, adj, out):
        return out if self.post is None else self.post @ out


def check_history(name, got, g, key, model):
    got = np.array(got, dtype=np.float64)
    rep = oracle.truth_report(got[:, 0], g[key + "|history"][:, 0], g[key + "|history64"][:, 0])
    print(name, got[:, 0], g[key + "|history"][:, 0], rep)
    assert rep["ok"], (name, rep)
    assert np.array_equal(got[:, 1:], g[key + "|history"][:, 1:]), (name, got, g[key + "|history"])     # the same predictions: the same accuracies
    if model is not None:
        for p in ("lin.weight", "lin.bias"):
            rep = oracle.truth_report(model.state_dict()[p].cpu().numpy(), g[f"{key}|final|{p}"], g[f"{key}|final64|{p}"])
            print(name, p, rep)
            assert rep["ok"], (name, p, rep)


def test_reference_fixture_step_and_accuracy(cuda, goldens):
    """G21 (a) and (b) through the public functions"""
    g = goldens.npz("g21_node_classification")
    z, y = g["step|z"], g["step|labels"]
    cond = step_references(z, y)["cond"]
    eps = 1.0 - math.log(2)
    chain = 1.0 / (eps + float(g["step|ce|loss64"]))
    for name, fn, scale in (("ce", cross_entropy, 1.0), ("loge", loge_cross_entropy, chain)):
        for fused in (True, False):
            out = torch.from_numpy(z).to(cuda).requires_grad_(True)
            loss = fn(out, y, fused=fused)
            loss.backward()
            reps = (oracle.truth_report(float(loss.detach()), g[f"step|{name}|loss"], g[f"step|{name}|loss64"], cond=cond[0] * scale),
                    oracle.truth_report(out.grad.cpu().numpy(), g[f"step|{name}|grad"], g[f"step|{name}|grad64"], cond=cond[1] * scale))
            print(name, fused, float(loss.detach()), reps)
            assert reps[0]["ok"] and reps[1]["ok"], (name, fused, reps)
    t = torch.from_numpy(g["acc|z"]).to(cuda)
    assert np.array_equal(predict(t).cpu().numpy(), g["acc|pred"])
    assert accuracy(t, g["acc|labels"]) == float(g["acc|value"]) == accuracy(t, torch.from_numpy(g["acc|labels"]).to(cuda))


@pytest.mark.parametrize("loss_fn", ("cross_entropy", "loge", "callable"))
def test_reference_fixture_full_batch_loop(cuda, goldens, loss_fn):
    """G21 (c): three epochs of train + evaluate"""
    g = goldens.npz("g21_node_classification")
    model = Stub(g, cuda).to(cuda)
    opt = torch.optim.Adam(model.parameters(), lr=float(g["loop|lr"]), weight_decay=0.0)
    y = torch.from_numpy(g["loop|y"]).to(cuda)
    fn = (lambda out, lab: torch.nn.functional.cross_entropy(out, lab)) if loss_fn == "callable" else loss_fn
    rows = []
    for _ in range(int(g["loop|epochs"])):
        loss, acc = train(model, g["loop|train_idx"], y, cuda, opt, fn)
        assert isinstance(loss, float) and isinstance(acc, float)
        rows.append((loss, acc) + evaluate(model, g["loop|val_idx"], g["loop|test_idx"], y, cuda))
    check_history(loss_fn, rows, g, "full|loge" if loss_fn == "loge" else "full|ce", model)


def test_reference_fixture_mini_batch_loop(cuda, goldens):
    """G21 (c): three epochs of mini_batch_train + mini_batch_evaluate over the recorded batch lists"""
    g = goldens.npz("g21_node_classification")
    model = Stub(g, cuda).to(cuda)
    opt = torch.optim.Adam(model.parameters(), lr=float(g["loop|lr"]), weight_decay=0.0)
    y = torch.from_numpy(g["loop|y"]).to(cuda)
    step_ = int(g["loop|eval_batch"])
    cut = lambda idx: [idx[i:i + step_] for i in range(0, len(idx), step_)]
    rows = []
    for _ in range(int(g["loop|epochs"])):
        loss, acc = mini_batch_train(model, g["loop|train_idx"], list(g["loop|train_batches"]), y, cuda, opt, "cross_entropy")
        rows.append((loss, acc) + mini_batch_evaluate(model, g["loop|val_idx"], cut(g["loop|val_idx"]), g["loop|test_idx"], cut(g["loop|test_idx"]),
                                                      y, cuda))
    check_history("mini", rows, g, "mini|ce", model)


def test_reference_fixture_task(cuda, goldens):
    """G21 (d): NodeClassification._execute, full batch and with the recorded mini-batches"""
    g = goldens.npz("g21_node_classification")
    kw = dict(epochs=int(g["loop|epochs"]), lr=float(g["loop|lr"]), weight_decay=0.0, device=cuda)
    idx = (g["loop|train_idx"], g["loop|val_idx"], g["loop|test_idx"])
    res = node_classification(Stub(g, cuda, post=True), "adj", None, g["loop|y"], *idx, **kw)
    check_history("task", [[h["loss"], h["acc_train"], h["acc_val"], h["acc_test"]] for h in res.history[:-1]], g, "task", None)
    assert res.history[-1] == dict(epoch="post", acc_val=g["task|post|acc"][0], acc_test=g["task|post|acc"][1])
    assert [res.best_val, res.best_test] == g["task|best"].tolist()
    res = node_classification(Stub(g, cuda), "adj", None, g["loop|y"], *idx, eval_batch_size=int(g["loop|eval_batch"]),
                              batches={"train": list(g["loop|train_batches"])}, **kw)
    check_history("task mini", [[h["loss"], h["acc_train"], h["acc_val"], h["acc_test"]] for h in res.history[:-1]], g, "mini|ce", None)


# ---- the task on a planted graph ----------------------------------------------------------------------------------------------------------
def test_node_classification_on_a_planted_graph(cuda):
    """N = 2000, 4 planted blocks, SGC (two hops, then a Linear layer), 3 epochs: the history is reproducible for one seed, full batch
    and mini-batch, and every accuracy is the one numpy computes from model_forward"""
    import scipy.sparse as sp
    from sgl_amd.models.homo import SGC
    n, k, f = 2000, 4, 16
    rng = np.random.default_rng(73000)
    block = rng.integers(0, k, n)
    prob = np.where(block[:, None] == block[None, :], 0.02, 0.001)
    upper = np.triu(rng.random((n, n)) < prob, 1)
    adj = sp.csr_matrix((upper | upper.T).astype(np.float32))
    x = (rng.standard_normal((k, f))[block] * 0.5 + rng.standard_normal((n, f))).astype(np.float32)
    order = rng.permutation(n)
    tr, va, te = order[:800], order[800:1400], order[1400:]

    def run(**kw):
        torch.manual_seed(7)
        model = SGC(2, f, k)
        res = node_classification(model, adj, x, block, tr, va, te, epochs=3, lr=0.05, weight_decay=0.0, seed=11, device=cuda, **kw)
        return model, res

    model, res = run()
    assert res.history == run()[1].history, "one seed, two histories"
    assert len(res.history) == 4 and all(np.isfinite(h["loss"]) for h in res.history[:-1])
    assert res.history[2]["loss"] < res.history[0]["loss"] and res.best_val > 1.5 / k
    model.eval()
    with torch.no_grad():
        out = model.model_forward(range(n), cuda).cpu().numpy()
    pred = out.argmax(1)
    assert res.history[-1] == dict(epoch="post", acc_val=float((pred[va] == block[va]).mean()), acc_test=float((pred[te] == block[te]).mean()))
    yt = torch.from_numpy(block).to(cuda)
    assert evaluate(model, va, te, yt, cuda) == (res.history[-1]["acc_val"], res.history[-1]["acc_test"])
    mini = run(train_batch_size=256, eval_batch_size=512)[1]
    assert mini.history == run(train_batch_size=256, eval_batch_size=512)[1].history
    assert mini.history[0]["loss"] != res.history[0]["loss"] and mini.best_val > 1.5 / k


# ---- offsets beyond 2^32 elements -----------------------------------------------------------------------------------------------------------
def test_far_offsets(cuda):
    """Z and dZ as column ranges of rows of one table whose last rows start beyond 2^32 elements (2^31 at the smaller tier): the
    acceptance rule, the bits of the same rows computed in a small matrix, and the table swept for words off its fill afterwards"""
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    tier = pick_tier(free)
    if tier is None:
        pytest.skip(f"the far-offset case needs {TIERS['B'][0] / GIB:.0f} GiB of free device memory, {free / GIB:.1f} GiB are free")
    flat = torch.empty(table_elems(tier), dtype=torch.float32, device=cuda)
    words = flat.view(torch.int32)
    words.fill_(FILL32)
    table = FarTable(flat, TIERS[tier][1])
    lay = table.layout(N_ROWS)
    bad = []
    for c in (47, 1030):                                              # a register instance and the streaming one
        z_h, y_h = inputs(c)
        z, dz = lay.take(c), lay.take(c)
        assert z.far_rows(table.threshold) > 0 and dz.far_rows(table.threshold) > 0
        assert int(y_h[-1]) != IGNORE                                 # the farthest row is live
        z.t.copy_(torch.from_numpy(z_h))
        y = torch.from_numpy(y_h).to(cuda)
        w = weight(y_h, c)
        rows = torch.full((N_ROWS,), float("nan"), device=cuda)
        pred = torch.full((N_ROWS,), -1, dtype=torch.int64, device=cuda)
        dev.class_loss_grad(z.t, y, w, dz=dz.t, row_loss=rows, pred=pred)
        check_truth(bad, ("far", c), float(rows.double().sum() * w), dz.t, references(c))
        zn = dev.alloc_rows(N_ROWS, c, cuda)                          # the same call on ordinary buffers: the same bits
        zn.copy_(torch.from_numpy(z_h))
        near = dev.class_loss_grad(zn, y, w, dz=True, row_loss=True, pred=True)
        assert expected_instance(z.t, dz.t) == expected_instance(zn, near[0])
        if not (same(dz.t.contiguous(), near[0].contiguous()) and same(rows, near[1]) and same(pred, near[2])):
            bad.append(("far and near buffers give different bits", c))
        lay.refill()
    stray = 0
    for lo in range(0, words.numel(), 1 << 28):
        stray += int(torch.count_nonzero(words[lo:lo + (1 << 28)] != FILL32))
    print(f"\n[far class_loss] tier {tier}, pitch {lay.ld}: words off the fill afterwards: {stray}")
    del table, lay, z, dz, words, flat
    torch.cuda.empty_cache()
    assert not bad, bad
    assert stray == 0
