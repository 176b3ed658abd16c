"""Every kernel whose launcher caps its grid, run in its STRIDED form -- a workgroup walks more than one batch of rows or block of
elements -- against the reference its own test file uses, on a real MI355X: run with `-m gpu`.

The other GPU tests run at 1031, 77 or 257 rows, where no launch reaches its cap: every loop of the form
`for (b = blockIdx.x; b < n_batches; b += gridDim.x)` runs at most once per workgroup there.  Here each such loop runs two times or
more, with uneven trip counts and a partial last batch (test_strided_cpu.py proves that from the restated launch arithmetic, case by
case), in three ways:
(a) the tuning key loss_blocks caps the grid of K9 (k-means assignment), K12 (cluster loss), K14 (class loss) and K11's fold at 1,
    then 3 workgroups (and one more value where 3 would leave every workgroup the same trip count) at the shapes of their own tests;
(b) the tuning key agg_blocks does the same for the streaming aggregators behind stream_grid();
(c) K9, K12, K11's fold, K13 / K15 (CSR select / merge), the wsum1d backward and edge_fill run at the smallest sizes that exceed
    their own caps.  (K14's cap of 2^20 workgroups needs 9 GB of logits: it is reached through the key alone.)

The references, tolerances and acceptance rules are those of test_gpu_kmeans.py, test_gpu_cluster_loss.py, test_gpu_class_loss.py,
test_gpu_edge_loss.py, test_gpu_csr_select.py, test_gpu_csr_merge.py and test_gpu_far_offsets.py, imported from there: none is chosen
here.  On top of them every strided run must have the bits of the run with the key at 0 (a: the kernels' results do not depend on
the position of a row, on n or on the grid -- test_bits_do_not_depend_on_* of the files above), or of calls on slices short enough not
to stride (c).  Outputs start filled with a sentinel; what lies outside them must keep it in every round.

A tuning key is set inside try / finally only, and an autouse fixture checks that both keys read 0 before and after every test: the
multi-process tests are collected later in the same process."""
import contextlib

import numpy as np
import pytest
import torch

import class_loss_common as zlc
import cluster_loss_common as clc
import csr_merge_common as cmc
import csr_select_common as csc
import kmeans_common as kc
import oracle
import strided_common as sc
import test_gpu_class_loss as tz
import test_gpu_cluster_loss as tc
import test_gpu_edge_loss as te
from agg_rows_common import reduce_statement, rne, same_bits32
from edge_loss_common import labels_for, references as edge_references, step_references as edge_step_references
from edge_scores_common import host_matrix
from inputs import hash_matrix
from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.transforms import drop_threshold
from sgl_amd.tricks import EdgePlan
from test_gpu_csr_merge import raw_merge
from test_gpu_csr_merge import upload as upload_merge
from test_gpu_csr_select import agrees as select_agrees
from test_gpu_csr_select import raw_select
from test_gpu_csr_select import upload as upload_select
from test_gpu_kmeans import check_case

pytestmark = pytest.mark.gpu

KEYS = ("loss_blocks", "agg_blocks")
FILL32 = 0x7FC0BEEF                                # a NaN with a payload: the sentinel of the aggregator outputs
FILL16 = 0x7FDE
NAN = float("nan")
OPS = {"sum": _lib.SGL_REDUCE_SUM, "mean": _lib.SGL_REDUCE_MEAN, "max": _lib.SGL_REDUCE_MAX, "min": _lib.SGL_REDUCE_MIN,
       "wsum": _lib.SGL_REDUCE_WSUM}


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def keys_at_rest():
    assert [_lib.get_tuning(k) for k in KEYS] == [0, 0], "a tuning key was left set before this test"
    yield
    left = [_lib.get_tuning(k) for k in KEYS]
    for k in KEYS:
        _lib.set_tuning(k, 0)
    assert left == [0, 0], "this test left a tuning key set"


@contextlib.contextmanager
def capped(key, value):
    try:
        _lib.set_tuning(key, value)
        yield
    finally:
        _lib.set_tuning(key, 0)


def raw(t):
    kind = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.contiguous().view(kind)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(raw(a), raw(b))


class Outside:
    """the elements of a view's storage that lie outside the view -- pad columns, guard rows, the buffer's ends: unchanged() says
    whether they still hold what they held"""

    def __init__(self, view):
        kind = {2: torch.int16, 4: torch.int32, 8: torch.int64}[view.element_size()]
        words = view.untyped_storage().nbytes() // view.element_size()
        self.flat = torch.as_strided(view.view(kind), (words,), (1,), 0)
        self.mask = torch.ones(words, dtype=torch.bool, device=view.device)
        torch.as_strided(self.mask, view.shape, view.stride(), view.storage_offset()).fill_(False)
        self.before = self.flat[self.mask].clone()

    def unchanged(self):
        return torch.equal(self.flat[self.mask], self.before)


# =========================================================================================================================================
# (a) forced caps at today's shapes
# =========================================================================================================================================
def assign_in(d, k, layout, cuda):
    return kc.in_layout(kc.host_x(d), layout, cuda), kc.in_layout(kc.host_centres(d, k), layout, cuda)


def k9_forced(d, k, layout, cuda):
    """check_case under every forced cap, and the bits of the uncapped run"""
    bad = []
    x, c = assign_in(d, k, layout, cuda)
    base = dev.kmeans_assign(x, c)
    for cap in sc.forced_caps(sc.k9_grid(d, k, sc.vec_of(layout, d, k), kc.N_ROWS).work):
        with capped("loss_blocks", cap):
            bad += [("cap", cap) + b for b in check_case(d, k, layout, cuda)]
            labels = torch.full((kc.N_ROWS + 2,), -7, dtype=torch.int64, device=cuda)         # nothing before or after the n outputs
            mindist = torch.full((kc.N_ROWS + 2,), -7.0, dtype=torch.float32, device=cuda)
            dev._call(cuda, "sgl_kmeans_assign_f32", _lib.ptr(x), dev._ld(x), kc.N_ROWS, d, _lib.ptr(c), dev._ld(c), k, _lib.ptr(labels[1:]),
                      _lib.ptr(mindist[1:]))
            only = dev.kmeans_assign(x, c, want_dist=False)[0]
        if not (same(labels[1:-1], base[0]) and same(mindist[1:-1], base[1]) and same(only, base[0])):
            bad.append((d, k, layout, cap, "bits differ from the uncapped run"))
        if not (labels[0] == -7 and labels[-1] == -7 and mindist[0] == -7 and mindist[-1] == -7):
            bad.append((d, k, layout, cap, "a guard element was written"))
    return bad


@pytest.mark.parametrize("layout", kc.LAYOUTS)
@pytest.mark.parametrize("d", kc.WIDTHS)
def test_k9_forced_caps_in_every_instance(cuda, d, layout):
    bad = []
    for k in kc.KS:
        bad += k9_forced(d, k, layout, cuda)
    assert not bad, bad


@pytest.mark.parametrize("layout", kc.LAYOUTS)
@pytest.mark.parametrize("d,k", kc.BIG)
def test_k9_forced_caps_across_tiles_and_in_the_stream_kernel(cuda, d, k, layout):
    bad = k9_forced(d, k, layout, cuda)
    assert not bad, bad


GUARD = 4


def k12_step(x, c, y, layout, cuda, w=None):
    """one launch into a NaN-filled dX of the given layout between guard rows of -7 (its pads poisoned by in_layout) and a NaN-filled
    row_loss between guard elements: (loss, dX, row_loss); nothing outside the n x d and n outputs may change"""
    n, d = x.shape
    whole = kc.in_layout(np.full((n + 2 * GUARD, d), -7.0, dtype=np.float32), layout, cuda)
    dx = whole[GUARD:GUARD + n]
    dx.fill_(NAN)
    rows_all = torch.full((n + 2 * GUARD,), -7.0, device=cuda)
    rows = rows_all[GUARD:GUARD + n]
    rows.fill_(NAN)
    outside = Outside(dx)
    w = 1.0 / n if w is None else w
    dev.cluster_loss_grad(x, c, y, w, dx=dx, row_loss=rows)
    assert outside.unchanged(), "an element of dX's buffer outside its n x d entries was written"
    assert bool((rows_all[:GUARD] == -7).all()) and bool((rows_all[GUARD + n:] == -7).all()), "a guard element of row_loss was written"
    return float(rows.double().sum() * w), dx, rows


def k12_forced(d, k, layout, cuda):
    bad = []
    x, c, y = tc.on_device(d, k, layout, cuda)
    base = k12_step(x, c, y, layout, cuda)
    assert clc.expected_instance(x, c, base[1]) == sc.k12_instance(d, sc.vec_of(layout, d, k))
    for cap in sc.forced_caps(sc.k12_grid(d, k, sc.vec_of(layout, d, k), kc.N_ROWS).work):
        with capped("loss_blocks", cap):
            loss, dx, rows = k12_step(x, c, y, layout, cuda)
        tc.check_truth(bad, (d, k, layout, cap), loss, dx, clc.references(d, k))
        if not (loss == base[0] and same(dx, base[1]) and same(rows, base[2])):
            bad.append((d, k, layout, cap, "bits differ from the uncapped run"))
    return bad


@pytest.mark.parametrize("layout", kc.LAYOUTS)
@pytest.mark.parametrize("d", clc.WIDTHS)
def test_k12_forced_caps_in_every_instance(cuda, d, layout):
    bad = []
    for k in clc.KS:
        bad += k12_forced(d, k, layout, cuda)
    assert not bad, bad


@pytest.mark.parametrize("layout", kc.LAYOUTS)
@pytest.mark.parametrize("d,k", kc.BIG)
def test_k12_forced_caps_across_tiles_and_in_the_stream_kernel(cuda, d, k, layout):
    bad = k12_forced(d, k, layout, cuda)
    assert not bad, bad


_TIES = {}


def k14_hostile(c):
    """(z, labels) of class_loss_common.inputs(c) with NaN rows in the middle and -- the last 64 rows, a later round under every forced
    cap -- the constructed arg-max ties and NaNs of argmax_cases(c)"""
    if c not in _TIES:
        z, y = zlc.inputs(c)
        z, y = z.copy(), y.copy()
        z[[300, 301, 777], [0, c - 1, c // 2]] = np.nan
        if c >= 3:
            z[-64:] = zlc.argmax_cases(c)
        _TIES[c] = (z, y)
    return _TIES[c]


@pytest.mark.parametrize("layout", kc.LAYOUTS)
@pytest.mark.parametrize("c", zlc.WIDTHS)
def test_k14_forced_caps_in_every_instance(cuda, c, layout):
    """dZ, row_loss and pred together under the rule of test_gpu_class_loss.py, with ignored labels; then NaN rows and the arg-max tie
    cases, pred exactly torch's CPU arg-max, with the other outputs and alone; all with the bits of the uncapped run"""
    bad = []
    z_h, y_h = zlc.inputs(c)
    z, y = tz.on_device(c, layout, cuda)
    vec = 1 if layout == "odd_view" else 4
    t_h, _ = k14_hostile(c)
    t = kc.in_layout(t_h, layout, cuda)
    want_pred, want_t = zlc.reference_pred(z_h), zlc.reference_pred(t_h)
    ignored = torch.from_numpy(y_h == zlc.IGNORE).to(cuda)
    clean = np.ones(zlc.N_ROWS, dtype=bool)
    clean[[300, 301, 777]] = False
    clean[-64:] = c < 3
    clean = torch.from_numpy(clean).to(cuda)
    base, base_t = tz.step(z, y, layout), tz.step(t, y, layout)
    assert zlc.expected_instance(z, base[1]) == sc.k14_instance(c, vec)[:3]
    for cap in sc.forced_caps(sc.k14_grid(c, vec, zlc.N_ROWS).work):
        with capped("loss_blocks", cap):
            loss, dz, rows, pred = tz.step(z, y, layout)
            _, dz_t, rows_t, pred_t = tz.step(t, y, layout)
            alone = dev.class_loss_grad(t, None, 1.0, pred=torch.full((zlc.N_ROWS,), -1, dtype=torch.int64, device=cuda))[2]
        tz.check_truth(bad, (c, layout, cap), loss, dz, zlc.references(c))
        if not np.array_equal(pred.cpu().numpy(), want_pred):
            bad.append((c, layout, cap, "pred"))
        if not (np.array_equal(pred_t.cpu().numpy(), want_t) and np.array_equal(alone.cpu().numpy(), want_t)):
            bad.append((c, layout, cap, "pred of the tie and NaN rows"))
        if not (bool((dz[ignored] == 0).all()) and bool((rows[ignored] == 0).all())):
            bad.append((c, layout, cap, "an ignored row is not zero"))
        if not (loss == base[0] and all(same(a, b) for a, b in zip((dz, rows, pred), base[1:]))):
            bad.append((c, layout, cap, "bits differ from the uncapped run"))
        if not all(same(a, b) for a, b in zip((dz_t, rows_t, pred_t), base_t[1:])):
            bad.append((c, layout, cap, "tie and NaN rows: bits differ from the uncapped run"))
        if not (same(dz_t[clean], dz[clean]) and same(rows_t[clean], rows[clean])):
            bad.append((c, layout, cap, "a NaN row or a tie touched another row"))
    assert not bad, bad


@pytest.mark.parametrize("which,max_piece", (("edges", 1), ("edges", 8), ("hub", 1), ("hub", 8)))
def test_k11_fold_forced_caps(cuda, which, max_piece):
    """the plans of test_gpu_edge_loss.py that have cut rows: dZ against the float64 step references, bit-equal to the uncapped run"""
    plan = te.plan_for(cuda, which, max_piece)
    n_fold = int(plan.fold.shape[0])
    assert n_fold > 0 and plan.n_partial > n_fold
    bad = []
    with te.Trace() as tr:
        for d in te.BIT_WIDTHS:
            for layout in te.LAYOUTS:
                z = te.LAYOUTS[layout](host_matrix(d), cuda)
                for mode in ("sigmoid", "none"):
                    refs = edge_references(d, mode, which)
                    base = te.step(tr, d, z, plan, mode, layout)
                    for cap in sc.forced_caps(sc.fold_grid(n_fold).work):
                        with capped("loss_blocks", cap):
                            loss, dz, score, coef = te.step(tr, d, z, plan, mode, layout)
                        te.check_truth(bad, (d, layout, mode, cap), loss, dz, refs)
                        if not (loss == base[0] and same(dz, base[1]) and same(score, base[2]) and same(coef, base[3])):
                            bad.append((d, layout, mode, cap, "bits differ from the uncapped run"))
    assert not bad, bad


# =========================================================================================================================================
# (b) forced agg_blocks
# =========================================================================================================================================
_HOPS = {}


def hops_host(n, d, H):
    have = _HOPS.setdefault((n, d), [])
    for h in range(len(have), H):
        have.append(np.ascontiguousarray((hash_matrix(n, d, seed=8100 + 31 * d + h) * np.float32(1.0 - 0.04 * h)).astype(np.float32)))
    return have[:H]


def hop_weights(H):
    return (np.float32(0.75) ** np.arange(H, dtype=np.float32) * np.where(np.arange(H) % 3 == 2, -1, 1)).astype(np.float32)


class Buffers:
    """inputs and sentinel-filled outputs of one launch.  vec4: row-padded buffers from dev.alloc_rows (16-byte rows), else odd-pitch
    ones -- dense inputs, outputs as columns 1 .. of a buffer three columns wider.  check(): every element outside the outputs'
    declared columns still holds the sentinel"""

    def __init__(self, vec4, cuda):
        self.vec4, self.cuda, self.watch = vec4, cuda, []

    def inp(self, host):
        host = host if torch.is_tensor(host) else torch.from_numpy(np.ascontiguousarray(host))
        if not self.vec4:
            return host.to(self.cuda)
        t = dev.alloc_rows(host.shape[0], host.shape[1], self.cuda, zero_pad=False, dtype=host.dtype)
        self.fill(dev.padded_parent(t))
        t.copy_(host)
        return t

    @staticmethod
    def fill(t):
        if t.element_size() == 4:
            t.view(torch.int32).fill_(FILL32)
        else:
            t.view(torch.int16).fill_(FILL16)

    def out(self, n, width, dtype=torch.float32, aligned=None):
        if self.vec4 if aligned is None else aligned:
            whole = dev.alloc_rows(n + 2, width, self.cuda, zero_pad=False, dtype=dtype)      # a guard row on either side
            self.fill(dev.padded_parent(whole))
            t = whole[1:-1]
        else:
            parent = torch.empty((n + 2, width + 3), dtype=dtype, device=self.cuda)
            self.fill(parent)
            t = parent[1:-1, 1:1 + width]
        self.watch.append(Outside(t))
        return t

    def check(self):
        return all(w.unchanged() for w in self.watch)


def call(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.current_stream_ptr()), name)


def P(t):
    return None if t is None else _lib.ptr(t)


def ld(t):
    return t.stride(0)


def agg_launch(case, cuda):
    """one launch of the case's entry point(s) into fresh sentinel-filled outputs: ({name: output}, Buffers)"""
    name, _, n, d, H, vec4, pad = case
    b = Buffers(vec4, cuda)
    hosts = hops_host(n, d, H)
    out = {}
    if name in ("reduce16", "reduce_odd"):
        xs = [b.inp(h) for h in hosts]
        ptrs, lds = _lib.hop_arrays(xs)
        w1d = torch.from_numpy(hop_weights(H)).to(cuda)
        for kind, op in OPS.items():
            out[kind] = b.out(n, d)
            call("sgl_hop_reduce_f32", op, H, ptrs, lds, P(w1d) if kind == "wsum" else None, P(out[kind]), ld(out[kind]), n, d)
    elif name == "wsum2d":
        xs, w = [b.inp(h) for h in hosts], b.inp(oracle.softmax32(hash_matrix(n, H, seed=d + H), 1))
        ptrs, lds = _lib.hop_arrays(xs)
        out["fma"] = b.out(n, d)
        call("sgl_hop_wsum2d_f32", H, ptrs, lds, P(w), ld(w), P(out["fma"]), ld(out["fma"]), n, d)
        out["nafs"], out["W"] = b.out(n, d), b.out(n, H, aligned=True)
        try:                                                              # the two-pass NAFS path: rounded products, then adds
            _lib.set_tuning("nafs_fused", 0)
            call("sgl_nafs_padded_f32", H, ptrs, lds, P(out["nafs"]), ld(out["nafs"]), 0, P(out["W"]), ld(out["W"]), n, d)
        finally:
            _lib.set_tuning("nafs_fused", 1)
    elif name == "wsum2d_dx":
        xs, w, g = [b.inp(h) for h in hosts], b.inp(oracle.softmax32(hash_matrix(n, H, seed=d + H), 1)), b.inp(hash_matrix(n, d, seed=5 * d + 2))
        dxs = [None if h == 1 else b.out(n, d) for h in range(H)]                          # hop 1: nobody asked for its gradient
        ptrs, lds = _lib.hop_arrays(xs)
        dptrs, dlds = _lib.hop_arrays(dxs)
        call("sgl_hop_wsum2d_bwd_f32", H, ptrs, lds, P(w), ld(w), P(g), ld(g), None, 0, dptrs, dlds, n, d)
        out = {f"dX{h}": t for h, t in enumerate(dxs) if t is not None}
    elif name == "select_bwd":
        base = select_hosts(n, d, H)
        xs, g = [b.inp(h) for h in base], b.inp(hash_matrix(n, d, seed=5 * d + 3))
        ptrs, lds = _lib.hop_arrays(xs)
        for op, kind in ((_lib.SGL_REDUCE_MAX, "max"), (_lib.SGL_REDUCE_MIN, "min")):
            dxs = [b.out(n, d) for _ in base]
            dptrs, dlds = _lib.hop_arrays(dxs)
            call("sgl_hop_select_bwd_f32", op, H, ptrs, lds, P(g), ld(g), dptrs, dlds, n, d)
            out.update({f"{kind}{h}": t for h, t in enumerate(dxs)})
    elif name == "lincomb":
        xs = [b.inp(h) for h in lincomb_hosts(n, d, H)]
        outs = [b.out(n, d) for _ in range(3)]
        wld = torch.from_numpy(lincomb_weights(d, H)).to(cuda)
        ptrs, lds = _lib.hop_arrays(xs)
        optrs, olds = _lib.hop_arrays(outs)
        call("sgl_hop_lincomb_f32", H, ptrs, lds, 3, optrs, olds, P(wld), H, n, d)
        out = {f"out{k}": o for k, o in enumerate(outs)}
    elif name in ("concat4", "concat_any", "concat1"):
        xs = [b.inp(h) for h in hosts]
        ptrs, lds = _lib.hop_arrays(xs)
        out["out"] = b.out(n, H * d + pad, aligned=True)                     # (a declared pad needs rows of whole 16-byte vectors)
        call("sgl_hop_concat_padded_f32", H, ptrs, lds, P(out["out"]), ld(out["out"]), pad, n, d)
    elif name == "bf16_reduce":
        xs = [b.inp(rne(h)) for h in hosts]
        ptrs, lds = _lib.hop_arrays(xs)
        w1d = torch.from_numpy(hop_weights(H)).to(cuda)
        for kind, op in OPS.items():
            out[kind] = b.out(n, d)
            call("sgl_hop_reduce_bf16_f32", op, H, ptrs, lds, P(w1d) if kind == "wsum" else None, P(out[kind]), ld(out[kind]), 0, n, d)
    elif name == "bf16_concat":
        xs = [b.inp(rne(h)) for h in hosts]
        ptrs, lds = _lib.hop_arrays(xs)
        out["bf16"], out["f32"] = b.out(n, H * d, torch.bfloat16), b.out(n, H * d)
        call("sgl_hop_concat_bf16", H, ptrs, lds, P(out["bf16"]), ld(out["bf16"]), 0, n, d)
        call("sgl_hop_concat_bf16_f32", H, ptrs, lds, P(out["f32"]), ld(out["f32"]), 0, n, d)
    else:
        raise ValueError(name)
    torch.cuda.synchronize()
    return out, b


def select_hosts(n, d, H):
    base = [h.copy() for h in hops_host(n, d, H)]
    base[2][0] = base[0][0]                                                    # ties, in the first row and in the last
    base[3][n - 1] = base[1][n - 1]
    base[1][3, 0] = base[0][n - 2, d - 1] = np.nan
    return base


def lincomb_hosts(n, d, H):
    base = [h.copy() for h in hops_host(n, d, H)]
    base[0][5, 1] = base[0][n - 1, d - 1] = np.nan                            # a NaN hop entry that a zero weight faces
    return base


def lincomb_weights(d, H):
    wl = np.ascontiguousarray(hash_matrix(3, H, seed=d + 3 * H))
    wl[1, 0] = 0.0                                                            # a skipped hop
    return wl


def agg_check(case, got, cuda):
    """the statement the entry point's own test uses (test_gpu_far_offsets.py, test_gpu_bf16_agg.py), on the CPU copies of `got`"""
    name, _, n, d, H, vec4, pad = case
    hosts = hops_host(n, d, H)
    y = {k: v.cpu() for k, v in got.items()}
    if name in ("reduce16", "reduce_odd", "bf16_reduce"):
        wide = [rne(h).float().numpy() for h in hosts] if name == "bf16_reduce" else hosts
        w1 = hop_weights(H)
        for kind in OPS:
            if kind == "wsum":
                assert oracle.parity_ok(y[kind].numpy(), oracle.one_dim_weighted_add(wide, w1), 1e-5, rowwise=False), (case, kind)
            else:
                want = {"sum": oracle.agg_sum, "mean": oracle.agg_mean, "max": oracle.agg_max, "min": oracle.agg_min}[kind](wide, 0, H)
                assert np.array_equal(y[kind].numpy(), want), (case, kind)
            if kind != "wsum" or name == "bf16_reduce":
                assert same_bits32(y[kind].numpy(), reduce_statement(kind, wide, w1)), (case, kind)
    elif name == "wsum2d":
        w2 = oracle.softmax32(hash_matrix(n, H, seed=d + H), 1)
        assert oracle.parity_ok(y["fma"].numpy(), oracle.two_dim_weighted_add(hosts, w2), 1e-5, rowwise=False), case
        assert np.isfinite(y["nafs"].numpy()).all() and np.allclose(y["W"].numpy(), oracle.nafs_weights(hosts), rtol=5e-5, atol=5e-6), case
        assert oracle.parity_ok(y["nafs"].numpy(), oracle.agg_over_smooth_distance(hosts), 2e-5, rowwise=False), case
    elif name == "wsum2d_dx":
        w2, g = oracle.softmax32(hash_matrix(n, H, seed=d + H), 1), hash_matrix(n, d, seed=5 * d + 2)
        assert sorted(y) == [f"dX{h}" for h in range(H) if h != 1]
        assert all(np.array_equal(y[f"dX{h}"].numpy(), w2[:, h:h + 1] * g) for h in range(H) if h != 1), case
    elif name == "select_bwd":
        base, g = select_hosts(n, d, H), hash_matrix(n, d, seed=5 * d + 3)
        for kind in ("max", "min"):
            leaves = [torch.from_numpy(x.copy()).to(cuda).requires_grad_(True) for x in base]
            getattr(torch.stack(leaves, 0), kind)(0)[0].backward(torch.from_numpy(g).to(cuda))
            assert all(torch.equal(y[f"{kind}{h}"], leaves[h].grad.cpu()) for h in range(H)), (case, kind)
    elif name == "lincomb":
        base, wl = lincomb_hosts(n, d, H), lincomb_weights(d, H)
        holes = np.isnan(base[0])
        assert holes.sum() == 2
        stack = np.stack(base).astype(np.float64)
        stack[0][holes] = 0.0
        want = np.einsum("kj,jnd->knd", wl.astype(np.float64), stack)
        scale = np.einsum("kj,jnd->knd", np.abs(wl).astype(np.float64), np.abs(stack))
        for k in range(3):
            o = y[f"out{k}"].numpy()
            if wl[k, 0] == 0:                                                 # the skipped hop's NaN does not reach this output
                assert np.isfinite(o).all(), (case, k)
            else:
                assert np.isnan(o[holes]).all() and np.isfinite(o[~holes]).all(), (case, k)
                o = np.where(holes, want[k], o)
            assert np.abs(o - want[k]).max() <= 1e-6 * max(scale[k].max(), 1e-30), (case, k)
    elif name in ("concat4", "concat_any", "concat1"):
        o, width = y["out"].numpy(), H * d
        assert np.array_equal(o[:, :width], np.hstack(hosts)) and not o[:, width:].view(np.uint32).any(), case
    elif name == "bf16_concat":
        h16 = [rne(h) for h in hosts]
        assert np.array_equal(raw(y["bf16"]).numpy(), raw(torch.cat(h16, dim=1)).numpy()), case
        assert np.array_equal(y["f32"].numpy().view(np.uint32), np.hstack([h.float().numpy() for h in h16]).view(np.uint32)), case


@pytest.mark.parametrize("case", sc.AGG_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_streaming_aggregators_under_forced_agg_blocks(cuda, case):
    base, buf = agg_launch(case, cuda)
    assert buf.check(), (case, "uncapped: an element outside the outputs was written")
    agg_check(case, base, cuda)
    for cap in sc.forced_caps(sc.stream_grid(sc.agg_threads(case)).work):
        with capped("agg_blocks", cap):
            got, buf = agg_launch(case, cuda)
        assert buf.check(), (case, cap, "an element outside the outputs was written")
        agg_check(case, got, cuda)
        assert sorted(got) == sorted(base) and all(same(got[k], base[k]) for k in got), (case, cap, "bits differ from the uncapped run")


# =========================================================================================================================================
# (c) natural caps: the smallest n that strides
# =========================================================================================================================================
def k9_input(d, n, layout, cuda):
    host = kc.host_x(d, n)
    return torch.from_numpy(host).to(cuda) if layout == "contiguous" else kc.in_layout(host, layout, cuda)


@pytest.mark.parametrize("d,k,n,layout", sc.K9_NATURAL)
def test_k9_natural_cap(cuda, d, k, n, layout):
    """the float64 reference on all rows (labels off the near-tie rows, mindist within dist_tol), and the bits of calls on slices of at
    most 2048 batches, which do not stride"""
    hx, hc, want, d1, near = sc.k9_reference(d, k, n)
    x = k9_input(d, n, layout, cuda)
    c = torch.from_numpy(hc).to(cuda) if layout == "contiguous" else kc.in_layout(hc, layout, cuda)
    labels = torch.full((n + 2,), -7, dtype=torch.int64, device=cuda)
    mindist = torch.full((n + 2,), -7.0, dtype=torch.float32, device=cuda)
    dev._call(cuda, "sgl_kmeans_assign_f32", _lib.ptr(x), dev._ld(x), n, d, _lib.ptr(c), dev._ld(c), k, _lib.ptr(labels[1:]), _lib.ptr(mindist[1:]))
    assert labels[0] == -7 and labels[-1] == -7 and mindist[0] == -7 and mindist[-1] == -7
    labels, mindist = labels[1:-1], mindist[1:-1]
    got_l, got_m = labels.cpu().numpy(), mindist.cpu().numpy().astype(np.float64)
    print(f"K9 natural d = {d}, k = {k}, n = {n}: near-tie share {near.mean():.4f}")
    assert near.mean() <= kc.MAX_LEFT_OUT
    wrong = np.flatnonzero((got_l != want) & ~near)
    assert wrong.size == 0, (wrong.size, wrong[:5].tolist())
    err = np.abs(got_m - d1) / np.maximum(d1, np.finfo(np.float64).tiny)
    assert np.isfinite(got_m).all() and err.max() <= kc.dist_tol(d), (float(err.max()), kc.dist_tol(d))
    vec = sc.vec_of(layout, d)
    step = sc.CAP_K9 * sc.per_batch(sc.k9_instance(d, vec))
    assert step < n
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        pl, pm = dev.kmeans_assign(x[lo:hi], c)
        assert same(pl, labels[lo:hi]) and same(pm, mindist[lo:hi]), ("the strided launch differs from the launch on a slice", lo, hi)


_K12_REFS = {}


@pytest.mark.parametrize("d,k,n", sc.K12_NATURAL)
def test_k12_natural_cap(cuda, d, k, n):
    hx, hc, hy = clc.inputs(d, k, n=n)
    if (d, k, n) not in _K12_REFS:
        _K12_REFS[(d, k, n)] = clc.step_references(hx, hc, hy)
    x, c, y = kc.in_layout(hx, "padded", cuda), kc.in_layout(hc, "padded", cuda), torch.from_numpy(hy).to(cuda)
    assert sc.k12_instance(d, 4) == clc.expected_instance(x, c)
    loss, dx, rows = k12_step(x, c, y, "padded", cuda)
    bad = []
    tc.check_truth(bad, (d, k, n), loss, dx, _K12_REFS[(d, k, n)])
    assert not bad, bad
    # the sampled rows' losses against float64, row by row, under the bound of test_out_of_range_labels_read_nothing_out_of_bounds:
    # ((d + 3) / 2 + 1 + k + 3) roundings of the sum of the absolute terms
    sample = sc.row_sample(n, sc.per_batch(sc.k12_instance(d, 4)), sc.CAP_K12, seed=d)
    x64, c64 = hx[sample].astype(np.float64), hc.astype(np.float64)
    dist = np.sqrt(np.stack([((x64 - cj) ** 2).sum(1) for cj in c64], 1))
    assigned = dist[np.arange(len(sample)), hy[sample]]
    tol = ((d + 3) / 2 + 1 + k + 3) * 2.0 ** -24
    got = rows[torch.from_numpy(sample).to(cuda)].cpu().numpy().astype(np.float64)
    assert (np.abs(got - (2.0 * assigned - dist.mean(1))) <= tol * (2.0 * assigned + dist.mean(1))).all()
    step = sc.CAP_K12 * sc.per_batch(sc.k12_instance(d, 4))
    assert step < n
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        _, pdx, prows = k12_step(x[lo:hi], c, y[lo:hi].clone(), "padded", cuda, w=1.0 / n)
        assert same(pdx, dx[lo:hi]) and same(prows, rows[lo:hi]), ("the strided launch differs from the launch on a slice", lo, hi)


_FOLD = {}


@pytest.mark.parametrize("d", sc.FOLD_WIDTHS)
def test_k11_fold_natural_cap(cuda, d):
    """a ring of 8300 nodes and a hub, one incidence per piece: 8301 cut rows, more than 4 x 2048"""
    edges, n = sc.fold_graph()
    labels = labels_for(len(edges))
    if "plan" not in _FOLD:
        _FOLD["plan"] = EdgePlan(edges, labels, n, max_piece=1, device=cuda)
    plan = _FOLD["plan"]
    assert int(plan.fold.shape[0]) == sc.FOLD_RING + 1 > 4 * sc.CAP_FOLD
    z_h = np.ascontiguousarray(hash_matrix(n, d, seed=77 * d + 6))
    if d not in _FOLD:
        _FOLD[d] = edge_step_references(z_h, edges, labels, "sigmoid")
    bad = []
    with te.Trace() as tr:
        for layout in te.LAYOUTS:
            z = te.LAYOUTS[layout](z_h, cuda)
            loss, dz, _, _ = te.step(tr, d, z, plan, "sigmoid", layout)
            te.check_truth(bad, (d, layout), loss, dz, _FOLD[d])
            if not bool((dz[sc.FOLD_RING + 1:] == 0).all()):                   # the dZ buffer was full of NaN
                bad.append((d, layout, "a node without edges is not exact zeros"))
            again = te.step(tr, d, z, plan, "sigmoid", layout)
            if not (again[0] == loss and same(again[1], dz)):
                bad.append((d, layout, "two runs differ"))
    assert not bad, bad


_CSR = {}


def csr_pair(lanes, n_rows):
    if (lanes, n_rows) not in _CSR:
        _CSR.clear()                                                          # one pair at a time: the largest is 2 x 9.4 M entries
        a = sc.big_csr(n_rows, 1, long_row=sc.csr_long_row(n_rows, lanes))
        fa = sc.big_csr(n_rows, 2, long_row=sc.csr_long_row(n_rows, lanes), finite=True)
        fb = sc.big_csr(n_rows, 5, shared_with=fa, finite=True)
        _CSR[(lanes, n_rows)] = (a, fa, fb)
    return _CSR[(lanes, n_rows)]


@pytest.mark.parametrize("lanes,n_rows", sc.CSR_NATURAL)
def test_csr_select_natural_cap(cuda, lanes, n_rows):
    a = csr_pair(lanes, n_rows)[0]
    length = np.diff(a.indptr)
    assert length[0] == 0 and length[-1] == 0 and length.max() == sc.CSR_LONG_ROW and set(range(10)) <= set(length.tolist())
    rmap, nr = csc.mask_to_map(np.random.RandomState(11).rand(n_rows) < 0.8)
    per = sc.csr_grid(n_rows, lanes).per_unit
    assert (rmap[:sc.CAP_CSR * per] < 0).any() and (rmap[sc.CAP_CSR * per:] < 0).any()              # rows dropped in both rounds
    kw = dict(row_map=rmap, n_rows_out=nr, drop_self=True, drop_below=drop_threshold(0.2), seed=4)
    want = csc.oracle_select(a, **kw)
    assert 0.3 * a.nnz < len(want[3]) < 0.8 * a.nnz
    got = raw_select(cuda, upload_select(a, cuda), lanes=lanes, **kw)
    assert select_agrees(got, want), (lanes, n_rows)


@pytest.mark.parametrize("lanes,n_rows,mode", [(g, n, m) for g, n in sc.CSR_NATURAL for m in sorted(cmc.MODES)])
def test_csr_merge_natural_cap(cuda, lanes, n_rows, mode):
    _, a, b = csr_pair(lanes, n_rows)
    want = cmc.merge_reference(a, b, cmc.MODES[mode])
    both = int(((want[3] >= 0) & (want[4] >= 0)).sum())
    assert 0.1 * a.nnz < both < 0.9 * a.nnz and np.diff(a.indptr).max() == sc.CSR_LONG_ROW
    got = raw_merge(cuda, upload_merge(a, cuda), upload_merge(b, cuda), lanes=lanes, mode=cmc.MODES[mode])
    assert cmc.agrees(got, want), (lanes, n_rows, mode)


@pytest.mark.parametrize("n,d,H,vec4", sc.W1D_NATURAL)
def test_wsum1d_backward_natural_cap(cuda, n, d, H, vec4):
    """dw[h] = <dOut, X_h> against the float64 sum under the rule of test_gpu_parity.py's wsum1d gradient check; two runs bit-equal"""
    b = Buffers(vec4, cuda)
    hosts = [np.ascontiguousarray(hash_matrix(n, d, seed=50 + h) * np.float32(1.0 - 0.1 * h)) for h in range(H)]
    g = hash_matrix(n, d, seed=78)
    xs, go = [b.inp(h) for h in hosts], b.inp(g)
    assert all((x.stride(0) % 4 == 0) == vec4 for x in xs)
    ptrs, lds = _lib.hop_arrays(xs)
    scratch = torch.empty(int(_lib.lib().sgl_hop_wsum1d_bwd_scratch(H)), dtype=torch.float32, device=cuda)
    runs = []
    for _ in range(2):
        dw = torch.full((H + 2,), -7.0, dtype=torch.float32, device=cuda)
        call("sgl_hop_wsum1d_bwd_f32", H, ptrs, lds, P(go), ld(go), P(dw[1:]), P(scratch), n, d)
        assert dw[0] == -7 and dw[-1] == -7
        runs.append(dw[1:-1].clone())
    ref = np.array([(g.astype(np.float64) * x).sum() for x in hosts])
    print("wsum1d backward", (n, d, H, vec4), runs[0].cpu().numpy(), ref)
    assert np.allclose(runs[0].cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(ref).max()))
    assert same(runs[0], runs[1]), "two runs differ"


def test_edge_fill_natural_cap(cuda):
    """sgl_edge_dot_f32 against a matrix without rows: every index is out of range, every output NaN, 1024 workgroups striding over
    262151 edges; the element after the last keeps its sentinel"""
    e, d = sc.FILL_EDGES, 12
    edges = torch.zeros((e, 2), dtype=torch.int64, device=cuda)
    bmat = torch.ones((5, d), device=cuda)
    out = torch.full((e + 2,), -7.0, device=cuda)
    call("sgl_edge_dot_f32", None, d, 0, P(bmat), d, 5, P(edges), e, d, P(out[1:]))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[1:-1]).all()) and out[0] == -7 and out[-1] == -7
