"""The aggregators that read bfloat16 hop matrices in place (csrc/sgl_aggregate_bf16.hip: sgl_hop_reduce_bf16_f32,
sgl_hop_concat_bf16(_f32), sgl_nafs_bf16_f32) on a real MI355X: run with `-m gpu`.

The contract is bit identity with "widen every hop exactly, then the float32 kernel", so every expected value is stated exactly:
on the CPU (numpy float32 in the documented order / torch.cat) and by the unchanged float32 kernels over exact float32 copies.
For the row kernels (NAFS) the copies are device.widen_hops' -- row-padded like every hop matrix of the project, the route the
new entry replaces -- because the float32 entry picks its kernel from its inputs' alignment: a dense `.float()` copy with d % 4 != 0
has unaligned rows and takes the float32 two-pass route, which sums in another order than the register-resident kernel; dense
copies are compared as well wherever d % 4 == 0.
Nothing in this file chooses a tolerance; the one comparison with a float64 truth goes through oracle.truth_report.

Inputs are hash_matrix rounded to bfloat16 with torch's round-to-nearest-even.  They live in buffers larger than their rows whose
pad columns hold NaN patterns (0x7FC0) in one run and 0x7F7F (3.39e38) in the other; raw entry points write into sentinel-filled
slices of larger matrices and the sentinels must survive."""
import numpy as np
import pytest
import torch

import oracle
from agg_rows_common import bits32, case_list, compiled_variants, expected_kernel, reduce_statement, rne, same_bits32, tuned
from inputs import hash_matrix
from sgl_amd import _lib, config
from sgl_amd import device as dev
from spmm_order_common import parse_template_args

pytestmark = pytest.mark.gpu

POISONS = (0x7FC0, 0x7F7F)          # bf16 patterns: a quiet NaN, the largest finite value
SENTINEL = 7.0                      # (exact in bfloat16 too)
NAFS_KERNEL = "nafs_bf16_fused_kernel"
OPS = {"sum": _lib.SGL_REDUCE_SUM, "mean": _lib.SGL_REDUCE_MEAN, "max": _lib.SGL_REDUCE_MAX, "min": _lib.SGL_REDUCE_MIN,
       "wsum": _lib.SGL_REDUCE_WSUM}


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def call(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.current_stream_ptr()), name)


def ld(t):
    return t.stride(0)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def poisoned(values, cuda, poison, layout):
    """a bf16 [n, d] device view of `values` (a CPU bf16 tensor) inside a larger buffer full of the poison pattern:
    "pitch"  rows on row_pitch(d, 2): 16-byte aligned rows, 16-byte lanes
    "odd"    rows on a pitch of d + 1 elements: alignment differs from row to row, the narrowest lanes
    "off2"   the first layout moved by 2 elements: rows that are 4-byte aligned only"""
    n, d = values.shape
    pitch = d + 1 if layout == "odd" else dev.row_pitch(d, elem_size=2)
    off = 2 if layout == "off2" else 0
    flat = torch.full((n * pitch + 16,), poison, dtype=torch.int16, device=cuda).view(torch.bfloat16)
    assert flat.data_ptr() % 16 == 0
    view = torch.as_strided(flat, (n, d), (pitch, 1), off)
    view.copy_(values)
    return view


_PLANTED, _POISONED = {}, {}


def planted(n, d, n_hops, seed):
    """[CPU bf16 hop h]: hash_matrix rounded to bf16 with -0.0, NaN and +-inf at known places of row 0 (and of the last element of
    the last row), as far as the shape has them; built once per shape and left unchanged"""
    key = (n, d, n_hops, seed)
    if key not in _PLANTED:
        _PLANTED[key] = _planted(n, d, n_hops, seed)
    return _PLANTED[key]


def device_hops(n, d, n_hops, seed, cuda, poison, layout):
    """planted() on the device in the given layout with the given pad pattern, uploaded once"""
    key = (n, d, n_hops, seed, poison, layout)
    if key not in _POISONED:
        _POISONED[key] = [poisoned(h, cuda, poison, layout) for h in planted(n, d, n_hops, seed)]
    return _POISONED[key]


def _planted(n, d, n_hops, seed):
    hops = [rne(hash_matrix(n, d, seed=seed + h) * np.float32(1.0 - 0.01 * h)) for h in range(n_hops)]
    last = n_hops - 1
    for h in hops:
        h[0, 0] = -0.0                                              # every hop: 0 + (-0) = +0 for sum / mean, -0 for max / min
    if d > 1:
        hops[min(1, last)][0, 1] = float("nan")
    if d > 2:
        hops[0][0, 2] = float("inf")
    if d > 3:
        hops[last][0, 3] = float("-inf")
    if d > 4:
        hops[0][0, 4] = float("inf")
        hops[last][0, 4] = float("-inf")                            # inf - inf over more than one hop
    if n > 1:
        hops[last // 2][n - 1, d - 1] = float("nan")
    return hops


# ---- 1. reduce ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(OPS))
def test_reduce_bits(cuda, kind):
    bad, cases = [], 0
    for n in (1, 77):
        for d in (1, 7, 8, 100, 147, 520):
            for H in (1, 2, 4, 11, 64):
                host = planted(n, d, H, 1000 + d)
                wide = [h.float().numpy() for h in host]
                w = (np.float32(0.75) ** np.arange(H, dtype=np.float32) * np.where(np.arange(H) % 3 == 2, -1, 1)).astype(np.float32)
                want = reduce_statement(kind, wide, w)
                wt = torch.from_numpy(w).to(cuda)
                ref32 = None
                for layout in ("pitch", "odd", "off2"):
                    outs = []
                    for poison in POISONS:
                        feats = device_hops(n, d, H, 1000 + d, cuda, poison, layout)
                        if layout == "off2":
                            assert all(f.data_ptr() % 4 == 0 and f.data_ptr() % 8 != 0 for f in feats)
                        got = dev.hop_reduce(OPS[kind], feats, wt if kind == "wsum" else None)
                        assert got.dtype == torch.float32 and got.shape == (n, d)
                        outs.append(got)
                        if dev.own_pad(got):
                            assert not dev.padded_parent(got)[:, d:].cpu().numpy().view(np.uint32).any()
                        if poison == POISONS[0]:
                            # the entry itself, pad_cols = 0, into a slice of a larger sentinel matrix: rows as aligned as the
                            # inputs' (16 / 8 / 4 bytes), so that the lane width follows the inputs
                            c0 = {"pitch": 4, "off2": 2, "odd": 1}[layout]
                            wide_out = torch.full((n + 2, dev.round_up(d, 4) + 8), SENTINEL, dtype=torch.float32, device=cuda)
                            view = wide_out[:n, c0:c0 + d]
                            ptrs, lds = _lib.hop_arrays(feats)
                            call("sgl_hop_reduce_bf16_f32", OPS[kind], H, ptrs, lds, _lib.ptr(wt), _lib.ptr(view), ld(view), 0, n, d)
                            if not same_bits32(view.cpu().numpy(), want):
                                bad.append((kind, n, d, H, layout, "entry into a slice"))
                            wide_out[:n, c0:c0 + d] = SENTINEL
                            if not bool((wide_out == SENTINEL).all()):
                                bad.append((kind, n, d, H, layout, "sentinels around the slice"))
                    g0, g1 = outs[0].cpu().numpy(), outs[1].cpu().numpy()
                    if not same_bits32(g0, want):
                        bad.append((kind, n, d, H, layout, "against the float32 statement"))
                    if not same_bits32(g1, want):
                        bad.append((kind, n, d, H, layout, "0x7F7F pads"))
                    if ref32 is None:
                        ref32 = dev.hop_reduce(OPS[kind], [f.float() for f in feats], wt if kind == "wsum" else None).cpu().numpy()
                    if not same_bits32(g0, ref32):
                        bad.append((kind, n, d, H, layout, "against the float32 kernel over widened copies"))
                    cases += 1
    print(f"\n[reduce {kind}] {cases} cases, {len(bad)} failed checks")
    assert cases == 2 * 6 * 5 * 3
    assert not bad, (len(bad), bad[:10])


# ---- 2. concat ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_concat_bits(cuda, out_dtype):
    bad, cases = [], 0
    entry = "sgl_hop_concat_bf16" if out_dtype == torch.bfloat16 else "sgl_hop_concat_bf16_f32"

    def raw(t):
        return bits16(t) if out_dtype == torch.bfloat16 else bits32(t.detach().cpu().numpy())

    for n in (1, 77):
        for d in (1, 7, 8, 100, 147):
            for H in (1, 2, 4, 11):
                host = planted(n, d, H, 2000 + d)
                want = torch.cat(host, dim=1) if out_dtype == torch.bfloat16 else torch.cat([h.float() for h in host], dim=1)
                want = raw(want)
                for layout in ("pitch", "odd"):
                    first = None
                    for poison in POISONS:
                        feats = device_hops(n, d, H, 2000 + d, cuda, poison, layout)
                        # the wrapper: an alloc_rows output whose own padding the kernel writes as zeros
                        got = dev.hop_concat(feats, out_dtype=out_dtype) if out_dtype == torch.bfloat16 else dev.hop_concat(feats)
                        ok = got.dtype == out_dtype and got.shape == (n, H * d) and np.array_equal(raw(got), want)
                        parent = dev.padded_parent(got)
                        ok = ok and not raw(parent[:, H * d:]).any()
                        if not ok:
                            bad.append((n, d, H, layout, hex(poison), "wrapper: bits / zero pad columns"))
                        first = got if first is None else first
                        # the entry, pad_cols = 0, into a slice of a larger sentinel matrix; aligned and unaligned
                        for c0 in (8, 1):
                            wide_out = torch.full((n + 2, dev.round_up(H * d, 8) + 16), SENTINEL, dtype=out_dtype, device=cuda)
                            view = wide_out[:n, c0:c0 + H * d]
                            ptrs, lds = _lib.hop_arrays(feats)
                            call(entry, H, ptrs, lds, _lib.ptr(view), ld(view), 0, n, d)
                            if not np.array_equal(raw(view), want):
                                bad.append((n, d, H, layout, hex(poison), c0, "entry into a slice"))
                            wide_out[:n, c0:c0 + H * d] = SENTINEL
                            if not bool((wide_out == SENTINEL).all()):
                                bad.append((n, d, H, layout, hex(poison), c0, "sentinels around the slice"))
                        # declared pad columns of a caller's matrix: zeros, and nothing beyond them
                        pad = (-(H * d)) % 4 + 4
                        wide_out = torch.full((n + 2, H * d + pad + 8), SENTINEL, dtype=out_dtype, device=cuda)
                        view = wide_out[:n, :H * d]
                        ptrs, lds = _lib.hop_arrays(feats)
                        call(entry, H, ptrs, lds, _lib.ptr(view), ld(view), pad, n, d)
                        ok = np.array_equal(raw(view), want) and not raw(wide_out[:n, H * d:H * d + pad]).any()
                        ok = ok and bool((wide_out[:n, H * d + pad:] == SENTINEL).all()) and bool((wide_out[n:] == SENTINEL).all())
                        if not ok:
                            bad.append((n, d, H, layout, hex(poison), "declared pad columns"))
                    cases += 1
    print(f"\n[concat {entry}] {cases} cases, {len(bad)} failed checks")
    assert cases == 2 * 5 * 4 * 2
    assert not bad, (len(bad), bad[:10])


def test_concat_refuses_what_it_cannot_return(cuda):
    f32 = [torch.zeros((5, 8), device=cuda) for _ in range(2)]
    with pytest.raises(TypeError):
        dev.hop_concat(f32, out_dtype=torch.bfloat16)              # nothing is rounded here
    with pytest.raises(ValueError):
        dev.hop_concat(f32, out_dtype=torch.float16)
    b = rne(hash_matrix(5, 8, seed=3)).to(cuda)
    mixed = dev.hop_concat([b, b.float()])                          # a mixed list widens its bf16 members: today's result
    assert mixed.dtype == torch.float32 and torch.equal(mixed, torch.cat([b.float(), b.float()], dim=1))
    out = torch.empty((5, 16), dtype=torch.bfloat16, device=cuda)
    ptrs, lds = _lib.hop_arrays([out[:, :8], b])
    rc = _lib.lib().sgl_hop_concat_bf16(2, ptrs, lds, _lib.ptr(out), 16, 0, 5, 8, _lib.current_stream_ptr())
    assert rc != 0 and "alias" in _lib.last_error()


# ---- 3. NAFS: every compiled instance, by name ------------------------------------------------------------------------------------------
class NafsTrace:
    """runs launches under torch.profiler; at exit the instances of nafs_bf16_fused_kernel that really ran must be, in order, the
    ones `expect()` announced.  A name of the kernel without its three template arguments is an error, never a skip."""

    def __init__(self):
        self.expected, self.seen, self.others = [], set(), 0

    def expect(self, label, args):
        self.expected.append((label, tuple(args)))

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
        got = []
        for e in evs:
            at = e.name.find(NAFS_KERNEL)
            if at < 0:
                self.others += 1
                continue
            args = parse_template_args(e.name[at + len(NAFS_KERNEL):])
            assert args is not None and len(args) == 3, f"no (LPR, CH, HMAX) in the kernel name {e.name!r}"
            got.append(tuple(args))
        assert len(got) == len(self.expected), (len(got), len(self.expected), len(evs), got[:3], self.expected[:3])
        wrong = [(i, lab, g, w) for i, (g, (lab, w)) in enumerate(zip(got, self.expected)) if g != w]
        assert not wrong, (len(wrong), wrong[:8])
        self.seen.update(got)
        return False


_NAFS_HOST = {}


def nafs_host(n, d, n_hops):
    """[CPU bf16 hop h]: hop h = hash_matrix scaled by (1 - 0.04 h), rounded; row 1 of hop 0 is zero (cosine 0 with every hop)
    and row 3 of every hop -- the hostile rows of test_gpu_agg_variants.host_hops"""
    have = _NAFS_HOST.setdefault((n, d), [])
    for h in range(len(have), n_hops):
        x = np.ascontiguousarray((hash_matrix(n, d, seed=31 * d + h) * np.float32(1.0 - 0.04 * h)).astype(np.float32))
        if n > 2 and h == 0:
            x[1] = 0.0
        if n > 4:
            x[3] = 0.0
        have.append(rne(x))
    return have[:n_hops]


_NAFS_DEV = {}


def nafs_device(n, d, n_hops, cuda):
    """[[hop tensors with NaN pads], [hop tensors with 0x7F7F pads]] in row_pitch(d, 2) buffers, uploaded once per (n, d)"""
    host = nafs_host(n, d, n_hops)
    per = _NAFS_DEV.setdefault((n, d), [[] for _ in POISONS])
    for k, poison in enumerate(POISONS):
        for h in range(len(per[k]), n_hops):
            per[k].append(poisoned(host[h], cuda, poison, "pitch"))
    return [p[:n_hops] for p in per]


def nafs_statement(host, dt):
    """over_smooth_distance_op.py:11-33 on the widened inputs, in dtype dt, on the CPU"""
    ff = [h.float().to(dt) for h in host]
    x0 = ff[0]
    n0 = torch.norm(x0, 2, 1).add(1e-10)
    scores = [torch.div(torch.div((x0 * f).sum(1), torch.norm(f, 2, 1).add(1e-10)), n0).unsqueeze(-1) for f in ff]
    w = torch.softmax(torch.cat(scores, dim=1), dim=1)
    out = 0.0
    for h, f in enumerate(ff):
        out = out + w[:, h:h + 1] * f
    return out, w


def wrapper_output_qualifies(n, d):
    """device.nafs_aggregate hands the entry points the pitch of the output it allocates, which for a single row is d itself (as
    it does for float32 hops): a one-row output whose d is no multiple of 4 is not "a pitch that is a multiple of 4 floats", the
    entry answers SGL_ERR_UNSUPPORTED and the wrapper takes the widening route -- the float32 wrapper takes its two-pass route for
    the same reason, so the values stay what they were.  This is expected_kernel's `aligned` argument."""
    return n > 1 or d % 4 == 0


def test_nafs_every_instance(cuda):
    """Every case of the list goes through dev.nafs_aggregate (two pad patterns) AND through the entry point itself (output and
    weights as slices of sentinel matrices).  Every launch is checked against expected_kernel; the entry launches the predicted
    instance in every case, the wrapper in every case whose output it can hand over as the entry requires
    (wrapper_output_qualifies: all but the one-row cases with d % 4 != 0, where it must launch none)."""
    cases = case_list("nafs")
    results = []
    with NafsTrace() as tr:
        for n, d, H, tuning in cases:
            label = (n, d, H, tuple(tuning.items()))
            kern = expected_kernel("nafs", d, H, tuning)
            assert kern is not None and kern[0] == "nafs", label
            via_wrapper = expected_kernel("nafs", d, H, tuning, aligned=wrapper_output_qualifies(n, d))
            assert via_wrapper in (kern, None)
            by_poison = nafs_device(n, d, H, cuda)
            with tuned(**tuning):
                for k in range(2):
                    if via_wrapper is not None:
                        tr.expect(label + ("wrapper", k), kern[1])
                outs = [dev.nafs_aggregate(by_poison[k], return_weights=True) for k in range(2)]
                # the entry, pad_cols = 0, output and weights into slices of larger sentinel matrices
                wide_out = torch.full((n + 3, dev.round_up(d, 4) + 8), SENTINEL, dtype=torch.float32, device=cuda)
                view = wide_out[:n, 4:4 + d]
                wide_w = torch.full((n + 3, H + 5), SENTINEL, dtype=torch.float32, device=cuda)
                wv = wide_w[:n, 2:2 + H]
                ptrs, lds = _lib.hop_arrays(by_poison[0])
                tr.expect(label + ("entry",), kern[1])
                call("sgl_nafs_bf16_f32", H, ptrs, lds, _lib.ptr(view), ld(view), 0, _lib.ptr(wv), ld(wv), n, d)
                # and without weights
                view2 = torch.full((n + 3, dev.round_up(d, 4) + 8), SENTINEL, dtype=torch.float32, device=cuda)[:n, 4:4 + d]
                tr.expect(label + ("entry, no weights",), kern[1])
                call("sgl_nafs_bf16_f32", H, ptrs, lds, _lib.ptr(view2), ld(view2), 0, None, 0, n, d)
            results.append((outs[0][0], outs[0][1], outs[1][0], outs[1][1], view, wide_out, wv, wide_w, view2))
    bad, worst = [], {"out": 0.0, "W": 0.0}
    for (n, d, H, tuning), (out, w, out2, w2, view, wide_out, wv, wide_w, view2) in zip(cases, results):
        label = (n, d, H, tuple(tuning.items()))
        host = nafs_host(n, d, H)
        by_poison = nafs_device(n, d, H, cuda)
        assert out.dtype == torch.float32 and w.dtype == torch.float32 and out.shape == (n, d) and w.shape == (n, H)
        wide = dev.widen_hops(by_poison[0])             # exact float32 copies in row-padded buffers: the route this replaces
        with tuned(**tuning):
            ref_out, ref_w = dev.nafs_aggregate(wide, return_weights=True)
            if d % 4 == 0:                              # dense copies have 16-byte aligned rows too: the same float32 route
                dense_out, dense_w = dev.nafs_aggregate([f.float() for f in by_poison[0]], return_weights=True)
                if not (torch.equal(out, dense_out) and torch.equal(w, dense_w)):
                    bad.append((label, "wrapper: bits of dev.nafs_aggregate over dense .float() copies"))
            # the float32 entry over the widened copies, into slices laid out like the bf16 entry's
            ref_view = torch.full((n + 3, dev.round_up(d, 4) + 8), SENTINEL, dtype=torch.float32, device=cuda)[:n, 4:4 + d]
            ref_wv = torch.full((n + 3, H + 5), SENTINEL, dtype=torch.float32, device=cuda)[:n, 2:2 + H]
            ptrs, lds = _lib.hop_arrays(wide)
            call("sgl_nafs_padded_f32", H, ptrs, lds, _lib.ptr(ref_view), ld(ref_view), 0, _lib.ptr(ref_wv), ld(ref_wv), n, d)
        if not (torch.equal(out, ref_out) and torch.equal(w, ref_w)):
            bad.append((label, "wrapper: bits of dev.nafs_aggregate over widened copies"))
        if not (torch.equal(out2, out) and torch.equal(w2, w)):
            bad.append((label, "wrapper: 0x7F7F pads"))
        if not (torch.equal(view, ref_view) and torch.equal(wv, ref_wv)):
            bad.append((label, "entry: bits of sgl_nafs_padded_f32 over widened copies"))
        if not torch.equal(view2, view):
            bad.append((label, "entry without weights"))
        if wrapper_output_qualifies(n, d) and not (torch.equal(view, out) and torch.equal(wv, w)):
            bad.append((label, "entry against wrapper"))
        if dev.own_pad(out) and dev.padded_parent(out)[:, d:].cpu().numpy().view(np.uint32).any():
            bad.append((label, "pad columns of the padded output"))
        y64, w64 = nafs_statement(host, torch.float64)
        y32, w32 = nafs_statement(host, torch.float32)
        for who, o_, w_ in (("wrapper", out, w), ("entry", view, wv)):
            got, gw = o_.cpu().numpy(), w_.cpu().numpy()
            if not (np.isfinite(got).all() and np.isfinite(gw).all()):
                bad.append((label, who, "finite"))
                continue
            for what, g, r32, r64 in (("out", got, y32, y64), ("W", gw, w32, w64)):
                rep = oracle.truth_report(g, r32.numpy(), r64.numpy())
                worst[what] = max(worst[what], rep["err_got"] / max(rep["bound"], 1e-300))
                if not rep["ok"]:
                    bad.append((label, who, what, rep))
        wide_out[:n, 4:4 + d] = SENTINEL                # (last: view and wv are slices of these)
        wide_w[:n, 2:2 + H] = SENTINEL
        if not (bool((wide_out == SENTINEL).all()) and bool((wide_w == SENTINEL).all())):
            bad.append((label, "sentinels around the slices"))
    want = compiled_variants("nafs")
    print(f"\n[nafs bf16] {len(cases)} cases, {len(tr.seen)} of {len(want)} instances seen; worst error / bound: {worst}")
    assert not bad, (len(bad), bad[:10])
    assert len(want) == 54
    assert tr.seen == want, sorted(want - tr.seen)


@pytest.mark.parametrize("d,H", [(100, 17), (513, 4)])
def test_nafs_falls_back_beyond_sixteen_hops_or_512_columns(cuda, d, H):
    """one hop or one column too many: no bf16 NAFS kernel is launched, and the float32 route's bits come back"""
    n = 77
    assert expected_kernel("nafs", d, H) is None
    feats = nafs_device(n, d, H, cuda)[0]
    with NafsTrace() as tr:
        out, w = dev.nafs_aggregate(feats, return_weights=True)
    assert not tr.seen and tr.others > 0
    ref_out, ref_w = dev.nafs_aggregate(dev.widen_hops(feats), return_weights=True)
    assert out.dtype == torch.float32 and torch.equal(out, ref_out) and torch.equal(w, ref_w)
    if d % 4 == 0:                                      # dense copies have 16-byte aligned rows too: the same float32 route
        dense_out, dense_w = dev.nafs_aggregate([f.float() for f in feats], return_weights=True)
        assert torch.equal(out, dense_out) and torch.equal(w, dense_w)
    ptrs, lds = _lib.hop_arrays(feats)
    rc = _lib.lib().sgl_nafs_bf16_f32(H, ptrs, lds, _lib.ptr(out), ld(out), 0, None, 0, n, d, _lib.current_stream_ptr())
    assert rc == _lib.SGL_ERR_UNSUPPORTED and "widen" in _lib.last_error()


# ---- 4. operators and models ----------------------------------------------------------------------------------------------------------
K = 3


def test_operators_aggregate_in_place(goldens, cuda, monkeypatch):
    from sgl_amd.operators.graph_op import LaplacianGraphOp
    from sgl_amd.operators.message_op import ConcatMessageOp, MeanMessageOp, OverSmoothDistanceWeightedOp
    adj = goldens.graph("pl2000")
    n, d = adj.shape[0], 100
    x = hash_matrix(n, d, seed=60)
    fp32_hops_before = [h.cpu().numpy() for h in LaplacianGraphOp(K, r=0.5).propagate(adj, x)]
    hops = LaplacianGraphOp(K, r=0.5, hop_dtype="bfloat16").propagate(adj, x)
    assert len(hops) == K + 1 and all(h.dtype == torch.bfloat16 and h.is_cuda for h in hops)
    wide = [h.float() for h in hops]
    ops = [MeanMessageOp(1, 4), ConcatMessageOp(0, 4), OverSmoothDistanceWeightedOp()]
    fp32_aggs_before = [op.aggregate(LaplacianGraphOp(K, r=0.5).propagate(adj, x)).cpu().numpy() for op in ops]
    want = [op.aggregate(wide) for op in ops]

    def no_widening(feats):
        raise AssertionError("widen_hops was called: a bf16 hop list was copied to float32")
    monkeypatch.setattr(dev, "widen_hops", no_widening)
    for op, ref in zip(ops, want):
        got = op.aggregate(hops)
        assert got.dtype == torch.float32 and got.shape == ref.shape, type(op).__name__
        assert torch.equal(got, ref), type(op).__name__
    monkeypatch.undo()
    # an fp32 operator on the same adjacency afterwards: bit-identical fp32 hops and aggregates
    after = LaplacianGraphOp(K, r=0.5).propagate(adj, x)
    for k in range(K + 1):
        assert after[k].dtype == torch.float32 and np.array_equal(after[k].cpu().numpy(), fp32_hops_before[k]), k
    for op, ref in zip(ops, fp32_aggs_before):
        assert np.array_equal(op.aggregate(after).cpu().numpy(), ref), type(op).__name__


@pytest.mark.parametrize("name", ["SIGN", "NAFS"])
def test_models_see_only_the_stored_values(goldens, cuda, name, monkeypatch):
    """logits under bf16 storage == logits of the same model (same seed) fed the widened copies of the same hops"""
    from sgl_amd.models.homo import NAFS, SIGN
    adj = goldens.graph("pl2000")
    n, d, classes = adj.shape[0], 100, 7
    x = hash_matrix(n, d, seed=50)
    idx = [int(i) for i in np.random.default_rng(3).integers(0, n, 300)]

    def build():
        torch.manual_seed(1234)
        m = SIGN(K, d, classes, 64, 2) if name == "SIGN" else NAFS(K, d, classes)
        return m.to(cuda).eval()
    monkeypatch.setattr(config, "hop_dtype", "bfloat16")
    model = build()
    real_widen = dev.widen_hops

    def no_widening(feats):
        raise AssertionError("widen_hops was called during preprocess()")
    monkeypatch.setattr(dev, "widen_hops", no_widening)
    model.preprocess(adj, x)
    monkeypatch.setattr(dev, "widen_hops", real_widen)
    hops = model._pre_graph_op.propagate(adj, x)
    assert all(h.dtype == torch.bfloat16 for h in hops)
    if name == "SIGN":
        assert model._processed_feature.dtype == torch.bfloat16 and model._processed_feature.shape == (n, (K + 1) * d)
        assert np.array_equal(bits16(model._processed_feature), bits16(torch.cat([h.cpu() for h in hops], dim=1)))
    else:
        assert model._processed_feature.dtype == torch.float32
    with torch.no_grad():
        got = model.model_forward(idx, cuda)
    monkeypatch.setattr(config, "hop_dtype", "float32")
    ref = build()
    wide = [h.float() for h in hops]
    ref._pre_msg_learnable = model._pre_msg_learnable
    ref._processed_feat_list = wide
    ref._processed_feature = ref._pre_msg_op.aggregate(wide)
    with torch.no_grad():
        want = ref.model_forward(idx, cuda)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
