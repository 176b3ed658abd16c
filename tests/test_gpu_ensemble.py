"""K16 on the device (sgl_ensemble_combine_f32 / sgl_ensemble_combine_bwd_f32 through device.ensemble_combine and the three
aggregator modules): values and weight gradients against float64 inside the derived bounds of ensemble_common.py, for every width
class, group size, batch size and input layout; the exact contracts (true division, NaN rows, padding, the strided grid, run-to-run
bits, stream order, the split by group)."""
import numpy as np
import pytest
import torch

import ensemble_common as ec
from stream_common import delay, independent_stream

from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.models import simple_models as sm

pytestmark = pytest.mark.gpu

M_POOL = max(ec.SUBGRAPHS) * max(ec.HOPS)
START = 5                                     # start_pos of the row views
_pool = {}


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def host_pool(d):
    """M_POOL float32 matrices [N_ROWS, d], made once per width and never changed"""
    if ("host", d) not in _pool:
        _pool[("host", d)] = np.random.default_rng(1000 + d).standard_normal((M_POOL, ec.N_ROWS, d)).astype(np.float32)
    return _pool[("host", d)]


def device_pool(d, layout, cuda):
    """the same matrices on the device, every byte around them NaN.  "rows": row views at start_pos START of taller buffers on a padded
    pitch (16-byte rows: the vector path); "cols": column slices of matrices whose pitch is no multiple of 4, every other one starting
    at column 1 (the element path)."""
    if (layout, d) not in _pool:
        x = torch.from_numpy(host_pool(d)).to(cuda)
        if layout == "rows":
            pitch = dev.round_up(d, 4) + 4
            buf = torch.full((M_POOL, START + ec.N_ROWS + 3, pitch), float("nan"), device=cuda)
            views = [buf[m, START:START + ec.N_ROWS, :d] for m in range(M_POOL)]
        else:
            pitch = d + 1 if (d + 1) % 4 else d + 2
            buf = torch.full((M_POOL, ec.N_ROWS, pitch), float("nan"), device=cuda)
            views = [buf[m, :, m % 2:m % 2 + d] for m in range(M_POOL)]
        for m, v in enumerate(views):
            v.copy_(x[m])
        assert all((v.stride(0) % 4 == 0 and v.data_ptr() % 16 == 0) == (layout == "rows") for v in views)
        _pool[(layout, d)] = views
    return _pool[(layout, d)]


def make_module(mode, S, H, d, W, cuda):
    """the aggregator of `mode` with the parameters W (ensemble_common.make_weights)"""
    if mode == "fast":
        mod = sm.FastOneDimConvolution(S, H).to(cuda)
        with torch.no_grad():
            next(mod.parameters()).copy_(torch.from_numpy(W))
        return mod
    mod = (sm.OneDimConvolution(S, H, d) if mode == "per_feature" else sm.OneDimConvolutionWeightSharedAcrossFeatures(S, H)).to(cuda)
    with torch.no_grad():
        for p, w in zip(mod.parameters(), W):
            p.copy_(torch.from_numpy(w))
    return mod


def run(mod, X, idx, G):
    """(outputs, parameter gradients) of one forward and backward of sum_h <out_h, G_h>"""
    mod.zero_grad(set_to_none=True)
    outs = mod.combine(X, idx)
    outs = outs if isinstance(outs, list) else [outs]
    sum((o * g).sum() for o, g in zip(outs, G)).backward()
    return outs, [p.grad for p in mod.parameters()]


def bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("layout", ("rows", "cols"))
@pytest.mark.parametrize("mode", ec.MODES)
@pytest.mark.parametrize("d", ec.WIDTHS)
def test_values_and_weight_gradients_inside_the_derived_bounds(cuda, d, mode, layout):
    host, views = host_pool(d), device_pool(d, layout, cuda)
    rng = np.random.default_rng(7 * d + len(mode))
    worst_f = worst_b = 0.0
    for S in ec.SUBGRAPHS:
        for H in ec.HOPS:
            X_h = [[host[h * S + s] for s in range(S)] for h in range(H)]
            X_d = [[views[h * S + s] for s in range(S)] for h in range(H)]
            W = ec.make_weights(mode, S, H, d, rng)
            mod = make_module(mode, S, H, d, W, cuda)
            n_groups, group_size, cs, divisor = ec.kernel_shape(mode, S, H)
            for B in ec.BATCHES:
                idx = ec.make_index(B, rng)
                n_out = ec.N_ROWS if B is None else B
                G_h = [rng.standard_normal((n_out, d)).astype(np.float32) for _ in range(n_groups)]
                outs, grads = run(mod, X_d, None if idx is None else torch.from_numpy(idx).to(cuda), [torch.from_numpy(g).to(cuda) for g in G_h])
                T, bound = ec.forward_f64(mode, X_h, W, idx)
                assert len(outs) == len(T)
                for o, t, b in zip(outs, T, bound):
                    err = np.abs(o.detach().cpu().numpy().astype(np.float64) - t)
                    assert np.all(err <= b), (S, H, B, float((err - b).max()))
                    worst_f = max(worst_f, float((err / np.maximum(b, 1e-300)).max()))
                # the gradient buffer autograd hands over is contiguous: 16-byte rows when d is a multiple of 4
                k = ec.bwd_roundings(n_out, d, cs, 4 if (layout == "rows" and d % 4 == 0) else 1, divisor != 1.0)
                dT, mag = ec.backward_f64(mode, X_h, G_h, idx)
                dT, mag = (dT, mag) if isinstance(dT, list) else ([dT], [mag])
                assert len(grads) == len(dT)
                for g, t, m in zip(grads, dT, mag):
                    assert g.shape == t.shape
                    err = np.abs(g.cpu().numpy().astype(np.float64) - t)
                    assert np.all(err <= ec.gamma(k) * m), (S, H, B, k, float((err - ec.gamma(k) * m).max()))
                    worst_b = max(worst_b, float((err / np.maximum(ec.gamma(k) * m, 1e-300)).max()))
    print(f"d={d} {mode} {layout}: worst forward error / bound {worst_f:.3f}, worst backward error / bound {worst_b:.3f}")


@pytest.mark.parametrize("layout", ("rows", "cols"))
def test_true_division_bit_for_bit(cuda, layout):
    """one member per group, divisor 3: float32(x w) / float32(3), not a multiplication by a rounded third"""
    for d in (3, 100):
        host, views = host_pool(d), device_pool(d, layout, cuda)
        rng = np.random.default_rng(d)
        idx = ec.make_index(1031, rng)
        for w in (rng.uniform(-2, 2, (2, d)).astype(np.float32), rng.uniform(-2, 2, (2,)).astype(np.float32)):
            outs = dev.ensemble_combine([[views[0]], [views[1]]], torch.from_numpy(w).to(cuda), idx=torch.from_numpy(idx).to(cuda), divisor=3.0)
            for g, o in enumerate(outs):
                want = (host[g][idx] * (w[g][None, :] if w.ndim == 2 else w[g])).astype(np.float32) / np.float32(3)
                assert np.array_equal(o.cpu().numpy().view(np.int32), want.view(np.int32))
                third = (host[g][idx] * (w[g][None, :] if w.ndim == 2 else w[g])).astype(np.float32) * np.float32(1 / 3)
                assert not np.array_equal(want, third)           # (the two roundings do differ on these inputs)


@pytest.mark.parametrize("layout", ("rows", "cols"))
def test_a_bad_index_gives_a_nan_row_and_leaves_the_others_exact(cuda, layout):
    d, S, H = 100, 3, 3
    views = device_pool(d, layout, cuda)
    X = [[views[h * S + s] for s in range(S)] for h in range(H)]
    rng = np.random.default_rng(3)
    w = torch.from_numpy(rng.standard_normal((S * H, d)).astype(np.float32)).to(cuda)
    good = ec.make_index(63, rng)
    ref = dev.ensemble_combine(X, w, idx=torch.from_numpy(good).to(cuda), divisor=float(S))
    for at, value in ((0, ec.N_ROWS), (17, -ec.N_ROWS - 1), (62, 2 ** 40)):
        bad = good.copy()
        bad[at] = value
        outs = dev.ensemble_combine(X, w, idx=torch.from_numpy(bad).to(cuda), divisor=float(S))
        keep = torch.ones(63, dtype=torch.bool, device=cuda)
        keep[at] = False
        for o, r in zip(outs, ref):
            assert torch.isnan(o[at]).all()
            assert torch.equal(bits(o[keep]), bits(r[keep]))
    with pytest.raises(IndexError):                                  # host indices are validated on the host, as everywhere
        dev.ensemble_combine(X, w, idx=[0, ec.N_ROWS])


def test_pad_columns_are_zeros_and_nothing_beyond_them_is_touched(cuda):
    d, S, H, B = 147, 2, 3, 63
    views = device_pool(d, "rows", cuda)
    flat = [views[m] for m in range(S * H)]
    rng = np.random.default_rng(5)
    w = torch.from_numpy(rng.standard_normal((S * H, d)).astype(np.float32)).to(cuda)
    idx = torch.from_numpy(ec.make_index(B, rng)).to(cuda)
    plain = dev.ensemble_combine([flat[h * S:(h + 1) * S] for h in range(H)], w, idx=idx, divisor=2.0)
    for pad in (0, 1, 5):                                            # d + pad a whole number of vectors, or no padding at all
        bufs = [torch.full((B + 1, 156), 77.0, device=cuda) for _ in range(H)]
        outs = [b[:B, :d] for b in bufs]
        dev._ensemble_forward(flat, H, S, w, 1, idx, 2.0, outs, pad)
        for b, o, p in zip(bufs, outs, plain):
            assert torch.equal(bits(o), bits(p))
            assert torch.all(b[:B, d:d + pad] == 0) and torch.all(b[:B, d + pad:] == 77.0) and torch.all(b[B] == 77.0)
    # our own outputs: the whole tail of the pitch is zeros
    for o in plain:
        parent = dev.padded_parent(o)
        assert parent.shape[1] > d and torch.all(parent[:, d:] == 0)


def test_strided_grid_gives_the_same_bits(cuda):
    d, S, H = 100, 3, 3
    rng = np.random.default_rng(11)
    for layout in ("rows", "cols"):
        views = device_pool(d, layout, cuda)
        X = [[views[h * S + s] for s in range(S)] for h in range(H)]
        w = torch.from_numpy(rng.standard_normal((S * H, d)).astype(np.float32)).to(cuda)
        for B in (1031, None):
            idx = None if B is None else torch.from_numpy(ec.make_index(B, rng)).to(cuda)
            free = dev.ensemble_combine(X, w, idx=idx, divisor=3.0)
            try:
                _lib.set_tuning("agg_blocks", 3)                      # 1031 rows are 129 blocks of 8 rows and more: every block strides
                capped = dev.ensemble_combine(X, w, idx=idx, divisor=3.0)
            finally:
                _lib.set_tuning("agg_blocks", 0)
            assert _lib.get_tuning("agg_blocks") == 0
            for a, b in zip(free, capped):
                assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("mode", ec.MODES)
def test_two_runs_give_the_same_bits(cuda, mode):
    d, S, H = 100, 8, 3
    views = device_pool(d, "rows", cuda)
    X = [[views[h * S + s] for s in range(S)] for h in range(H)]
    rng = np.random.default_rng(13)
    mod = make_module(mode, S, H, d, ec.make_weights(mode, S, H, d, rng), cuda)
    idx = torch.from_numpy(ec.make_index(1031, rng)).to(cuda)
    G = [torch.from_numpy(rng.standard_normal((1031, d)).astype(np.float32)).to(cuda) for _ in range(ec.kernel_shape(mode, S, H)[0])]
    o1, g1 = run(mod, X, idx, G)
    o2, g2 = run(mod, X, idx, G)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(o1, o2))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(g1, g2)) and all(torch.isfinite(g).all() for g in g1)


def test_the_call_runs_on_the_callers_stream_behind_a_delayed_producer(cuda):
    """matrices, index and incoming gradient hold decoys until a copy on the side stream, behind a delay, puts the real values there;
    forward and backward are made on that stream and must see them.  A launch on any other stream reads NaN or the rotated index."""
    d, S, H, B = 100, 3, 3, 1031
    rng = np.random.default_rng(17)
    real = [torch.from_numpy(rng.standard_normal((ec.N_ROWS, d)).astype(np.float32)).to(cuda) for _ in range(S * H)]
    idx_real = torch.from_numpy(ec.make_index(B, rng)).to(cuda)
    G_real = [torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32)).to(cuda) for _ in range(H)]
    mod = make_module("per_feature", S, H, d, ec.make_weights("per_feature", S, H, d, rng), cuda)
    lists = lambda flat: [flat[h * S:(h + 1) * S] for h in range(H)]          # noqa: E731
    want_o, want_g = run(mod, lists(real), idx_real, G_real)
    want_o, want_g = [o.detach().clone() for o in want_o], [g.clone() for g in want_g]
    x = [torch.full_like(r, float("nan")) for r in real]
    idx = torch.roll(idx_real, 1)
    G = [torch.full_like(g, float("nan")) for g in G_real]
    side = independent_stream(cuda)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        delay(side, 20.0)
        for dst, src in zip(x + G + [idx], real + G_real + [idx_real]):
            dst.copy_(src, non_blocking=True)
        got_o, got_g = run(mod, lists(x), idx, G)
        got_o = [o.detach().to("cpu", non_blocking=True) for o in got_o]
        got_g = [g.to("cpu", non_blocking=True) for g in got_g]
    side.synchronize()
    for a, b in zip(got_o + got_g, want_o + want_g):
        assert np.array_equal(a.numpy().view(np.int32), b.cpu().numpy().view(np.int32))


def test_more_matrices_than_a_call_takes_are_split_by_group(cuda):
    d, B = 4, 63
    views = device_pool(d, "rows", cuda)
    rng = np.random.default_rng(19)
    idx = torch.from_numpy(ec.make_index(B, rng)).to(cuda)
    n_groups, S = 5, 64                                               # 320 matrices: more than SGL_ENSEMBLE_MAX_MEMBERS
    groups = [[views[(g * 7 + s) % M_POOL] for s in range(S)] for g in range(n_groups)]
    w = torch.from_numpy(rng.standard_normal((n_groups * S, d)).astype(np.float32)).to(cuda).requires_grad_()
    G = [torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32)).to(cuda) for _ in range(n_groups)]
    outs = dev.ensemble_combine(groups, w, idx=idx, divisor=float(S))
    sum((o * g).sum() for o, g in zip(outs, G)).backward()
    for g in range(n_groups):
        wg = w.detach()[g * S:(g + 1) * S].clone().requires_grad_()
        one = dev.ensemble_combine([groups[g]], wg, idx=idx, divisor=float(S))[0]
        (one * G[g]).sum().backward()
        assert torch.equal(bits(one), bits(outs[g])) and torch.equal(bits(wg.grad), bits(w.grad[g * S:(g + 1) * S]))
    with pytest.raises(_lib.SglHipError, match="group_size=65"):      # a group cannot be split: refused by name
        dev.ensemble_combine([[views[s % M_POOL] for s in range(65)]], torch.ones(65, device=cuda), idx=idx)


def test_slab_output_and_argument_checks(cuda):
    d, S, H, B = 100, 2, 3, 63
    views = device_pool(d, "rows", cuda)
    X = [[views[h * S + s] for s in range(S)] for h in range(H)]
    rng = np.random.default_rng(23)
    w = torch.from_numpy(rng.standard_normal((S * H,)).astype(np.float32)).to(cuda)
    idx = torch.from_numpy(ec.make_index(B, rng)).to(cuda)
    outs = dev.ensemble_combine(X, w, idx=idx, divisor=2.0)
    slab = torch.full((B, H * d), float("nan"), device=cuda)
    back = dev.ensemble_combine(X, w, idx=idx, divisor=2.0, out=slab)
    assert all(b.data_ptr() == slab.data_ptr() + 4 * h * d for h, b in enumerate(back))
    assert torch.equal(bits(slab), bits(torch.cat(outs, dim=1)))
    assert torch.equal(bits(torch.cat(dev.ensemble_combine(X, w.view(-1, 1), idx=idx, divisor=2.0), dim=1)), bits(slab))
    grad_x = views[0].clone().requires_grad_()
    with pytest.raises(TypeError, match="constants of the model"):
        dev.ensemble_combine([[grad_x]], torch.ones(1, device=cuda))
    with pytest.raises(TypeError, match="bfloat16"):
        dev.ensemble_combine([[views[0].to(torch.bfloat16)]], torch.ones(1, device=cuda))
    with pytest.raises(ValueError):
        dev.ensemble_combine(X, torch.ones(S * H + 1, device=cuda))
    empty = dev.ensemble_combine(X, w, idx=torch.zeros(0, dtype=torch.int64, device=cuda))
    assert all(tuple(o.shape) == (0, d) for o in empty)
