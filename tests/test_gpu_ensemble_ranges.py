"""K16's weight gradient (sgl_ensemble_combine_bwd_f32) at the sizes ensemble_common.BATCHES never reaches: with at most 1500 rows
a first-level range is one row step (bwd_per_block = 32), there are at most 47 blocks, and the second level's chain over every 64th
block never takes a second step.  Here: 65, 130, 513 and 625 blocks, ranges of one and of two row steps -- the value check and the
run-to-run bits of test_gpu_ensemble.py, inside the bounds of ensemble_common.py as they are.  Run with `-m gpu`."""
import numpy as np
import pytest
import torch

import ensemble_common as ec
from test_gpu_ensemble import bits, device_pool, host_pool, make_module, run          # one pool, one module set-up for K16's GPU tests

from sgl_amd import _lib

pytestmark = pytest.mark.gpu

# n_idx -> (blocks, rows per block) of the launch arithmetic restated in ensemble_common
SIZES = {2049: (65, 32), 4133: (130, 32), 32769: (513, 64), 40000: (625, 64)}
WIDTHS = (3, 4, 100)
GROUP_SIZES = (1, 9)
assert max(GROUP_SIZES) * 2 <= 51                                   # members taken from test_gpu_ensemble's pool of 51 matrices


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def members(mode, group_size):
    """(S, H) that give groups of `group_size` members: `fast` has one group of S * H, the others H groups of S"""
    if mode == "fast":
        return (1, 1) if group_size == 1 else (3, 3)
    return group_size, 2


def test_the_sizes_are_the_ones_the_small_batches_miss():
    assert all(ec.bwd_per_block(B) == 32 and ec.bwd_blocks(B) <= 47 for B in (1, 63, 1031, ec.N_ROWS))
    for n_idx, (blocks, per_block) in SIZES.items():
        assert (ec.bwd_blocks(n_idx), ec.bwd_per_block(n_idx)) == (blocks, per_block)
    assert {-(-b // 64) for b, _ in SIZES.values()} == {2, 3, 9, 10}        # steps of a lane's chain over every 64th block
    # the bounds below are ensemble_common's as they are: gamma(k) with k from the launches this file makes.  The least of them, 15,
    # is `fast` at d = 3 (no division, one column per lane); the two dividing modes range from 16 to 56.
    ks = [ec.bwd_roundings(n, d, cs, vec, div) for n in SIZES for d in WIDTHS for cs, div in ((1, True), (0, True), (0, False))
          for vec in ((1, 4) if d % 4 == 0 else (1,))]
    assert (min(ks), max(ks)) == (15, 56)


@pytest.mark.parametrize("layout", ("rows", "cols"))
@pytest.mark.parametrize("mode", ec.MODES)
@pytest.mark.parametrize("n_idx", list(SIZES))
def test_values_gradients_and_repeat_bits_at_many_blocks(cuda, n_idx, mode, layout):
    worst_f = worst_b = 0.0
    for d in WIDTHS:
        host, views = host_pool(d), device_pool(d, layout, cuda)
        rng = np.random.default_rng(11 * d + n_idx + len(mode))
        for group_size in GROUP_SIZES:
            S, H = members(mode, group_size)
            X_h = [[host[h * S + s] for s in range(S)] for h in range(H)]
            X_d = [[views[h * S + s] for s in range(S)] for h in range(H)]
            W = ec.make_weights(mode, S, H, d, rng)
            mod = make_module(mode, S, H, d, W, cuda)
            n_groups, gs, cs, divisor = ec.kernel_shape(mode, S, H)
            assert gs == group_size
            idx = ec.make_index(n_idx, rng)
            G_h = [rng.standard_normal((n_idx, d)).astype(np.float32) for _ in range(n_groups)]
            idx_d, G_d = torch.from_numpy(idx).to(cuda), [torch.from_numpy(g).to(cuda) for g in G_h]
            outs, grads = run(mod, X_d, idx_d, G_d)
            outs, grads = [o.detach().clone() for o in outs], [g.clone() for g in grads]
            T, bound = ec.forward_f64(mode, X_h, W, idx)
            assert len(outs) == len(T)
            for o, t, b in zip(outs, T, bound):
                err = np.abs(o.cpu().numpy().astype(np.float64) - t)
                assert np.all(err <= b), (d, group_size, float((err - b).max()))
                worst_f = max(worst_f, float((err / np.maximum(b, 1e-300)).max()))
            # the gradient buffer autograd hands over is contiguous: 16-byte rows when d is a multiple of 4
            k = ec.bwd_roundings(n_idx, d, cs, 4 if (layout == "rows" and d % 4 == 0) else 1, divisor != 1.0)
            dT, mag = ec.backward_f64(mode, X_h, G_h, idx)
            dT, mag = (dT, mag) if isinstance(dT, list) else ([dT], [mag])
            assert len(grads) == len(dT)
            for g, t, m in zip(grads, dT, mag):
                assert g.shape == t.shape
                err = np.abs(g.cpu().numpy().astype(np.float64) - t)
                assert np.all(err <= ec.gamma(k) * m), (d, group_size, k, float((err - ec.gamma(k) * m).max()))
                worst_b = max(worst_b, float((err / np.maximum(ec.gamma(k) * m, 1e-300)).max()))
            o2, g2 = run(mod, X_d, idx_d, G_d)
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(outs, o2))
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(grads, g2)) and all(torch.isfinite(g).all() for g in grads)
    blocks, per_block = SIZES[n_idx]
    print(f"n_idx={n_idx} ({blocks} blocks of {per_block} rows) {mode} {layout}: worst forward error / bound {worst_f:.3f}, "
          f"worst backward error / bound {worst_b:.3f}")
