"""Greedy k-means++ seeding (csrc/sgl_kmeans_seed.hip, include/sgl_kmeans_seed.h; device.kmeans_seed, kmeans init="greedy-k-means++") on a
real MI355X: run with `-m gpu`.  The reference is kmeans_seed_common.seed_reference, the step rule in numpy float64.  Integer rows in
[-4, 4] make every squared distance an exact integer and every float64 sum of them exact in any order: the three outputs must EQUAL
the reference.  Float rows: the distances come from kmeans_assign against the one candidate row, and inside the asserted margin the
float64 summation order cannot move a draw or a winner."""
import ctypes

import numpy as np
import pytest
import torch

from kmeans_common import LAYOUTS, N_ROWS, blob_set, in_layout
from kmeans_seed_common import FLOAT_CASES, MARGIN, draws_table, seed_reference
from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.tricks import kmeans

pytestmark = pytest.mark.gpu
TRIALS = (1, 2, 5, 8)
KS = (1, 2, 7)
_INT = {}


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def rule(n, d, trials):
    out = (ctypes.c_int64 * 5)()
    _lib.check(_lib.lib().sgl_kmeans_seed_rule(n, d, trials, out), "sgl_kmeans_seed_rule")
    return tuple(out)                                                   # B, R, chunk, chunks, LDS bytes


ROWS = rule(N_ROWS, 100, 1)[1]                                          # R: a function of n alone
WIDTHS = (1, 3, 4, 100, 131, rule(N_ROWS, 1 << 20, 8)[2] + 3)           # the last: beyond one column chunk of 8 candidates
# (rows, loss_blocks): below one block; R - 1, R, R + 1; five blocks with a ragged last one; one block over all rows; three blocks
RUNS = ((100, 0), (ROWS - 1, 0), (ROWS, 0), (ROWS + 1, 0), (N_ROWS, 0), (N_ROWS, 1), (N_ROWS, 3))


def integer_rows(d):
    """(x, all squared distances in float64, exact) -- once per width, left unchanged; every seventh row repeats the one before it"""
    if d not in _INT:
        x = np.random.default_rng(2000 + d).integers(-4, 5, (N_ROWS, d)).astype(np.float32)
        x[1::7] = x[0::7][:len(x[1::7])]
        sq = (x.astype(np.float64) ** 2).sum(1)
        _INT[d] = (x, sq[:, None] + sq[None, :] - 2.0 * (x.astype(np.float64) @ x.astype(np.float64).T))
    return _INT[d]


def edge_draws(k, trials, seed):
    draws = np.random.default_rng(seed).random((k, trials))
    draws[-1, 0], draws[-1, -1], draws[k // 2, 0] = 0.0, 1.0 - 2.0 ** -53, 1.0 - 2.0 ** -53
    return draws


def seed_on(cuda, x, k, draws, trials, blocks=0):
    try:
        _lib.set_tuning("loss_blocks", blocks)
        ids, near, pot = dev.kmeans_seed(x, k, torch.from_numpy(draws).to(cuda), trials)
    finally:
        _lib.set_tuning("loss_blocks", 0)
    return ids.cpu().numpy(), near.cpu().numpy(), pot.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("layout", ("contiguous",) + LAYOUTS)
@pytest.mark.parametrize("d", WIDTHS)
def test_exact_on_integer_rows(cuda, d, layout):
    if d == WIDTHS[-1]:
        assert rule(N_ROWS, d, 8)[3] > 1 and rule(N_ROWS, d, 1)[3] == 1, "no case with more than one column chunk is left"
    x, dist = integer_rows(d)
    bad = []
    for n, blocks in RUNS:
        xd = torch.from_numpy(x[:n]).to(cuda) if layout == "contiguous" else in_layout(x[:n], layout, cuda)
        for trials in TRIALS:
            for k in KS:
                draws = edge_draws(k, trials, 31 * d + 7 * trials + k)
                ids, near, pot, _ = seed_reference(lambda c: dist[c, :n].astype(np.float32), n, k, trials, draws)
                got = seed_on(cuda, xd, k, draws, trials, blocks)
                if not (np.array_equal(got[0], ids) and np.array_equal(got[1], near) and np.array_equal(got[2], pot)):
                    bad.append((n, blocks, trials, k, got[0].tolist(), ids.tolist(), int((got[1] != near).sum())))
    assert not bad, bad[:5]


def float_reference(cuda, xd, n, k, trials, draws):
    """the distances of the reference are the EXISTING assignment kernel's against the one candidate row, not the code under test"""
    return seed_reference(lambda c: dev.kmeans_assign(xd, xd[c:c + 1])[1].cpu().numpy(), n, k, trials, draws)


@pytest.mark.parametrize("blob,trials,seed", FLOAT_CASES)
def test_float_rows_and_the_public_interface(cuda, blob, trials, seed):
    n, d, k, spread = blob
    x = blob_set(n, d, k, spread)[0]
    xd, draws = torch.from_numpy(x).to(cuda), draws_table(k, trials, seed)
    ids, near, pot, margin = float_reference(cuda, xd, n, k, trials, draws)
    assert margin >= MARGIN, margin                                     # a condition on the inputs
    got = seed_on(cuda, xd, k, draws, trials)
    assert np.array_equal(got[0], ids) and same_bits(got[1], near)
    assert np.allclose(got[2], pot, rtol=2 * n * 2.0 ** -53, atol=0)    # two float64 sums of n terms >= 0 in different orders
    for again in [seed_on(cuda, xd, k, draws, trials)] + [seed_on(cuda, in_layout(x, layout, cuda), k, draws, trials) for layout in LAYOUTS]:
        assert np.array_equal(again[0], got[0]) and same_bits(again[1], got[1]) and np.array_equal(again[2], got[2]), "runs or layouts differ"
    # kmeans draws the same table from its generator: the seeded run must be the run from the reference's centres, bit for bit
    want = kmeans(xd, k, init=xd[torch.from_numpy(ids).to(cuda)])
    run = kmeans(xd, k, init="greedy-k-means++", n_local_trials=trials, seed=seed, n_init=1)
    assert torch.equal(run.labels, want.labels) and torch.equal(run.centres.view(torch.int32), want.centres.view(torch.int32))
    assert run.inertia == want.inertia and run.n_iter == want.n_iter


def test_non_finite_and_degenerate_rows(cuda):
    (n, d, k, spread), trials, seed = FLOAT_CASES[3]
    x = blob_set(n, d, k, spread)[0].copy()
    x[40, d // 2] = float("nan")
    xd, draws = torch.from_numpy(x).to(cuda), draws_table(k, trials, seed)
    ids, near, pot = seed_on(cuda, xd, k, draws, trials)
    want = float_reference(cuda, xd, n, k, trials, draws)
    assert np.isnan(near[40]) and np.isfinite(np.delete(near, 40)).all() and 40 not in ids[1:] and np.isfinite(pot).all()
    assert want[3] >= MARGIN and np.array_equal(ids, want[0]) and same_bits(near, want[1])
    same = torch.from_numpy(np.repeat(x[:1], 300, axis=0)).to(cuda)     # all rows identical: nothing can be drawn, the clamp decides
    ids, near, pot = seed_on(cuda, same, k, draws, trials)
    assert (ids[1:] == 299).all() and not near.any() and not pot.any()


def test_the_refusals(cuda):
    x = torch.zeros((8, 16), dtype=torch.float32, device=cuda)
    draws = torch.zeros((2, 2), dtype=torch.float64, device=cuda)
    for trials in (0, 9):
        with pytest.raises(ValueError, match="trials"):
            dev.kmeans_seed(x, 2, torch.zeros((2, trials), dtype=torch.float64, device=cuda), trials)
        with pytest.raises(ValueError, match="n_local_trials"):
            kmeans(x, 2, init="greedy-k-means++", n_local_trials=trials)
    with pytest.raises(ValueError, match="n_samples"):
        dev.kmeans_seed(x, 9, torch.zeros((9, 2), dtype=torch.float64, device=cuda), 2)
    with pytest.raises(TypeError, match="bfloat16"):
        dev.kmeans_seed(x.to(torch.bfloat16), 2, draws, 2)
    for wrong in (draws.cpu(), draws.to(torch.float32), draws[:, :1]):
        with pytest.raises(ValueError, match="draws"):
            dev.kmeans_seed(x, 2, wrong, 2)
    with pytest.raises(ValueError, match="init"):
        kmeans(x, 2, init="greedy")
