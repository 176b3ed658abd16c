"""The learnable hop aggregators on stored hop rows (include/sgl_hop_rows.h; device.hop_scores2_rows, hop_wsum2d_rows,
hop_colsum_rows, MessageOp.aggregate_rows, config.aggregate_in_place) on a real MI355X: run with `-m gpu`.

Two references per case.  (1) float64 numpy on the stored values (a bfloat16 element widens exactly).  A float32 sum of k terms in any
order is within gamma_k * sum|terms|, gamma_k = k u / (1 - k u), u = 2^-24: k = d for the per-hop scores P and for dW, d * |mask| for
the reference part A (that is its length), m for the column sums; the fma chain of the weighted sum is within (H + 1) u sum|w x|.
(2) The contract: scores, the weighted sum and its dW bit-equal to gather_hops + hop_scores2 (without a reference part: hop_scores,
the plain row-dot) / hop_wsum2d."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from sgl_amd import config
from sgl_amd import device as dev
from sgl_amd.models.homo import GAMLP, PASCA_V2
from sgl_amd.operators.message_op import LearnableWeightedMessageOp
from test_gpu_linear_head import U, cuda, same  # noqa: F401 (cuda: the fixture)

pytestmark = pytest.mark.gpu
DTYPES = (torch.float32, torch.bfloat16)
DS, HS, MS = (1, 3, 4, 100, 147, 260, 512), (1, 3, 16), (1, 63, 1031, None)
# every d (one-lane rows, the straddling vector, every lane / chunk class, the limit) with every H; m and the layout walk through
# their values along the way (None: no index, every row; view: rows at an offset inside a larger NaN-filled buffer)
CASES = [(d, H, MS[(i + j) % 4], (i + 2 * j) % 3 == 0) for i, d in enumerate(DS) for j, H in enumerate(HS)]
N_ROWS = 203


def gamma(k):
    return k * U / (1 - k * U)


def make_tables(rng, n_rows, d, H, dtype, view, cuda):
    out = []
    for _ in range(H):
        src = torch.from_numpy(rng.standard_normal((n_rows, d)).astype(np.float32)).to(dtype)
        t = (torch.full((n_rows + 5, dev.round_up(d, 4) + 8), float("nan"), dtype=dtype, device=cuda)[3:3 + n_rows, 4:4 + d] if view
             else dev.alloc_rows(n_rows, d, cuda, dtype=dtype))
        t.copy_(src)
        out.append(t)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("d,H,m,view", CASES)
def test_row_kernels_against_float64_and_the_gathered_route(cuda, dtype, d, H, m, view):
    rng = np.random.default_rng(d * 1009 + H * 17 + (m or 0))
    tabs = make_tables(rng, N_ROWS, d, H, dtype, view, cuda)
    at = np.arange(N_ROWS) if m is None else rng.integers(-N_ROWS, N_ROWS, m)
    if m is not None:
        at[:3] = (-1, 0, N_ROWS - 1)[:m]                                  # negative, first, last; duplicates
        at[m // 2] = at[0]
    n = len(at)
    bad = at.copy()
    keep = torch.ones(n, dtype=torch.bool, device=cuda)
    if m is not None and m > 4:
        bad[m // 3] = N_ROWS                                              # one index out of range; the references get a valid stand-in
        keep[m // 3] = False
    idx, idx_bad = (None, None) if m is None else (torch.from_numpy(at).to(cuda), torch.from_numpy(bad).to(cuda))
    v, u = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(cuda) for s in ((d,), (H, d)))
    w, g = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(cuda) for s in ((n, H), (n, d)))
    mask, h0, h1 = sum(1 << j for j in range(0, H, 2)), (0 if H < 3 else 1), H
    # the rows route, on the index with the bad entry
    vr, ur, wr = v.clone().requires_grad_(), u.clone().requires_grad_(), w.clone().requires_grad_()
    p, a = dev.hop_scores2_rows(tabs, idx_bad, vr, ur, mask, h0, h1)
    out = dev.hop_wsum2d_rows(tabs, idx_bad, wr)
    out.backward(g)
    out_v = dev.hop_wsum2d_rows(tabs, idx_bad, w[0])                      # one weight vector for every row
    cs_bad = dev.hop_colsum_rows(tabs, idx_bad, w)
    cs, cs_again, cs_shared = (dev.hop_colsum_rows(tabs, idx, *args) for args in ((w,), (w,), (w[:, 0], True)))
    gp = torch.from_numpy(rng.standard_normal((n, h1 - h0)).astype(np.float32)).to(cuda)
    pv, _ = dev.hop_scores2_rows(tabs, idx, vr, None, 0, h0, h1)         # the plain gate scores; their backward is a column sum
    pv.backward(gp)
    # the gathered route, on valid indices
    G = dev.gather_hops(tabs, torch.from_numpy(at).to(cuda))
    w0 = w.clone().requires_grad_()
    p0, a0 = dev.hop_scores2(G, v, u, mask, h0, h1)
    out0 = dev.hop_wsum2d(G, w0)
    out0.backward(g)
    torch.cuda.synchronize()
    assert same(pv.detach()[keep], dev.hop_scores(G, v)[:, h0:h1][keep]) and same(p.detach()[keep], p0[keep]) and same(a.detach()[keep], a0[keep]), "scores: not the gathered bits"
    assert same(out.detach()[keep], out0.detach()[keep]) and same(wr.grad[keep], w0.grad[keep]), "weighted sum / dW: not the gathered bits"
    assert same(out_v[keep], dev.hop_wsum2d(G, w[0].expand(n, H).contiguous())[keep]), "weight vector: not the gathered bits"
    assert same(cs, cs_again), "two runs of the column sums differ"
    # exact properties: NaN where the bad row enters and nowhere else; pad columns zero
    gone = ~keep
    assert bool(torch.isnan(p[gone]).all()) and bool(torch.isnan(a[gone]).all()) and bool(torch.isnan(out[gone]).all())
    assert bool(torch.isnan(wr.grad[gone]).all()) and (not gone.any() or bool(torch.isnan(cs_bad).all()))
    assert not bool(torch.isnan(p[keep]).any() | torch.isnan(out[keep]).any() | torch.isnan(wr.grad[keep]).any() | torch.isnan(cs).any())
    assert not dev.padded_parent(out.detach())[:, d:].any(), "pad columns are not zero"
    # float64 on the stored values
    x64 = np.stack([t.double().cpu().numpy()[at] for t in tabs])         # [H, n, d]
    v64, u64, w64, g64, gp64 = (t.double().cpu().numpy() for t in (v, u, w, g, gp))
    ok = keep.cpu().numpy()
    ref = [j for j in range(H) if (mask >> j) & 1]
    checks = {
        "P": (p.detach()[:, :], np.stack([x64[h] @ v64 for h in range(h0, h1)], 1), gamma(d) * np.stack([np.abs(x64[h]) @ np.abs(v64) for h in range(h0, h1)], 1)),
        "A": (a.detach(), sum(x64[j] @ u64[j] for j in ref), gamma(d * len(ref)) * sum(np.abs(x64[j]) @ np.abs(u64[j]) for j in ref)),
        "out": (out.detach(), np.einsum("nh,hnd->nd", w64, x64), (H + 1) * U * np.einsum("nh,hnd->nd", np.abs(w64), np.abs(x64))),
        "out_v": (out_v, np.einsum("h,hnd->nd", w64[0], x64), (H + 1) * U * np.einsum("h,hnd->nd", np.abs(w64[0]), np.abs(x64))),
        "dW": (wr.grad, np.einsum("nd,hnd->nh", g64, x64), gamma(d) * np.einsum("nd,hnd->nh", np.abs(g64), np.abs(x64))),
        "colsum": (cs, np.einsum("nh,hnd->hd", w64, x64), gamma(n) * np.einsum("nh,hnd->hd", np.abs(w64), np.abs(x64))),
        "colsum_shared": (cs_shared, np.einsum("n,hnd->hd", w64[:, 0], x64), gamma(n) * np.einsum("n,hnd->hd", np.abs(w64[:, 0]), np.abs(x64))),
        "dv": (vr.grad, np.einsum("nh,hnd->d", gp64, x64[h0:h1]), gamma(n * (h1 - h0)) * np.einsum("nh,hnd->d", np.abs(gp64), np.abs(x64[h0:h1]))),
    }
    worst = {}
    for name, (got, want, tol) in checks.items():
        ratio = np.abs(got.cpu().numpy().astype(np.float64) - want) / np.maximum(tol, 1e-300)
        if name in ("P", "A", "out", "out_v", "dW"):
            ratio = ratio[ok]
        worst[name] = float(ratio.max())
    print((d, H, m, view, str(dtype)), worst)
    assert all(np.isfinite(r) and r <= 1.0 for r in worst.values()), worst


@pytest.mark.parametrize("hop_dtype", ("float32", "bfloat16"))
@pytest.mark.parametrize("kind", ("jk", "gate"))
def test_models_in_place_give_the_gathered_logits_and_the_gradients_of_a_step(cuda, monkeypatch, kind, hop_dtype):
    """GAMLP ('jk') and PASCA_V2 ('gate': gathered, its rows take the one-pass gate kernel), one forward and backward with the option
    off and on.  Logits, dOut (the gradient that reaches the aggregate) and the head's gradients: the same bits.  The aggregator's
    gradients are column sums of ds[i, h] x_h[idx_i, c]; ds64, the score gradients, come from a float64 replay of the aggregator on
    the stored values and this dOut.  T = sum|ds64 x| over the k terms of an element (k = m H for the per-hop weights, m for a row
    of the reference part).  The float32 ds of a route is not ds64: it is a short float32 expression (at most 16 roundings after
    each of the H hop terms, no intermediate above E = max_h <|dOut_i|, |x_h|>) of dW, which itself carries gamma_d: |ds32 - ds64|
    <= (gamma_d + 32 H u) E, summed against |x| in S (the score at flat position q belongs to weights row i for 'gate', to row q // H
    under the scrambled pairing of 'jk').
    So a route is within gamma_k (T + S) + S of the float64 gradient; the two routes of 'jk' share their ds bits and are within
    2 gamma_k (T + S) of each other, those of 'gate' evaluate ds by two expressions: 2 gamma_k (T + S) + 2 S."""
    n, d, c, K, m = 300, 20, 5, 3, 131
    rng = np.random.default_rng(5)
    adj = sp.random(n, n, density=0.02, random_state=3, format="csr", dtype=np.float32)
    adj = ((adj + adj.T) > 0).astype(np.float32).tocsr()
    monkeypatch.setattr(config, "hop_dtype", hop_dtype)
    torch.manual_seed(0)
    model = (GAMLP if kind == "jk" else PASCA_V2)(K, d, c, 16, 2)
    model.preprocess(adj, rng.standard_normal((n, d)).astype(np.float32))
    model.to(cuda).eval()
    assert model._processed_feat_list[0].dtype == dev.hop_torch_dtype(hop_dtype)
    idx = rng.integers(0, n, m)
    gl = torch.from_numpy(rng.standard_normal((m, c)).astype(np.float32)).to(cuda)
    seen = []
    hook = model._base_model.register_forward_pre_hook(lambda mod, args: seen.append(args[0]) or args[0].retain_grad())
    runs = []
    for on in (False, True):
        monkeypatch.setattr(config, "aggregate_in_place", on)
        model.zero_grad()
        logits = model.model_forward(idx, cuda)
        logits.backward(gl)
        runs.append((logits.detach(), seen[-1].grad, {k_: p.grad.clone() for k_, p in model.named_parameters()}))
    hook.remove()
    (off_logits, off_dout, off), (on_logits, on_dout, on_) = runs
    assert same(off_logits, on_logits) and same(off_dout, on_dout), float((off_logits - on_logits).abs().max())
    assert all(same(off[k_], on_[k_]) for k_ in off if k_.startswith("_base_model")), "the head's gradients differ"
    # float64 replay of the aggregator on the stored values
    op = model._pre_msg_op
    s_, e_ = op._start, op._end
    H = e_ - s_
    lin = op._LearnableWeightedMessageOp__learnable_weight
    x = torch.stack([t.double()[torch.from_numpy(idx).to(cuda)] for t in model._processed_feat_list])       # [L, m, d]
    L = x.shape[0]
    w, bias = lin.weight.detach().double().view(-1), lin.bias.detach().double()
    d_ref = L * d if kind == "jk" else 0
    P = torch.einsum("hmd,d->hm", x[s_:e_], w[d_ref:]).requires_grad_()
    A = (torch.einsum("lmd,ld->m", x, w[:d_ref].view(L, d)) if d_ref else torch.zeros(m, dtype=torch.float64, device=cuda)).requires_grad_()
    flat = (P + A + bias).reshape(-1)
    W = torch.softmax(torch.sigmoid(flat.view(-1, H) if kind == "jk" else flat.view(H, -1).T), dim=1)
    torch.einsum("mh,hmd->md", W, x[s_:e_]).backward(on_dout.double())
    ax, ds, da = x.abs(), P.grad.abs(), A.grad.abs()
    E = torch.einsum("md,hmd->mh", on_dout.double().abs(), ax[s_:e_]).max(1).values
    # E of the score at flat position q = h m + i: 'gate' weights row i, 'jk' (the scrambled pairing) weights row q // H
    E = E.repeat_interleave(H).view(H, m) if kind == "jk" else E.expand(H, m)
    eps = gamma(d) + 32 * H * U
    want = {"weight": torch.cat([torch.einsum("m,lmd->ld", A.grad, x).reshape(-1)[:d_ref], torch.einsum("hm,hmd->d", P.grad, x[s_:e_])]),
            "bias": P.grad.sum().reshape(1)}
    T = {"weight": torch.cat([torch.einsum("m,lmd->ld", da, ax).reshape(-1)[:d_ref], torch.einsum("hm,hmd->d", ds, ax[s_:e_])]),
         "bias": ds.sum().reshape(1)}
    S = {"weight": eps * torch.cat([torch.einsum("m,lmd->ld", E.sum(0), ax).reshape(-1)[:d_ref], torch.einsum("hm,hmd->d", E, ax[s_:e_])]),
         "bias": eps * E.sum().reshape(1)}
    gk = {"weight": torch.cat([torch.full((d_ref,), gamma(m)), torch.full((d,), gamma(m * H))]).to(cuda), "bias": gamma(m * H)}
    worst = {}
    for name in ("weight", "bias"):
        key = f"_pre_msg_op._LearnableWeightedMessageOp__learnable_weight.{name}"
        g_off, g_on = off[key].double().view(-1), on_[key].double().view(-1)
        between = 2 * gk[name] * (T[name] + S[name]) + (2 * S[name] if kind == "gate" else 0)
        exact = gk[name] * (T[name] + S[name]) + S[name]
        worst[name] = (float(((g_on - g_off).abs() / between).max()), float(((g_on - want[name]).abs() / exact).max()),
                       float(((g_off - want[name]).abs() / exact).max()))
    print(kind, hop_dtype, "fractions of the bounds (on - off, on - float64, off - float64):", worst, "largest bound / largest |gradient|:",
          float((gk["weight"] * (T["weight"] + S["weight"]) + S["weight"]).max() / want["weight"].abs().max()))
    assert all(np.isfinite(r) and r <= 1.0 for rs in worst.values() for r in rs), worst


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("kind", ("simple", "simple_allow_neg"))
def test_vector_kinds_in_place_against_the_gathered_route(cuda, kind, dtype):
    """one weight vector for every row (ldw = 0).  Gathered, these kinds go through another kernel (the 1-D weighted sum); both are a
    float32 sum of H products per element, each within (H + 1) u sum|w x| of the exact sum of the same float32 weights.  The
    gradient of the weights is a sum over the m d products of a hop: gamma_{m d} sum|dOut x| per route."""
    m, d, H = 257, 147, 4
    rng = np.random.default_rng(13)
    tabs = make_tables(rng, N_ROWS, d, H, dtype, False, cuda)
    at = rng.integers(-N_ROWS, N_ROWS, m)
    g = torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32)).to(cuda)
    torch.manual_seed(1)
    op = LearnableWeightedMessageOp(0, H, kind, H - 1).to(cuda)
    got = []
    for rows in (True, False):
        op.zero_grad()
        out = op.aggregate_rows(tabs, at) if rows else op.aggregate(dev.gather_hops(tabs, at))
        out.backward(g)
        got.append((out.detach().double(), next(op.parameters()).grad.double()))
    x = torch.stack([t.double()[torch.from_numpy(at).to(cuda)] for t in tabs])
    wts = op.hop_weights(tabs).detach().double().requires_grad_()
    want = torch.einsum("h,hmd->md", wts, x)
    want.backward(g.double())
    tol_out = (H + 1) * U * torch.einsum("h,hmd->md", wts.detach().abs(), x.abs())
    dw_terms = torch.einsum("md,hmd->h", g.double().abs(), x.abs())
    assert all(bool(((out - want.detach()).abs() <= tol_out).all()) for out, _ in got), "the weighted sum misses its bound"
    if kind == "simple_allow_neg":                                       # the weights are the parameter itself: its gradient is dW summed
        assert all(bool(((grad - wts.grad).abs() <= gamma(m * d) * dw_terms).all()) for _, grad in got)
    assert bool(torch.isfinite(got[0][1]).all()) and bool(((got[0][1] - got[1][1]).abs() <= 2 * gamma(m * d) * dw_terms.max()).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("d,H", ((147, 5), (20, 16), (260, 16), (100, 6)))   # narrow lane groups; more hops than lanes; two chunks
def test_gate_in_place_has_the_bits_of_the_one_pass_kernel(cuda, dtype, d, H):
    rng = np.random.default_rng(d + H)
    tabs = make_tables(rng, N_ROWS, d, H, dtype, False, cuda)
    at = rng.integers(-N_ROWS, N_ROWS, 1031)
    torch.manual_seed(d)
    op = LearnableWeightedMessageOp(0, H, "gate", d).to(cuda)
    with torch.no_grad():
        assert same(op.aggregate_rows(tabs, at), op.aggregate(dev.gather_hops(tabs, at)))
