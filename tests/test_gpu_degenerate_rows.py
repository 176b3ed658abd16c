"""The aggregator kernels (csrc/sgl_aggregate.hip, sgl_aggregate_bf16.hip, sgl_rows.h) and K16 on non-finite, saturated and
degenerate rows, on a real MI355X: run with `-m gpu`.

Every wrapper of sgl_amd/device.py over the aggregator entry points is driven through the rule of degenerate_common.py -- one
element of one hop replaced by NaN, +-inf or +-3e38: what does not depend on it keeps its bits, what does has the statement's
NaN / inf masks and, where finite, its value -- and through the finite ill-conditioned regimes (NAFS at five scales with
correlated, duplicate and negated hops; gates saturated at +-20, +-90, +-200), each compared on its own with
oracle.truth_report.  The inputs, the statements, the case list and the rule are in degenerate_common.py; the conditions they rest
on are checked in test_degenerate_cpu.py.  No tolerance is chosen in this file."""
import numpy as np
import pytest
import torch

import degenerate_common as dc
import oracle
from agg_rows_common import tuned
from sgl_amd import _lib
from sgl_amd import device as dev
from test_gpu_ensemble import make_module, run as ensemble_pass

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def upload(x, dense, cuda, bf16=False):
    """one hop on the device: a dev.alloc_rows buffer (16-byte rows, zero pad columns), or a dense tensor (d % 4 != 0: rows that
    are only 4-byte aligned)"""
    t = torch.from_numpy(np.ascontiguousarray(x))
    if bf16:
        t = t.to(torch.bfloat16)                                        # exact: the values are bfloat16 numbers
    if dense:
        return t.to(cuda)
    out = dev.alloc_rows(x.shape[0], x.shape[1], cuda, dtype=t.dtype)
    out.copy_(t)
    return out


def device_parameters(p, cuda):
    return {k: torch.from_numpy(a).to(cuda) for k, a in p.items()}


def show(bad, most=12):
    """the first failures in full (pytest shortens the assertion's own message)"""
    for b in bad[:most]:
        print("   FAILED CHECK:", b)


def run(fam, X, p):
    """{statement's name: numpy array} of the family's wrapper; an output the wrapper returns twice is kept under both names"""
    got = {k: v.detach().float().cpu().numpy() for k, v in fam.gpu(X, p).items()}
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("name", list(dc.FAMILIES))
def test_one_poisoned_element_reaches_what_the_statement_says_and_nothing_else(cuda, name):
    fam = dc.FAMILIES[name]
    bad, worst, reached, n_cases = [], {}, set(), 0
    for k, s in enumerate(dc.family_shapes(fam)):
        hops, p = dc.host_hops(s.d, s.H, fam.bf16), dc.parameters(s.d, s.H)
        pd = device_parameters(p, cuda)
        kern = dc.kernel_of(fam, s)
        reached.add(kern[1] if kern else s.tag)
        with tuned(**s.tuning):
            X = [upload(x, s.dense, cuda, fam.bf16) for x in hops]
            clean_got = run(fam, X, pd)
            clean32 = dc.statement(fam, hops, p, torch.float32)
            for what, g in clean_got.items():                          # the clean run itself is finite
                if not np.isfinite(g).all():
                    bad.append((dc.sid(s), "clean", what, "not finite"))
            for inj in dc.injections(s, k, fam.bf16):
                bad_hops = dc.poisoned(hops, inj)
                Xp = list(X)
                Xp[inj.hop] = upload(bad_hops[inj.hop], s.dense, cuda, fam.bf16)
                got = run(fam, Xp, pd)
                s32 = dc.statement(fam, bad_hops, p, torch.float32)
                s64 = dc.statement(fam, bad_hops, p, torch.float64)
                for what, g in got.items():
                    ref = dc.ALIASES.get(what, what)
                    bad += [(dc.sid(s), tuple(inj)) + b for b in
                            dc.apply_rule(what, clean32[ref], s32[ref], s64[ref], clean_got[what], g, worst.setdefault(what, {}),
                                          cond=s64.get("cond:" + ref))]
                n_cases += 1
    print(f"\n[{name}] {n_cases} injections over {len(dc.family_shapes(fam))} shapes; reached {sorted(map(str, reached))}; "
          f"worst err / bound on touched finite entries: { {k: round(v.get('ratio', 0.0), 3) for k, v in worst.items()} }")
    show(bad)
    assert not bad, (len(bad), bad[:8])


# ---- the regimes -----------------------------------------------------------------------------------------------------------------------
class Regimes:
    """collects failed checks and the worst err / bound per regime"""

    def __init__(self, family):
        self.family, self.bad, self.worst = family, [], {}

    def truth(self, label, regime, what, got, ref32, ref64, rows=None, axis=0, cond=None):
        got, ref32, ref64 = (np.asarray(a) for a in (got, ref32, ref64))
        if rows is not None:
            got, ref32, ref64 = (np.take(a, rows, axis=axis) for a in (got, ref32, ref64))
        if not np.isfinite(got).all():
            self.bad.append((label, regime, what, "not finite"))
            return
        rep = oracle.truth_report(got, ref32, ref64, cond=cond)
        self.worst[regime] = max(self.worst.get(regime, 0.0), rep["err_got"] / max(rep["bound"], rep["cond_bound_max"], 1e-300))
        if not rep["ok"]:
            self.bad.append((label, regime, what, rep))

    def weights(self, label, regime, w, roundings=4):
        ok, roundings = dc.weight_rows(w, roundings)
        self.worst["weight row sum - 1 (roundings)"] = max(self.worst.get("weight row sum - 1 (roundings)", 0.0), roundings)
        if not ok:
            self.bad.append((label, regime, "weight rows", roundings))

    def finish(self):
        print(f"\n[{self.family}] worst err / bound per regime: { {k: round(v, 3) for k, v in self.worst.items()} }")
        show(self.bad)
        assert not self.bad, (len(self.bad), self.bad[:8])


REGIME_SHAPES = [s for s in dc.shapes() if s != dc.ONLY_16X3]


@pytest.mark.parametrize("scale", dc.NAFS_SCALES)
def test_nafs_at_every_scale_with_correlated_duplicate_and_negated_hops(cuda, scale):
    """nafs_aggregate, every prefix of nafs_prefix and the bfloat16 NAFS: each scale is a regime of its own.  The weight rows are
    finite and non-negative; how far they are from summing to 1 is printed, not bounded: the row of thirteen hops with the scores
    (0.75, -0.75 x 12) of a negated row at 2^-33 adds twelve equal terms one after the other, every addition rounds the same way, and
    torch's own float32 soft-max is 4.75 roundings off on that row as well."""
    rep = Regimes(f"nafs 2^{scale}")
    regime = f"2^{scale}"
    for s in REGIME_SHAPES:
        hops = dc.nafs_regime(s.d, s.H, scale)
        p = dc.parameters(s.d, s.H)
        pd = device_parameters(p, cuda)
        for name in ("nafs", "prefix_0", "bf16_nafs"):
            fam = dc.FAMILIES[name]
            if not fam.takes(s):
                continue
            hh = [torch.from_numpy(x).to(torch.bfloat16).float().numpy() for x in hops] if fam.bf16 else hops
            with tuned(**s.tuning):
                got = run(fam, [upload(x, s.dense, cuda, fam.bf16) for x in hh], pd)
            s32, s64 = dc.statement(fam, hh, p, torch.float32), dc.statement(fam, hh, p, torch.float64)
            for what, g in got.items():
                rep.truth((name, dc.sid(s)), regime, what, g, s32[what], s64[what])
            if "W" in got:
                rep.weights((name, dc.sid(s)), regime, got["W"], roundings=None)
    rep.finish()


@pytest.mark.parametrize("name,make", [("gate", dc.gate_regime), ("recursive", dc.recursive_regime)])
def test_saturated_gates(cuda, name, make):
    """pre-sigmoid scores of +-20, +-90 and +-200 (the recursion: at every step) next to O(1) rows: the forward, W, G and every
    gradient; the rows of one target are a regime, compared on their own.  Aligned hops take the fused kernel, the same hops as
    dense tensors (d % 4 != 0) the two-pass path behind the same call."""
    fam = dc.FAMILIES[name]
    rep = Regimes(name)
    for s in REGIME_SHAPES:
        hops, p, rows = make(s.d, s.H)
        pd = device_parameters(p, cuda)
        s32, s64 = dc.statement(fam, hops, p, torch.float32), dc.statement(fam, hops, p, torch.float64)
        rest = [r for r in range(dc.N) if all(r not in rr for rr in rows.values())]
        for dense in sorted({s.dense, s.d % 4 != 0}):
            label = (name, dc.sid(s), "dense" if dense else "aligned")
            Xd = [upload(x, dense, cuda) for x in hops]
            assert dev.gate_fusable(Xd) == (dc.kernel_of(fam, s) is not None and not dense)
            with tuned(**s.tuning):
                got = run(fam, Xd, pd)
            for what, g in got.items():
                ref = dc.ALIASES.get(what, what)
                if dc.row_axis(fam, ref, s32[ref]) is None:
                    rep.truth(label, "summed over the rows", what, g, s32[ref], s64[ref], cond=s64.get("cond:" + ref))
                    continue
                axis = s32[ref].ndim - 2
                cond = s64.get("cond:" + ref)
                for t, rr in list(rows.items()) + [("O(1)", rest)]:
                    rep.truth(label, f"score {t}", what, g, s32[ref], s64[ref], rows=rr, axis=axis,
                              cond=None if cond is None else np.take(cond, rr, axis=axis))
            rep.weights(label, "all", got["W"])
    rep.finish()


# ---- K16 -----------------------------------------------------------------------------------------------------------------------------
def ensemble_run(mode, X, W, idx, G, cuda):
    e = dc.ENSEMBLE_SHAPE
    mod = make_module(mode, e["S"], e["H"], e["d"], W, cuda)
    Xd = [[upload(x, False, cuda) for x in row] for row in X]
    outs, grads = ensemble_pass(mod, Xd, torch.from_numpy(idx).to(cuda), [torch.from_numpy(g).to(cuda) for g in G])
    return {"out": torch.stack([o.detach() for o in outs]).cpu().numpy(), "dW": torch.stack([g.reshape(-1) for g in grads]).cpu().numpy()}


@pytest.mark.parametrize("mode", dc.ec.MODES)
def test_ensemble_combine_with_one_poisoned_matrix_element_or_weight(cuda, mode):
    X, W, idx, G = dc.ensemble_problem(mode)
    clean_got = ensemble_run(mode, X, W, idx, G, cuda)
    clean32 = dc.ensemble_statement(mode, X, W, idx, G, torch.float32)
    bad, worst = [], {}
    for inj in dc.ensemble_injections(mode):
        Xp, Wp = dc.ensemble_poisoned(mode, X, W, inj)
        got = ensemble_run(mode, Xp, Wp, idx, G, cuda)
        s32 = dc.ensemble_statement(mode, Xp, Wp, idx, G, torch.float32)
        s64 = dc.ensemble_statement(mode, Xp, Wp, idx, G, torch.float64)
        for what in ("out", "dW"):
            bad += [(inj,) + b for b in dc.apply_rule(what, clean32[what], s32[what], s64[what], clean_got[what], got[what], worst.setdefault(what, {}))]
    print(f"\n[ensemble {mode}] {len(dc.ensemble_injections(mode))} injections; worst err / bound on touched finite entries: "
          f"{ {k: round(v.get('ratio', 0.0), 3) for k, v in worst.items()} }")
    show(bad)
    assert not bad, (len(bad), bad[:8])
