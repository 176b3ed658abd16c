"""The conditions test_gpu_degenerate_rows.py rests on, checked without a GPU (degenerate_common.py):

  * the non-finite masks of the float32 statement do not depend on the order of the columns, for every injection case of every
    family, and equal those of the float64 statement wherever no float32 overflow is involved;
  * the case list reaches every lane layout of every register-resident kernel family, and each general path;
  * the independent set of a case is never empty, and for a row-local output the touched entries lie in the injected row;
  * the regime rows land in their regime in float64."""
import numpy as np
import pytest
import torch

import degenerate_common as dc
from agg_rows_common import compiled_variants

_CLEAN = {}


def clean(fam, s):
    key = (fam.name, dc.sid(s))
    if key not in _CLEAN:
        _CLEAN[key] = dc.statement(fam, dc.host_hops(s.d, s.H, fam.bf16), dc.parameters(s.d, s.H), torch.float32)
    return _CLEAN[key]


@pytest.mark.parametrize("name", list(dc.FAMILIES))
def test_masks_are_order_independent_and_the_independent_set_is_what_the_rule_assumes(name):
    """Per case: the float32 statement of the poisoned input, the same with the columns reversed, and the float64 statement.

    NaN, +inf and -inf injections: the three agree on every mask.  +-3e38 (bfloat16: +-0x7F7F): the two float32 orders agree; the
    float64 statement cannot overflow where float32 does (a square of 3e38, a product with a weight above 1.13), so its non-finite
    entries are only required to be non-finite in float32 as well.  The kernels are held to the float32 masks."""
    fam = dc.FAMILIES[name]
    bad = []
    for k, s in enumerate(dc.family_shapes(fam)):
        hops, p = dc.host_hops(s.d, s.H, fam.bf16), dc.parameters(s.d, s.H)
        base = clean(fam, s)
        assert all(np.isfinite(a).all() for a in base.values()), (name, s)
        for inj in dc.injections(s, k, fam.bf16):
            bad_x = dc.poisoned(hops, inj)
            s32 = dc.statement(fam, bad_x, p, torch.float32)
            s64 = dc.statement(fam, bad_x, p, torch.float64)
            rx, rp = dc.reversed_columns(bad_x, p)
            rev = dc.unreverse(dc.statement(fam, rx, rp, torch.float32), s.d)
            any_independent = False
            for out, a in dc.outputs(s32).items():
                if [m.tolist() for m in dc.masks(a)] != [m.tolist() for m in dc.masks(rev[out])]:
                    bad.append((dc.sid(s), inj, out, "column order"))
                overflow = inj.name.startswith(("+3", "-3", "+7", "-7"))
                if not overflow and any(not np.array_equal(m32, m64) for m32, m64 in zip(dc.masks(a), dc.masks(s64[out]))):
                    bad.append((dc.sid(s), inj, out, "float64 masks"))
                if overflow and (~np.isfinite(s64[out]) & np.isfinite(a)).any():
                    bad.append((dc.sid(s), inj, out, "float64 not finite where float32 is"))
                ind = dc.independent(base[out], a)
                any_independent |= bool(ind.any())
                axis = dc.row_axis(fam, out, a)
                if axis is not None:                                     # row-local: every other row is independent
                    other = np.delete(ind, inj.row, axis=axis)
                    if not other.all():
                        bad.append((dc.sid(s), inj, out, "another row touched"))
            if not any_independent:
                bad.append((dc.sid(s), inj, "no independent entry"))
    assert not bad, (len(bad), bad[:10])


def test_every_combination_of_row_hop_column_and_value_is_injected():
    for name, fam in dc.FAMILIES.items():
        seen = set()
        for k, s in enumerate(dc.family_shapes(fam)):
            inj = dc.injections(s, k, fam.bf16)
            assert len({i.name for i in inj}) == 5 and {i.row for i in inj} == set(dc.ROWS) and len({i.hop for i in inj}) == 2
            assert {i.col for i in inj} == {0, s.d - 1, s.d // 2}
            seen |= {(i.row, i.hop == 0, (0, s.d - 1, s.d // 2).index(i.col), i.name) for i in inj}
        assert len(seen) == 90, (name, len(seen))


def test_the_case_list_reaches_every_layout_and_each_general_path():
    for name, fam in dc.FAMILIES.items():
        if fam.kernel is None:
            continue
        ks = [(s, dc.kernel_of(fam, s)) for s in dc.family_shapes(fam)]
        reached = {k[1][:2] for _, k in ks if k is not None}
        want = {v[:2] for v in compiled_variants(fam.kernel)}
        if fam.kernel == "rowdot2":
            assert (8, 5) in reached and (16, 3) in reached
        else:
            want -= {(8, 5)}
        assert reached == want, (name, sorted(want - reached))
        general = {s.tag for s, k in ks if k is None}
        if name == "scores2":                                            # the two-part scores have no general kernel
            assert not general
        elif fam.kernel == "prefix":                                     # any hop count; wider or unaligned rows are refused
            assert not general and any(s.H == 17 for s, _ in ks)
        else:
            assert general == {"wide", "hops17", "dense"}, (name, general)
    # more hops than lanes: the array form of the gate, the recursion and NAFS
    assert any(s.d == 29 and s.H == 13 for s in dc.shapes())
    for fam in ("gate", "recursive", "nafs"):
        assert dc.kernel_of(dc.FAMILIES[fam], dc.shapes()[2])[1] == (8, 1, 14)
    assert dc.kernel_of(dc.FAMILIES["nafs"], next(s for s in dc.shapes() if s.d == 147 and s.H == 13))[1][:2] == (32, 2)


def test_nafs_regimes_are_where_they_are_meant_to_be():
    for d, H in ((29, 5), (147, 13), (509, 5)):
        full = [r for r in range(dc.N) if r not in (1, 3)]
        cos = {s: dc.nafs_cosines(dc.nafs_regime(d, H, s)) for s in dc.NAFS_SCALES}
        assert np.all((cos[-33][full, 0] > 0.1) & (cos[-33][full, 0] < 0.9)), (d, cos[-33][full, 0].min(), cos[-33][full, 0].max())
        assert np.all(np.abs(cos[-50][:, 0]) < 1e-6) and np.all(cos[-50][full, 0] > 0)        # the norm is far below the epsilon
        for s in (0, 50):
            assert np.allclose(cos[s][full, 0], 1.0, atol=1e-6)
            assert np.allclose(cos[s][list(dc.DUPLICATE_ROWS)], 1.0, atol=1e-6)
            assert np.allclose(cos[s][list(dc.NEGATED_ROWS), 1:], -1.0, atol=1e-6)
            spread = cos[s][full][:, 1:]
            assert spread.max() - spread.min() > 0.5                                         # correlated hops: not all near 0
        x = dc.nafs_regime(d, H, -70)[0]
        assert np.all((x.astype(np.float32) ** 2)[full] < np.finfo(np.float32).tiny)         # the squares are denormal or zero
        assert np.isfinite(dc.nafs_regime(d, H, 50)[0].astype(np.float32) ** 2 * d).all()
        for s in dc.NAFS_SCALES:                                           # the float32 statement stays finite in all five
            out, W = dc.nafs_statement([torch.from_numpy(a) for a in dc.nafs_regime(d, H, s)])
            assert torch.isfinite(out).all() and torch.isfinite(W).all(), (d, H, s)


def test_gate_regimes_are_where_they_are_meant_to_be():
    for d, H in ((29, 13), (147, 5), (600, 5)):
        for make, scores in ((dc.gate_regime, dc.gate_scores), (dc.recursive_regime, dc.recursive_scores)):
            hops, p, rows = make(d, H)
            z = scores(hops, p)
            for t, rr in rows.items():
                assert np.all(np.abs(z[rr] - t) <= 0.1 * abs(t)), (make.__name__, d, H, t, z[rr])
            rest = [r for r in range(dc.N) if all(r not in rr for rr in rows.values())]
            assert np.abs(z[rest]).max() < 10.0                              # some rows stay O(1)


def test_ensemble_injections_are_inside_the_problem():
    for mode in dc.ec.MODES:
        X, W, idx, G = dc.ensemble_problem(mode)
        base = dc.ensemble_statement(mode, X, W, idx, G, torch.float32)
        assert all(np.isfinite(a).all() for a in base.values())
        for inj in dc.ensemble_injections(mode):
            Xp, Wp = dc.ensemble_poisoned(mode, X, W, inj)
            s32 = dc.ensemble_statement(mode, Xp, Wp, idx, G, torch.float32)
            s64 = dc.ensemble_statement(mode, Xp, Wp, idx, G, torch.float64)
            assert any(dc.independent(base[k], s32[k]).any() for k in s32)
            # the same sums with the rows taken and the columns in the opposite order: the masks do not depend on the order
            rev = dc.ensemble_statement(mode, [[x[:, ::-1].copy() for x in row] for row in Xp],
                                        [w[::-1].copy() for w in Wp] if mode == "per_feature" else Wp, idx[::-1].copy(),
                                        [g[::-1, ::-1].copy() for g in G], torch.float32)
            rev = {"out": rev["out"][:, ::-1, ::-1], "dW": rev["dW"].reshape(len(rev["dW"]), -1, dc.ENSEMBLE_SHAPE["S"])[:, ::-1].reshape(rev["dW"].shape)
                   if mode == "per_feature" else rev["dW"]}
            assert all(np.array_equal(a, b) for k in s32 for a, b in zip(dc.masks(s32[k]), dc.masks(rev[k]))), (mode, inj)
            if not inj[2].startswith(("+3", "-3")):
                assert all(np.array_equal(a, b) for k in s32 for a, b in zip(dc.masks(s32[k]), dc.masks(s64[k]))), (mode, inj)
