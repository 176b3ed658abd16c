"""CPU-side tests of K16 (include/sgl_ensemble.h, sgl_amd/csrc/sgl_ensemble.hip): the header against its binding table and the
library's exports, the argument contract and the limit refusals (no launch), the launch arithmetic of the weight gradient behind the
GPU tests' bounds, the aggregator modules' parameters, and the numpy restatement against the reference's recorded results."""
import ctypes
import os
from ctypes import c_int64, c_void_p

import numpy as np
import pytest
import torch

import ensemble_common as ec
import test_host_cpu as host
from conftest import GOLDEN, ROOT, has_gpu

from sgl_amd import _lib
from sgl_amd import device as dev
from sgl_amd.models import simple_models as sm

ENTRIES = ("sgl_ensemble_combine_f32", "sgl_ensemble_combine_bwd_f32")


def test_header_binding_and_exports_agree():
    names = host.header_functions("sgl_ensemble.h")
    assert names == sorted(_lib.ENSEMBLE_PROTOTYPES) == sorted(ENTRIES + ("sgl_ensemble_combine_bwd_scratch",))
    assert not set(names) & set(_lib.PROTOTYPES) and not set(names) & set(host.header_functions("sgl_hip.h"))
    decls = host.header_declarations("sgl_ensemble.h")
    assert sorted(decls) == names
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, params) in decls.items():
        assert hasattr(handle, name), f"{name} declared in include/sgl_ensemble.h but not exported by libsgl_hip.so"
        restype, argtypes = _lib.ENSEMBLE_PROTOTYPES[name]
        assert host.binding_matches(ret, restype, returned=True), (name, ret, restype)
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        for i, (c_type, ctype) in enumerate(zip(params, argtypes)):
            assert host.binding_matches(c_type, ctype), (name, i, c_type, ctype)
        bound = getattr(_lib.lib(), name)                       # bound on the handle lib() returns
        assert bound.restype is restype and list(bound.argtypes) == list(argtypes)
    text = open(os.path.join(ROOT, "include", "sgl_ensemble.h")).read()
    assert f"#define SGL_ENSEMBLE_MAX_GROUP {ec.MAX_GROUP} " in text and f"#define SGL_ENSEMBLE_MAX_MEMBERS {ec.MAX_MEMBERS} " in text
    assert (_lib.SGL_ENSEMBLE_MAX_GROUP, _lib.SGL_ENSEMBLE_MAX_MEMBERS) == (ec.MAX_GROUP, ec.MAX_MEMBERS)


class Args:
    """a legal call of both entry points on host memory (nothing is dereferenced: without a device no kernel runs)"""

    def __init__(self, n_groups=2, group_size=3, n_rows=10, n_idx=5, d=8, cs=1):
        self.n_groups, self.group_size, self.n_rows, self.n_idx, self.d, self.cs = n_groups, group_size, n_rows, n_idx, d, cs
        m = n_groups * group_size
        self.x = np.zeros((max(m, 1), n_rows, d), np.float32)
        self.out = np.zeros((max(n_groups, 1), n_idx, d), np.float32)
        self.w = np.zeros((max(m, 1), d), np.float32)
        self.idx = np.zeros(n_idx, np.int64)
        self.scratch = np.zeros(1 << 16, np.float32)

    def tables(self):
        m = self.n_groups * self.group_size
        px = (c_void_p * max(m, 1))(*[self.x[min(i, len(self.x) - 1)].ctypes.data for i in range(max(m, 1))])
        lx = (c_int64 * max(m, 1))(*[self.d] * max(m, 1))
        po = (c_void_p * max(self.n_groups, 1))(*[self.out[min(g, len(self.out) - 1)].ctypes.data for g in range(max(self.n_groups, 1))])
        lo = (c_int64 * max(self.n_groups, 1))(*[self.d] * max(self.n_groups, 1))
        return px, lx, po, lo

    def forward(self, divisor=1.0, pad=0):
        px, lx, po, lo = self.tables()
        return _lib.lib().sgl_ensemble_combine_f32(self.n_groups, self.group_size, px, lx, self.n_rows, self.idx.ctypes.data, self.n_idx,
                                                   self.w.ctypes.data, self.d, self.cs, divisor, po, lo, pad, self.d, None)

    def backward(self, divisor=1.0):
        px, lx, po, lo = self.tables()
        return _lib.lib().sgl_ensemble_combine_bwd_f32(self.n_groups, self.group_size, px, lx, self.n_rows, self.idx.ctypes.data, self.n_idx,
                                                       po, lo, self.cs, divisor, self.w.ctypes.data, self.d, self.scratch.ctypes.data, self.d, None)

    def both(self, **kw):
        """(name, return code) of each entry, one call at a time: the caller reads last_error() in between"""
        yield ENTRIES[0], self.forward(**kw)
        yield ENTRIES[1], self.backward(**{k: v for k, v in kw.items() if k == "divisor"})


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_entries_fail_by_name_without_a_gpu():
    for name, rc in Args().both():
        assert rc != 0 and name in _lib.last_error(), (name, rc, _lib.last_error())
    # the scratch query is host arithmetic: the same with or without a device
    assert _lib.lib().sgl_ensemble_combine_bwd_scratch(2, 3, 5, 8, 1) == ec.bwd_scratch(2, 3, 5, 8, 1)


def test_limits_and_bad_arguments_are_refused_by_name_before_any_launch():
    """the refusals come before the first launch: they read the same with or without a device"""
    for a, needle in ((Args(n_groups=1, group_size=ec.MAX_GROUP + 1), "group_size=65"),
                      (Args(n_groups=ec.MAX_MEMBERS // 4 + 1, group_size=4), "n_groups * group_size=260")):
        for name, rc in a.both():
            err = _lib.last_error()
            assert rc == _lib.SGL_ERR_UNSUPPORTED and err.startswith(name + ": ") and needle in err, (name, rc, err)
    wide = Args()
    wide.d = 2 ** 31 - 1
    for name, rc in wide.both():
        assert rc == _lib.SGL_ERR_UNSUPPORTED and _lib.last_error().startswith(name + ": ") and "SGL_MAX_WIDTH" in _lib.last_error()
    for a, kw in ((Args(n_groups=0), {}), (Args(group_size=0), {}), (Args(cs=2), {}), (Args(), {"divisor": 0.0}), (Args(), {"divisor": float("nan")})):
        for name, rc in a.both(**kw):
            assert rc == 1001 and _lib.last_error().startswith(name + ": "), (name, rc, _lib.last_error())
    a = Args()
    assert a.forward(pad=3) == 1001 and "pad_cols" in _lib.last_error()          # d + pad_cols beyond the output pitch
    # nothing to do needs no device: no rows taken, or no columns
    assert Args(n_idx=0).forward() == 0 and Args(d=0).forward() == 0 and Args(d=0).backward() == 0


def test_scratch_query_is_the_restated_launch_arithmetic():
    for n_idx in (1, 31, 32, 33, 63, 1031, 1500, 32768, 32769, 50000, 10 ** 6, 10 ** 7):
        for d in (1, 3, 4, 100, 147, 260):
            for cs in (0, 1):
                assert _lib.lib().sgl_ensemble_combine_bwd_scratch(3, 8, n_idx, d, cs) == ec.bwd_scratch(3, 8, n_idx, d, cs), (n_idx, d, cs)
        assert ec.bwd_blocks(n_idx) <= ec.BWD_MAX_BLOCKS and ec.bwd_per_block(n_idx) % ec.BWD_ROW_STEP == 0
        assert ec.bwd_blocks(n_idx) * ec.bwd_per_block(n_idx) >= n_idx > (ec.bwd_blocks(n_idx) - 1) * ec.bwd_per_block(n_idx)


def test_backward_bound_is_never_wider_than_the_issue_allows():
    """gamma counts the kernel's longest chain and stays inside (B + d (1 - cs) + 2) u for every shape the GPU tests use"""
    for B in (1, 2, 63, 1031, ec.N_ROWS):
        for d in ec.WIDTHS:
            for cs in (0, 1):
                for vec in (1, 4):
                    for divided in (False, True):
                        k = ec.bwd_roundings(B, d, cs, vec, divided)
                        assert 1 <= k and k + 1 <= B + d * (1 - cs) + 2, (B, d, cs, vec, divided, k)
                        assert ec.gamma(k) <= (B + d * (1 - cs) + 2) * ec.U
    assert ec.bwd_roundings(1, 100, 1, 4, True) == 2 and ec.bwd_roundings(1, 1, 0, 1, False) == 1
    assert ec.bwd_roundings(1031, 260, 1, 4, False) == 8 + 3 + 0 + 6        # 32 rows on 4 row lanes, LDS, 33 blocks one per lane, butterfly
    assert ec.bwd_roundings(2, 3, 0, 1, True) == 1 + 2 + 1 + 1              # a product, 3 column lanes, 2 row lanes, the division


def test_aggregator_parameters_are_the_references():
    S, H, d = 3, 4, 5
    torch.manual_seed(0)
    a = sm.OneDimConvolution(S, H, d)
    assert list(a.state_dict()) == [f"_OneDimConvolution__learnable_weight.{h}" for h in range(H)]
    assert all(tuple(p.shape) == (d, S) for p in a.parameters())
    b = sm.OneDimConvolutionWeightSharedAcrossFeatures(S, H)
    assert list(b.state_dict()) == [f"_OneDimConvolutionWeightSharedAcrossFeatures__learnable_weight.{h}" for h in range(H)]
    assert all(tuple(p.shape) == (1, S) for p in b.parameters())
    c = sm.FastOneDimConvolution(S, H)
    assert list(c.state_dict()) == ["_FastOneDimConvolution__learnable_weight"]
    w = c.state_dict()["_FastOneDimConvolution__learnable_weight"]
    assert tuple(w.shape) == (S * H, 1) and torch.equal(w, torch.ones(S * H, 1))
    assert torch.equal(c.subgraph_weight, torch.full((S,), float(H)))
    # xavier_uniform_ on [d, S] / [1, S]: inside its bound, not constant
    for mod, fan in ((a, d + S), (b, 1 + S)):
        for p in mod.parameters():
            assert p.abs().max() <= (6.0 / fan) ** 0.5 and p.std() > 0
    # the member-major tables the kernel reads: row h * S + s
    ta, tb = a.weight_table(), b.weight_table()
    assert tuple(ta.shape) == (H * S, d) and tuple(tb.shape) == (H * S,)
    pa, pb = list(a.parameters()), list(b.parameters())
    for h in range(H):
        for s in range(S):
            assert torch.equal(ta[h * S + s], pa[h][:, s]) and tb[h * S + s] == pb[h][0, s]
    assert ta.requires_grad and tb.requires_grad


def test_wrapper_refuses_what_the_kernel_has_no_form_for():
    x = torch.zeros(4, 3)
    with pytest.raises(TypeError, match="bfloat16"):
        dev.ensemble_combine([[x.to(torch.bfloat16)]], torch.ones(1))
    with pytest.raises(TypeError):                                   # host matrices: there is no CPU path
        dev.ensemble_combine([[x]], torch.ones(1))
    with pytest.raises(ValueError):
        dev.ensemble_combine([[x, x], [x]], torch.ones(3))
    with pytest.raises(ValueError):
        dev.ensemble_combine([], torch.ones(1))
    with pytest.raises(TypeError, match="3-d tensor"):
        sm.FastOneDimConvolution(2, 2)(torch.zeros(4, 3, 4))
    with pytest.raises(ValueError):
        sm.OneDimConvolution(2, 3, 3)([[x, x]])                      # one hop list where three are expected


@pytest.mark.parametrize("mode", ec.MODES)
def test_restatement_is_the_references_aggregator_and_the_reference_sits_inside_the_bounds(goldens, mode):
    """the float64 restatement equals the reference's module in .double() (G23) to float64 rounding; the reference's own float32
    outputs and weight gradients lie inside the bounds the GPU tests hold the kernel to -- the bounds hold for the reference alone"""
    g = goldens.npz("g23_hetero")
    X, W, idx, G, keys = ec.g23_aggregator(g, mode)
    H, S, d, B = len(X), len(X[0]), X[0][0].shape[1], len(idx)
    _, _, cs, _ = ec.kernel_shape(mode, S, H)
    T, bound = ec.forward_f64(mode, X, W, idx)
    truth, ref32 = g[f"agg|{mode}|out|f64"], g[f"agg|{mode}|out|f32"]
    assert truth.dtype == np.float64 and ref32.dtype == np.float32 and len(T) == len(truth)
    for t, b, t64, r32 in zip(T, bound, truth, ref32):
        assert np.allclose(t, t64, rtol=1e-13, atol=1e-15)
        assert np.all(np.abs(r32.astype(np.float64) - t) <= b)
    dT, mag = ec.backward_f64(mode, X, G, idx)
    dT, mag = (dT, mag) if isinstance(dT, list) else ([dT], [mag])
    cap = ec.gamma(B + d * (1 - cs) + 1)                              # the widest bound any reduction shape is allowed
    for k, t, m in zip(keys, dT, mag):
        t64, r32 = g[f"agg|{mode}|grad|f64|{k}"], g[f"agg|{mode}|grad|f32|{k}"]
        assert t.shape == t64.shape and np.allclose(t, t64, rtol=1e-12, atol=1e-14)
        assert np.all(np.abs(r32.astype(np.float64) - t) <= cap * m)


def test_state_dict_keys_equal_the_recorded_ones(goldens):
    g = goldens.npz("g23_hetero")
    X = g["agg|X"]
    H, S, d = X.shape[0], X.shape[1], X.shape[3]
    for mode, mod in (("per_feature", sm.OneDimConvolution(S, H, d)), ("shared", sm.OneDimConvolutionWeightSharedAcrossFeatures(S, H)),
                      ("fast", sm.FastOneDimConvolution(S, H))):
        keys = [str(k) for k in g[f"agg|{mode}|keys"]]
        assert list(mod.state_dict().keys()) == keys
        mod.load_state_dict({k: torch.from_numpy(g[f"agg|{mode}|param|{k}"]) for k in keys})          # a reference checkpoint loads
        assert mod.num_subgraphs == S
    from sgl_amd.models import hetero
    for name in ("NARS_SIGN", "Fast_NARS_SGC_WithLearnableWeights"):
        model = getattr(hetero, name)(*ec.G23_MODEL.values(), 3)
        keys = [str(k) for k in g[f"model|{name}|keys"]]
        assert list(model.state_dict().keys()) == keys
        model.load_state_dict({k: torch.from_numpy(g[f"model|{name}|param|{k}"]) for k in keys})
