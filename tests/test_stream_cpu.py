"""The case table of the stream-order tests (tests/stream_common.py), checked without a GPU: it holds exactly the header functions
that take a stream, every decoy is a legal input that differs from the real one (a violation must give a wrong value, never a
fault), the numpy oracles there are tell decoy from real, and every case tagged "syncs" quotes the sentence that documents it."""
import importlib
import os
import re

import numpy as np
import pytest

import stream_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_the_parser_reads_a_declaration_that_spans_lines():
    text = """/* int fake(void *stream); */
    int sgl_a(const float *d_x, int64_t n,
              void *stream);
    int sgl_b(void *stream, int n);
    void *sgl_c(void);
    int sgl_d(sgl_graph_t *graph, void *stream);"""
    assert sc.stream_functions(text) == ["sgl_a", "sgl_d"]


def test_the_table_holds_exactly_the_functions_that_take_a_stream():
    """the project's "case list proven complete" idiom: dropping a row, or adding an entry point without one, fails here"""
    declared = sc.stream_functions(header("sgl_hip.h")) + sc.stream_functions(header("sgl_probe.h"))
    assert len(declared) == len(set(declared)) == 72 + 5
    assert not set(sc.EXCLUDED) & set(sc.CASES)
    assert set(sc.EXCLUDED) <= set(declared)
    assert sorted(sc.CASES) == sorted(set(declared) - set(sc.EXCLUDED))
    assert all(len(reason) > 20 for reason in sc.EXCLUDED.values())
    # every case of the main header calls a symbol the binding declares with a trailing stream pointer
    from sgl_amd import _lib
    for name in sc.CASES:
        protos = _lib.PROTOTYPES if name in _lib.PROTOTYPES else _lib.PROBE_PROTOTYPES
        assert protos[name][1][-1] is _lib.c_void_p, name


def test_dropping_a_function_from_the_table_is_noticed():
    declared = set(sc.stream_functions(header("sgl_hip.h")) + sc.stream_functions(header("sgl_probe.h"))) - set(sc.EXCLUDED)
    for gone in ("sgl_csr_select_fill", "sgl_synth_fill", "sgl_hop_reduce_f32"):
        assert sorted(set(sc.CASES) - {gone}) != sorted(declared)


def test_shapes_reach_the_launches_the_cases_are_about():
    g = sc.graph()
    from sgl_amd.device import default_long_row_nnz
    assert np.diff(g.rowptr).max() > default_long_row_nnz(g.nnz)               # a split row: the SpMM fix-up kernel launches
    assert sc.N % 64 and sc.N > 256 and sc.missing_diagonal(g) > 0 and sc.missing_diagonal(sc.graph(7, 1)) == 0
    assert (sc.diag_positions(sc.graph(7, 1)) >= 0).all()
    r, c, _ = sc.coo_list()
    assert len(np.unique(r * sc.N + c)) < len(r)                                # duplicate pairs
    a = np.stack((np.repeat(np.arange(g.n), np.diff(g.rowptr)), g.col), 1)
    assert {tuple(p) for p in a} == {tuple(p[::-1]) for p in a}                 # symmetric: what the reorder rounds expect


@pytest.mark.parametrize("entry,d", sc.case_ids())
def test_every_decoy_is_a_legal_input_that_differs(entry, d):
    c = sc.CASES[entry]
    host = c.host(d)
    delayed = {k: v for k, v in host.items() if isinstance(v, sc.Delayed)}
    assert bool(delayed) != c.inputless, "a case delays at least one input, unless it has none"
    for name, dl in delayed.items():
        assert sc.legal(dl) is None, (name, sc.legal(dl))
        if dl.kind == "float":
            words = np.ascontiguousarray(dl.decoy).view(np.uint32)
            assert (words == sc.FILL32).all() and not np.array_equal(np.ascontiguousarray(dl.real).view(np.uint32), words)
    for name, v in host.items():
        if not isinstance(v, sc.Delayed):
            assert isinstance(v, np.ndarray), name


def test_the_legality_check_refuses_what_would_fault():
    g = sc.graph()
    good = sc.cc(g.rowptr, g.col, sc.N)
    assert sc.legal(good) is None
    assert "range" in sc.legal(good._replace(decoy=good.decoy + sc.N))
    assert "increasing" in sc.legal(good._replace(decoy=good.decoy[::-1].copy()))
    assert "range" in sc.legal(sc.ix(np.arange(5), 5)._replace(decoy=np.arange(1, 6)))
    assert "equals" in sc.legal(sc.ix(np.zeros(5, dtype=np.int64), 5))
    rp = sc.rp(g.rowptr)
    assert sc.legal(rp) is None and len(rp.decoy) == len(g.rowptr)
    assert "monotone" in sc.legal(rp._replace(decoy=rp.decoy - 1))
    assert "monotone" in sc.legal(rp._replace(decoy=np.where(np.arange(len(rp.decoy)) == 3, rp.decoy[-1], rp.decoy)))
    # the decoy row pointers have no long row, the real ones do: the plan sgl_csr_create builds says which it saw
    assert np.diff(rp.decoy).max() <= 32 < np.diff(rp.real).max()


ORACLES = [(e, d) for e, d in sc.case_ids() if sc.CASES[e].oracle is not None]


@pytest.mark.parametrize("entry,d", ORACLES)
def test_the_oracle_tells_the_decoy_from_the_real_input(entry, d):
    c = sc.CASES[entry]
    host = c.host(d)
    real = {k: (v.real if isinstance(v, sc.Delayed) else v) for k, v in host.items()}
    decoy = {k: (v.decoy if isinstance(v, sc.Delayed) else v) for k, v in host.items()}
    with np.errstate(all="ignore"):
        a, b = np.asarray(c.oracle(real)), np.asarray(c.oracle(decoy))
    assert a.shape == b.shape and not np.array_equal(a, b, equal_nan=True)
    # and one delayed input at a time: each of them changes the result on its own
    for name, v in host.items():
        if isinstance(v, sc.Delayed):
            with np.errstate(all="ignore"):
                one = np.asarray(c.oracle(dict(real, **{name: v.decoy})))
            assert not np.array_equal(a, one, equal_nan=True), name


def test_there_are_oracles_for_the_index_decoys():
    assert len({e for e, _ in ORACLES}) >= 12


def _wrapper_doc(dotted):
    mod, _, attr = dotted.rpartition(".")
    obj = importlib.import_module(mod)
    return getattr(obj, attr).__doc__ or ""


@pytest.mark.parametrize("entry", [e for e, c in sc.CASES.items() if c.klass == "syncs"])
def test_a_case_tagged_syncs_is_documented_as_synchronising(entry):
    where, quote = sc.CASES[entry].doc
    text = sc.normalised(header("sgl_hip.h")) if where == "header" else sc.normalised(_wrapper_doc(where))
    assert re.search(r"synchron", quote, re.I), quote
    assert sc.normalised(quote).strip() in text, (entry, quote)
    # the two kinds of wait are told apart in words: "the DEVICE" (temporaries freed with hipFree) against the call's own stream
    assert bool(re.search(r"synchronises? the DEVICE", quote)) == (sc.CASES[entry].waits == "device"), quote
    if sc.CASES[entry].waits == "device":          # ... and the header's list of them names the entry point
        listed = text[text.index("hipFree waits for every stream"):text.index("none on the hop loop")]
        assert entry in listed, entry


def test_the_header_lists_exactly_the_calls_that_synchronise_the_device():
    text = sc.normalised(header("sgl_hip.h"))
    listed = set(re.findall(r"sgl_\w+", text[text.index("hipFree waits for every stream"):text.index("none on the hop loop")]))
    assert listed == {e for e, c in sc.CASES.items() if c.waits == "device"} | {"sgl_reorder_lpa_round"}
    assert all(c.waits is None for c in sc.CASES.values() if c.klass == "async")


def test_a_case_that_bypasses_the_wrappers_says_why():
    bare = {e for e, c in sc.CASES.items() if c.via == "device._call"}
    assert bare == set(sc.CALL_REASONS) and all(len(r) > 30 for r in sc.CALL_REASONS.values())


def test_the_issue_s_synchronising_entry_points_are_tagged_syncs():
    for entry in ("sgl_csr_create", "sgl_csr_set_rowmap", "sgl_norm_prepare", "sgl_csr_select_rowptr", "sgl_csr_merge_rowptr",
                  "sgl_coo_to_csr"):
        assert sc.CASES[entry].klass == "syncs"
    # sgl_chain_graph_create takes no stream (it synchronises the device, as documented): its launch is the case, the creation
    # runs in that case's setup
    assert "sgl_chain_graph_create" not in sc.stream_functions(header("sgl_hip.h")) and sc.CASES["sgl_chain_graph_launch"].klass == "async"
    assert {c.klass for c in sc.CASES.values()} == {"async", "syncs"}
