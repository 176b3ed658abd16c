"""Every entry point runs on the caller's stream, behind a delayed producer -- on a real MI355X: run with `-m gpu`.

tests/stream_common.py states the technique and holds the case table.  Here: (a) a negative control on torch operations alone, which
shows that the harness sees an operation queued on the wrong stream; (b) the table, one test per entry point and width; (c) the
wrapper-level flows (propagation, aggregators, transforms, edge split, k-means, the three losses) with their feature matrix delayed;
(d) the two cross-stream loops of the project -- ShardedPropagator's alternating row pieces and the pooled host download of
GraphOp.propagate -- with a delay INSIDE them, so that a missing wait between the streams shows as NaN or as a stale hop.

Nothing here synchronises the device while a delay is in force or reads a result through the default stream: outputs travel to
pinned host memory on the side stream, which alone is synchronised.  The delay D is a cap on host time, not a tolerance: at least
4 x the longest plain call of an "async" case, measured in the same session (and at least stream_common.DELAY_FLOOR_MS).  D, the
calibration and every case's host time are printed, and written as JSON to the file the environment variable SGL_STREAM_ORDER_JSON
names (profiles/stream_order.json is such a record)."""
import contextlib
import json
import os
import time

import numpy as np
import pytest
import torch

import stream_common as sc
from sgl_amd import _lib
from sgl_amd import device as dev

pytestmark = pytest.mark.gpu

IDS = [f"{e}-{'d%d' % d if d else 'graph'}" for e, d in sc.case_ids()]


@pytest.fixture(scope="module")
def cuda():
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


# What a case that was set up wrongly raises: a refused argument (the library's code >= 1001, the wrappers' checks, a case's own
# assertion).  Anything else -- and a HIP error under whatever type -- ends the module: on a device that has faulted nothing more is
# started (the module fixture fails once, and every test that needs it reports that failure without running).
REFUSALS = (_lib.SglHipError, ValueError, TypeError, IndexError, AssertionError)


def gpu_fault(err):
    text = str(err)
    if isinstance(err, _lib.SglHipError):
        code = text.split("(code ", 1)[1].split(")", 1)[0] if "(code " in text else ""
        return not (code.isdigit() and int(code) >= 1001)        # below 1001: a hipError_t the runtime returned
    return any(w in text for w in ("HIP error", "hipError", "illegal memory access", "device-side assert"))


class Session:
    def __init__(self):
        self.cases, self.observed, self.flows, self.flow_cases = {}, {}, {}, {}
        self.delay_ms = self.t_plain_max_ms = None

    def report(self):
        return {"delay_ms": self.delay_ms, "largest_async_t_plain_ms": self.t_plain_max_ms, "t_plain_factor": sc.T_PLAIN_FACTOR,
                "delay_floor_ms": sc.DELAY_FLOOR_MS, "calibration": dict(sc._CAL),
                "cases": {f"{e}-{d}": dict(klass=sc.CASES[e].klass, via=sc.CASES[e].via, t_plain_ms=self.cases[(e, d)].get("t_plain_ms"), **obs)
                          for (e, d), obs in self.observed.items()},
                "flows": self.flows}


@pytest.fixture(scope="module")
def session(cuda):
    """The plain runs of every case (after a warm-up run: module loading and allocator growth are out of the way), the plain runs
    on the decoys, and the delay that follows from the plain calls' host times."""
    s = Session()
    sc.calibrate(cuda)
    for e, d in sc.case_ids():
        c = sc.CASES[e]
        try:
            sc.plain_run(c, d, cuda)
            want, t_plain, poisoned = sc.plain_run(c, d, cuda, before=True)
            decoy = None if c.inputless else sc.plain_run(c, d, cuda, "decoy")[0]
            s.cases[(e, d)] = {"want": want, "t_plain_ms": t_plain * 1e3, "decoy": decoy, "poisoned": poisoned}
        except pytest.skip.Exception as why:
            s.cases[(e, d)] = {"skip": str(why)}
        except REFUSALS as err:                       # a refused argument: reported by the case's own test, the others go on
            if gpu_fault(err):
                raise
            s.cases[(e, d)] = {"error": err}
    for name, c in sc.FLOWS.items():
        try:
            sc.plain_run(c, sc.FLOW_WIDTH, cuda)
            want, t_plain = sc.plain_run(c, sc.FLOW_WIDTH, cuda)
            decoy = sc.plain_run(c, sc.FLOW_WIDTH, cuda, "decoy")[0]        # every decoy is a legal input: no flow may refuse it
            s.flow_cases[name] = {"want": want, "t_plain_ms": t_plain * 1e3, "decoy": decoy}
        except REFUSALS as err:
            if gpu_fault(err):
                raise
            s.flow_cases[name] = {"error": err}
    times = [r["t_plain_ms"] for (e, _), r in s.cases.items() if "t_plain_ms" in r and sc.CASES[e].klass == "async"]
    s.t_plain_max_ms = max(times)
    s.delay_ms = max(sc.T_PLAIN_FACTOR * s.t_plain_max_ms, sc.DELAY_FLOOR_MS)
    print(f"\nstream order: D = {s.delay_ms:.2f} ms, largest async t_plain = {s.t_plain_max_ms:.3f} ms, "
          f"{sc._CAL['cycles_per_ms']:.0f} sleep cycles per ms")
    yield s
    path = os.environ.get("SGL_STREAM_ORDER_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(s.report(), f, indent=1, sort_keys=True)
            f.write("\n")


# ---- (a) the negative control ----------------------------------------------------------------------------------------------------------
def test_an_operation_queued_on_the_default_stream_reads_the_decoy(cuda, session):
    """torch operations only: with S delayed and x holding the decoy, x * 2 on the DEFAULT stream yields the decoy's result -- the
    harness detects a mis-queued operation, and S does not block the null stream"""
    real = torch.arange(1, 4097, dtype=torch.float32, device=cuda)
    x = torch.empty_like(real)
    x.view(torch.int32).fill_(sc.FILL32)
    host = torch.zeros(4096, dtype=torch.float32, pin_memory=True)
    torch.cuda.synchronize()
    side, filled, done = sc.independent_stream(cuda), torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(side):
        sc.delay(side, session.delay_ms)
        x.copy_(real, non_blocking=True)
        filled.record(side)
    y = x * 2                                            # the mis-queued operation: on the default stream
    host.copy_(y, non_blocking=True)
    done.record()
    done.synchronize()                                   # the default stream's own event: nothing waits for S
    assert not filled.query(), "the default stream's work finished while S was still delayed"
    assert torch.isnan(host).all()                       # the decoy's result, not 2 x real
    side.synchronize()
    assert torch.equal(x.cpu(), real.cpu())


def test_the_delay_lasts_about_as_long_as_asked(cuda, session):
    side = sc.independent_stream(cuda)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        a.record(side)
        sc.delay(side, session.delay_ms)
        b.record(side)
    queued_ms = (time.perf_counter() - t0) * 1e3
    b.synchronize()
    ms = a.elapsed_time(b)
    print(f"delay({session.delay_ms:.2f} ms) took {ms:.2f} ms")
    assert 0.5 * session.delay_ms <= ms <= 3.0 * session.delay_ms and queued_ms < session.delay_ms


# ---- (b) the table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,d", sc.case_ids(), ids=IDS)
def test_entry_point_runs_on_the_callers_stream(cuda, session, entry, d):
    c, rec = sc.CASES[entry], session.cases[(entry, d)]
    if "skip" in rec:
        pytest.skip(rec["skip"])
    if "error" in rec:
        raise rec["error"]
    if c.inputless:
        assert rec["want"] != rec["poisoned"], "the call leaves the sentinel: the case is blind"
    else:
        assert rec["decoy"] != rec["want"], "the decoy gives the real result: the case is blind"
    obs = sc.run_behind_delay(c, d, cuda, session.delay_ms, rec["want"])
    session.observed[(entry, d)] = {k: obs[k] for k in ("host_ms", "pending_before", "pending_after", "equal")}
    print(f"{entry} d={d} [{c.klass}] host {obs['host_ms']:.3f} ms (plain {rec['t_plain_ms']:.3f} ms), D = {session.delay_ms:.2f} ms, "
          f"pending before / after the call: {obs['pending_before']} / {obs['pending_after']}")
    assert obs["pending_before"], "the delay had run out before the call was issued"
    if c.klass == "async":
        assert obs["pending_after"], "the call waited for the stream (or outlived the delay)"
        assert obs["host_ms"] < session.delay_ms / 2
    assert obs["equal"], obs["first_difference"]
    # the mirror image: the default stream is the busy one, so what the call queued there happens late, and a device-wide
    # synchronisation inside the call is seen
    late = sc.run_ahead_of_bystander(c, d, cuda, session.delay_ms, rec["want"])
    session.observed[(entry, d)].update(waits=c.waits, bystander_host_ms=late["host_ms"], bystander_pending_after=late["pending_after"],
                                        bystander_equal=late["equal"] and late["equal_later"])
    print(f"    default stream busy: host {late['host_ms']:.3f} ms, still busy after the call: {late['pending_after']}")
    if c.waits == "device":          # documented: temporaries go back with hipFree, which waits for every stream
        assert not late["pending_after"], "documented to synchronise the device, but it did not wait for the busy default stream"
    else:                            # async, or documented to wait for its OWN stream alone
        assert late["pending_after"], "the call waited for the default stream: it synchronised the device"
        assert late["host_ms"] < session.delay_ms / 2
    assert late["equal"] and late["equal_later"], late["first_difference"]


# ---- (c) wrapper-level flows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.FLOWS))
def test_wrapper_flow_is_bit_equal_behind_the_delay(cuda, session, name):
    """the feature matrix (the value array where there is none) arrives behind the delay on S; the flow's results, copied out on S,
    have the bits of its plain run"""
    c, rec = sc.FLOWS[name], session.flow_cases[name]
    if "error" in rec:
        raise rec["error"]
    assert rec["decoy"] != rec["want"], "the decoy gives the real result: the flow is blind"
    obs = sc.run_behind_delay(c, sc.FLOW_WIDTH, cuda, session.delay_ms, rec["want"])
    session.flows[name] = {"host_ms": obs["host_ms"], "t_plain_ms": rec["t_plain_ms"], "pending_before": obs["pending_before"], "equal": obs["equal"]}
    print(f"{name}: host {obs['host_ms']:.3f} ms (plain {rec['t_plain_ms']:.3f} ms), pending before the call: {obs['pending_before']}")
    assert obs["pending_before"], "the delay had run out before the flow was started"
    assert obs["equal"], obs["first_difference"]


# ---- (d) the two cross-stream loops, with the delay inside them ------------------------------------------------------------------------------
K_HOPS = 3


def slowed(fn, spin_ms, device):
    """f(x, out) that, on whichever stream is current, fills `out` with NaN, spins for about spin_ms and then calls the real f: while
    it spins, anything that was not made to wait for this stream finds NaN (or the previous hop) where the result is expected"""
    cycles = int(sc.calibrate(device) * spin_ms)

    def piece(x, out):
        out.fill_(float("nan"))
        torch.cuda._sleep(cycles)
        return fn(x, out)
    return piece


@pytest.fixture(scope="module")
def chain(cuda):
    """the graph of the table with values small enough for three hops, X, and the bits of the single-handle spmm_chain"""
    g = sc.graph()
    rp, col = torch.from_numpy(g.rowptr).to(cuda), torch.from_numpy(g.col).to(cuda)
    val = torch.from_numpy(g.val / np.float32(16)).to(cuda)
    x = torch.from_numpy(np.ascontiguousarray(sc.feats(100)[0])).to(cuda)
    whole = dev.DeviceCSR(rp, col, val, (sc.N, sc.N))
    assert whole.info()["n_long_rows"] >= 1
    hops = whole.spmm_chain(x, K_HOPS)
    want = sc.snapshot([h.cpu() for h in hops])
    torch.cuda.synchronize()
    return {"g": g, "rp": rp, "col": col, "val": val, "x": x, "want": want}


def on_stream(stream):
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


@pytest.mark.parametrize("caller", ["default", "side"])
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("piece_streams", [True, False])
@pytest.mark.parametrize("pieces", [2, 3, 4])
def test_sharded_propagator_joins_its_two_streams(cuda, session, chain, pieces, piece_streams, in_place, caller):
    """ShardedPropagator.propagate on one rank (nothing is exchanged): every row piece NaN-fills its output, spins for D / 8 and only
    then multiplies, on whichever of the two streams it was given.  All hops equal the single-handle spmm_chain bit for bit; a
    missing wait_stream in either direction shows as NaN or as a stale hop.  The auxiliary stream is one with a hardware queue of
    its own (two streams that share a queue are ordered by it, wait or no wait)."""
    from sgl_amd.dist import ShardedPropagator, all_piece_bounds, device_piece_spmms
    g, x = chain["g"], chain["x"]
    pb = all_piece_bounds(g.rowptr, 1, pieces)
    fns, handles = device_piece_spmms(chain["rp"], chain["col"], chain["val"], sc.N, pb[0], rowptr_host=g.rowptr)
    assert (np.diff(pb[0]) > 0).all()
    prop = ShardedPropagator([slowed(f, session.delay_ms / 8, cuda) for f in fns], pb, 0, 1, sc.N)
    prop.piece_streams = piece_streams
    side = sc.independent_stream(cuda) if caller == "side" else None
    prop._aux = sc.independent_stream(cuda, others=[sc.independent_stream(cuda)], key="aux")
    x_buffers = [torch.full_like(x, float("nan")) for _ in range(2)]
    y_buffers = [torch.full_like(x, float("nan")) for _ in range(K_HOPS)]
    torch.cuda.synchronize()
    with on_stream(side):
        hops = prop.propagate(x, K_HOPS, x_buffers=x_buffers, y_buffers=y_buffers, in_place=in_place)
        host = sc.to_host(hops[1:], pinned=True)
        torch.cuda.current_stream(cuda).synchronize()
    got = sc.snapshot(host)
    assert len(hops) == K_HOPS + 1 and got == chain["want"], sc.first_difference(got, chain["want"])
    torch.cuda.synchronize()
    del handles


@pytest.mark.parametrize("caller", ["default", "side"])
def test_pooled_host_download_waits_for_its_hop(cuda, session, caller):
    """GraphOp.propagate(host_output=True) with destinations from the pinned pool: hop h travels on the download stream while hop
    h + 1 is computed.  Every SpMM NaN-fills its output and spins before it multiplies, so a download that is not ordered behind its
    hop copies NaN; every returned host hop equals the plain propagation bit for bit."""
    from sgl_amd.operators.graph_op import LaplacianGraphOp
    adj, x = sc.scipy_graph(), np.ascontiguousarray(sc.feats(100)[0])
    op = LaplacianGraphOp(K_HOPS, r=0.5, host_output=True)
    plain = op.propagate(adj, x)
    want = sc.snapshot(plain)
    assert len(plain) == K_HOPS + 1 and all(h.is_pinned() for h in plain[1:]), "the pooled path did not run"
    real = op._adj.spmm
    calls = []

    def slow_spmm(x_, out=None, accumulate=False):
        calls.append(1)
        out.fill_(float("nan"))
        torch.cuda._sleep(int(sc.calibrate(cuda) * session.delay_ms / 8))
        return real(x_, out=out, accumulate=accumulate)
    op._adj.spmm = slow_spmm
    side = sc.independent_stream(cuda) if caller == "side" else None
    op._download_stream = sc.independent_stream(cuda, others=[sc.independent_stream(cuda)], key="aux")
    torch.cuda.synchronize()
    with on_stream(side):
        hops = op.propagate(adj, x)
        torch.cuda.current_stream(cuda).synchronize()
    got = sc.snapshot(hops)
    assert len(calls) == K_HOPS and all(h.is_pinned() for h in hops[1:])
    assert got == want, sc.first_difference(got, want)
    torch.cuda.synchronize()
