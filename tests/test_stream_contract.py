"""Every device handle held to its stream contract on a side stream (include/ccd.h; DESIGN.md section 4.9, "The stream contract").

The header promises, for nearly every entry point with a `void* stream`, that the call only enqueues on that stream, reads its
device inputs in stream order, that what is enqueued on the stream afterwards sees its results, and that the handle's destroy
drains the streams it was given.  The other GPU tests run on stream 0 and synchronise between the step that makes an input and
the call that reads it, so a launch or a table upload on another stream, a missing join with a side stream, a staging block
reused too early or a destroy that does not drain would pass them all.

Here every entry point runs on a side stream behind a bounded delay (tests/stream_contract.py): the tensors its handle was added
with hold POISON - another valid input - until a copy on the side stream, behind the delay, brings the real input.

  P1  inputs in stream order: after the handle's wait on the side stream the results are the expected ones, not the poison's.
  P2  only enqueues: the delay still runs when the call returns (entry points the header calls asynchronous).
  P3  results in stream order: a copy enqueued on the side stream after the call and before any wait, from a result address the
      caller may hold early, holds the expected result - the handle had run on the poison before, so stale memory is the poison's.
  P4  destroy drains: close() without a wait returns only after the delay has ended.

and a wait on a stream other than the run's gives the same results.  A case is conclusive only if the delay still runs where the
property says so; an inconclusive attempt is repeated with the delay doubled, at most twice, and a mismatch never is.  Expected
results: the same job on the default stream with torch.cuda.synchronize() on both sides, bit for bit.

Measured on the MI355X: see DESIGN.md section 4.9."""
import os

import numpy as np
import pytest

import stream_contract as sc
from conftest import ROOT

LMBDA = 1e-3


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_every_stream_entry_point_has_a_case_or_an_exemption():
    """Every function of include/ccd.h with a `void* stream` is in the case table's coverage map or in the short list of
    exemptions with a reason, and in one of them only: a new entry point fails here until it has a case."""
    with open(os.path.join(ROOT, "include", "ccd.h")) as f:
        names = sc.stream_entry_points(f.read())
    assert len(names) == len(set(names)) >= 30 and "ccd_rdoq_step_rounds" in names and "ccd_inter_reconstruct" in names, names
    assert "ccd_batch_create" not in names and "ccd_rdoq_set_maps" not in names
    missing = [n for n in names if n not in sc.COVERAGE and n not in sc.EXEMPT]
    assert not missing, f"no stream-contract case and no exemption: {missing}"
    assert not set(sc.COVERAGE) & set(sc.EXEMPT)
    stale = [n for n in list(sc.COVERAGE) + list(sc.EXEMPT) if n not in names]
    assert not stale, f"not an entry point with a stream: {stale}"
    assert all(cases for cases in sc.COVERAGE.values()) and all(len(r) > 10 for r in sc.EXEMPT.values())
    # the exemptions are the ones the decoder's own tests cover, the synchronous copies and the one-shot decode
    assert sorted(sc.EXEMPT) == sorted(["ccd_batch_prepare", "ccd_batch_run", "ccd_batch_run_stage", "ccd_batch_wait", "ccd_batch_copy_latent",
                                        "ccd_batch_copy_plane", "ccd_batch_copy_output", "ccd_batch_copy_dense", "ccd_decode_coolchic"])


def test_the_header_parser_reads_declarations_not_comments():
    text = """/* int ccd_in_a_comment(void* stream); */
    int ccd_one(ccd_x* x, void* stream);
    int ccd_two(int device, void* stream, const float* a,
                float* b);
    int ccd_three(const ccd_x* x, void** dev_ptr);
    int64_t ccd_four(ccd_x* x, void *stream);
    void ccd_five(void* streams);"""
    assert sc.stream_entry_points(text) == ["ccd_one", "ccd_two", "ccd_four"]


def test_the_case_tables_name_cases():
    names = set(sc.CASE_NAMES)
    for table in (sc.NO_HANDLE, sc.MAY_SYNCHRONISE, sc.EARLY, sc.FOREIGN_WAIT):
        assert set(table) <= names, set(table) - names
    assert not set(sc.FOREIGN_WAIT) & set(sc.NO_HANDLE)
    # one foreign-wait case for every handle whose wait takes a stream
    assert {n.split("_")[0] for n in sc.FOREIGN_WAIT} == {n.split("_")[0] for n in names - set(sc.NO_HANDLE)}


def test_the_delay_rule():
    """20 times the call's host time, never less than 20 ms, never more than 500 ms."""
    assert sc.first_delay(0.05) == 20.0 and sc.first_delay(1.0) == 20.0 and sc.first_delay(3.0) == 60.0 and sc.first_delay(40.0) == 500.0
    assert sc.ATTEMPTS == 3


def test_canonical_forms_compare_bits():
    nan = float("nan")
    assert sc.canon((1, nan, [np.float32(0.0)])) == sc.canon((1, nan, [np.float32(0.0)]))
    assert sc.canon(0.0) != sc.canon(-0.0)
    assert sc.canon(np.zeros(2, np.int8)) != sc.canon(np.zeros(2, np.uint8))
    assert sc.canon(np.zeros((2, 1), np.int8)) != sc.canon(np.zeros((1, 2), np.int8))


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gate():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cool_chic_amd import _lib

    _lib.lib()
    g = sc.Gate()
    yield g
    if g.host_ms:
        print(f"stream contract: {len(g.host_ms)} gated calls, host time of a call {min(g.host_ms):.3f} .. {max(g.host_ms):.3f} ms, "
              f"delays {min(g.delay_ms):.1f} .. {max(g.delay_ms):.1f} ms, {g.cycles_per_ms:.0f} spin cycles per ms")


def _case(name, oracle):
    case = sc.case(name, oracle)
    assert case.has_handle == (name not in sc.NO_HANDLE) and case.enqueues == (name not in sc.MAY_SYNCHRONISE)
    assert case.foreign_wait or name not in sc.FOREIGN_WAIT
    return case, sc.reference(case)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_inputs_and_results_in_stream_order(gate, oracle, name):
    """P1, P2 and, where the caller may hold a result's address before the wait, P3."""
    case, ref = _case(name, oracle)
    snapshot = name in sc.EARLY
    h = case.open()
    try:
        warm_ms = sc.warm_up(case, h)

        def check(o):
            assert not case.same(o.got, ref.poison), "P1: the entry point read its inputs before the copy that the stream put in front of it"
            assert case.same(o.got, ref.want), "P1: the results are neither the expected ones nor the poison's"
            if snapshot:
                assert case.same_early(o.snaps, ref.want_early), "P3: work enqueued on the stream behind the call did not see its results"

        def conclusive(o):  # P2 is this: the delay still runs when the call has returned (and the snapshots are enqueued)
            return not case.enqueues or not (o.after_snapshot if snapshot else o.after_call)

        sc.conclusive_call(case, gate, lambda: h, warm_ms, "P1 P2 P3" if snapshot else "P1 P2", conclusive, check, snapshot=snapshot)
    finally:
        case.close(h)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sc.FOREIGN_WAIT)
def test_a_wait_on_another_stream_gives_the_same_results(gate, oracle, name):
    """The run on the gated side stream, the handle's wait on a second, idle stream: the results are behind the run on the
    stream the run was given, whichever stream the wait names (include/ccd.h says so at ccd_rdoq_wait)."""
    case, ref = _case(name, oracle)
    h = case.open()
    try:
        warm_ms = sc.warm_up(case, h)

        def check(o):
            assert not case.same(o.got, ref.poison), "the wait returned the results of the run before: it did not wait for the run's stream"
            assert case.same(o.got, ref.want), "the results are neither the expected ones nor the poison's"

        sc.conclusive_call(case, gate, lambda: h, warm_ms, "wait on another stream", lambda o: not o.after_call, check, wait_on=gate.other)
    finally:
        case.close(h)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in sc.CASE_NAMES if n not in sc.NO_HANDLE])
def test_destroy_drains_the_stream(gate, oracle, name):
    """P4: a gated call, then close() with no wait - it returns only when the delay, and so the run behind it, has ended."""
    case, _ = _case(name, oracle)
    h = case.open()
    warm_ms = sc.warm_up(case, h)
    ready = [h]

    def make_handle():
        if not ready:
            ready.append(case.open())
            sc.warm_up(case, ready[0])
        return ready.pop()

    def check(o):
        assert o.after_close, "P4: the destroy returned while the run it was given still waited behind the delay"

    try:
        sc.conclusive_call(case, gate, make_handle, warm_ms, "P4", lambda o: not o.before_close, check, destroy=True)
    finally:
        for left in ready:
            case.close(left)


@pytest.mark.gpu
def test_the_harness_reports_a_launch_on_another_stream(gate, oracle):
    """Sensitivity: compute_rate is handed a second, idle stream in place of the gated one - what a launch on the wrong stream
    would be.  It completes while the delay still runs, and the harness must report the poison's result.  The inputs are valid
    either way."""
    case, ref = _case("rate", oracle)
    warm_ms = sc.warm_up(case, None)

    def check(o):
        assert case.same(o.got, ref.poison) and not case.same(o.got, ref.want), "a launch outside the gated stream went unnoticed"

    o = sc.conclusive_call(case, gate, lambda: None, warm_ms, "sensitivity", lambda o: not o.after_call, check, call_on=gate.other)
    assert not o.after_call


# ---- end to end: the evaluators under torch.cuda.stream(side) ------------------------------------------------------------------------
def _under(gate, latents, make, go):
    """(expected, poison's, gated) canonical results of go(make(tensors), tensors, between): the first two on the default stream
    with torch.cuda.synchronize() on both sides, the third under torch.cuda.stream(side) behind a delay, with the real latents
    copied over the poison on the side stream.  `latents`: [(real, poison)] device tensors; every run gets fresh copies, which it
    may move in place.  The evaluator is made before the delay: its sources are uploaded on the stream current in add()."""
    import torch

    out = []
    for which in (0, 1):
        dev = [pair[which].clone() for pair in latents]
        with make(dev) as ev:
            torch.cuda.synchronize()
            out.append(go(ev, dev, lambda: None))
            torch.cuda.synchronize()
    dev = [poison.clone() for _, poison in latents]

    def on_side():
        assert torch.cuda.current_stream(0) == gate.side, "a wrapper left another stream current"

    with make(dev) as ev:
        torch.cuda.synchronize()
        gate.arm(sc.MIN_DELAY_MS)
        with torch.cuda.stream(gate.side):
            for t, (real, _) in zip(dev, latents):
                t.copy_(real, non_blocking=True)
            out.append(go(ev, dev, on_side))
            on_side()
        gate.side.synchronize()
        torch.cuda.synchronize()
    return out


@pytest.mark.gpu
def test_rd_evaluator_on_a_side_stream(gate, oracle):
    """RdEvaluator.evaluate with every meter on, then a descent of two steps of eight rounds, on rgb192 under
    torch.cuda.stream(side): Candidate tuples, every StepReport, step_moves and the final latents are those of a second evaluator
    on the default stream from the same starting latents.  evaluate() synchronises, so the case is conclusive as it is."""
    import torch

    from cool_chic_amd import RdEvaluator

    sc.case("enc_run", oracle)
    rgb = sc._CASES["rgb192"]
    pic, geo = rgb.pic, rgb.geo

    def make(dev):
        ev = RdEvaluator(0)
        ev.add(geo.arch, geo.nn, pic.ptrs(dev[0]), pic.source, owner=dev[0])
        return ev

    def go(ev, dev, between):
        between()
        cands = ev.evaluate(LMBDA, ms_ssim=True, rate_deltas=True, distortion_deltas=True)
        between()
        reports = ev.descend(LMBDA, max_steps=2, grids=(0, 1, 2), rounds=8)
        between()
        moves = [torch.as_tensor(ev.step_moves(0, g), device="cuda").clone() for g in range(geo.n)]
        assert reports and reports[0][0].step.n_moves >= 2
        return sc.canon((cands, reports, moves, dev[0].clone()))

    want, poison, got = _under(gate, [(rgb.real, rgb.poison)], make, go)
    assert want != poison
    assert got != poison, "the evaluator read its latents before the copy that the stream put in front of it"
    assert got == want


@pytest.mark.gpu
def test_inter_rd_evaluator_on_a_side_stream(gate, oracle):
    """InterRdEvaluator: one evaluate and one joint step of eight rounds on vid3_ldp frame 1 under torch.cuda.stream(side)."""
    import torch

    import inter_cases as ic
    from cool_chic_amd import InterRdEvaluator
    from test_inter_deltas import _frame_data

    case = ic.case("vid3_ldp", 1)
    latents = [(case.cc[r].lat_dev, sc._dev(case.cc[r].flat(case.cc[r].lat2))) for r in ic.ROLES]

    def make(dev):
        ev = InterRdEvaluator(0)
        ev.add(case.frame_type, *[(case.cc[r].arch, case.cc[r].nn, case.cc[r].ptrs(t)) for r, t in zip(ic.ROLES, dev)], case.refs,
               case.gflow, case.taps, _frame_data(case.src, case.bd, case.fdt), owner=dev)
        return ev

    def go(ev, dev, between):
        between()
        cands = ev.evaluate(LMBDA)
        between()
        reports = ev.descend(LMBDA, max_steps=1, grids=(0, 1, 2), rounds=8, joint=True)
        between()
        moves = [torch.as_tensor(ev.step_moves(0, r, g), device="cuda").clone() for r in ic.ROLES for g in range(case.cc[r].n)]
        assert sum(s.n_moves for s in reports[0][0].steps) >= 2
        return sc.canon((cands, reports, moves, [t.clone() for t in dev]))

    want, poison, got = _under(gate, latents, make, go)
    assert want != poison
    assert got != poison, "the evaluator read its latents before the copy that the stream put in front of it"
    assert got == want
