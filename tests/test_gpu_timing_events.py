"""The event timing of a launch sequence (inq_ctx_timing_enable / _read): a sequence that is locus_call_small alone - a depth hint of at
most 64 reads, no side output - is timed by the two events around that kernel, and no third event is recorded behind it; every other
sequence keeps its third event.  Either way the launches are counted, the sequence is never shorter than its first kernel, and the
rows are the same."""
import numpy as np
import pytest

from tests import gen
from tests.test_gpu_evidence import _device_call as _evidence_call
from tests.test_gpu_launch_geometry import _device_call

pytestmark = pytest.mark.gpu

CALLS = 3


@pytest.fixture(scope="module")
def ctx():
    from inquistr_amd import hipcall

    c = hipcall.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch():
    """128 loci of 30 reads each: within a hint of 30."""
    from inquistr_amd import synth

    b = synth.generate_numpy(synth.WORKLOADS["unphased100k"], 0, 128)
    assert int(np.diff(b.locus_pair_off.astype(np.int64)).max()) <= 30
    return b


def _timed(ctx, hint, call):
    """CALLS calls with timing on under the hint: (ms of the sequences, ms of their first kernels, launches counted, last result)."""
    ctx.set_option("max_reads_hint", hint)
    ctx.timing_enable(True)
    try:
        ctx.timing_reset()
        for _ in range(CALLS):
            got = call()
        kernel_ms, n_kernel = ctx.timing_read(1)
        sequence_ms, n_sequence = ctx.timing_read(0)
        assert n_kernel == n_sequence
        # a second read gives the same answer: reading consumes nothing
        assert ctx.timing_read(0) == (sequence_ms, n_sequence) and ctx.timing_read(1) == (kernel_ms, n_kernel)
        return sequence_ms, kernel_ms, n_sequence, got
    finally:
        ctx.timing_enable(False)
        ctx.set_option("max_reads_hint", 0)


def test_one_kernel_sequence_is_timed_by_two_events(ctx, orc, batch):
    oc, want = orc.call_batch(batch, debug=True)
    assert oc == 0

    def plain():
        got, rc, _ = _device_call(ctx, batch)
        assert rc == 0
        return got

    def with_side_outputs():
        code, rc, got, _flags, _ev = _evidence_call(ctx, batch)
        assert code == 0 and rc == 0
        return got

    results = []
    # hint 30: the sequence is the one kernel
    seq, kern, n, got = _timed(ctx, 30, plain)
    assert n == CALLS and kern > 0.0 and seq == kern
    results.append(got)
    # no hint: two more launches behind the kernel, and the third event behind them
    seq, kern, n, got = _timed(ctx, 0, plain)
    assert n == CALLS and kern > 0.0 and seq >= kern
    results.append(got)
    # hint 30 with tie flags and evidence asked for: the counting kernel stands behind the first
    seq, kern, n, got = _timed(ctx, 30, with_side_outputs)
    assert n == CALLS and kern > 0.0 and seq >= kern
    results.append(got)
    # ... and the one-kernel form again behind it: the mark belongs to a sequence, not to the context
    seq, kern, n, got = _timed(ctx, 30, plain)
    assert n == CALLS and seq == kern
    results.append(got)
    for k, got in enumerate(results):
        assert gen.same_f64(got.phase1, want.phase1) and gen.same_f64(got.phase2, want.phase2), k
        assert np.array_equal(got.pair_call, want.pair_call) and np.array_equal(got.pair_bits, want.pair_bits), k
        assert got.n_tie_loci == want.n_tie_loci, k
