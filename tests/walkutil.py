"""What the GPU tests of the CIGAR walks share (test_gpu_window_walk, test_gpu_walk_phases, test_gpu_line_pieces): the
device context, the bit-for-bit comparison with the oracle, and a batch called under every promise variant of tests/gen.py.
"""
import numpy as np

from inquistr_amd import batch as B
from tests import gen


def open_ctx():
    """The body of the modules' `ctx` fixtures: a context on device 0, closed when the module is done."""
    from inquistr_amd import hipcall

    c = hipcall.Context(0)
    assert c.backend.startswith("hip:gfx950")
    yield c
    c.close()


def _assert_same(got, want, what):
    assert gen.same_f64(got.phase1, want.phase1), f"phase1 differs {what}"
    assert gen.same_f64(got.phase2, want.phase2), f"phase2 differs {what}"
    bad = np.nonzero(got.pair_call != want.pair_call)[0]
    assert bad.size == 0, f"pair_call differs at {bad[:8]} {what}"
    bad = np.nonzero(got.pair_bits != want.pair_bits)[0]
    assert bad.size == 0, f"pair_bits differs at {bad[:8]} {what}"
    assert got.n_tie_loci == want.n_tie_loci, what


def _all_variants(ctx, orc, batch, what="", code=B.INQ_OK):
    """One oracle result (the oracle never reads the promise byte, tests/test_window_bytes.py), whose status must be `code`;
    the batch called under every promise variant of tests/gen.py: the oracle's status, and its results when that is INQ_OK.
    Returns the status code."""
    oc, want = orc.call_batch(batch, debug=True)
    assert oc == code, (what, oc)
    for name in gen.promise_variants(batch):
        rc, got = ctx.call_batch(batch, debug=True, check=False)
        assert rc == oc, (what, name, rc, oc)
        if rc == B.INQ_OK:
            _assert_same(got, want, f"{what} {name}")
    return oc
