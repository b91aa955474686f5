"""locus_call_mid_walk and locus_call_tail at launch geometries other than the default one: "grid_medium" / "grid_tail" (and the
cache policy "nt_loads") are tuning knobs of the ABI, reachable through `inquistr call --ctx-option`, and "grid_tail" is clamped
to the device's CU count besides - 32 on a CPX partition.  The geometry decides how the work lists are dealt (csrc/kernels.hip
medium_part, walk_part: a locus of more than kWalkSplit reads is walked by gridDim / items workgroups), the slice of a locus of
more than kGridSelectMin reads a workgroup works on in every pass of csrc/deep_select.hip, the grid barrier's target and the exit
ticket that empties the lists.  None of it may change a row, a per-pair Call or bit, or a tie count: all exact against the oracle.

Against the ladder's six loci on list 2 the grids give (per_item = max(1, grid_medium / 6), groups = grid_medium / per_item):
    grid_medium      1      2      3      7     64    8192   65535
    per_item         1      1      1      1     10    1365   10922
    groups           1      2      3      7      6       6       6
    left over        0      0      0      0      4       2       3
"""
import numpy as np
import pytest

from tests import gen
from tests.test_gpu_parity import _assert_same, _other_variants

gpu = pytest.mark.gpu

GEOMETRIES = [(1, 1, -1), (2, 3, 0), (3, 2, 1), (7, 32, -1), (64, 255, 1), (8192, 256, 0), (65535, 1, -1)]
LADDER_SEED = 31
LISTED = [(n, 65) for n in (1, 4, 5, 32, 33, 132, 1025)] + [(n, 257) for n in (5, 33, 132)]


@pytest.fixture(scope="module", params=GEOMETRIES, ids=[f"medium{m}_tail{t}_nt{n}" for m, t, n in GEOMETRIES])
def ctx(request):
    """A context of its own per geometry.  "grid_tail" is clamped to the device's CU count by the library: nothing here assumes
    that it was not."""
    from inquistr_amd import hipcall

    c = hipcall.Context(0)
    c.set_option("grid_medium", request.param[0])
    c.set_option("grid_tail", request.param[1])
    c.set_option("nt_loads", request.param[2])
    yield c
    c.close()


# ---- batches and oracle results, built once per module -------------------------------------------------------------------
_CACHE = {}


def _oracle(orc, key, batch):
    if ("want",) + key not in _CACHE:
        oc, want = orc.call_batch(batch, debug=True, threads=8)
        assert oc == 0
        _CACHE[("want",) + key] = want
    return _CACHE[("want",) + key]


def _ladder(orc, unphased, big_support):
    """The ladder batch in one mode at support 3 or at the support that makes the clip rule bite on its deepest locus (from the
    group counts of the support-3 oracle run), and the oracle's result for it."""
    key = ("ladder", unphased, big_support)
    if key not in _CACHE:
        batch, depths = gen.depth_ladder_case(LADDER_SEED, unphased, 3)
        if big_support:
            probe = _oracle(orc, ("ladder", unphased, False), _ladder(orc, unphased, False)[0])
            support, group, ng, ns = gen.clip_rule_support(batch, probe, depths.index(max(depths)))
            assert ns < support < ng
            batch.support = support
            _CACHE[("clip_rule_group", unphased)] = group
        _CACHE[key] = (batch, depths)
    batch, depths = _CACHE[key]
    return batch, depths, _oracle(orc, key, batch)


def _shallow(orc, unphased):
    key = ("shallow", unphased)
    if key not in _CACHE:
        _CACHE[key] = gen.random_case(7, n_loci=60, unphased=unphased)[0]
    return _CACHE[key], _oracle(orc, key, _CACHE[key])


def _listed(orc, n_loci, depth, unphased):
    key = ("listed", n_loci, depth, unphased)
    if key not in _CACHE:
        _CACHE[key] = gen.all_listed_case(n_loci, depth, unphased=unphased)
    return _CACHE[key], _oracle(orc, key, _CACHE[key])


def _device_call(ctx, batch):
    """The batch through the device-resident entry.  inq_call_batch knows the batch's deepest locus and passes it on as the depth
    hint of that call, which skips the launches no locus needs; here the context's own "max_reads_hint" holds (0: none - all
    three launches whatever the batch holds).  Returns (Result with the per-pair outputs, the status code, the tie count)."""
    import torch

    from inquistr_amd import batch as B

    dev = torch.device("cuda:0")

    def up(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)

    t = {k: up(getattr(batch, k)) for k in ("cigar", "reads", "pair_read", "locus_pair_off", "locus_start", "locus_end")}
    out = {"phase1": torch.full((batch.n_loci,), 7.0, dtype=torch.float64, device=dev),
           "phase2": torch.full((batch.n_loci,), 7.0, dtype=torch.float64, device=dev),
           "pair_call": torch.zeros(max(batch.n_pairs, 1), dtype=torch.int64, device=dev),
           "pair_bits": torch.zeros(max(batch.n_pairs, 1), dtype=torch.uint8, device=dev)}
    b = B.InqBatchC()
    b.n_reads, b.n_cigar_words, b.n_pairs, b.n_loci = batch.n_reads, int(batch.cigar.shape[0]), batch.n_pairs, batch.n_loci
    for k, v in t.items():
        setattr(b, k, v.data_ptr())
    b.minlen, b.support, b.unphased, b.reserved = int(batch.minlen), int(batch.support), int(batch.unphased), 0
    r = B.InqResultC()
    for k, v in out.items():
        setattr(r, k, v.data_ptr())
    torch.cuda.synchronize()  # the uploads and fills are there: the context's own stream does not wait for torch's
    ctx.call_batch_device(b, r, torch.cuda.current_stream().cuda_stream)
    rc, ties = ctx.status()  # (waits for the device)
    got = B.Result(phase1=out["phase1"].cpu().numpy(), phase2=out["phase2"].cpu().numpy(),
                   pair_call=out["pair_call"].cpu().numpy()[: batch.n_pairs], pair_bits=out["pair_bits"].cpu().numpy()[: batch.n_pairs],
                   n_tie_loci=ties)
    return got, rc, ties


# ---- the generators against the oracle alone: what keeps the GPU tests below honest ------------------------------------------
def test_the_generators_put_loci_on_every_list_and_both_sides_of_every_threshold(orc):
    """No GPU: the ladder holds every depth-class boundary, six loci deeper than kWalkSplit and two deeper than kGridSelectMin; at
    support 3 every locus of at least 64 reads gets two numbers, no two loci the same ones, and the unphased run meets a tie locus;
    at the large support the deepest locus still gets a number through the clip rule and shallower loci are NaN; every
    read of the ladder may be promised; the listed batches put every locus on the list they are meant for."""
    for unphased in (False, True):
        batch, depths, want = _ladder(orc, unphased, False)
        d = np.diff(batch.locus_pair_off.astype(np.int64))
        assert sorted(d.tolist()) == sorted(gen.LADDER_DEPTHS) == sorted(depths) and d.tolist() == depths
        assert int((d > 16_384).sum()) == 6 and int((d > 65_536).sum()) == 2
        for edge in (64, 256, 2048, 16_384, 65_536):
            assert edge in depths and edge + 1 in depths
        assert 0 in depths and 1 in depths and batch.n_pairs == sum(gen.LADDER_DEPTHS)
        deep = d >= 64
        assert not np.isnan(want.phase1[deep]).any() and not np.isnan(want.phase2[deep]).any()
        rows = {(a, b) for a, b in zip(want.phase1[deep], want.phase2[deep])}
        assert len(rows) == int(deep.sum()), "two loci with the same answer: a result written to the wrong locus would not show"
        assert len(set(zip(batch.locus_start.tolist(), batch.locus_end.tolist()))) == batch.n_loci
        if unphased:
            assert want.n_tie_loci >= 1
        assert gen.checked_share(batch) == 1.0
        big, _, want_big = _ladder(orc, unphased, True)
        deepest = depths.index(max(depths))
        row = (want_big.phase1, want_big.phase2)[_CACHE[("clip_rule_group", unphased)] - 1]
        assert big.support > 3 and not np.isnan(row[deepest])
        assert np.isnan(want_big.phase1[np.arange(batch.n_loci) != deepest]).any()
        assert np.array_equal(want_big.pair_call, want.pair_call) and np.array_equal(want_big.pair_bits, want.pair_bits)
        shallow, _ = _shallow(orc, unphased)
        assert int(np.diff(shallow.locus_pair_off.astype(np.int64)).max()) <= 64
    for n_loci, depth in LISTED:
        batch, want = _listed(orc, n_loci, depth, n_loci % 2 == 1)
        d = np.diff(batch.locus_pair_off.astype(np.int64))
        assert batch.n_loci == n_loci and d.min() == depth and d.max() == min(depth + 3, depth + n_loci - 1)
        assert (d > 64).all() and ((d <= 256).all() if depth == 65 else ((d > 256) & (d <= 2048)).all())
        assert not np.isnan(want.phase1).all()


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("big_support", [False, True], ids=["support3", "clip_rule_support"])
@pytest.mark.parametrize("unphased", [False, True], ids=["phased", "unphased"])
def test_depth_ladder_at_this_geometry(ctx, orc, unphased, big_support):
    """The ladder, then - on the same context - a batch whose loci are all at most 64 reads deep, through the host entry (its depth
    hint: locus_call_small alone) and through the device entry (all three launches, over empty lists), then the ladder again,
    through the device entry, where inq_ctx_status must report the oracle's tie count: what leave() of locus_call_tail left of list
    counters, barrier words and the exit ticket under this grid would show in either.  Then the ladder under the promised
    variants (the row walk)."""
    batch, depths, want = _ladder(orc, unphased, big_support)
    shallow, want_shallow = _shallow(orc, unphased)
    what = f"ladder unphased={unphased} support={batch.support}"
    rc, got = ctx.call_batch(batch, debug=True)
    assert rc == 0
    _assert_same(got, want, what)
    rc, got = ctx.call_batch(shallow, debug=True)
    assert rc == 0
    _assert_same(got, want_shallow, what + ": the shallow batch behind it")
    got, rc, ties = _device_call(ctx, shallow)
    assert rc == 0 and ties == want_shallow.n_tie_loci
    _assert_same(got, want_shallow, what + ": the shallow batch behind it, device entry")
    got, rc, ties = _device_call(ctx, batch)  # (the host entry reads the status itself: inq_ctx_status reports a device call's)
    assert rc == 0 and ties == want.n_tie_loci
    _assert_same(got, want, what + ": second call, device entry")
    assert ctx.status() == (0, 0)
    try:
        _other_variants(ctx, batch, want, what, gen.DEEP_PROMISE_VARIANTS)
    finally:  # the batch is every geometry's: a variant that fails leaves no promise byte behind for the next one
        gen.set_promise(batch, "none")


@gpu
@pytest.mark.parametrize("unphased", [False, True], ids=["phased", "unphased"])
@pytest.mark.parametrize("n_loci,depth", LISTED)
def test_batches_whose_every_locus_is_listed(ctx, orc, n_loci, depth, unphased):
    """Every locus on list 0 (65 - 68 reads) or on list 1 (257 - 260), at locus counts that put grid_small, xcd_remap's
    blocks_per_xcd and shard_cap on and off their rounding steps: through the device entry without a depth hint (the lists are
    emptied by the persistent tail's last workgroup out) and with the hint at the batch's depth (65: by clear_lists), twice each so
    that the second call meets what the first one left, and once through the host entry."""
    batch, want = _listed(orc, n_loci, depth, unphased)
    what = f"{n_loci} loci of {depth} reads unphased={unphased}"
    try:
        for hint in (0, 0, int(np.diff(batch.locus_pair_off.astype(np.int64)).max()), depth + 3, 0):
            ctx.set_option("max_reads_hint", hint)
            got, rc, ties = _device_call(ctx, batch)
            assert rc == 0, f"{what} hint={hint}"
            _assert_same(got, want, f"{what} hint={hint}")
    finally:
        ctx.set_option("max_reads_hint", 0)
    rc, got = ctx.call_batch(batch, debug=True)
    assert rc == 0
    _assert_same(got, want, what + " host entry")
