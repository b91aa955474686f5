"""Call multisets built to break a locus reduce: what tests/deflate_craft.py is to the inflate kernel and tests/bam_craft.py to the
record scan.  No GPU.

A locus' per-read Calls are reduced to its two rows by five pieces of code, chosen by depth (csrc/kernels.hip reduce_locus_in_lanes
with one and with four reads per lane, csrc/deep_reduce.h sort_reduce_locus and reduce_deep_select, csrc/deep_select.hip phase B).
All implement one rule - median_str_length src/call.rs:497-522, the unphased split :308-322, the phased bins :341-369 - and each
has its own way of ranking, breaking ties, counting the clip lump and finding the lower median.  Here a locus is written down as
its Calls, a SPEC: a list, in file order, of

    (value, kind in {SPAN, CLIP}, phase in {None, 0, 1, 2}, kept)

and `build` realises every Call with the fewest CIGAR ops: a read `M a, I v, M b` gives Span(v), `S v` in place of `I v` gives
Clip(v), a `D` op gives a negative Call, k ops of 2^28 - 1 plus a remainder op anything beyond 28 bits (2^46 is 262 144 ops of
2^28 - 1 plus one `I 262144`); an op no longer than `minlen` does not count (src/call.rs:377-413), so a small value v is an `I` / `S`
of |v| + minlen + 1 against a `D` of minlen + 1 (or the converse).  One read per distinct tuple of a batch; the pair list names it
as often as the specs say.  kept = False is a mapq the filter drops: the read keeps its Call, which must not matter.  A kept Call
with phase None is kept by the unphased filter and dropped by the phased one; phase 0 is kept and in no haplotype group.

`rows_by_definition` is the rule in plain Python on the value list (sorted() with a stable key), independent of the oracle and of
any CIGAR.  `group_facts` restates what the kernels' selects look for (threshold, lump, upper median, Calls below it) so that a
test can assert, from the spec alone, that a distribution reaches the branch it is named for.

The distributions (DISTRIBUTIONS, each `n -> loci`, scaled to the depth class by repeating its pattern) and where each exists
(TABLE; what is left out of a class is left out by name, in OMITTED).  `support` is a scalar of the batch, so distributions are
grouped into batches by (depth class, mode, support rule): support 3, and `depth_support(n)` for the clip-rule cases.

Out of reach from a CIGAR, and so from here:
  - the negative sort-key limit -2^46 (and -2^46 - 1): a negative Call is a sum of D ops, and the reference spans less than 2^31;
  - passes 6 and 7 of the rebased grid-wide select: a spread of 2^48 or more needs a read of a million ops or more.
"""
from __future__ import annotations

import bisect
import collections
import functools
import math
import random
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from inquistr_amd.batch import Batch, BatchBuilder

SPAN, CLIP = "Span", "Clip"
OP_MAX = (1 << 28) - 1  # the longest CIGAR op
MINLEN = 5

DEPTH_CLASSES = (64, 256, 257, 2048, 2049, 16384, 16385, 65537)  # the smallest depths at which each reduce can still go wrong
GRIDS = (1, 3, 32, 256)  # grid_tail of the GPU test's contexts (256: the default; a smaller device clamps it)
CLAMPED_GRIDS = (32, 64, 128)  # what the default becomes on a partition of the device (its CU count): placement is asserted for these too
K_FIT = {1: 1 << 25, 4: 1 << 23}  # wave_locus: packed i32 keys below, i64 compares from here on (reads per lane -> limit)
SORT_KEY_LIMIT = 1 << 46  # sort_reduce_locus: a kept Call of this size does not fit the key
HEAVY_OPS = 4096  # a read of more ops than this ...
HEAVY_NAMED = 36  # ... is named at most this often per locus

Call = Tuple[int, str]
Entry = Tuple[int, str, Optional[int], bool]


# ---- the rule, by definition -----------------------------------------------------------------------------------------------------
def _median_str_length(calls: List[Call], support: int) -> float:
    """src/call.rs:497-522"""
    if len(calls) < support:
        return math.nan
    spanning = [v for v, k in calls if k == SPAN]
    if len(spanning) <= support:
        clipped = sorted((v for v, k in calls if k == CLIP), reverse=True)
        spanning += clipped[: support - len(spanning)]
    spanning.sort()
    m = len(spanning)
    if m % 2 == 0:
        return float(spanning[m // 2 - 1] + spanning[m // 2]) / 2.0  # i64 add, then f64
    return float(spanning[m // 2])


def groups_by_definition(spec: List[Entry], unphased: bool):
    """(h1, h2, tie, seen): the two haplotype groups' Calls in file order (unphased: in sorted order), whether the unphased split
    cuts through equal values of mixed kind, and the Calls the reduce looks at at all (unphased: the kept ones; phased: h1 + h2)."""
    if unphased:
        kept = sorted(((v, k) for v, k, _, keep in spec if keep), key=lambda c: c[0])  # stable: equal values stay in file order
        h = len(kept) // 2
        tie = 1 <= h < len(kept) and kept[h - 1][0] == kept[h][0] and len({k for v, k in kept if v == kept[h][0]}) == 2
        return kept[:h], kept[h:], tie, kept
    g1 = [(v, k) for v, k, ph, keep in spec if keep and ph == 1]
    g2 = [(v, k) for v, k, ph, keep in spec if keep and ph == 2]
    return g1, g2, False, g1 + g2


def rows_by_definition(spec: List[Entry], support: int, unphased: bool):
    """(row1, row2, tie) of one locus from its Calls alone (src/call.rs:308-322, 341-369, 497-522)."""
    g1, g2, tie, _ = groups_by_definition(spec, unphased)
    return _median_str_length(g1, support), _median_str_length(g2, support), tie


def group_facts(calls: List[Call], support: int) -> dict:
    """What the selects of one haplotype group look for, from the definition: ng / ns / nc, take, the chosen Calls' count M, the
    clip threshold `thr` (the smallest clipped value taken), `eq` clipped Calls equal to it, `lump` of them taken, the upper median
    `hi`, `below` = chosen Calls smaller than it, the lower median `lo`, and `between` = chosen Calls strictly between thr and hi."""
    spans = sorted(v for v, k in calls if k == SPAN)
    clips = sorted((v for v, k in calls if k == CLIP), reverse=True)
    f = {"ng": len(calls), "ns": len(spans), "nc": len(clips), "live": len(calls) >= support}
    f["take"] = support - len(spans) if len(spans) <= support else 0
    taken = clips[: f["take"]]
    chosen = sorted(spans + taken)
    f["M"] = len(chosen)
    if taken:
        f["thr"] = taken[-1]
        f["eq"] = clips.count(taken[-1])
        f["lump"] = taken.count(taken[-1])
    if f["live"] and chosen:
        f["hi"] = chosen[len(chosen) // 2]
        f["below"] = bisect.bisect_left(chosen, f["hi"])
        f["lo"] = chosen[len(chosen) // 2 - 1] if len(chosen) % 2 == 0 else f["hi"]
        if taken:
            f["between"] = bisect.bisect_left(chosen, f["hi"]) - bisect.bisect_right(chosen, f["thr"])
    return f


def select_top(spec: List[Entry], unphased: bool) -> int:
    """The byte index of kmax - kmin over the Calls the grid-wide select looks at (key_space().top of csrc/deep_select.hip)."""
    seen = [v for v, _ in groups_by_definition(spec, unphased)[3]]
    if not seen or max(seen) == min(seen):
        return 0
    return ((max(seen) - min(seen)).bit_length() - 1) >> 3


def slice_geometry(n: int, grid: int):
    """(slice, n_slices, part): locus_call_tail cuts a locus of n reads into slices of ceil(ceil(n / grid) / 256) * 256 reads, at
    most one per workgroup; in the unphased grouping a thread takes ceil(len / 256) consecutive reads of a slice (`part`, of a full
    slice).  Used only to place runs and to assert where they fall."""
    sl = -(-(-(-n // grid)) // 256) * 256
    return sl, -(-n // sl), -(-min(sl, n) // 256)


# ---- CIGARs ----------------------------------------------------------------------------------------------------------------------
def _chunks(v: int, minlen: int) -> List[int]:
    """v > minlen as the fewest op lengths, each longer than minlen."""
    k, rem = divmod(v, OP_MAX)
    if 0 < rem <= minlen:  # the remainder op would not count: take it from the last full one
        return [OP_MAX] * (k - 1) + [OP_MAX - (minlen + 1 - rem), minlen + 1]
    return [OP_MAX] * k + ([rem] if rem else [])


def compose(value: int, kind: str, minlen: int) -> List[Tuple[str, np.ndarray]]:
    """The ops between the leading and the trailing M run that make Call (value, kind): [(op, lengths)], I / S ops in front of the
    D op (nothing behind a D starts at the same reference position)."""
    m1 = minlen + 1
    ins = "I" if kind == SPAN else "S"
    plus, minus = [], 0
    if kind == SPAN and value == 0:
        return []
    if value >= m1:
        plus = _chunks(value, minlen)
    elif value > 0:
        plus, minus = [value + m1], m1
    elif kind == CLIP:  # a clipped Call needs an S op that counts
        plus, minus = [m1], m1 - value
    elif value <= -m1:
        minus = -value
    else:
        plus, minus = [m1], m1 - value
    assert minus <= OP_MAX, "a negative Call is one D op: the reference spans less than 2^31"
    assert sum(plus) - minus == value and all(x > minlen for x in plus) and (minus == 0 or minus > minlen)
    out = [(ins, np.array(plus, dtype=np.int64))] if plus else []
    return out + ([("D", np.array([minus], dtype=np.int64))] if minus else [])


_OP = {c: i for i, c in enumerate("MIDNSHP=X")}
_S0, _W = 1_000_000, 40  # locus j of a batch has the window [_S0 - j, _S0 + _W + j]: nested, every locus its own
_POS, _AT, _TAIL = _S0 - 400, _S0 + 20, 800  # every read starts at _POS, its ops start at reference position _AT, M _TAIL follows


def _cigar_words(value: int, kind: str, minlen: int) -> np.ndarray:
    parts = [np.array([((_AT - _POS - 1) << 4) | _OP["M"]], dtype=np.int64)]
    parts += [(ln << 4) | _OP[op] for op, ln in compose(value, kind, minlen)]
    parts.append(np.array([(_TAIL << 4) | _OP["M"]], dtype=np.int64))
    return np.concatenate(parts).astype(np.uint32)


def build(specs: List[List[Entry]], minlen: int, support: int, unphased: bool) -> Batch:
    """One locus per spec, every locus with its own window; one read per distinct (value, kind, phase, kept) of the batch."""
    assert len(specs) <= 300
    bb = BatchBuilder(minlen=minlen, support=support, unphased=unphased)
    ids: Dict[Entry, int] = {}
    heavy = set()
    for j, spec in enumerate(specs):
        named = collections.Counter(spec)  # (in order of first appearance)
        for e in named:
            if e not in ids:
                w = _cigar_words(e[0], e[1], minlen)
                ids[e] = bb.add_read(_POS, w, mapq=60 if e[3] else 5, phase=e[2])
                if w.shape[0] > HEAVY_OPS:
                    heavy.add(e)
        assert sum(c for e, c in named.items() if e in heavy) <= HEAVY_NAMED, "the walk and the oracle stay cheap"
        bb.add_locus(_S0 - j, _S0 + _W + j, np.fromiter((ids[e] for e in spec), dtype=np.int64, count=len(spec)))
    return bb.build()


# ---- helpers of the distributions -------------------------------------------------------------------------------------------------
def depth_support(n: int) -> int:
    """The batch's `support` for the clip-rule cases of depth class n: even, and two groups of a few more Calls than it fit n."""
    return n // 4 + n // 16


def weave(*lists):
    """The lists merged into one file order, each spread evenly over it and kept in its own order."""
    keyed = [((i + 0.5) / len(l), k, i) for k, l in enumerate(lists) for i in range(len(l))]
    keyed.sort()
    return [lists[k][i] for _, k, i in keyed]


_FILL = ((999, SPAN), ((1 << 30) + 5, CLIP), (-50, SPAN), (77, CLIP))


def filler(count: int) -> List[Entry]:
    """Offered but not kept: Calls that are not zero - the first few far beyond every kept one -, every phase."""
    out = [((1 << 40) + 1, SPAN, (None, 0, 1, 2)[i], False) for i in range(min(4, count))]
    return out + [_FILL[i % 4] + ((None, 0, 1, 2)[(i // 4) % 4], False) for i in range(count - len(out))]


def shuffled(calls: List[Call], seed: int) -> List[Call]:
    calls = list(calls)
    random.Random(seed).shuffle(calls)
    return calls


def offer(n: int, g1: List[Call], g2: List[Call], other: List[Entry] = ()) -> List[Entry]:
    """n offered reads: g1 with HP 1, g2 with HP 2, `other` as given, the rest filler, woven into one file order."""
    fill = n - len(g1) - len(g2) - len(other)
    assert fill >= 0, (n, len(g1), len(g2), len(other))
    lists = [[(v, k, 1, True) for v, k in g1], [(v, k, 2, True) for v, k in g2], list(other), filler(fill)]
    return weave(*[l for l in lists if l])


def shift(calls: List[Call], by: int) -> List[Call]:
    return [(v + by, k) for v, k in calls]


class Locus(NamedTuple):
    dist: str
    variant: str
    spec: List[Entry]
    meta: dict


_OFF = 1000  # group 2 = group 1's pattern this much higher: the unphased split of the two puts them back into h1 and h2


# ---- the distributions: (n, support) -> [(variant, spec, meta)] ----------------------------------------------------------------------
def all_equal_mixed(n, support):
    """One value; kinds alternate.  Unphased: a tie.  Under the clip rule every taken clipped Call is lump."""
    kept = n - n // 8
    spec = [(37, SPAN if i % 2 == 0 else CLIP, 1 + (i // 2) % 2, True) for i in range(kept)]
    return [("one_value", weave(spec, filler(n - kept)), {})]


def _even_split(h, a, b):
    return shuffled([(a, SPAN)] * h + [(b, SPAN)] * h, h)


def two_values_even_split(n, support):
    """Per group: the lower half A, the upper half B, A + B odd: exactly M / 2 chosen Calls lie below the upper median."""
    h = n // 5
    return [("even", offer(n, _even_split(h, 10, 21), _even_split(h, 10 + _OFF, 21 + _OFF)), {"want": (15.5, 15.5 + _OFF)})]


def two_values_off_by_one(n, support):
    """... and one Call moved across: the lower median equals the upper one."""
    h = n // 5
    out = []
    for name, d, want in (("one_up", -1, 21.0), ("one_down", 1, 10.0)):
        g = shuffled([(10, SPAN)] * (h + d) + [(21, SPAN)] * (h - d), h)
        out.append((name, offer(n, g, shift(g, _OFF)), {"want": (want, want + _OFF)}))
    return out


def lower_median_is_the_lump(n, support):
    """Per group: s Span(100), c >= s Clip(50), support = 2 s: chosen = s x 50 (all lump) + s x 100, median 75 - the lower median
    exists only as nameless lump Calls.  `named`: one Clip(60) above the threshold: the lower median is a named Call, the lump
    lies below it."""
    s = support // 2
    assert support == 2 * s
    out = []
    for name, extra, want in (("lump", [], 75.0), ("named", [(60, CLIP)], 80.0)):
        g = shuffled([(100, SPAN)] * s + [(50, CLIP)] * (s + 3) + extra, s)
        out.append((name, offer(n, g, shift(g, _OFF)), {"want": (want, want + _OFF)}))
    return out


_THR_VARIANTS = {"at_median": 0, "below_median": -1, "above_median": 1}  # variant -> threshold minus upper median


def _threshold_group(name, support, T, low=None, high=()):
    """One group of threshold_ties_partial_lump around T; `low` takes the place of one spanning Call below T, `high` of as many above."""
    ns = support * 3 // 4 if name == "above_median" else support // 2
    t = support - ns  # take
    k = max(1, t // 4)  # clipped Calls above T
    lump = t - k
    clips = [(T, CLIP)] * (lump + 3) + [(T + 5, CLIP)] * k + [(T - 20, CLIP)] * 2
    if name == "at_median":
        x, z = ns - lump // 2, 0
    elif name == "below_median":
        z = max(2, t // 4)
        x = support // 2 - lump - z // 2
    else:
        x, z = support * 5 // 8, 0
    y = ns - x - z
    assert x >= (low is not None) and y >= len(high), (name, support, x, y, z)
    lows = [(T - 1, SPAN)] * x
    highs = [(T + 9, SPAN)] * y
    if low is not None:
        lows[0] = (low, SPAN)
    highs[: len(high)] = [(v, SPAN) for v in high]
    return shuffled(lows + [(T + 1, SPAN)] * z + highs + clips, t)


def threshold_ties_partial_lump(n, support):
    """Many clipped Calls equal to the threshold T, 0 < lump < eq; the threshold equal to, just below and just above the upper median."""
    out = []
    for name, d in _THR_VARIANTS.items():
        g = _threshold_group(name, support, 500)
        out.append((name, offer(n, g, shift(g, _OFF)), {"thr_minus_hi": d}))
    return out


_WIDE_MIN, _WIDE_FAR = -7, 1 << 40
_WIDE_T = ((1 << 24) + _WIDE_MIN, (1 << 32) + (1 << 24) + _WIDE_MIN)  # the groups' thresholds: rebased, 2^24 and 2^32 + 2^24 exactly


def lump_in_a_wide_key_space(n, support):
    """The clip rule where the rebased keys have six bytes: h1 holds the smallest Call, -7, and the threshold 2^24 - 7 - rebased
    2^24, byte 3 set and nothing below it, one above the spanning Calls of rebased key 2^24 - 1 -; h2 lies 2^32 higher and holds the
    largest, 2^40.  The three variants of threshold_ties_partial_lump (0 < lump < eq, the lump a term of every histogram from byte 5
    down), and `lump_is_lower_median`: per group s + 1 spanning Calls - one below the threshold, s (s - 1 and the far one) above -
    and s + 3 clipped ones at the threshold, support 2 s: chosen = the low one, s - 1 lump, s above: the lower median is lump."""
    t1, t2 = _WIDE_T
    out = []
    for name, d in _THR_VARIANTS.items():
        g1 = _threshold_group(name, support, t1, low=_WIDE_MIN)
        g2 = _threshold_group(name, support, t2, high=(_WIDE_FAR, _WIDE_FAR - 7))
        out.append((name, offer(n, g1, g2), {"thr_minus_hi": d, "thr": _WIDE_T}))
    s = support // 2
    h1, h2 = t1 + (1 << 16), t2 + (1 << 16)
    g1 = shuffled([(_WIDE_MIN, SPAN)] + [(h1, SPAN)] * s + [(t1, CLIP)] * (s + 3), s)
    g2 = shuffled([(1 << 32, SPAN)] + [(h2, SPAN)] * (s - 1) + [(_WIDE_FAR, SPAN)] + [(t2, CLIP)] * (s + 3), s + 1)
    out.append(("lump_is_lower_median", offer(n, g1, g2), {"thr": _WIDE_T, "want": ((t1 + h1) / 2.0, (t2 + h2) / 2.0)}))
    return out


def equal_run_across_boundaries(n, support):
    """Unphased.  A run of Calls equal to the split value X: c Clips first in file order, then s Spans; q Span(A) below, p Span(B)
    above, support = 2 q.  r = mcount / 2 - below = c + q cuts inside the Spans: h1 = q A + c Clip X + q Span X has as many
    spanning Calls as `support` says (no clipped Call taken, median (A + X) / 2), h2 = p Span X + p B (median (X + B) / 2).  One
    equal Call more in h1 makes it X, one fewer makes h2's X; h1 with other equal Calls than the first r has another count of
    spanning Calls, and the clip rule gives another row."""
    A, X, B = 10, 30, 60
    q = support // 2
    c = max(2, n // 32 // 2 * 2)
    p = q + c // 2
    s = q + p
    others = weave([(A, SPAN, None, True)] * q, [(B, SPAN, 1, True)] * p, filler(n - (2 * q + 2 * p + c)))
    run_lo = min(n * 5 // 16 + n // 50, len(others))  # (+ n / 50: the cut on no boundary itself)
    run = [(X, CLIP, 2, True)] * c + [(X, SPAN, None, True)] * s
    spec = others[:run_lo] + run + others[run_lo:]
    assert len(spec) == n
    return [("cut_in_the_spans", spec, {"run": (run_lo, run_lo + c + s), "cut": run_lo + c + q, "r": c + q, "eq": c + s,
                                        "want": ((A + X) / 2.0, (X + B) / 2.0)})]


_BYTE_EDGES = (1 << 8, 1 << 16, 1 << 24, 1 << 32)
_BYTE_MIN = -7  # the smallest Call: the rebased key of v is v + 7


def byte_boundaries(n, support):
    """Calls at and next to 0, 2^8, 2^16, 2^24, 2^32 and 2^40, raw (B - 1, B) and rebased (B - 8, B - 7: the rebased keys cross a byte
    boundary the raw ones do not), from a smallest Call of -7.  Four tenths of each group lie in 2^24 .. 2^24 + 2^16 + 1 as Spans,
    the upper median among them, and as many Clips the median does not choose share those upper bytes.  Spread >= 2^40: top = 5."""
    cluster = [(1 << 24) + d for d in (0, 1, 248, 249, 255, 256, 257, 65528, 65529, 65535, 65536, 65537)]
    low = [0, 1, 248, 249, 255, 256, (1 << 16) - 8, (1 << 16) - 7, (1 << 16) - 1, 1 << 16, (1 << 24) - 8, (1 << 24) - 7, (1 << 24) - 1]
    high = [(1 << 32) - 8, (1 << 32) - 7, (1 << 32) - 1, 1 << 32, (1 << 32) + 1]
    far = [(1 << 40) - 8, (1 << 40) - 7, (1 << 40) - 1, 1 << 40]
    m = (n - n // 8) // 2
    groups = []
    for g in (0, 1):
        n_far = min(8, max(2, m // 16))
        n_cl = m * 4 // 10
        n_clip = m * 2 // 10
        n_low = (m - n_cl - n_clip - n_far - 1) * 5 // 9
        n_high = m - n_cl - n_clip - n_far - 1 - n_low
        calls = [(_BYTE_MIN, SPAN)] + [(low[(i + g) % len(low)], SPAN) for i in range(n_low)]
        calls += [(cluster[(i + 5 * g) % len(cluster)], SPAN) for i in range(n_cl)] + [(cluster[(i + g) % len(cluster)], CLIP) for i in range(n_clip)]
        calls += [(high[(i + g) % len(high)], SPAN) for i in range(n_high)] + [(far[(2 * i + g) % len(far)], SPAN) for i in range(n_far)]
        groups.append(shuffled(calls, m + g))
    return [("top5", offer(n, groups[0], groups[1]), {"top": 5, "cluster": (cluster[0], cluster[-1])})]


def signs(n, support):
    """Negative (D ops) and positive Calls, the group medians at -1 / 0 / +1 (and between -1 and 0), the unphased split value the
    same: both groups hold the same Calls, so the split cuts the run of the median value, of mixed kind."""
    m = (n - n // 8) // 2
    m -= 1 - m % 2  # odd
    side = (m - 3) // 2
    neg, pos = [-300, -8, -2], [2, 8, 300]
    out = []
    for name, mid in (("minus_one", [-1] * 3), ("zero", [0] * 3), ("plus_one", [1] * 3), ("minus_half", [-1, -1, 0, 0])):
        g = [(neg[i % 3], SPAN if i % 4 else CLIP) for i in range(side)] + [(v, SPAN if i % 2 else CLIP) for i, v in enumerate(mid)]
        g += [(pos[i % 3], SPAN if i % 4 else CLIP) for i in range(side)]
        want = -0.5 if name == "minus_half" else float(mid[0])
        out.append((name, offer(n, shuffled(g, side), shuffled(g, side + 1)), {"want_phased": (want, want), "split": mid[len(mid) // 2]}))
    return out


def _limit_locus(n, x, kept):
    """Five small kept Calls and x: 10 20 30 40 50, HP 1 2 1 2 1 2 in ascending order of the six - the three of x's group have their
    median next to x's end, and the unphased halves theirs: x on the wrong end of the order moves both.  Unkept, x sits beside six
    small kept Calls."""
    vals = sorted([10, 20, 30, 40, 50] + [x if kept else 60])
    six = [(v, SPAN, 1 + i % 2, True) for i, v in enumerate(vals)]
    other = six if kept else six + [(x, SPAN, 2, False)] * 3
    return offer(n, [], [], other=shuffled(other, abs(x) % 1000))


def fit_limits(n, support):
    """Kept Calls kFit - 1, kFit, -kFit, -kFit - 1 of the wave reduce of this class (one limit per locus: it sits alone on its side),
    and the two beyond the limit unkept next to small kept ones (the packed path must be taken and must be right).  `inside`: the
    kept Calls fit the packed key."""
    kfit = K_FIT[1 if n <= 64 else 4]
    out = []
    for name, x, inside in (("fit_minus_1", kfit - 1, True), ("fit", kfit, False), ("minus_fit", -kfit, True), ("minus_fit_minus_1", -kfit - 1, False)):
        out.append((name, _limit_locus(n, x, True), {"x": x, "kept": True, "inside": inside}))
        if not inside:
            out.append((name + "_unkept", _limit_locus(n, x, False), {"x": x, "kept": False, "inside": True}))
    return out


def sort_key_limits(n, support):
    """2^46 - 1 (must sort in LDS) and 2^46 (must defer or select), kept; 2^46 unkept (must sort).  -2^46: see the module docstring."""
    return [(name, _limit_locus(n, x, kept), {"x": x, "kept": kept, "inside": inside})
            for name, x, kept, inside in (("limit_minus_1", SORT_KEY_LIMIT - 1, True, True), ("limit", SORT_KEY_LIMIT, True, False),
                                          ("limit_unkept", SORT_KEY_LIMIT, False, True))]


def count_boundaries(n, support):
    """The count edges of plan_group: a group of `support` and of `support - 1` Calls (the full one takes every clipped Call it
    has); ns in {support - 1, support, support + 1} with clipped Calls to take from; 0, 1 and 2 kept Calls among n offered; every
    Call in HP 1 (the other group empty); every Call in HP 0 or without HP."""
    s = support
    lo = lambda cnt, base: [(base + 3 * (i % 5), SPAN) for i in range(cnt)]
    clips = lambda cnt, base: [(base + 40 + 7 * (i % 3), CLIP) for i in range(cnt)]
    out = [("support_and_one_short", offer(n, lo(max(0, s - 3), 100) + clips(min(2, s - 1), 100), lo(s - min(2, s), 100 + _OFF) + clips(min(2, s), 100 + _OFF)),
            {"ng": (s - 1, s), "take_all": 2})]
    out.append(("ns_one_short_and_equal", offer(n, lo(s - 1, 100) + clips(4, 100), lo(s, 100 + _OFF) + clips(3, 100 + _OFF)), {"ns": (s - 1, s)}))
    out.append(("ns_one_more_and_equal", offer(n, lo(s + 1, 100) + clips(2, 100), lo(s, 100 + _OFF) + clips(3, 100 + _OFF)), {"ns": (s + 1, s)}))
    for k in (0, 1, 2):
        out.append((f"kept_{k}", offer(n, [(11, SPAN)] * (k // 2), [(12 + _OFF, CLIP)] * (k - k // 2)), {"kept": k}))
    out.append(("one_group_empty", offer(n, lo(s + 2, 100) + clips(3, 100), []), {}))
    none = [(100 + 3 * (i % 5), SPAN if i % 3 else CLIP, (None, 0)[i % 2], True) for i in range(min(n, s + 4))]
    out.append(("all_in_hp0_or_none", offer(n, [], [], other=none), {}))
    return out


def two_deep_loci_of_different_spread(n, support):
    """In one batch: a locus of more than 65 536 reads with a spread below 256 (top = 0) beside one with byte_boundaries (top = 5)."""
    narrow = offer(n, _even_split(n // 5, 10, 21), _even_split(n // 5, 110, 121))
    return [("narrow", narrow, {"top": 0}), ("wide", byte_boundaries(n, support)[0][1], {"top": 5})]


# name -> (function, support rules, modes (False: phased, True: unphased))
DISTRIBUTIONS = {
    "all_equal_mixed": (all_equal_mixed, ("3", "depth"), (False, True)),
    "two_values_even_split": (two_values_even_split, ("3",), (False, True)),
    "two_values_off_by_one": (two_values_off_by_one, ("3",), (False, True)),
    "lower_median_is_the_lump": (lower_median_is_the_lump, ("depth",), (False, True)),
    "threshold_ties_partial_lump": (threshold_ties_partial_lump, ("depth",), (False, True)),
    "lump_in_a_wide_key_space": (lump_in_a_wide_key_space, ("depth",), (False, True)),
    "equal_run_across_boundaries": (equal_run_across_boundaries, ("depth",), (True,)),
    "byte_boundaries": (byte_boundaries, ("3",), (False, True)),
    "signs": (signs, ("3",), (False, True)),
    "fit_limits": (fit_limits, ("3",), (False, True)),
    "sort_key_limits": (sort_key_limits, ("3",), (False, True)),
    "count_boundaries": (count_boundaries, ("3", "depth"), (False, True)),
    "two_deep_loci_of_different_spread": (two_deep_loci_of_different_spread, ("3",), (False, True)),
}
# where each distribution exists ...
TABLE = {name: DEPTH_CLASSES for name in DISTRIBUTIONS}
TABLE["fit_limits"] = (64, 256)
TABLE["sort_key_limits"] = (257, 2048, 2049, 16384)
TABLE["two_deep_loci_of_different_spread"] = (65537,)
# ... and why not elsewhere (no skip: these pairs are not cases)
OMITTED = {
    "fit_limits": "kFit is a limit of the two wave reduces (up to 64 and up to 256 offered reads); deeper loci never pack a key into an i32",
    "sort_key_limits": "the 47-bit key is the LDS sort's (257 .. 16 384 offered reads): the wave reduces compare i64 values, the selects whole keys",
    "two_deep_loci_of_different_spread": "only loci of more than 65 536 reads share the passes of the grid-wide select",
}
# the number of loci each distribution gives per batch
VARIANTS = {"all_equal_mixed": 1, "two_values_even_split": 1, "two_values_off_by_one": 2, "lower_median_is_the_lump": 2, "threshold_ties_partial_lump": 3,
            "lump_in_a_wide_key_space": 4, "equal_run_across_boundaries": 1, "byte_boundaries": 1, "signs": 4, "fit_limits": 6, "sort_key_limits": 3,
            "count_boundaries": 8, "two_deep_loci_of_different_spread": 2}
# properties that exist at some classes only (asserted where they exist, by tests/test_call_craft.py):
#   equal_run_across_boundaries: the run straddles a chunk of reduce_deep_select's 256 at 16 385; a slice boundary (grids 3, 32, 256), a
#   thread-part boundary (every grid) and a multiple of 256 at 65 537.  At 64 .. 16 384 there is no slice, part or chunk to straddle.
#   byte_boundaries, lump_in_a_wide_key_space: top = 5 is a property of the spec at every class; only the grid-wide select (65 537) acts on it.
RULES = ("3", "depth")
MODES = (False, True)


def support_of(n: int, rule: str) -> int:
    return 3 if rule == "3" else depth_support(n)


def cases():
    """Every (distribution, depth class, unphased) that exists."""
    return [(d, n, u) for d, (_, _, modes) in DISTRIBUTIONS.items() for n in TABLE[d] for u in modes]


def batch_keys():
    return [(n, u, r) for n in DEPTH_CLASSES for u in MODES for r in RULES]


@functools.lru_cache(maxsize=None)
def batch_of(n: int, unphased: bool, rule: str):
    """(Batch, loci): every distribution of depth class n that exists in this mode under this support rule, one locus per variant."""
    support = support_of(n, rule)
    loci = []
    for dist, (fn, rules, modes) in DISTRIBUTIONS.items():
        if n in TABLE[dist] and rule in rules and unphased in modes:
            loci += [Locus(dist, variant, spec, meta) for variant, spec, meta in fn(n, support)]
    assert all(len(l.spec) == n for l in loci)
    return build([l.spec for l in loci], MINLEN, support, unphased), tuple(loci)


_ORACLE = {}


def oracle_of(orc, n: int, unphased: bool, rule: str):
    """The C oracle's result for batch_of(...), computed once per process (the promise byte is not read by the oracle)."""
    key = (n, unphased, rule)
    if key not in _ORACLE:
        oc, want = orc.call_batch(batch_of(*key)[0], debug=True, threads=8)
        assert oc == 0
        _ORACLE[key] = want
    return _ORACLE[key]


def definition_rows(n: int, unphased: bool, rule: str):
    """(phase1, phase2, ties) of batch_of(...) by definition."""
    _, loci = batch_of(n, unphased, rule)
    rows = [rows_by_definition(l.spec, support_of(n, rule), unphased) for l in loci]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), sum(int(r[2]) for r in rows)
