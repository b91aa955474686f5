"""Hand-built DEFLATE streams no encoder writes (tests/deflate_craft.py), pinned on the CPU before the GPU sees them.

Every case of corpus() states which path of inquistr_amd/csrc/bgzf_inflate_wg.hip it was built for.  Here, without a GPU:
  * zlib gives the verdict: a case built as valid inflates with zlib.decompressobj(-15) to exactly the writer's own replay and
    ends the stream; a case built as a reject raises in zlib or does not end with its isize bytes.  A case whose intent and
    zlib disagree is a bug of the test and fails here;
  * the coverage predicate of the case holds, computed from the writer's trace and the geometry model;
  * the model's constants are the kernel's #define defaults.
tests/test_gpu_inflate_crafted.py imports corpus() and runs the same cases through the device inflate.
"""
import os
import random
import zlib
from dataclasses import dataclass
from typing import Callable, Optional

import pytest

from tests import deflate_craft as dc
from tests.deflate_craft import DS, EOB, LIT, LL, MATCH, Raw, Stream, balanced, kraft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM = random.Random(1951).randbytes(65536)  # bytes in front of far matches: a wrong distance copies other bytes


@dataclass
class Case:
    name: str
    group: str               # one launch per group on the GPU
    payload: bytes
    isize: int
    valid: bool              # the intent; zlib_verdict() must agree
    path: str                # the kernel path the case was built for
    predicate: Callable      # (case) -> bool, from the trace and the geometry model
    cr: Optional[dc.Crafted] = None
    want: Optional[bytes] = None  # the writer's replay (valid cases)


def zlib_verdict(payload: bytes, n: int):
    """(accepted, bytes): accepted = zlib ends the stream having produced exactly n bytes."""
    d = zlib.decompressobj(-15)
    try:
        got = d.decompress(payload, n + 1)
    except zlib.error:
        return False, None
    return (d.eof and len(got) == n), got


# ---------------------------------------------------------------- code construction
def complete(lens, spare):
    """Fills what a set of code lengths leaves of the code space with one code per set bit of the remainder, given to the
    symbols of `spare` (symbols no body uses)."""
    lens = list(lens)
    left = 32768 - kraft(lens)
    assert left >= 0
    spare = iter(spare)
    for n in range(1, 16):
        if left & (1 << (15 - n)):
            lens[next(spare)] = n
    assert kraft(lens) == 32768
    return lens


def make_ll(spec, size=286, spare=range(128, 256)):
    lens = [0] * size
    for s, n in spec.items():
        lens[s] = n
    return complete(lens, (s for s in spare if s not in spec))


def make_dl(spec, size=30):
    lens = [0] * size
    for s, n in spec.items():
        lens[s] = n
    if len(spec) == 1 and list(spec.values()) == [1]:
        return lens  # a single one-bit code: the one incomplete set zlib accepts
    return complete(lens, (s for s in range(size) if s not in spec))


def ladder(symbols, size):
    """Lengths 1, 2, ..., k - 1, k - 1 over k symbols in the order given: complete, every length once."""
    lens = [0] * size
    for i, s in enumerate(symbols):
        lens[s] = min(i + 1, len(symbols) - 1)
    assert kraft(lens) == 32768
    return lens


class Body:
    """Lays a body out by bit position: knows what every token costs and where the kernel's round would put its stage."""

    def __init__(self, pos, out, ll, dl, pads, alt258=False):
        self.pos, self.out, self.ll, self.dl, self.alt = pos, out, ll, dl, alt258
        self.stage0 = pos & ~31
        self.toks = []
        self.pads = sorted(pads, key=lambda s: -ll[s])  # literals to pad with, longest first
        self._plan = {}

    @property
    def rel(self):
        return self.pos - self.stage0

    def cost(self, t):
        if type(t) is int:
            return self.ll[t]
        s, _, xb = dc.length_symbol(t[0], self.alt)
        d, _, dxb = dc.dist_symbol(t[1])
        return self.ll[s] + xb + self.dl[d] + dxb

    def add(self, *ts):
        for t in ts:
            if self.pos - self.stage0 >= dc.T * dc.SEG_BITS:  # this symbol starts the next round
                self.stage0 = self.pos & ~31
            self.toks.append(t)
            self.pos += self.cost(t)
            self.out += 1 if type(t) is int else t[0]
        return self

    def plan(self, r):
        """Fewest pad literals that take exactly r bits, or None."""
        if r == 0:
            return []
        if r < 0:
            return None
        if r not in self._plan:
            best = None
            for s in self.pads:
                sub = self.plan(r - self.ll[s])
                if sub is not None and (best is None or len(sub) + 1 < len(best)):
                    best = [s] + sub
            self._plan[r] = best
        return self._plan[r]

    def reachable(self, r):
        big = self.ll[self.pads[0]]
        if r > 4 * big:
            r -= (r - 4 * big + big - 1) // big * big
        return self.plan(r) is not None

    def pad(self, r):
        big = self.ll[self.pads[0]]
        while r > 4 * big:
            self.add(self.pads[0])
            r -= big
        p = self.plan(r)
        assert p is not None, r
        self.add(*p)
        return self

    def pad_to_mod(self, m, mod=dc.SEG_BITS):
        """Pads until the next symbol starts at m modulo `mod`, relative to the round's stage."""
        r = (m - self.rel) % mod
        while not self.reachable(r):
            r += mod
        return self.pad(r)

    def pad_to_rel(self, x):
        assert x >= self.rel
        return self.pad(x - self.rel)


# workbench code: pad literals of 2, 3 and 8 bits (every distance >= 2 is reachable), four 4-bit data literals, the six lengths
# of the match tests, end-of-block at 5 bits
X, Y, Z = 0x78, 0x79, 0x7A
DATA = [0x61, 0x62, 0x63, 0x64]
WB_LENS = {3: 257, 4: 258, 5: 259, 7: 261, 8: 262, 258: 285}


def wb_ll(more=None):
    spec = {X: 2, Y: 3, Z: 8, 256: 5}
    spec.update({s: 4 for s in DATA})
    spec.update({s: 5 for s in WB_LENS.values()})
    spec.update(more or {})
    return make_ll(spec)


WB_DL = make_dl({0: 3, 1: 3, 2: 3, 3: 3, 4: 3, 5: 3})  # distances 1, 2, 3, 4, 5, 7-8; the rest of the space: unused symbols


_ROUNDS = {}


def block_rounds(cr, bi):
    key = (id(cr), bi)
    if key not in _ROUNDS:
        _ROUNDS[key] = dc.rounds(cr, bi)
    return _ROUNDS[key]


def all_rounds(cr):
    return [(bi, rd) for bi, b in enumerate(cr.blocks) if b.type in (1, 2) and b.t1 > b.t0 for rd in block_rounds(cr, bi)]


def rel_starts(cr, want):
    """{(symbol start relative to its round's stage) for the symbols `want` selects}, with the round's index in the block."""
    res = []
    for bi, b in enumerate(cr.blocks):
        if b.type not in (1, 2):
            continue
        for ri, rd in enumerate(block_rounds(cr, bi)):
            for g in rd.segs[: rd.ncommit]:
                for i in g.syms:
                    if want(cr.trace[i]):
                        res.append((ri, cr.trace[i].start - rd.stage0, i))
    return res


CASES = []


def case(name, group, stream_or_cr, path, predicate, valid=True, isize=None, payload=None):
    cr = stream_or_cr.finish() if isinstance(stream_or_cr, Stream) else stream_or_cr
    payload = cr.payload if payload is None else payload
    if isize is None:
        isize = len(cr.output)
    CASES.append(Case(name, group, payload, isize, valid, path, predicate, cr, cr.output if valid else None))
    return CASES[-1]


# ---------------------------------------------------------------- symbols and codes
def _codes():
    # every code length 1 .. 15 in both sets; literal, length symbol and end-of-block behind the 10-bit table (11 .. 15 bits),
    # distance codes behind the 8-bit table (9 .. 15 bits): one block per end-of-block length
    for eob_len in (11, 12, 13, 14, 15):
        spec = {0x41 + n: n for n in range(1, 8)}            # literals of 1 .. 7 bits
        spec.update({0x30: 9, 0x31: 10})
        spec.update({0x50 + n: n for n in range(11, 16)})     # literals of 11 .. 15 bits
        spec.update({265 + (n - 11): n for n in range(11, 16)})  # length symbols 265 .. 269 (one extra bit) of 11 .. 15 bits
        spec[256] = eob_len
        ll = make_ll(spec)
        dsyms = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
        dl = ladder(dsyms, 30)                               # lengths 1 .. 15, 15
        toks = [0x41 + 1 + i % 7 for i in range(300)]
        for n in range(11, 16):
            toks.append(0x50 + n)
        for i, n in enumerate(range(11, 16)):
            for k, d in enumerate(dsyms):                     # every distance code length, with extra bits all-zero / all-one
                lo = dc.DIST_BASE[d]
                hi = lo + (1 << dc.DIST_XB[d]) - 1
                toks.append((dc.LEN_BASE[8 + i] + (k & 1), hi if (k + i) & 1 else lo))
                toks.append(0x50 + n)
        s = Stream().dynamic(toks, ll, dl, final=True)

        def pred(c, eob_len=eob_len):
            tr = c.cr.trace
            lits = {t.code_bits for t in tr if t.kind == LIT}
            lens = {t.code_bits for t in tr if t.kind == MATCH}
            dists = {t.dcode_bits for t in tr if t.kind == MATCH}
            eobs = {t.code_bits for t in tr if t.kind == EOB}
            return set(range(11, 16)) <= lits and set(range(11, 16)) <= lens and set(range(9, 16)) <= dists and eobs == {eob_len} \
                and eob_len > dc.LIT_BITS and min(range(9, 16)) > dc.DIST_BITS
        case(f"long_codes_eob{eob_len}", "codes", s, "canon_entry behind both tables: literal, length, end-of-block of 11-15 bits, distance of 9-15",
             pred)
    # one set with every length 1 .. 15 (the ladder), literal/length and distance
    lsyms = [0x41 + i for i in range(13)] + [257, 256, 258]
    ll = ladder(lsyms, 286)
    dl = ladder(list(range(16)), 30)
    toks = [0x41 + i % 13 for i in range(260)] + [(3, 1 + i) for i in range(16)] + [(4, dc.DIST_BASE[d]) for d in range(16)]
    s = Stream().dynamic(toks, ll, dl, final=True)
    case("ladder_1_to_15", "codes", s, "build_tables: a set with every code length 1 .. 15, both tables",
         lambda c: {t.code_bits for t in c.cr.trace} == set(range(1, 16)) and {t.dcode_bits for t in c.cr.trace if t.kind == MATCH} == set(range(1, 16)))

    # all 29 length symbols and all 30 distance symbols, extra bits all-zero and all-one; 258 as 285 and as 284 + 31
    def every_symbol():
        t = []
        for i in range(29):
            lo = dc.LEN_BASE[i]
            hi = lo + (1 << dc.LEN_XB[i]) - 1
            for ln in (lo, hi) if i != 27 else (lo, 257):  # 284 + 31 is 258: written by the alt258 blocks
                t += [(ln, 1 + (ln * 7 + i) % 3000), RANDOM[ln] | 1]
        for d in range(30):
            lo = dc.DIST_BASE[d]
            hi = lo + (1 << dc.DIST_XB[d]) - 1
            for k, dist in enumerate((lo, hi)):
                t += [(3 + (d + k) % 6, dist), RANDOM[dist % 999] | 2]
        return t

    def sym_pred(c):
        seen_l, seen_d = set(), set()
        for t in c.cr.trace:
            if t.kind == MATCH:
                s_, ex, xb = dc.length_symbol(t.a)
                seen_l.add((s_, ex == 0, ex == (1 << xb) - 1))
                d_, dex, dxb = dc.dist_symbol(t.b)
                seen_d.add((d_, dex == 0, dex == (1 << dxb) - 1))
        ok_l = all(any(s_ == 257 + i and z for s_, z, o in seen_l) and any(s_ == 257 + i and (o or i == 27) for s_, z, o in seen_l) for i in range(29))
        ok_d = all(any(d_ == i and z for d_, z, o in seen_d) and any(d_ == i and o for d_, z, o in seen_d) for i in range(30))
        return ok_l and ok_d

    def has_284_31(c):  # a match of 258 whose length took 5 extra bits
        return any(t.kind == MATCH and t.a == 258 and t.nbits - t.code_bits - t.dcode_bits - dc.dist_symbol(t.b)[2] == 5 for t in c.cr.trace)
    toks = every_symbol()
    s = Stream().stored(RANDOM[:32768]).fixed(toks).fixed([(258, 32768), 7, (258, 1)], alt258=True, final=True)
    case("every_symbol_fixed", "codes", s, "ll_entry / dist_entry: all 29 length and 30 distance symbols, extra bits 0 and all-one, 258 as 285 and 284+31",
         lambda c: sym_pred(c) and has_284_31(c) and any(t.kind == MATCH and t.a == 258 and t.nbits == 8 + 5 + 5 + 13 for t in c.cr.trace))
    used = {256} | {dc.length_symbol(t[0])[0] for t in toks if type(t) is tuple} | {t for t in toks if type(t) is int} | {284, 7}
    ll = balanced(used, 286)
    dl = balanced(range(30), 30)
    s = Stream().stored(RANDOM[:32768]).dynamic(toks, ll, dl).dynamic([(258, 32768), 7, (258, 2)], ll, dl, alt258=True, final=True)
    case("every_symbol_dynamic", "codes", s, "the same through a dynamic block's tables", lambda c: sym_pred(c) and has_284_31(c))


# ---------------------------------------------------------------- geometry: the 48-bit symbol, literal pairs, token cap, stretches
def _geometry():
    # the longest symbol: 15-bit length code + 5 extra + 15-bit distance code + 13 extra
    ll = make_ll({X: 2, Y: 3, Z: 8, 0x61: 4, 284: 15, 256: 6})
    dl = ladder([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 28, 29], 30)
    big = (258, 32768)  # 284 + 31, distance symbol 29 with 13 extra bits of ones

    def body(pos, out):
        b = Body(pos, out, ll, dl, [X, Y, Z], alt258=True)
        b.pad_to_mod(127).add(big, 0x61)          # last bit in front of a half-segment edge
        b.pad_to_mod(255).add(big, 0x61)          # ... of a segment edge
        b.pad_to_rel(32767).add(big, 0x61)        # ... of the round's edge: lane 127 reads it from the stage's look-ahead
        b.pad_to_mod(127).add(big, 0x61)
        b.pad_to_rel(32767).add(big, 0x61)        # the same in a round whose stage starts in the middle of the block
        b.pad_to_mod(255).add(big)
        return b.toks
    s = Stream().stored(RANDOM[:32768]).dynamic(body, ll, dl, alt258=True, final=True)

    def pred48(c):
        at = rel_starts(c.cr, lambda t: t.kind == MATCH and t.nbits == 48)
        rels = [(ri, r) for ri, r, _ in at]
        return any(r % 256 == 127 for _, r in rels) and any(r % 256 == 255 and r != 32767 for _, r in rels) and (0, 32767) in rels \
            and (1, 32767) in rels and any(ri == 2 for ri, _ in rels) and 32767 + 48 <= 32 * (dc.T * dc.SEG_BITS // 32 + dc.STAGE_LOOKAHEAD_DWORDS)
    case("longest_symbol_at_edges", "geometry", s, "SegBits / decode_segment: a 48-bit symbol starting at the last bit in front of a half-segment, "
         "segment and round edge (= the last lane's look-ahead), in a first and a later round", pred48)

    # the literal pair form: where the second literal may and may not join the first
    ll = wb_ll({0x6C: 12})
    L12 = 0x6C

    def body(pos, out):
        b = Body(pos, out, ll, WB_DL, [X, Y, Z])
        b.add(*DATA * 3)
        for edge in (256, 128):
            b.pad_to_mod(edge - 2, edge).add(X, 0x61)     # the second literal starts exactly at the limit: not paired
            b.pad_to_mod(edge - 3, edge).add(X, 0x62)     # one bit in front of it: paired
            b.pad_to_mod(edge - 4, edge).add(0x63, 0x64)  # the first one ends at the limit
        b.add(0x61, L12, 0x62, (3, 2), 0x63, (258, 5), X, L12, L12, 0x64)  # behind a literal: a long-code literal, a length symbol
        b.pad_to_rel(32768 - 2).add(X, 0x61)                 # the round's limit
        b.pad_to_rel(32768 - 3).add(X, 0x62, 0x61)           # ... ends on: a literal, then end-of-block
        return b.toks
    s = Stream().dynamic(body, ll, WB_DL, final=True)

    def pred_pairs(c):
        tr = c.cr.trace
        at = {m: set() for m in (128, 256, 32768)}
        for ri, r, i in rel_starts(c.cr, lambda t: t.kind == LIT):
            if i and tr[i - 1].kind == LIT and tr[i - 1].start + tr[i - 1].nbits == tr[i].start:
                for m in at:
                    at[m].add(r % m if m < 32768 else r - m)
        seq = [(t.kind, t.code_bits) for t in tr]
        follows = lambda k: any(a[0] == LIT and a[1] <= 10 and k(b) for a, b in zip(seq, seq[1:]))
        rds = [rd for _, rd in all_rounds(c.cr)]
        at_round = any(b.P == a.stage0 + 32768 and tr[b.segs[0].syms[0]].kind == LIT and tr[b.segs[0].syms[0] - 1].kind == LIT for a, b in zip(rds, rds[1:]))
        return all({0, m - 1} <= {x % m for x in at[m]} for m in (128, 256)) and at_round and -1 in at[32768] and \
            follows(lambda b: b[0] == LIT and b[1] > dc.LIT_BITS) and follows(lambda b: b[0] == EOB) and follows(lambda b: b[0] == MATCH)
    case("literal_pairs_at_limits", "geometry", s, "decode_segment FORM 1: b.pos + n < lim, at half-segment, segment and round limits; a literal "
         "followed by a long-code literal, a length symbol, end-of-block", pred_pairs)

    # the token cap: segments of exactly 63, 64 and 65 symbols from codes of 4 bits and fewer
    lits4 = list(range(0x61, 0x61 + 12))
    ll = [0] * 286
    for s_ in lits4 + [257, 256]:
        ll[s_] = 4
    ll[Y] = 3
    assert kraft(ll) == 32768
    dl = [4] * 16

    def body(pos, out):
        b = Body(pos, out, ll, dl, [Y, 0x61])
        b.add(*lits4)
        b.pad_to_mod(0)
        b.add(*[lits4[i % 12] for i in range(64)])                       # 64 x 4 bits
        b.add(*[lits4[i % 12] for i in range(61)], Y, Y, Y, Y)           # 61 x 4 + 4 x 3 bits: 65 symbols
        b.add(*[lits4[i % 12] for i in range(31)], (3, 2), *[lits4[i % 12] for i in range(31)])  # 62 literals and a match of 4 + 4 bits: 63
        b.add(*[lits4[i % 12] for i in range(64)], (3, 1))
        return b.toks
    s = Stream().dynamic(body, ll, dl, final=True)

    def pred_tok(c, ll=ll):
        n = [g.nsym for _, rd in all_rounds(c.cr) for g in rd.segs[: rd.ncommit]]
        return {63, 64, 65} <= set(n) and dc.TOK_CAP == 64 and max(ll) <= 4
    case("token_cap_63_64_65", "geometry", s, "ntok <= kTokCap: segments that leave 63, 64 (kept) and 65 (decoded again) tokens", pred_tok)

    # a 1-bit literal code: 256 symbols a segment, 32768 bytes a round, stretches cut by the 4096-byte cap; a stretch of exactly
    # 4096 bytes, and a lane that would make 4097
    A, B = 0x41, 0x42
    ll = ladder([A, B, 260, 256, 257], 286)  # 1, 2, 3, 4, 4 bits; 260 = length 6
    dl = make_dl({0: 1})

    def body(pos, out):
        b = Body(pos, out, ll, dl, [A, B])
        b.add(*[A] * 32768)                               # a whole round when the body starts on a dword
        b.add(*[A] * (256 * 15), *[A] * 250, B, (6, 1))   # 15 full lanes, then one of 257 bytes in 256 bits
        b.add(*[A] * 600, B, (3, 1))
        return b.toks
    header_bits = Stream().dynamic([], ll, dl).blocks[0].body_bit
    s = _aligner(Stream(), -header_bits % 32, 32).dynamic(body, ll, dl, final=True)  # ... which the block in front arranges
    assert s.blocks[-1].body_bit % 32 == 0

    def pred_1bit(c):
        rds = [rd for _, rd in all_rounds(c.cr)]
        full = [rd for rd in rds if sum(g.nbytes for g in rd.segs) == 32768 and all(g.nsym == 256 for g in rd.segs)]
        cuts = [(rd.segs[st.k1].off + rd.segs[st.k1].nbytes - rd.segs[st.k0].off) for rd in rds for st in rd.stretches if st.k1 < rd.ncommit]
        return bool(full) and all(len(rd.stretches) == 8 and all(st.nbytes == 4096 for st in rd.stretches) for rd in full) and 4097 in cuts \
            and len(rds) >= 3
    case("one_bit_literals_stretch_fill", "geometry", s, "stretch cuts by kRoundCap: 32768 bytes a round in eight stretches of exactly 4096, and a "
         "cut one lane earlier where the lane would make 4097", pred_1bit)

    # sparse output: 15-bit literals, 17 bytes a segment: the stretch is cut by its 64 segments, not by its bytes
    ll = make_ll({0x20: 1, 256: 2, 0x41: 15, 0x42: 15})

    def body(pos, out):
        b = Body(pos, out, ll, WB_DL, [0x20])
        b.add(*[0x41, 0x42] * 1500)
        return b.toks
    s = Stream().dynamic(body, ll, [0], final=True)
    case("sparse_output_64_segment_cut", "geometry", s, "stretch cut at INQ_WG_STRETCH_SEGS: a round of 128 segments and ~2200 bytes "
         "(a segment holds at least five symbols, so never fewer bytes than segments)",
         lambda c: any(st.k1 - st.k0 == 64 and st.nbytes < 2048 for _, rd in all_rounds(c.cr) for st in rd.stretches))


# ---------------------------------------------------------------- matches: root_match
RM_DISTS, RM_LENS = (1, 2, 3, 4, 5, 8), (3, 4, 5, 7, 8, 258)


def _match_classes(cr):
    """For every match of a committed (not lone) job: (distance, length, where its source lies relative to the job's first byte,
    first / last symbol of its job, ends at the job's end)."""
    res = []
    for bi, rd in all_rounds(cr):
        for k, i0, i1, o, nb, si in dc.jobs(rd):
            if rd.stretches[si].lone:
                continue
            body = [i for i in range(i0, i1) if cr.trace[i].kind != EOB]
            for i in body:
                t = cr.trace[i]
                if t.kind != MATCH:
                    continue
                sp0 = t.out - t.b
                where = "front" if sp0 + t.a <= o else "inside" if sp0 >= o else "straddle"
                st = rd.stretches[si]
                res.append(dict(d=t.b, l=t.a, where=where, first=i == body[0], last=i == body[-1], at_end=t.out + t.a == o + nb,
                                stretch_first=t.out == st.out0, round_first=t.out == rd.out0 and rd.P != cr.blocks[bi].body_bit,
                                block_first=i == cr.blocks[bi].t0, prev=cr.blocks[bi - 1].type if bi else -1, src_before_stretch=sp0 < st.out0))
    return res


def _matches():
    ll = wb_ll()

    def body(pos, out):
        b = Body(pos, out, ll, WB_DL, [X, Y, Z])
        b.add(*DATA * 4)
        k = 0
        for d in RM_DISTS:
            for ln in RM_LENS:
                for lead in (0, 1, d - 1, d, d + 3, 12):  # literals between the job's first byte and the match
                    b.pad_to_mod(0, 128)
                    b.add(*[DATA[(k + j) % 4] for j in range(lead)], (ln, d), DATA[k % 4])
                    k += 1
                # the match as the last symbol of a job: it ends where the half segment ends
                b.add(DATA[k % 4], DATA[(k + 1) % 4])
                r = (-(b.rel + b.cost((ln, d)))) % 128
                while not b.reachable(r):
                    r += 128
                b.pad(r).add((ln, d))
                assert b.rel % 128 == 0
        return b.toks
    s = Stream().stored(RANDOM[:40]).dynamic(body, ll, WB_DL, final=True)

    def pred(c):
        m = _match_classes(c.cr)
        ok = True
        for d in RM_DISTS:
            for ln in RM_LENS:
                mm = [x for x in m if x["d"] == d and x["l"] == ln]
                where = {x["where"] for x in mm}
                ok &= {"inside", "straddle"} <= where and ("front" in where) == (d >= ln)  # (a source that ends in front needs d >= len)
                ok &= any(x["first"] for x in mm) and any(x["last"] and x["at_end"] for x in mm)
        return ok
    case("root_match_grid", "matches", s, "root_match: distances 1,2,3,4,5,8 x lengths 3,4,5,7,8,258, source inside the job's bytes, in front of "
         "them and straddling its first byte; first and last symbol of a job, ending at lane_end (put4's tail)", pred)

    # a source that crosses a stretch start, a round start, a deflate-block edge (previous block stored, fixed, dynamic)
    def edge_body(kind, d, ln):
        def body(pos, out):
            b = Body(pos, out, ll, WB_DL, [X, Y, Z])
            if kind == "stretch":
                b.add(*DATA * 3).pad_to_rel(64 * 256).add((ln, d), *DATA)
            elif kind == "round":
                b.add(*DATA * 3).pad_to_rel(32768).add((ln, d), *DATA)
            else:
                b.add((ln, d), *DATA)
            return b.toks
        return body
    for d in RM_DISTS:
        s = Stream()
        for ln in (3, 8, 258):
            s.dynamic(edge_body("stretch", d, ln), ll, WB_DL)
            s.dynamic(edge_body("round", d, ln), ll, WB_DL)
            s.stored(bytes(RANDOM[100 + d : 110 + d])).dynamic(edge_body("block", d, ln), ll, WB_DL)
            s.fixed(list(RANDOM[200 + d : 209 + d])).dynamic(edge_body("block", d, ln), ll, WB_DL)
            s.dynamic(list(DATA * 3), ll, WB_DL).dynamic(edge_body("block", d, ln), ll, WB_DL)
        s.fixed([1], final=True)

        def pred(c, d=d):
            m = [x for x in _match_classes(c.cr) if x["d"] == d]
            ok = True
            for ln in (3, 8, 258):
                mm = [x for x in m if x["l"] == ln and x["src_before_stretch"] and x["stretch_first"]]
                ok &= any(not x["round_first"] and not x["block_first"] for x in mm) and any(x["round_first"] for x in mm)
                ok &= {0, 1, 2} <= {x["prev"] for x in mm if x["block_first"]}
            return ok
        case(f"root_match_sources_across_edges_d{d}", "matches", s, "root_match: the source crosses a stretch start, a round start, a block edge "
             "behind a stored, a fixed and a dynamic block", pred)


# ---------------------------------------------------------------- distance 32768 and the bytes produced
def _far():
    ll = wb_ll({272: 6})  # 272: lengths 31 .. 34
    dl = make_dl({0: 2, 29: 1, 28: 3, 27: 3})
    for name, pre, lead, dist in (("offset0", 32768, 0, 32768), ("offset1", 32767, 1, 32768), ("d32767", 32768, 1, 32767),
                                  ("d32511", 32768, 0, 32769 - 258)):
        toks = DATA[:lead] + [(258, dist), 0x61, (258, dist), (3, dist), (33, dist)]
        s = Stream().stored(RANDOM[:pre]).dynamic(toks, ll, dl, final=True)

        def pred(c, lead=lead, dist=dist, name=name):
            rd = block_rounds(c.cr, 1)[0]
            t = c.cr.trace[c.cr.blocks[1].t0 + lead]
            # (the source's first byte relative to the stretch, + 32768, is what root_match stores: 0 is its edge)
            return t.kind == MATCH and t.b == dist and t.out - rd.stretches[0].out0 == lead and t.out - dist - rd.stretches[0].out0 + 32768 == \
                {"offset0": 0, "offset1": 1, "d32767": 2, "d32511": 257}[name]
        case(f"distance_{name}", "matches", s, "root_match: source in front of the stretch encoded as sp0 + 32768, at its edge v == 0 and next to it", pred)


# ---------------------------------------------------------------- the lone-lane path: copy_match
LONE_DISTS, LONE_LENS = (1, 2, 3, 7, 8, 9, 15, 16, 17), (3, 15, 16, 17, 258)
LONE_LL = make_ll({285: 1, 0x61: 4, 0x62: 4, 0x63: 4, X: 4, 257: 5, 267: 5, 268: 5, 256: 5, Y: 3})
LONE_DL = make_dl({0: 3, 1: 3, 2: 3, 5: 3, 6: 3, 7: 3, 8: 3, 16: 4})  # ... and 257-384: a distance >= every length


def _lone_body(dists, tail=None, far=None):
    def body(pos, out):
        b = Body(pos, out, LONE_LL, LONE_DL, [X, Y])
        b.add(*[RANDOM[i] & 3 | 0x60 if RANDOM[i] & 3 else X for i in range(330)])
        for d in dists:
            b.pad_to_mod(0)
            grp = [0x61, 0x62, 0x63] + [(ln, d) for ln in LONE_LENS] + [0x62] + [(258, d)] * 16 + [(ln, d) for ln in reversed(LONE_LENS)]
            if far:
                grp += [(258, far), (3, far)]
            b.add(*grp)
        if tail:
            b.pad_to_mod(0).add(0x61, 0x62, 0x63, *[(258, tail)] * 16, (3, 1))
        return b.toks
    return body


def _lone_segments(cr):
    """{(distance, length)} of the matches that a lone lane copies."""
    res, last = set(), None
    for bi, rd in all_rounds(cr):
        for st in rd.stretches:
            if st.lone:
                for i in rd.segs[st.k0].syms:
                    t = cr.trace[i]
                    if t.kind == MATCH:
                        res.add((t.b, t.a))
                        last = t
    return res, last


def _lone():
    s = Stream().dynamic(_lone_body(LONE_DISTS, far=300), LONE_LL, LONE_DL, final=True)
    case("lone_lane_copy_match", "lone", s, "decode_segment MODE 2 / copy_match: one segment of more than 4096 bytes; distances 1,2,3,7,8,9,15,16,17 "
         "and one >= the length, lengths 3,15,16,17,258: the dd == 1 fill, the byte loop's idx wrap and lo/hi split, the 16-byte groups",
         lambda c: {(d, ln) for d in LONE_DISTS for ln in LONE_LENS} | {(300, 258), (300, 3)} <= _lone_segments(c.cr)[0])


def _lone_last():
    # the last match of the call's last block, (3, 1), ends on the output's last byte: copy_match loads 16 bytes from dst - 1, so
    # 16 - 1 - 3 = 12 of them lie behind the output
    s = Stream().dynamic(_lone_body((), tail=3), LONE_LL, LONE_DL, final=True)

    def pred(c):
        seen, last = _lone_segments(c.cr)
        return last is not None and (last.a, last.b) == (3, 1) and last.out + last.a == len(c.cr.output) and c.cr.trace[-2] is last \
            and 16 - last.b - last.a == 12
    case("lone_lane_last_match_ends_the_output", "lone", s, "copy_match: loads 16 bytes from src whatever the distance: 12 bytes behind the "
         "output's last byte here, the most a short-period match can reach (the output buffers carry 64 bytes of slack: span.hip kPad)", pred)


# ---------------------------------------------------------------- sizes
def _sizes():
    case("isize0_fixed", "sizes", Stream().fixed([], final=True), "a block of end-of-block only", lambda c: c.isize == 0 and len(c.cr.trace) == 1)
    ll = [0] * 257
    ll[256] = 1
    case("isize0_dynamic_single_code", "sizes", Stream().dynamic([], ll, [0], final=True),
         "build_tables: an incomplete literal/length set of a single 1-bit code is legal",
         lambda c, ll=ll: c.isize == 0 and kraft(ll) == 16384 and len(c.cr.trace) == 1)
    s = Stream().stored(RANDOM[:65535]).stored(RANDOM[65535:65536], final=True)
    case("isize65536_two_stored", "sizes", s, "stored blocks of 65535 and 1 bytes: isize 65536", lambda c: c.isize == 65536 and len(c.payload) > 65536)
    ll = balanced([0x55, 285, 257, 256], 286)
    s = Stream().dynamic([0x55] + [(258, 1)] * 254 + [(3, 1)], ll, make_dl({0: 1}), final=True)
    case("isize65536_one_dynamic", "sizes", s, "one dynamic block inflating to 65536 bytes", lambda c: c.isize == 65536)
    toks = list(RANDOM[:300]) + [(20, 200), (9, 1)]
    cr = Stream().fixed(toks, final=True).finish()
    case("isize_one_less", "rejects", cr, "L.out != isize / tot_b > isize - out0", lambda c: c.cr.replay_ok and c.isize == len(c.cr.output) - 1, valid=False,
         isize=len(cr.output) - 1)
    case("isize_one_more", "rejects", cr, "L.out != isize", lambda c: c.cr.replay_ok and c.isize == len(c.cr.output) + 1, valid=False, isize=len(cr.output) + 1)
    case("isize_exact_neighbour", "rejects", cr, "the same stream with its own isize", lambda c: c.isize == len(c.cr.output))


# ---------------------------------------------------------------- block sequences
def _aligner(s, want, mod):
    """A fixed block of literals after which the next header starts at `want` modulo `mod` bits."""
    for n9 in range(0, 33):
        for n8 in range(0, 5):
            if (s.pos + 10 + 9 * n9 + 8 * n8) % mod == want:
                return s.fixed([0x90 + i for i in range(n9)] + [0x41 + i for i in range(n8)])
    raise AssertionError((want, mod))


def _blocks():
    ll = balanced([0x61, 0x62, 0x63, 257, 256], 286)
    dl = make_dl({1: 1})
    s = Stream()
    s.fixed(list(b"start"))
    for m in range(32):
        _aligner(s, m % 8, 8)
        s.stored(RANDOM[m : m + (0, 1, 7, 300)[m % 4]])        # a stored block behind every bit alignment 0 .. 7; lengths 0 and 1 among them
        _aligner(s, m, 32)
        s.dynamic([0x61, 0x62, 0x63, (3, 2), 0x61 + m % 3], ll, dl)  # a dynamic header at every bit offset 0 .. 31 of a dword
    s.fixed([0x45], final=True)

    def pred(c):
        b = c.cr.blocks
        dyn = {x.header_bit % 32 for x in b if x.type == 2}
        sto = {x.header_bit % 8 for x in b if x.type == 0}
        slen = {(x.end_bit - x.body_bit) // 8 for x in b if x.type == 0}
        return len(b) >= 40 and dyn == set(range(32)) and sto == set(range(8)) and {0, 1} <= slen and [x.final for x in b] == [0] * (len(b) - 1) + [1]
    case("block_cycle_every_header_offset", "blocks", s, "the block loop: 129 deflate blocks in one BGZF block, stored / fixed / dynamic in turn, a dynamic "
         "header at every bit offset 0-31, a stored block behind every bit alignment 0-7, lengths 0 and 1", pred)

    # the final bit on a block that is not the last: what lies behind it is ignored
    s = Stream().fixed(list(b"kept")).dynamic([0x61, 0x62, (3, 2)], ll, dl, final=True).fixed(list(b"ignored")).stored(b"xyz", final=True)
    case("final_bit_before_more_blocks", "blocks", s, "L.last: the stream ends at the first final block; the bytes behind it are not looked at",
         lambda c: [b.final for b in c.cr.blocks] == [0, 1, 0, 1] and c.cr.output == b"keptababa")

    # the stream's end against the payload's end
    for want in range(8):       # ... so that the last block ends on a byte's last bit
        s = Stream().fixed(list(b"end"))
        _aligner(s, want, 8)
        cr = s.dynamic([0x61, 0x62], balanced([0x61, 0x62, 0x63, 256], 257), [0], final=True).finish()
        if cr.nbits % 8 == 0:
            break
    on_last_bit = lambda c: c.cr.nbits % 8 == 0 and c.cr.nbits == 8 * len(c.cr.payload)
    case("stream_ends_on_last_bit", "blocks", cr, "L.P > payload_bits: a stream that ends on the payload's last bit", on_last_bit)
    case("garbage_byte_behind_stream", "blocks", cr, "a byte behind the stream's end is not looked at",
         lambda c: on_last_bit(c) and c.payload == c.cr.payload + b"\xff", payload=cr.payload + b"\xff")
    case("last_byte_cut", "rejects", cr, "INPUT_OVERRUN: the same stream without its last byte",
         lambda c: on_last_bit(c) and c.payload == c.cr.payload[:-1], valid=False, payload=cr.payload[:-1])
    case("last_byte_cut_neighbour", "rejects", cr, "the uncut stream", on_last_bit)


# ---------------------------------------------------------------- dynamic headers
def _rle(seq):
    """A plain run-length coding of code lengths, the way encoders do it (runs do not cross anything on purpose)."""
    out, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        n, v = j - i, seq[i]
        if v == 0:
            while n >= 11:
                k = min(n, 138)
                out.append((18, k - 11))
                n -= k
            if n >= 3:
                out.append((17, n - 3))
                n = 0
            out += [(0, 0)] * n
        else:
            out.append((v, 0))
            n -= 1
            while n >= 3:
                k = min(n, 6)
                out.append((16, k - 3))
                n -= k
            out += [(v, 0)] * n
        i = j
    return out


def _slices(c, bi=0):
    """The 32-bit slices of the block's code-length sequence, as header_lengths_wg deals them: the symbols starting in each."""
    b = c.cr.blocks[bi]
    sl = {}
    for t in c.cr.cl_trace[b.c0 : b.c1]:
        sl.setdefault((t.start - b.cl_bit) // dc.HEADER_SLICE_BITS, []).append(t)
    return b, sl


def _headers():
    body = [0x01, 0x02, 0x03, 0xFF, 0x80]
    # the smallest HCLEN that carries a complete set: 4 fields are 16, 17, 18, 0 - lengths of zero only, no end-of-block code -, the
    # fifth is 8: symbols 1 .. 256 at 8 bits
    ll = [0] + [8] * 256
    cl = [0] * 19
    cl[0], cl[8] = 1, 1
    s = Stream().dynamic(body, ll, [0], cl_lens=cl, final=True)
    case("hclen_smallest", "headers", s, "header_cl_lens: HCLEN = 5, fields beyond it zero", lambda c: c.cr.blocks[0].hclen == 5)
    # HCLEN 19, code-length codes of 1 .. 7 bits
    ll = [6, 7, 7] + [8] * 247 + [0] * 6 + [9, 9]
    assert kraft(ll) == 32768
    dlx = [0] * 12
    cl = [0] * 19
    for n, sy in zip((1, 2, 3, 4, 5, 6, 7, 7), (8, 0, 18, 17, 16, 7, 9, 6)):
        cl[sy] = n
    s = Stream().dynamic(body[:3], ll, dlx, cl_syms=_rle(ll) + [(0, 0)] + _rle(dlx[1:]), cl_lens=cl, final=True)
    case("cl_codes_1_to_7_bits", "headers", s, "header_cl_table / cl_walk: code-length codes of every length 1 .. 7",
         lambda c, cl=cl: {n for n in cl if n} == set(range(1, 8)) and {t.sym for t in c.cr.cl_trace} >= {8, 0, 18, 17, 16, 7, 9, 6})
    ll = [0] * 286
    for i in range(1, 255):
        ll[i] = 8
    for i in (255, 256, 257):
        ll[i] = 10
    ll[258] = 11
    ll[259] = 12
    ll[260] = 13
    ll[261] = 14
    ll[262] = ll[263] = 15
    ll[0] = ll[264] = 9
    assert kraft(ll) == 32768
    cl = balanced([0, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18], 19)
    s = Stream().dynamic(body[:3], ll, [0], cl_syms=_rle(ll + [0]), cl_lens=cl, final=True)
    case("hclen_19", "headers", s, "header_cl_lens: all 19 fields (symbol 15 is the last in the order)", lambda c: c.cr.blocks[0].hclen == 19)

    # runs that cross from the literal/length lengths into the distance lengths
    ll = [0] + [8] * 254 + [0] + [9, 9, 9, 9]            # ... 256, 257, 258, 259 at 9 bits
    assert kraft(ll) == 32768
    dl = [9, 9, 8, 7, 6, 5, 4, 3, 2, 1]
    seq = _rle(ll[:-1]) + [(16, 0)] + [(n, 0) for n in dl[2:]]  # "copy 9 three times": ll[259], dl[0], dl[1]
    s = Stream().dynamic([1, 2, (3, 1), (4, 2), 3], ll, dl, cl_syms=seq, final=True)

    def crosses(sym):
        def pred(c):
            hlit = 257 + (c.cr.payload[0] >> 3 & 31)
            return any(t.sym == sym and t.index < hlit < t.index + (3 + t.extra if sym == 16 else 11 + t.extra) for t in c.cr.cl_trace)
        return pred
    case("run16_crosses_hlit", "headers", s, "cl_walk FINAL: idx + r < hlit inside a 'copy previous' run", crosses(16))
    ll = [8] * 254 + [9] * 4 + [0] * 28
    dl = [0, 0, 0, 0, 1]
    seq = _rle(ll[:258]) + [(18, 28 + 4 - 11)] + [(1, 0)]
    s = Stream().dynamic([1, 2, 3, 4, 5, (3, 5), 3], ll, dl, cl_syms=seq, final=True)
    case("run18_crosses_hlit", "headers", s, "cl_walk: a zero run from the last literal/length slots into the distance lengths", crosses(18))

    # one length, then 43 x symbol 16 at one bit: lanes whose slice holds nothing but "copy the previous length"
    ll = [8] * 254 + [9] * 4
    assert kraft(ll) == 32768
    cl = [0] * 19
    cl[16], cl[8], cl[9], cl[0], cl[18] = 1, 2, 3, 4, 4
    seq = [(8, 0)] + [(16, 3)] * 41 + [(16, 1), (16, 0)] + [(9, 0)] * 4 + [(0, 0)]
    s = Stream().dynamic(body, ll, [0], cl_syms=seq, cl_lens=cl, final=True)

    def pred16(c):
        b, sl = _slices(c)
        only16 = [k for k in sorted(sl) if all(t.sym == 16 for t in sl[k])]
        run = max(sum(1 for _ in g) for g in _groups(only16)) if only16 else 0
        return run >= 3 and sum(t.sym == 16 for t in c.cr.cl_trace) >= 40
    case("forty_three_sym16", "headers", s, "header_lengths_wg: last_sh looked up across lanes that leave no length of their own (kNoLast)", pred16)

    # symbol 18 with its 7 extra bits split by a slice edge
    ll = [0] * 286
    ll[256] = 2
    ll[65] = 1
    ll[200] = 3
    ll[285] = 3
    cl = balanced([0, 1, 2, 3, 18], 19)  # 3 x 2 bits, 2 x 3 bits
    for lead in range(0, 12):
        seq = [(0, 0)] * lead + [(18, 65 - lead - 11)] + [(1, 0)] + [(18, 200 - 66 - 11)] + [(3, 0)] + [(18, 44)] + [(2, 0)] + [(18, 17)] + [(3, 0), (0, 0)]
        cr = Stream().dynamic([65, 200, 65], ll, [0], cl_syms=seq, cl_lens=cl, final=True).finish()
        b = cr.blocks[0]
        split = [t for t in cr.cl_trace if t.sym == 18 and (t.start + t.nbits - 7 - b.cl_bit) // 32 != (t.start + t.nbits - 1 - b.cl_bit) // 32
                 and (t.start + t.nbits - 7 - b.cl_bit) % 32 != 0]
        if split:
            break
    case("sym18_extra_bits_split", "headers", cr, "cl_walk: the 7 extra bits of symbol 18 lie on both sides of a 32-bit slice edge",
         lambda c, split=split: bool(split))

    # the longest header: 286 + 30 lengths, each sent singly through a 7-bit code: 316 x 7 = 2212 bits
    ll = [8] * 226 + [9] * 60
    dl = [4, 4] + [5] * 28
    assert kraft(ll) == 32768 and kraft(dl) == 32768
    cl = [0] * 19
    for n, sy in zip((1, 2, 3, 4, 5, 7, 7, 7, 7), (0, 16, 17, 18, 1, 8, 9, 4, 5)):
        cl[sy] = n
    assert kraft(cl) == 32768
    toks = [0, 225, 226, 255, (258, 1), (3, 2), (4, 3), 17]
    longest = lambda c, bi: c.cr.blocks[bi].body_bit - c.cr.blocks[bi].cl_bit == 2212 and c.cr.blocks[bi].hclen == 18
    s = Stream().dynamic(toks, ll, dl, cl_lens=cl, final=True)
    case("longest_header", "headers", s, "header_lengths_wg: the 2212-bit code-length sequence (70 lanes)", lambda c: longest(c, 0))
    s = Stream().fixed([0x90 + i for i in range(5)] + [0x41])
    s.dynamic(toks, ll, dl, cl_lens=cl, final=True)
    case("longest_header_at_bit_31", "headers", s, "the same header starting at bit 31 of a dword",
         lambda c: longest(c, 1) and c.cr.blocks[1].header_bit % 32 == 31)

    # accepts that sit next to rejects
    def _dist_sent(c):
        return dc.sent_lengths(c.cr, 0)[257 + dc.header_fields(c.cr, 0)["hlit"] :]

    def _raw_behind_257(c, bit):  # the body's fifth symbol is the raw bit, behind a length symbol 257
        t = c.cr.trace
        return (t[3].kind, t[3].a, t[4].kind, t[4].nbits) == (dc.OTHER, 257, dc.OTHER, 1) and dc.bits(c.payload, t[4].start, 1) == bit
    ll = balanced([0x61, 0x62, 257, 256], 286)
    d1 = [0, 0, 1]  # one distance code of one bit (distance 3): the pattern 0 is it, the pattern 1 is no code
    s = Stream().dynamic([0x61, 0x62, 0x61, (3, 3)], ll, d1, final=True)
    case("single_distance_code_bit0", "headers", s, "an incomplete distance set of one 1-bit code: its pattern 0", 
         lambda c: _dist_sent(c) == [0, 0, 1] and c.cr.trace[3].dcode_bits == 1
         and dc.bits(c.payload, c.cr.trace[3].start + c.cr.trace[3].code_bits, 1) == 0)
    s = Stream().dynamic([0x61, 0x62, 0x61, LL(257), Raw(1, 1), 0x61], ll, d1, final=True)
    case("single_distance_code_bit1", "rejects", s, "the same set, pattern 1: not a code",
         lambda c: _dist_sent(c) == [0, 0, 1] and _raw_behind_257(c, 1), valid=False, isize=6)
    s = Stream().dynamic([0x61, 0x62, 0x61], ll, [0], final=True)
    case("no_distance_code_literals_only", "headers", s, "an empty distance set under a body without matches",
         lambda c: _dist_sent(c) == [0] and all(t.kind in (LIT, EOB) for t in c.cr.trace))
    s = Stream().dynamic([0x61, 0x62, 0x61, LL(257), Raw(0, 1), 0x61], ll, [0], final=True)
    case("no_distance_code_one_match", "rejects", s, "an empty distance set and a length symbol",
         lambda c: _dist_sent(c) == [0] and _raw_behind_257(c, 0), valid=False, isize=7)


def _groups(xs):
    run = []
    for x in xs:
        if run and x != run[-1] + 1:
            yield run
            run = []
        run.append(x)
    if run:
        yield run


# ---------------------------------------------------------------- rejects
def _rejects():
    good_ll = balanced([0x61, 0x62, 0x63, 257, 256], 286)
    good_dl = [1]
    body = [0x61, 0x62, 0x63, (3, 1), 0x61]
    good = Stream().dynamic(body, good_ll, good_dl, final=True).finish()
    n = len(good.output)

    def rej(name, stream, path, why, isize=n):
        """why: what makes the stream a reject, read back from its payload and trace."""
        case(name, "rejects", stream, path, why, valid=False, isize=isize)
        case(name + "_neighbour", "rejects", good, "a valid block between two rejects", lambda c: True)

    def sets(c, bi=0):
        """(literal/length lengths, distance lengths, header fields) as block bi's header sends them."""
        f = dc.header_fields(c.cr, bi)
        sent = dc.sent_lengths(c.cr, bi)
        return sent[: 257 + f["hlit"]], sent[257 + f["hlit"] :], f

    def sound_except(c, ll_ok=True, dl_ok=True, cl_ok=True):
        """Everything else about the header is in order, so that the named defect alone is what refuses it."""
        ll, dl, f = sets(c)
        return f["type"] == 2 and f["hlit"] <= 29 and f["hdist"] <= 29 and (not cl_ok or kraft(f["cl_lens"]) == 32768) and \
            (not ll_ok or (kraft(ll) == 32768 and ll[256])) and (not dl_ok or dl == [1]) and len(ll) + len(dl) == 258 + f["hlit"] + f["hdist"]

    rej("sym16_first", Stream().dynamic(body, good_ll, good_dl, cl_syms=[(16, 0)] + _rle(good_ll[3:] + good_dl), final=True),
        "cl_walk: 'copy previous' with nothing in front",
        lambda c: (c.cr.cl_trace[0].sym, c.cr.cl_trace[0].index) == (16, 0) and sound_except(c, ll_ok=False) and sets(c)[0][3:] == good_ll[3:])
    seq = _rle(good_ll + good_dl)
    assert seq[-1] == (1, 0) and seq[-2][0] == 18

    def overshoots(c):
        f, t = dc.header_fields(c.cr, 0), c.cr.cl_trace[-1]
        total = 257 + f["hlit"] + 1 + f["hdist"]
        return t.sym == 18 and t.index < total and t.index + 11 + t.extra == total + 1 and kraft(f["cl_lens"]) == 32768
    rej("run_overshoots_by_1", Stream().dynamic(body, good_ll, good_dl, cl_syms=seq[:-2] + [(18, seq[-2][1] + 2)], final=True),
        "cl_walk: idx + rep > total, by one", overshoots)
    no_eob = balanced([0x61, 0x62, 0x63, 257], 286)
    rej("no_code_for_256", Stream().dynamic(body, no_eob, good_dl, final=True, eob=False), "lens[256] == 0: missing end-of-block code",
        lambda c: sets(c)[0][256] == 0 and kraft(sets(c)[0]) == 32768 and sound_except(c, ll_ok=False))
    o = list(good_ll)
    o[0x64] = 1
    rej("oversubscribed_literal_set", Stream().dynamic(body, o, good_dl, final=True), "build_tables: left < 0",
        lambda c: kraft(sets(c)[0]) > 32768 and sets(c)[0][256] and sound_except(c, ll_ok=False))
    o = list(good_ll)
    o[0x61] = 5
    rej("incomplete_literal_set", Stream().dynamic(body, o, good_dl, final=True), "build_tables: left > 0 with a code longer than one bit",
        lambda c: kraft(sets(c)[0]) < 32768 and max(sets(c)[0]) > 1 and sets(c)[0][256] and sound_except(c, ll_ok=False))
    rej("oversubscribed_distance_set", Stream().dynamic(body, good_ll, [1, 1, 1], final=True), "build_tables: distance set, left < 0",
        lambda c: kraft(sets(c)[1]) > 32768 and sound_except(c, dl_ok=False))
    rej("incomplete_distance_set_len2", Stream().dynamic(body, good_ll, [2], final=True), "build_tables: one distance code of length 2",
        lambda c: sets(c)[1] == [2] and sound_except(c, dl_ok=False))
    seq = [(n_, 0) for n_ in good_ll + good_dl]
    c_over = [0] * 19
    c_over[0], c_over[1], c_over[2], c_over[3] = 1, 1, 2, 2
    rej("oversubscribed_cl_code", Stream().dynamic(body, good_ll, good_dl, cl_syms=seq, cl_lens=c_over, final=True), "header_cl_table: left < 0",
        lambda c: kraft(dc.header_fields(c.cr, 0)["cl_lens"]) > 32768 and sound_except(c, cl_ok=False))
    c_inc = [0] * 19
    c_inc[0], c_inc[1], c_inc[2], c_inc[3] = 2, 2, 2, 3
    rej("incomplete_cl_code", Stream().dynamic(body, good_ll, good_dl, cl_syms=seq, cl_lens=c_inc, final=True), "header_cl_table: left > 0",
        lambda c: 0 < kraft(dc.header_fields(c.cr, 0)["cl_lens"]) < 32768 and sound_except(c, cl_ok=False))
    for f in (30, 31):
        ll2 = good_ll + [0] * (257 + f - 286)
        rej(f"hlit_field_{f}", Stream().dynamic(body, ll2, good_dl, final=True), "header_counts: more than 286 literal/length codes",
            lambda c, f=f: dc.header_fields(c.cr, 0)["hlit"] == f and dc.header_fields(c.cr, 0)["hdist"] == 0 and c.payload[0] >> 3 == f)
        dl2 = good_dl + [0] * f
        rej(f"hdist_field_{f}", Stream().dynamic(body, good_ll, dl2, final=True), "header_counts: more than 30 distance codes",
            lambda c, f=f: dc.header_fields(c.cr, 0)["hdist"] == f and dc.header_fields(c.cr, 0)["hlit"] == 29)
    rej("block_type_3", Stream().fixed(body).reserved(final=True), "block type 3",
        lambda c: [dc.header_fields(c.cr, i)["type"] for i in range(2)] == [1, 3] and c.cr.blocks[0].final == 0)
    rej("stored_wrong_nlen", Stream().stored(b"abcdefg", final=True, nlen=0x1234), "stored: LEN / NLEN",
        lambda c: dc.header_fields(c.cr, 0)["len"] == 7 and dc.header_fields(c.cr, 0)["nlen"] == 0x1234 != 7 ^ 0xFFFF, isize=7)

    # the fixed code's patterns that are no symbols
    def lone_other(c, sym, behind):
        """The only symbols of the fixed block that are not literals, matches or end-of-block: `behind`, then `sym`."""
        t = [x for x in c.cr.trace if x.kind == dc.OTHER]
        return dc.header_fields(c.cr, 0)["type"] == 1 and [x.a for x in t] == behind + [sym] and not any(x.kind == MATCH for x in c.cr.trace)
    for sym in (286, 287):
        rej(f"fixed_{sym}", Stream().fixed([0x61, 0x62, LL(sym), 0x63], final=True), "ll_entry: 286 / 287 take part in the fixed code only",
            lambda c, sym=sym: lone_other(c, sym, []) and dc.FIXED_LL[sym] == 8, isize=3)
    for sym in (30, 31):
        rej(f"fixed_distance_{sym}", Stream().fixed([0x61, 0x62, 0x63, LL(257), DS(sym), 0x63], final=True), "dist_entry: 30 / 31",
            lambda c, sym=sym: lone_other(c, sym, [257]), isize=7)

    # a distance one more than the bytes produced: in the first round, in a later round, on the lone-lane path
    def too_far(c, round_index, lone):
        """The stream's last match reaches one byte in front of the output, every other match is legal, and the model puts it in
        round `round_index` of its block, in a stretch that is / is not a lone lane's."""
        tr = c.cr.trace
        i = max(k for k, t in enumerate(tr) if t.kind == MATCH)
        ok = tr[i].b == tr[i].out + 1 and all(t.b <= t.out for t in tr[:i] if t.kind == MATCH)
        for ri, rd in enumerate(block_rounds(c.cr, 0)):
            for st in rd.stretches:
                if any(i in rd.segs[k].syms for k in range(st.k0, st.k1)):
                    return ok and ri == round_index and st.lone == lone and (not lone or rd.segs[st.k0].nbytes > dc.ROUND_CAP)
        return False
    rej("distance_too_far_first_round", Stream().fixed(list(RANDOM[:40]) + [(5, 41)], final=True), "dist > o + nb in the commit",
        lambda c: too_far(c, 0, False), isize=45)
    rej("distance_too_far_later_round", Stream().fixed([b & 0x7F for b in RANDOM[:4200]] + [(5, 4201)], final=True),
        "the same in the block's second round", lambda c: too_far(c, 1, False), isize=4205)
    dl = make_dl({0: 3, 1: 3, 2: 3, 5: 3, 6: 3, 7: 3, 8: 3, 24: 4})

    def lone_far(pos, out):
        b = Body(pos, out, LONE_LL, dl, [X, Y])
        b.add(0x61, 0x62, 0x63).pad_to_mod(0).add(0x61, *[(258, 1)] * 17)
        b.add((3, b.out + 1))
        return b.toks
    cr = Stream().dynamic(lone_far, LONE_LL, dl, final=True).finish()
    rej("distance_too_far_lone_lane", cr, "dist > o + nb on the lone-lane path", lambda c: too_far(c, 0, True), isize=len(cr.output) + 3)


def _build():
    _codes()
    _geometry()
    _matches()
    _far()
    _sizes()
    _blocks()
    _headers()
    _rejects()
    _lone()
    _lone_last()  # the last case of its group: the last block of that call
    return CASES


_CORPUS = _build()


def corpus():
    """Every crafted case, built once when this module is imported."""
    return _CORPUS


IDS = [c.name for c in _CORPUS]


def test_names_are_unique_and_every_group_has_cases():
    assert len(set(IDS)) == len(IDS)
    groups = {c.group for c in _CORPUS}
    assert groups == {"codes", "geometry", "matches", "lone", "sizes", "blocks", "headers", "rejects"}
    assert [c for c in _CORPUS if c.group == "lone"][-1].name == "lone_lane_last_match_ends_the_output"


@pytest.mark.parametrize("c", _CORPUS, ids=IDS)
def test_zlib_gives_the_verdict_the_case_was_built_for(c):
    ok, got = zlib_verdict(c.payload, c.isize)
    assert ok == c.valid, (c.name, "zlib accepts" if ok else "zlib rejects")
    if c.valid:
        assert c.cr.replay_ok and got == c.want and len(c.want) == c.isize


@pytest.mark.parametrize("c", _CORPUS, ids=IDS)
def test_case_reaches_the_path_it_was_built_for(c):
    assert c.predicate(c), (c.name, c.path)


def test_model_constants_are_the_kernels_defaults():
    src = open(os.path.join(ROOT, "inquistr_amd", "csrc", "bgzf_inflate_wg.hip")).read()
    got = dc.kernel_defines(src)
    for name, want in dc.MODEL_DEFINES.items():
        assert got[name] == want, (name, got[name], want)
    # what the model takes from the kernel's text besides the #defines
    assert "T * (int)kSegBits / 32 + 8" in src                       # the stage's look-ahead: STAGE_LOOKAHEAD_DWORDS
    assert "hp + 32u * ((uint32_t)tid + 1u)" in src                  # HEADER_SLICE_BITS
    assert dc.STAGE_LOOKAHEAD_DWORDS == 8 and dc.HEADER_SLICE_BITS == 32


def test_writer_builds_a_64k_block_quickly_and_traces_every_symbol():
    toks = list(RANDOM[:65000])
    s = Stream()
    s.fixed(toks, final=True)
    # bits go to a bytearray as they come: the accumulator never holds more than a few bytes (one growing int would make the
    # build quadratic; linear, it takes about 0.2 s)
    assert s.n < 32 and s.acc.bit_length() <= s.n and len(s.buf) >= len(toks)
    cr = s.finish()
    assert len(cr.trace) == 65001 and cr.trace[0].start == 3 and cr.headers == [0]
    assert all(a.start + a.nbits == b.start for a, b in zip(cr.trace, cr.trace[1:]))
    assert zlib.decompressobj(-15).decompress(cr.payload) == cr.output == bytes(toks)


def test_writer_emits_what_zlib_refuses_without_complaint():
    # checks nothing itself: each of these is built, and each is refused by zlib
    bad = [Stream().reserved(final=True), Stream().stored(b"ab", final=True, nlen=0), Stream().fixed([1], final=True).raw(0x5A5A, 16),
           Stream().dynamic([1], [1, 1, 1] + [0] * 254, [0], final=True, eob=False)]
    for i, s in enumerate(bad):
        cr = s.finish()
        ok, _ = zlib_verdict(cr.payload, 2 if i == 1 else 1)
        assert ok == (i == 2), i  # (raw bits behind a finished stream do not disturb it)


def test_geometry_model_on_a_stream_worked_by_hand():
    """8-bit literals of the fixed code behind a 3-bit header: symbol j starts at bit 3 + 8 j.  Segment 0 holds the 32 symbols
    that start below bit 256 and is entered in its second half at bit 131 with 16 bytes in front; the first round ends with the
    symbol that starts at bit 32763, so the second is staged from dword 1024 and starts at its bit 3; 128 segments of 32 bytes
    are two stretches of 64 segments."""
    cr = Stream().fixed([0x41] * 5000, final=True).finish()
    r0, r1 = dc.rounds(cr, 0)
    g = r0.segs[0]
    assert (r0.P, r0.stage0, g.start, g.nsym, g.nbytes, g.mid, g.mid_bytes, g.mid_sym) == (3, 0, 3, 32, 32, 131, 16, 16)
    assert [(s.k0, s.k1, s.lone, s.out0, s.nbytes) for s in r0.stretches] == [(0, 64, False, 0, 2048), (64, 128, False, 2048, 2048)]
    assert (r0.ncommit, r0.end, r1.P, r1.stage0, r1.out0) == (128, 32771, 32771, 32768, 4096)
    assert r1.segs[r1.ncommit - 1].eob and sum(g.nbytes for g in r1.segs) == 5000 - 4096
    assert [j[1:5] for j in dc.jobs(r0)[:2]] == [(0, 16, 0, 16), (16, 32, 16, 16)]
