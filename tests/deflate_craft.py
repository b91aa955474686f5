"""Token-level DEFLATE writer (RFC 1951) and a model of the inflate kernel's round geometry: test plumbing, pure Python.

The caller decides everything an encoder normally decides: block types and final bits, the code lengths of a dynamic block, the
sequence of code-length symbols that carries them, the code-length code itself, HCLEN, and the body as a list of tokens.  The
writer checks NOTHING: over-subscribed or incomplete sets, a missing end-of-block code, count fields above 29, block type 3,
a stored block with a wrong NLEN and raw bits all come out as asked.  Stream.finish() returns the payload, a trace (start bit,
bit length, first output byte of every body symbol and every code-length symbol), the bit offset of every block header, and
the output of a plain LZ77 replay of the tokens that never goes through zlib.

rounds() replays how inquistr_amd/csrc/bgzf_inflate_wg.hip cuts a Huffman block's bits into rounds, segments, half segments
and stretches, from the trace alone; the coverage claims of tests/test_deflate_craft.py are predicates over it.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field

# ---- the kernel's geometry, written once (tests/test_deflate_craft.py compares them with the kernel's #define defaults)
T = 128             # lanes = segments per round (INQ_WG_T)
SEG_BITS = 256      # compressed bits per segment (INQ_WG_SEGBITS)
ROUND_CAP = 4096    # output bytes a stretch's root array holds (INQ_WG_CAP)
TOK_CAP = 64        # tokens a segment may leave behind (INQ_WG_TOKCAP)
STRETCH_SEGS = 64   # segments per stretch at the most (INQ_WG_STRETCH_SEGS = T / 2)
LIT_BITS = 10       # index bits of the literal/length table (INQ_WG_LITBITS)
DIST_BITS = 8       # index bits of the distance table (INQ_WG_DISTBITS)
STAGE_LOOKAHEAD_DWORDS = 8  # dwords staged behind a round's T segments
HEADER_SLICE_BITS = 32      # bits of the code-length sequence per lane of the header parse
MODEL_DEFINES = {"INQ_WG_T": T, "INQ_WG_SEGBITS": SEG_BITS, "INQ_WG_CAP": ROUND_CAP, "INQ_WG_TOKCAP": TOK_CAP,
                 "INQ_WG_STRETCH_SEGS": STRETCH_SEGS, "INQ_WG_LITBITS": LIT_BITS, "INQ_WG_DISTBITS": DIST_BITS}


def kernel_defines(source: str) -> dict:
    """The `#ifndef X / #define X value` defaults of the kernel's source, evaluated (a value may name an earlier one)."""
    out = {}
    for name, expr in re.findall(r"#ifndef\s+(INQ_WG_\w+)\s*\n\s*#define\s+\1\s+(.+)", source):
        expr = re.sub(r"INQ_WG_\w+", lambda m: str(out[m.group(0)]), expr.split("//")[0].strip())
        assert re.fullmatch(r"[0-9()+\-*/ ]+", expr), expr
        out[name] = int(eval(expr.replace("/", "//")))  # integer arithmetic only, checked above
    return out


# ---- RFC 1951 3.2.5 / 3.2.7
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_XB = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_XB = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_XB = {16: 2, 17: 3, 18: 7}
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32

LIT, MATCH, EOB, OTHER = 0, 1, 2, 3


def length_symbol(n: int, alt258: bool = False):
    """(symbol, extra value, extra bits) of a match length; alt258 writes 258 as 284 + 31."""
    if n == 258 and alt258:
        return 284, 31, 5
    for s in range(28, -1, -1):
        if LEN_BASE[s] <= n:
            return 257 + s, n - LEN_BASE[s], LEN_XB[s]
    raise ValueError(n)


def dist_symbol(d: int):
    for s in range(29, -1, -1):
        if DIST_BASE[s] <= d:
            return s, d - DIST_BASE[s], DIST_XB[s]
    raise ValueError(d)


def canonical(lens):
    """RFC 1951 3.2.2 without its preconditions: (code with its first stream bit lowest, length) per symbol, None for length 0.
    A set that is not a prefix code still gets numbers (taken modulo 2^length)."""
    count = [0] * 17
    for n in lens:
        if n:
            count[n] += 1
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for n in lens:
        if not n:
            out.append(None)
            continue
        c = nxt[n] & ((1 << n) - 1)
        nxt[n] += 1
        out.append((int(format(c, "0%db" % n)[::-1], 2), n))
    return out


def balanced(used, size):
    """Code lengths of a complete set over the symbols in `used` (two at least), as flat as it can be; `size` entries."""
    used = sorted(set(used))
    k = len(used)
    assert k >= 2
    m = k.bit_length() - 1
    short = (1 << (m + 1)) - k  # symbols of m bits; the others take m + 1
    lens = [0] * size
    for i, s in enumerate(used):
        lens[s] = m if i < short else m + 1
    return lens


def kraft(lens):
    """Sum of 2^-length in units of 2^-15: 32768 = complete."""
    return sum(1 << (15 - n) for n in lens if n)


class Raw:
    """Raw bits inside a body (value's lowest bit first)."""
    def __init__(self, value, nbits):
        self.value, self.nbits = value, nbits


class LL:
    """A literal/length symbol by number, with explicit extra bits (286 and 287 of the fixed code, for instance)."""
    def __init__(self, sym, extra=0, xbits=0):
        self.sym, self.extra, self.xbits = sym, extra, xbits


class DS:
    """A distance symbol by number, with explicit extra bits (30 and 31 of the fixed code)."""
    def __init__(self, sym, extra=0, xbits=0):
        self.sym, self.extra, self.xbits = sym, extra, xbits


@dataclass
class Sym:
    start: int   # bit offset in the payload
    nbits: int   # code + extra bits (both halves of a match)
    out: int     # first output byte
    kind: int    # LIT / MATCH / EOB / OTHER
    a: int = 0   # literal value, or match length
    b: int = 0   # match distance
    code_bits: int = 0   # bits of the literal/length code alone
    dcode_bits: int = 0  # bits of the distance code alone


@dataclass
class ClSym:
    start: int
    nbits: int
    index: int   # first code length the symbol writes (its "output byte")
    sym: int
    extra: int


@dataclass
class Block:
    type: int
    header_bit: int
    body_bit: int = 0      # first body symbol (Huffman blocks), first data byte * 8 (stored)
    end_bit: int = 0
    t0: int = 0            # trace[t0:t1] = the block's body symbols, end-of-block included
    t1: int = 0
    c0: int = 0            # cl_trace[c0:c1] = its code-length symbols
    c1: int = 0
    cl_bit: int = 0        # where the code-length sequence starts (dynamic)
    hclen: int = 0
    out0: int = 0
    final: int = 0


@dataclass
class Crafted:
    payload: bytes
    trace: list
    cl_trace: list
    headers: list          # bit offset of every block header
    output: bytes          # the replay; meaningless behind the first thing the replay cannot follow (replay_ok False)
    blocks: list
    replay_ok: bool
    nbits: int             # bits written (the payload is padded with zero bits to a byte)


class Stream:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0
        self.out = bytearray()
        self.trace, self.cl_trace, self.blocks = [], [], []
        self.replay_ok = True
        self.stopped = False  # a final block has been written: what follows is not replayed

    # ---- bits
    @property
    def pos(self):
        return len(self.buf) * 8 + self.n

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        if self.n >= 32:
            k = self.n >> 3
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def raw(self, v, n):
        while n > 0:
            k = min(n, 24)
            self.put(v, k)
            v >>= k
            n -= k
        return self

    def align(self):
        if self.n & 7:
            self.put(0, 8 - (self.n & 7))

    def _flush(self):
        self.align()
        k = self.n >> 3
        self.buf += self.acc.to_bytes(k, "little") if k else b""
        self.acc, self.n = 0, 0

    # ---- blocks
    def _begin(self, btype, final):
        b = Block(btype, self.pos, out0=len(self.out), final=int(bool(final)), t0=len(self.trace), c0=len(self.cl_trace))
        self.blocks.append(b)
        self.put(int(bool(final)), 1)
        self.put(btype, 2)
        return b

    def _end(self, b, final):
        b.end_bit, b.t1, b.c1 = self.pos, len(self.trace), len(self.cl_trace)
        if final:
            self.stopped = True
        return self

    def reserved(self, final=False):
        """Block type 3."""
        return self._end(self._begin(3, final), final)

    def stored(self, data=b"", final=False, nlen=None):
        b = self._begin(0, final)
        self._flush()
        n = len(data)
        self.buf += n.to_bytes(2, "little") + ((n ^ 0xFFFF) if nlen is None else nlen).to_bytes(2, "little")
        b.body_bit = self.pos
        self.buf += data
        if not self.stopped and self.replay_ok:
            self.out += data
        return self._end(b, final)

    def fixed(self, tokens, final=False, alt258=False, eob=True):
        """tokens: literals (int), matches (length, distance), Raw / LL / DS; or a function of (first body bit, bytes produced so
        far) that returns them, for bodies laid out by bit position."""
        b = self._begin(1, final)
        b.body_bit = self.pos
        if callable(tokens):
            tokens = tokens(self.pos, len(self.out))
        self._body(tokens, canonical(FIXED_LL), canonical(FIXED_D), alt258, eob)
        return self._end(b, final)

    def dynamic(self, tokens, ll, dl, cl_syms=None, cl_lens=None, hclen=None, hlit_field=None, hdist_field=None, final=False,
                alt258=False, eob=True):
        """ll / dl: the code lengths as sent (HLIT = len(ll), HDIST = len(dl)); cl_syms: the (symbol, extra) sequence that
        sends them, every length singly if None; cl_lens: the 19 code-length-code lengths, a flat complete code over the
        symbols cl_syms uses if None; hclen: the count of 3-bit fields, the shortest that carries cl_lens if None."""
        b = self._begin(2, final)
        if cl_syms is None:
            cl_syms = [(n, 0) for n in list(ll) + list(dl)]
        if cl_lens is None:
            used = {s for s, _ in cl_syms}
            for spare_sym in (0, 18, 17):  # one symbol alone is no complete code: give codes to symbols the sequence does not use
                if len(used) < 2:
                    used.add(spare_sym)
            cl_lens = balanced(used, 19)
        if hclen is None:
            hclen = 19
            while hclen > 4 and cl_lens[CL_ORDER[hclen - 1]] == 0:
                hclen -= 1
        b.hclen = hclen
        self.put((len(ll) - 257) if hlit_field is None else hlit_field, 5)
        self.put((len(dl) - 1) if hdist_field is None else hdist_field, 5)
        self.put(hclen - 4, 4)
        for i in range(hclen):
            self.put(cl_lens[CL_ORDER[i]], 3)
        b.cl_bit = self.pos
        cc = canonical(cl_lens)
        idx = 0
        for sym, extra in cl_syms:
            code, n = cc[sym]
            xb = CL_XB.get(sym, 0)
            self.cl_trace.append(ClSym(self.pos, n + xb, idx, sym, extra))
            self.put(code, n)
            if xb:
                self.put(extra, xb)
            idx += 1 if sym < 16 else (3 + extra if sym < 18 else 11 + extra)
        b.body_bit = self.pos
        if callable(tokens):
            tokens = tokens(self.pos, len(self.out))
        self._body(tokens, canonical(list(ll) + [0] * (288 - len(ll))), canonical(list(dl) + [0] * (32 - len(dl))), alt258, eob)
        return self._end(b, final)

    def _body(self, tokens, lc, dc, alt258, eob):
        live = not self.stopped
        out, trace, put = self.out, self.trace, self.put
        for t in tokens:
            start = self.pos
            if type(t) is int:
                code, n = lc[t]
                put(code, n)
                trace.append(Sym(start, n, len(out), LIT, t, 0, n))
                if live and self.replay_ok:
                    out.append(t)
            elif type(t) is tuple:
                ln, dist = t
                s, ex, xb = length_symbol(ln, alt258)
                code, n = lc[s]
                put(code, n)
                if xb:
                    put(ex, xb)
                ds, dex, dxb = dist_symbol(dist)
                dcode, dn = dc[ds]
                put(dcode, dn)
                if dxb:
                    put(dex, dxb)
                trace.append(Sym(start, n + xb + dn + dxb, len(out), MATCH, ln, dist, n, dn))
                if live and self.replay_ok:
                    if dist > len(out):
                        self.replay_ok = False  # no defined bytes: only zlib's verdict (a reject) is left to compare
                    elif dist >= ln:
                        p = len(out) - dist
                        out += out[p : p + ln]
                    else:
                        pat = bytes(out[len(out) - dist :])
                        out += (pat * (ln // dist + 1))[:ln]
            elif isinstance(t, Raw):
                self.raw(t.value, t.nbits)
                trace.append(Sym(start, t.nbits, len(out), OTHER))
                self.replay_ok = self.replay_ok and not live
            else:
                code, n = (lc if isinstance(t, LL) else dc)[t.sym]
                put(code, n)
                if t.xbits:
                    put(t.extra, t.xbits)
                trace.append(Sym(start, n + t.xbits, len(out), OTHER, t.sym))
                self.replay_ok = self.replay_ok and not live
        if eob:
            code, n = lc[256]
            self.trace.append(Sym(self.pos, n, len(out), EOB, 0, 0, n))
            put(code, n)

    def finish(self) -> Crafted:
        nbits = self.pos
        self._flush()
        return Crafted(bytes(self.buf), self.trace, self.cl_trace, [b.header_bit for b in self.blocks], bytes(self.out), self.blocks,
                       self.replay_ok, nbits)


# ---------------------------------------------------------------- the kernel's geometry, from the trace
@dataclass
class Seg:
    index: int
    start: int = -1        # where its chain starts, relative to the round's stage bit 0 (-1: no symbol starts in it)
    nsym: int = 0          # symbols that start in it, end-of-block not counted (= the tokens its chain leaves behind)
    nbytes: int = 0
    off: int = 0           # first output byte, relative to the round's
    mid: int = -1          # first symbol start in its second half (may lie behind the segment's end; -1: chain ended before)
    mid_bytes: int = 0     # bytes in front of mid
    mid_sym: int = 0
    eob: bool = False
    syms: list = field(default_factory=list)  # indices into the trace (end-of-block included)


@dataclass
class Stretch:
    k0: int
    k1: int
    lone: bool
    out0: int              # first output byte (absolute)
    nbytes: int


@dataclass
class Round:
    P: int                 # bit the round starts at
    stage0: int            # bit 0 of its stage: P rounded down to a dword
    out0: int
    segs: list
    ncommit: int
    stretches: list
    end: int               # where the next round (or the next header) starts


def rounds(cr: Crafted, bi: int):
    """The rounds the kernel takes over Huffman block `bi` of a VALID stream: a round's stage starts at dword P >> 5, lane k
    owns the symbols that start in stage bits [256 k, 256 k + 256), 128 segments a round, the next round starts where the
    last committed chain ended; stretches are cut in front of the lane whose bytes pass 4096 and after 64 segments, and a
    lane that passes 4096 on its own commits alone."""
    blk = cr.blocks[bi]
    assert blk.type in (1, 2)
    tr = cr.trace
    i, P, out = blk.t0, blk.body_bit, blk.out0
    res = []
    while True:
        stage0 = P & ~31
        segs = [Seg(k) for k in range(T)]
        done, last, end = False, -1, P
        while i < blk.t1:
            s = tr[i]
            k = (s.start - stage0) // SEG_BITS
            if k >= T:
                break
            g = segs[k]
            rel = s.start - stage0
            if g.start < 0:
                g.start = rel
            if g.mid < 0 and rel >= k * SEG_BITS + SEG_BITS // 2:
                g.mid, g.mid_bytes, g.mid_sym = rel, g.nbytes, g.nsym
            g.syms.append(i)
            last, end = k, s.start + s.nbits
            i += 1
            if s.kind == EOB:
                g.eob = done = True
                break
            g.nsym += 1
            g.nbytes += (1 if s.kind == LIT else s.a if s.kind == MATCH else 0)
        ncommit = last + 1
        off = 0
        for g in segs:
            g.off = off
            off += g.nbytes if g.index < ncommit else 0
        st, k0 = [], 0
        while k0 < ncommit:
            k1 = ncommit
            for k in range(k0, ncommit):
                if segs[k].off + segs[k].nbytes - segs[k0].off > ROUND_CAP or k >= k0 + STRETCH_SEGS:
                    k1 = k
                    break
            lone = k1 == k0
            if lone:
                k1 = k0 + 1
            hi = segs[k1].off if k1 < ncommit else off
            st.append(Stretch(k0, k1, lone, out + segs[k0].off, hi - segs[k0].off))
            k0 = k1
        res.append(Round(P, stage0, out, segs, ncommit, st, end))
        out += off
        P = end
        if done or i >= blk.t1:
            return res


def jobs(rd: Round):
    """The commit jobs of a round: (segment, first trace index, end trace index, first output byte, bytes, stretch); two per
    segment, cut where the chain enters the segment's second half."""
    res = []
    for si, st in enumerate(rd.stretches):
        for k in range(st.k0, st.k1):
            g = rd.segs[k]
            body = g.syms
            if not body:
                continue
            if g.mid < 0 or st.lone:
                res.append((k, body[0], body[-1] + 1, rd.out0 + g.off, g.nbytes, si))
            else:
                m = g.mid_sym
                if m:
                    res.append((k, body[0], body[0] + m, rd.out0 + g.off, g.mid_bytes, si))
                if m < len(body):
                    res.append((k, body[0] + m, body[-1] + 1, rd.out0 + g.off + g.mid_bytes, g.nbytes - g.mid_bytes, si))
    return res


# ---------------------------------------------------------------- reading a payload back (what makes a reject a reject)
def bits(payload: bytes, pos: int, n: int) -> int:
    """n bits of the payload from bit `pos`, the first one lowest."""
    return (int.from_bytes(payload[pos >> 3 : (pos + n + 14) >> 3], "little") >> (pos & 7)) & ((1 << n) - 1)


def header_fields(cr: Crafted, bi: int) -> dict:
    """The fields of block bi's header as a decoder reads them from the payload: final, type; for a dynamic block the HLIT,
    HDIST and HCLEN field values and the 19 code-length-code lengths; for a stored block LEN and NLEN."""
    p = cr.blocks[bi].header_bit
    f = dict(final=bits(cr.payload, p, 1), type=bits(cr.payload, p + 1, 2))
    if f["type"] == 2:
        f.update(hlit=bits(cr.payload, p + 3, 5), hdist=bits(cr.payload, p + 8, 5), hclen=bits(cr.payload, p + 13, 4) + 4)
        cl = [0] * 19
        for i in range(f["hclen"]):
            cl[CL_ORDER[i]] = bits(cr.payload, p + 17 + 3 * i, 3)
        f["cl_lens"] = cl
    elif f["type"] == 0:
        q = (p + 3 + 7) // 8 * 8
        f.update(len=bits(cr.payload, q, 16), nlen=bits(cr.payload, q + 16, 16))
    return f


def sent_lengths(cr: Crafted, bi: int) -> list:
    """The code lengths block bi's code-length symbols write, in order (a 'copy previous' in first place copies 0 here)."""
    b, out = cr.blocks[bi], []
    for t in cr.cl_trace[b.c0 : b.c1]:
        if t.sym < 16:
            out.append(t.sym)
        elif t.sym == 16:
            out += [out[-1] if out else 0] * (3 + t.extra)
        else:
            out += [0] * ((3 if t.sym == 17 else 11) + t.extra)
    return out
