"""The device inflate on hand-built DEFLATE streams no encoder writes, and its CRC32 pass at every length class.

The streams come from tests/test_deflate_craft.py (corpus()), where zlib's verdict and the kernel path each one reaches are
pinned without a GPU.  Here every group of cases goes through Context.bgzf_inflate in one call, under the three forms of the
kernel: a block zlib accepts must come out with status 0 and zlib's bytes, a block zlib refuses with a status, and the
neighbours of a refused block exact.
"""
import random
import struct
import zlib

import numpy as np
import pytest

from inquistr_amd import hipcall
from tests.test_deflate_craft import corpus, zlib_verdict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[(0, 0, 1), (0, 1, 0), (0, -1, -1)],
                ids=["inflate_wg_literal_pairs", "inflate_wg_no_pairs_commit_from_tokens", "inflate_wg_form_by_the_data"])
def ctx(request):
    """The three forms of the inflate kernel, as in test_gpu_front.py: its symbol loop with and without the second literal per
    peek, its commit decoding again and fed from tokens, and the form chosen from the block headers as the product does."""
    c = hipcall.Context(0)
    c.set_option("inflate_algo", request.param[0])
    c.set_option("inflate_tokens", request.param[1])
    c.set_option("inflate_lit_pairs", request.param[2])
    yield c
    c.close()


def _table(items):
    """items: (payload, isize, crc32 for the trailer) -> (compressed buffer, hand-built block table)."""
    comp, rows, out_off = bytearray(), [], 0
    for payload, isize, crc in items:
        rows.append((len(comp), len(payload), isize, out_off))
        comp += payload + struct.pack("<II", crc, isize)
        out_off += isize
    return bytes(comp), np.array(rows, dtype=hipcall.BGZF_BLOCK_DTYPE)


_VERDICTS = {}


def _verdict(c):
    if c.name not in _VERDICTS:  # zlib's, computed once for the three forms
        _VERDICTS[c.name] = zlib_verdict(c.payload, c.isize)
    return _VERDICTS[c.name]


def _run_group(ctx, group, verify_crc):
    cases = [c for c in corpus() if c.group == group]
    assert cases
    verdicts = [_verdict(c) for c in cases]
    comp, blocks = _table([(c.payload, c.isize, zlib.crc32(got) if ok else 0) for c, (ok, got) in zip(cases, verdicts)])
    ctx.set_option("verify_crc", verify_crc)
    try:
        rc, out, status = ctx.bgzf_inflate(comp, blocks, check=False)
    finally:
        ctx.set_option("verify_crc", 1)
    assert rc in (0, hipcall.INQ_ERR_INFLATE), rc
    for c, (ok, want), b, st in zip(cases, verdicts, blocks, status):
        if ok:
            assert st == 0, (c.name, hex(int(st)), c.path)
            got = out[int(b["out_off"]) : int(b["out_off"]) + int(b["isize"])].tobytes()
            if got != want:
                at = next(i for i in range(len(want)) if got[i] != want[i])
                raise AssertionError((c.name, c.path, "first wrong byte", at, got[at : at + 8], want[at : at + 8]))
        else:
            assert st != 0 and not st & 0x40, (c.name, hex(int(st)), c.path)
    assert rc == (0 if all(ok for ok, _ in verdicts) else hipcall.INQ_ERR_INFLATE)
    return cases, verdicts


@pytest.mark.parametrize("group", ["codes", "geometry", "matches", "lone", "sizes", "blocks", "headers"])
def test_crafted_streams_inflate_to_zlibs_bytes(ctx, group):
    """Valid streams, CRC32 checked against correct trailers.  One launch per group; the groups and what each case reaches are
    listed in tests/test_deflate_craft.py.  ("lone" ends with the block whose last match ends on the call's last output byte.)"""
    cases, verdicts = _run_group(ctx, group, 1)
    assert all(ok for ok, _ in verdicts), [c.name for c, (ok, _) in zip(cases, verdicts) if not ok]


def test_crafted_rejects_report_a_status_and_leave_their_neighbours_exact(ctx):
    """Every stream zlib refuses (bad headers, codes that are none, distances in front of the output, wrong sizes, a cut
    payload) between valid blocks, without the CRC pass, as the fuzz test runs."""
    cases, verdicts = _run_group(ctx, "rejects", 0)
    n_bad = sum(not ok for ok, _ in verdicts)
    assert n_bad >= 27 and len(cases) - n_bad >= 20


# ---------------------------------------------------------------- the CRC32 pass
def _stored(data: bytes) -> bytes:
    """A deflate stream of stored blocks (two where the data is longer than 65535 bytes)."""
    out, parts = b"", [data[:65535], data[65535:]] if len(data) > 65535 else [data]
    for i, p in enumerate(parts):
        out += bytes([1 if i == len(parts) - 1 else 0]) + struct.pack("<HH", len(p), len(p) ^ 0xFFFF) + p
    return out


CRC_LENGTHS = list(range(0, 2081)) + list(range(65519, 65537))


def test_crc32_pass_at_every_length(ctx):
    """bgzf_crc32_kernel splits a block into 16-byte granules per lane, strides of 1024 bytes and a partial tail, then moves every
    lane's register through the zero bytes behind its last granule: every isize 0 .. 2080 (two strides and a tail) and
    65519 .. 65536, random bytes in stored blocks."""
    rng = random.Random(32)
    datas = [rng.randbytes(n) for n in CRC_LENGTHS]
    comp, blocks = _table([(_stored(d), len(d), zlib.crc32(d)) for d in datas])
    rc, out, status = ctx.bgzf_inflate(comp, blocks, check=False)
    assert rc == 0 and not status.any(), [(CRC_LENGTHS[i], hex(int(status[i]))) for i in np.flatnonzero(status)[:8]]
    assert out.tobytes() == b"".join(datas)


# one length per class of the pass: a tail alone; granules and a tail within one stride; whole granules only; the second stride
# begun, with a tail; two whole strides and granules; the largest block with and without a tail
CRC_FLIP_LENGTHS = [13, 1000, 1024, 1041, 2063, 2080, 65519, 65536]
CRC_FLIP_POSITIONS = [0, 15, 16, 17, 1007, 1008, 1023, 1024, 1039, 1040]


def test_crc32_pass_sees_one_flipped_bit_wherever_it_is(ctx):
    """One bit of one byte flipped under a trailer that holds the CRC32 of the unflipped bytes: in the first granules, on both
    sides of a lane's stride and of the wave's, in the last granules and the tail.  Exactly the flipped blocks report 0x40,
    and their bytes are the flipped input."""
    rng = random.Random(33)
    items, want, flipped = [], [], []
    for n in CRC_FLIP_LENGTHS:
        data = rng.randbytes(n)
        for pos in sorted({p for p in CRC_FLIP_POSITIONS + [n - 17, n - 16, n - 1] if 0 <= p < n}):
            bad = bytearray(data)
            bad[pos] ^= 1 << rng.randrange(8)
            items.append((_stored(bytes(bad)), n, zlib.crc32(data)))
            want.append(bytes(bad))
            flipped.append(True)
        items.append((_stored(data), n, zlib.crc32(data)))
        want.append(data)
        flipped.append(False)
    assert sum(flipped) >= 75
    comp, blocks = _table(items)
    rc, out, status = ctx.bgzf_inflate(comp, blocks, check=False)
    assert rc == hipcall.INQ_ERR_INFLATE
    assert [int(s) for s in status] == [0x40 if f else 0 for f in flipped]
    assert out.tobytes() == b"".join(want)
