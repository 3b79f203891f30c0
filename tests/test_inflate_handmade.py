"""Both inflate decoders -- the host's (trgt_amd/csrc/inflate_fast.hpp) and the device's (trgt_amd/csrc/inflate_dev.hip, its hand-written
symbol loop and the compiler's) -- on DEFLATE streams built by hand (tests/deflate_builder.py) for the paths zlib's compressor never
emits: distances up to 32 768, the copy routes of the hand-written loop and the hand-overs between them, the far copy left in flight,
lengths either side of the table split, 15-bit codes, literal pairs at the stops, the legal extremes of a block header, odd block
structure, output sizes around every gate, and streams that are wrong in ways a bit flip rarely produces.

Two references that share nothing with the decoders: expand(), the LZ77 expansion of the tokens a stream was written from, and zlib's
inflate of the stream.  A valid stream must be ACCEPTED with exactly those bytes; it may be declined only where the code says it leaves
the class to zlib (a single literal/length code: both decoders; a distance set of exactly one code: the host decoder), and that verdict
is asserted as well.  A malformed stream, or one announced one byte too short or too long, must be declined."""
import ctypes as C
import hashlib
import zlib

import numpy as np
import pytest

import deflate_builder as B

FAMILY_NAMES = list(B.FAMILIES)


def _lib():
    from trgt_amd import _lib
    L = _lib.lib()
    L.trgt_inflate_raw.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32]
    L.trgt_inflate_raw.restype = C.c_int32
    return L


def _fast(L, comp, n_out, mode=0):
    out = np.full(n_out + 16, 0xA5, np.uint8)
    rc = L.trgt_inflate_raw(comp, len(comp), out.ctypes.data, n_out, mode)
    assert (out[n_out:] == 0xA5).all(), "wrote beyond the output"
    return rc, out[:n_out].tobytes()


def test_the_moved_run_of_32_bit_matches_is_the_same_stream():
    # (the digest of the 16 streams of test_inflate.py's regression test, taken from the function that wrote them before it moved here)
    rng = np.random.default_rng(77)
    h = hashlib.sha256()
    for k in range(16):
        h.update(B.run_of_32_bit_matches(k, rng))
    assert h.hexdigest() == RUN_OF_MATCHES_SHA256


RUN_OF_MATCHES_SHA256 = "40226b16efcfacf14c420261a42e2f9505eae3ffe87a36f0210b1f9dce6c13bf"


def test_builder_tables():
    assert B.lsym(3) == (257, 0, 0) and B.lsym(10) == (264, 0, 0) and B.lsym(11) == (265, 0, 1) and B.lsym(50) == (274, 7, 3)
    assert B.lsym(51) == (275, 0, 3) and B.lsym(257) == (284, 30, 5) and B.lsym(258) == (285, 0, 0)
    assert B.dsym(1) == (0, 0, 0) and B.dsym(5) == (4, 0, 1) and B.dsym(24577) == (29, 0, 13) and B.dsym(32768) == (29, 8191, 13)
    assert B.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == {0: (2, 3), 1: (3, 3), 2: (4, 3), 3: (5, 3), 4: (6, 3), 5: (0, 2), 6: (14, 4), 7: (15, 4)}  # RFC 1951 3.2.2
    assert [r[:3] for r in B.rle_symbols([0] * 139 + [5] * 8 + [0] * 3 + [2, 2])] == [(18, 127, 7), (0, 0, 0), (5, 0, 0), (16, 3, 2), (5, 0, 0), (17, 0, 3), (2, 0, 0), (2, 0, 0)]


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_cases_agree_with_zlib(name):
    """the builder itself: zlib inflates every valid case to what expand() says, and takes no malformed one"""
    cases = B.family(name)
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert len(c.stream) > 0 and c.n_out <= 65536
        d = zlib.decompressobj(-15)
        try:
            got = d.decompress(c.stream)
        except zlib.error:
            got = None
        if c.expected is not None:
            assert got is not None and d.eof and got == c.expected and len(got) == c.n_out, c.name
        elif c.announced_wrongly:  # a valid stream of another size
            assert got is not None and d.eof and len(got) in (c.n_out - 1, c.n_out + 1), c.name
        else:
            assert got is None or not d.eof, c.name


def test_the_case_list_is_what_the_families_promise():
    n = {name: len(B.family(name)) for name in FAMILY_NAMES}
    assert 200 <= sum(n.values()) <= 500, n
    tags = [c.tag for name in FAMILY_NAMES for c in B.family(name) if c.tag]
    assert sorted(tags) == ["single_dist", "single_litlen"]
    assert max(len(c.expected) for c in B.family("max_reach")) == 65536 and any(len(c.expected) == 65536 for c in B.family("output_sizes") if c.expected)


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_host_decoder(name):
    L = _lib()
    for c in B.family(name):
        rc, got = _fast(L, c.stream, c.n_out)
        assert rc in (0, 1), c.name
        if c.expected is None:
            assert rc == 0, c.name
            continue
        rcz, gotz = _fast(L, c.stream, c.n_out, mode=1)
        assert rcz == 1 and gotz == c.expected, c.name
        if c.tag is not None:  # a single literal/length code; a distance set of one code (nz == 1): left to zlib
            assert rc == 0, c.name
        else:
            assert rc == 1 and got == c.expected, c.name


def _check_device(cases, got, status, what):
    for c, g, st in zip(cases, got, status):
        if c.expected is None or c.tag == "single_litlen":
            assert st == 0, (what, c.name, int(st))
        else:  # (a distance set of one code included: the device decoder takes it)
            assert st == 1, (what, c.name, int(st))
            if g != c.expected:
                a, b = np.frombuffer(g, np.uint8), np.frombuffer(c.expected, np.uint8)
                diff = np.nonzero(a != b)[0]
                raise AssertionError((what, c.name, "wrong bytes", len(diff), "first at", int(diff[0]), g[diff[0] - 4:diff[0] + 8], c.expected[diff[0] - 4:diff[0] + 8]))


@pytest.mark.gpu
@pytest.mark.parametrize("loop", ["hand-written", "compiler"])
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_device_decoder(name, loop, monkeypatch):
    from trgt_amd import _lib, ingest
    if loop == "compiler":
        monkeypatch.setenv("TRGT_INFLATE_COMPILER_LOOP", "1")
    else:
        monkeypatch.delenv("TRGT_INFLATE_COMPILER_LOOP", raising=False)
    ctx = _lib.Context(0)
    cases = B.family(name)
    got, status = ingest.inflate_blocks(ctx, [c.stream for c in cases], [c.n_out for c in cases])
    _check_device(cases, got, status, "in order")
    # (what a read past the window of compressed bytes finds depends on the neighbours in src: once more with other neighbours)
    back = cases[::-1]
    got, status = ingest.inflate_blocks(ctx, [c.stream for c in back], [c.n_out for c in back])
    _check_device(back, got, status, "reversed")


GUARD = 64


def _inflate_packed(ctx, cases, gap):
    """trgt_inflate_blocks itself, streams and outputs packed without alignment behind one odd byte, `gap` bytes of a pattern between the
    outputs.  The library brings back dst up to the end of the last descriptor, so the last one is an empty stored block (0 bytes of
    output) GUARD bytes behind the last real output: the bytes in front of it come back from the device like every gap.  Asserts that
    every byte outside the announced outputs is untouched; returns (per case the bytes of its output, status)."""
    from trgt_amd import _lib
    L = _lib.lib()
    streams = [c.stream for c in cases] + [b"\x01\x00\x00\xff\xff"]
    n = len(streams)
    src_len = np.array([len(x) for x in streams], np.uint32); dst_len = np.array([c.n_out for c in cases] + [0], np.uint32)
    src_off = (1 + np.concatenate([[0], np.cumsum(src_len[:-1], dtype=np.uint64)])).astype(np.uint64)
    dst_off = (1 + np.concatenate([[0], np.cumsum(dst_len[:-1].astype(np.uint64) + np.uint64(gap))])).astype(np.uint64)
    dst_off[-1] += np.uint64(GUARD - gap)
    end = int(dst_off[-1])  # what the library copies to the device and back: dst[0, end)
    src = np.frombuffer(b"\x5a" + b"".join(streams), np.uint8).copy()
    pattern = ((np.arange(end + GUARD) * 7 + 3) & 0xFF).astype(np.uint8)
    dst = pattern.copy()
    status = np.zeros(n, np.uint8)
    L.trgt_inflate_blocks.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7
    L.trgt_inflate_blocks.restype = C.c_int
    ctx.check(L.trgt_inflate_blocks(ctx.handle, n, src.ctypes.data, src_off.ctypes.data, src_len.ctypes.data, dst.ctypes.data, dst_off.ctypes.data, dst_len.ctypes.data,
                                    status.ctypes.data))
    assert status[-1] == 1
    inside = np.zeros(end + GUARD, bool)
    for o, k in zip(dst_off, dst_len):
        inside[int(o):int(o) + int(k)] = True
    assert not inside[0] and not inside[end - GUARD:].any() and int((~inside[:end]).sum()) == 1 + gap * (len(cases) - 1) + GUARD
    touched = np.nonzero(~inside & (dst != pattern))[0]
    assert touched.size == 0, ("wrote outside the announced outputs", touched[:8], [c.name for c, o in zip(cases, dst_off) if int(o) <= touched[0]][-1])
    return [dst[int(o):int(o) + int(k)].tobytes() for o, k in zip(dst_off[:-1], dst_len[:-1])], status[:-1], src_off, dst_off


@pytest.mark.gpu
def test_device_blocks_packed_without_alignment():
    """the layout the ingestion uses: every stream starts where the one before ends, and so does every output (ingest.inflate_blocks pads
    to 16 / 64); one odd byte in front makes the offsets odd and even in turn.  The byte in front and the bytes behind the last block
    stay as they were"""
    from trgt_amd import _lib
    ctx = _lib.Context(0)
    cases = B.family("copy_geometry")
    got, status, src_off, dst_off = _inflate_packed(ctx, cases, 0)
    assert (src_off & 1).any() and not (src_off & 1).all() and (dst_off & 3).any()
    assert all(int(dst_off[i + 1]) == int(dst_off[i]) + cases[i].n_out for i in range(len(cases) - 1))
    for c, g, st in zip(cases, got, status):
        assert st == 1 and g == c.expected, c.name


@pytest.mark.gpu
@pytest.mark.parametrize("loop", ["hand-written", "compiler"])
def test_device_writes_nothing_beyond_the_announced_size(loop, monkeypatch):
    """the output sizes, rightly and wrongly announced, with GUARD pattern bytes between the outputs (the padding ingest.inflate_blocks
    checks is empty where the announced size is a multiple of 64: 256, 1024, 2048, 4096, 65280, 65536)"""
    from trgt_amd import _lib
    if loop == "compiler":
        monkeypatch.setenv("TRGT_INFLATE_COMPILER_LOOP", "1")
    else:
        monkeypatch.delenv("TRGT_INFLATE_COMPILER_LOOP", raising=False)
    ctx = _lib.Context(0)
    cases = B.family("output_sizes")
    assert {256, 1024, 2048, 4096, 65280, 65536} <= {c.n_out for c in cases if c.expected is None}
    got, status, _, _ = _inflate_packed(ctx, cases, GUARD)
    _check_device(cases, [g if st == 1 else None for g, st in zip(got, status)], status, "guarded")
