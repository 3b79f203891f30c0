"""The library's own DEFLATE decoder (trgt_amd/csrc/inflate_fast.hpp, what ingestion inflates BGZF blocks with) against zlib: every
block of BAM files, streams of all block types and levels, damaged streams (declined or refused, never a wrong result)."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from deflate_builder import run_of_32_bit_matches as _run_of_32_bit_matches


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


def _raw(data, level, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=-15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return c.compress(data) + c.flush()


def _corpus():
    rng = np.random.default_rng(11)
    dna = b"ACGT"
    yield b""
    yield b"A"
    yield b"A" * 70000
    yield bytes(rng.integers(0, 256, 50000, dtype=np.uint8))                      # incompressible: stored blocks
    yield bytes(np.frombuffer(dna, np.uint8)[rng.integers(0, 4, 65000)])          # 2 bits of entropy per byte
    yield (b"CAG" * 7000 + bytes(np.frombuffer(dna, np.uint8)[rng.integers(0, 4, 3000)])) * 2
    yield bytes(rng.integers(0, 4, 60000, dtype=np.uint8)) + bytes(rng.integers(0, 256, 5280, dtype=np.uint8))
    yield bytes((np.arange(65280) % 251).astype(np.uint8))
    yield bytes(rng.choice(np.array([40] * 17 + list(range(2, 40)), np.uint8), 65280))   # binned qualities
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 12)), dtype=np.uint8)) for _ in range(300)]
    yield b" ".join(words[int(i)] for i in rng.integers(0, 300, 9000))[:65280]
    yield bytes(rng.integers(0, 256, 300, dtype=np.uint8)) * 200                  # long matches at distance 300
    # symbol frequencies 2^-k: code lengths up to the limit of 15, so that the header lists all 19 code-length codes (19 x 3 bits)
    skew = np.concatenate([np.full(1 << (17 - k), k, np.uint8) for k in range(18)])
    for lead in (0, 1, 2, 3, 5, 11, 50):
        yield bytes(rng.integers(0, 256, lead, dtype=np.uint8)) + bytes(rng.permutation(skew))[:65000]


def test_streams_of_every_kind_equal_zlib():
    L = _lib()
    n = 0
    for data in _corpus():
        for level in (0, 1, 2, 4, 6, 9):
            for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE):
                comp = _raw(data, level, strategy)
                rc, got = _fast(L, comp, len(data))
                rcz, gotz = _fast(L, comp, len(data), mode=1)
                assert rcz == 1 and gotz == data
                assert rc in (0, 1)
                if rc == 1:
                    assert got == data, (len(data), level, strategy)
                    n += 1
                else:  # declined: only the exceptions the decoder leaves to zlib (a single distance code, ...)
                    assert level > 0 and strategy in (zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_DEFAULT_STRATEGY), (len(data), level, strategy)
    assert n > 200


def test_bam_blocks_equal_zlib(tmp_path):
    from trgt_amd import synth_bam
    L = _lib()
    ds = synth_bam.write_dataset(str(tmp_path / "ds"), n_loci=12, read_len=3000)
    paths = [ds["bam"], os.path.join(os.path.dirname(__file__), "golden", "example", "sample.bam")]
    total = declined = 0
    for path in paths:
        if not os.path.exists(path):
            continue
        raw = open(path, "rb").read()
        p = 0
        while p < len(raw):
            bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
            comp, isize = raw[p + 18:p + bsize - 8], struct.unpack_from("<I", raw, p + bsize - 4)[0]
            want = zlib.decompress(comp, -15)
            assert len(want) == isize
            rc, got = _fast(L, comp, isize)
            total += 1
            declined += rc == 0
            assert rc == 0 or got == want
            p += bsize
    assert total > 20 and declined <= 2  # (the empty end-of-file blocks are fixed-code blocks: taken as well)


def test_damaged_streams_are_never_inflated_wrongly():
    L = _lib()
    rng = np.random.default_rng(5)
    data = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 20000)]) + b"CAG" * 500
    comp = bytearray(_raw(data, 6))
    ok = 0
    for trial in range(400):
        bad = bytearray(comp)
        kind = trial % 4
        if kind == 0:
            bad[int(rng.integers(0, len(bad)))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            bad = bad[:int(rng.integers(1, len(bad)))]                 # cut short
        elif kind == 2:
            bad += bytes(rng.integers(0, 256, 5, dtype=np.uint8))      # trailing bytes: still a complete stream in front
        n_out = len(data) + (0 if kind != 3 else int(rng.integers(-3, 4)))  # kind 3: a wrong announced size
        rc, got = _fast(L, bytes(bad), max(n_out, 0))
        if rc == 1:
            ok += 1
            # whatever it accepts must be what zlib makes of the same bytes, with exactly that size
            d = zlib.decompressobj(-15)
            try:
                ref = d.decompress(bytes(bad))
            except zlib.error:
                ref = None
            assert ref is not None and d.eof and ref == got and len(got) == n_out, (trial, kind)
    assert ok >= 50  # (the trailing-bytes and unchanged cases)


# ---- the device-side decoder (trgt_amd/csrc/inflate_dev.hip, trgt_inflate_blocks): the same vectors through the GPU
@pytest.mark.gpu
def test_device_streams_of_every_kind_equal_zlib():
    from trgt_amd import _lib, ingest
    ctx = _lib.Context(0)
    streams, datas = [], []
    for data in _corpus():
        data = data[:65536]
        for level in (0, 1, 2, 4, 6, 9):
            for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE):
                streams.append(_raw(data, level, strategy)); datas.append(data)
    got, status = ingest.inflate_blocks(ctx, streams, [len(d) for d in datas])
    n_ok = 0
    for g, d, st in zip(got, datas, status):
        assert st in (0, 1)
        if st == 1:
            assert g == d
            n_ok += 1
    assert n_ok >= len(streams) - 8, (n_ok, len(streams))  # (declined: the few streams with an incomplete code it leaves to zlib)


@pytest.mark.gpu
def test_device_bam_blocks_equal_zlib(tmp_path):
    from trgt_amd import _lib, ingest, synth_bam
    ctx = _lib.Context(0)
    ds = synth_bam.write_dataset(str(tmp_path / "ds"), n_loci=40, read_len=3000)
    paths = [ds["bam"], os.path.join(os.path.dirname(__file__), "golden", "example", "sample.bam")]
    streams, want = [], []
    for path in paths:
        raw = open(path, "rb").read()
        p = 0
        while p < len(raw):
            bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
            comp = raw[p + 18:p + bsize - 8]
            streams.append(comp); want.append(zlib.decompress(comp, -15))
            p += bsize
    got, status = ingest.inflate_blocks(ctx, streams, [len(w) for w in want])
    assert len(streams) > 40 and int((status == 0).sum()) <= 2
    for g, w, st in zip(got, want, status):
        assert st == 0 or g == w


@pytest.mark.gpu
def test_device_damaged_streams_are_never_inflated_wrongly():
    from trgt_amd import _lib, ingest
    ctx = _lib.Context(0)
    rng = np.random.default_rng(5)
    data = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 20000)]) + b"CAG" * 500
    comp = bytearray(_raw(data, 6))
    streams, sizes, kinds = [], [], []
    for trial in range(400):
        bad = bytearray(comp)
        kind = trial % 4
        if kind == 0:
            bad[int(rng.integers(0, len(bad)))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            bad = bad[:int(rng.integers(1, len(bad)))]
        elif kind == 2:
            bad += bytes(rng.integers(0, 256, 5, dtype=np.uint8))
        n_out = len(data) + (0 if kind != 3 else int(rng.integers(-3, 4)))
        streams.append(bytes(bad)); sizes.append(max(n_out, 0)); kinds.append(kind)
    got, status = ingest.inflate_blocks(ctx, streams, sizes)
    ok = 0
    for g, st, bad, n_out, kind in zip(got, status, streams, sizes, kinds):
        if st == 1:
            ok += 1
            d = zlib.decompressobj(-15)
            try:
                ref = d.decompress(bad)
            except zlib.error:
                ref = None
            assert ref is not None and d.eof and ref == g and len(g) == n_out, kind
    assert ok >= 50


# ---- a stream built by hand for the window bookkeeping of the device decoder's hand-written loop: after 25 000 stored bytes, 950 matches
#      that take EXACTLY 32 bits each (an 8-bit length code + 3 extra bits, an 8-bit distance code + 13 extra bits) behind 0 .. 15 two-bit
#      literals that set the phase of the bit buffer.  In some phases such a run never refills at a symbol boundary, only between a length
#      and its distance -- the refill that did not ask whether the window of compressed bytes was low until the end of round 6.
#      (deflate_builder.run_of_32_bit_matches: written with the DEFLATE writer of the hand-made streams)
@pytest.mark.gpu
def test_device_run_of_matches_that_refill_only_between_length_and_distance():
    from trgt_amd import _lib, ingest
    ctx = _lib.Context(0)
    rng = np.random.default_rng(77)
    streams = [_run_of_32_bit_matches(k, rng) for k in range(16)]
    want = [zlib.decompress(s, -15) for s in streams]
    assert all(25000 + 35 * 950 <= len(x) <= 65536 for x in want)
    for rep in range(3):  # (what a wrong read past the window finds there varies from launch to launch)
        got, status = ingest.inflate_blocks(ctx, streams, [len(x) for x in want])
        for k, (g, x, st) in enumerate(zip(got, want, status)):
            assert st == 1 and g == x, (rep, k, int(st))
