"""The random stream behind the reservoir of extract_reads (tr.rs:311-335: rand 0.9's StdRng::seed_from_u64(42).random_range) and the
reservoir itself on loci deeper than 3 x max_depth, on the host: StdRng of trgt_amd/csrc/ingest.hip, run draw by draw through the developer
build's trgt_dev_rng_draws, and the host reader on synthetic BAM files, against the separately written restatement in tests/pyreads.py.

What pins what: the ChaCha block function (pyreads.chacha_block and StdRng::refill) is compared with PUBLISHED vectors
(tests/golden/chacha_vectors.json); the seed expansion, the order of the words and the range sampling are compared between the
implementations only -- no value that rand itself produced is available.  Every branch of the sampler a test relies on is counted in the
mirror and the count asserted, so that a list which does not reach the branch fails instead of passing vacuously.
tests/test_ingest_device_gpu.py runs the same lists and files through DevRng / walk_kernel."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

from bamtools import write_bam, write_fasta

GOLD = os.path.join(os.path.dirname(__file__), "golden")
VECTORS = json.load(open(os.path.join(GOLD, "chacha_vectors.json")))["vectors"]
U64 = 1  # kind of a draw: raw next_u64 (0: range n, or raw next_u32 when n == 0)


# ---- the two native generators and the mirror, draw by draw -----------------------------------------------------------------------------
def native_draws(ns, kinds=None, seed=42, key=None, counter=0, stream=0, rounds=12, device=-1):
    """trgt_dev_rng_draws of trgt_amd/libtrgt_hip_dev.so: device < 0 the host's StdRng, else DevRng in a one-wave kernel on that GPU"""
    from trgt_amd import _lib
    _lib.lib()  # (binds the HIP runtime that torch brought, as every other test does, before the developer library loads)
    L = _lib.dev_lib()
    assert L is not None, "trgt_amd/libtrgt_hip_dev.so is missing: build() makes it"
    L.trgt_dev_rng_draws.restype = C.c_int
    L.trgt_dev_rng_draws.argtypes = [C.c_int32, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    n = np.array([int(x) for x in ns], np.uint64)
    k = None if kinds is None else np.array(kinds, np.uint8)
    kw = None if key is None else np.array(key, np.uint32)
    out = np.zeros(len(n), np.uint64)
    rc = L.trgt_dev_rng_draws(device, seed, None if kw is None else kw.ctypes.data, counter, stream, rounds, len(n), n.ctypes.data,
                              None if k is None else k.ctypes.data, out.ctypes.data)
    assert rc == 0, "trgt_dev_rng_draws: %d" % rc
    return [int(x) for x in out]


def mirror_draws(ns, kinds=None, **kw):
    import pyreads
    rng = pyreads.StdRng(**kw)
    out = []
    for i, n in enumerate(ns):
        if kinds is not None and kinds[i] == U64:
            out.append(rng.next_u64())
        else:
            out.append(rng.random_range(n) if n else rng.next_u32())
    return out, rng


def _vector_words(v):
    if "words_hex" in v:
        return [int(w, 16) for w in v["words_hex"]]
    raw = bytes.fromhex(v["keystream_hex"])
    return list(struct.unpack("<%dI" % (len(raw) // 4), raw[:len(raw) // 4 * 4]))


def vector_args(v):
    return dict(key=[int(w, 16) for w in v["key_words_hex"]], counter=int(v["counter64_hex"], 16), stream=int(v["stream64_hex"], 16), rounds=v["rounds"])


RANGE_LEN = 4096
SEEDS = (42, 0, 0xDEADBEEFCAFEF00D)


def range_lists():
    """(label, list of n, what the mirror must have met) -- the lists of both the host and the device test; lists with an n above
    2^32 - 1 are the host's alone (DevRng is a 32-bit type)"""
    out = []
    for r in (30, 750, 3000):  # the reservoir's own progression: draw k has the range r + k
        out.append(("reservoir%d" % r, [r + k for k in range(RANGE_LEN)], None))
    out.append(("one", [1] * RANGE_LEN, "never"))
    out.append(("two", [2] * RANGE_LEN, "never"))
    for p in (2, 6, 16, 31):  # the low half of the product is a multiple of n: at most 2^32 - n, never above it
        out.append(("pow2_%d" % p, [1 << p] * RANGE_LEN, "never"))
    for n in ((1 << 31) + 1, 3 << 30, (1 << 32) - 1):  # the second draw fires about n / 2^32 of the time
        out.append(("big32_%x" % n, [n] * RANGE_LEN, "often"))
    out.append(("switch_2p32", [1 << 32] * RANGE_LEN, "whole_u32"))   # the inclusive bound is u32::MAX: still the 32-bit sampler, span 0
    out.append(("switch_2p32_1", [(1 << 32) + 1] * RANGE_LEN, "u64"))  # the first range of the 64-bit sampler
    for n in ((1 << 63) + 1, (1 << 64) - 1):
        out.append(("big64_%x" % n, [n] * RANGE_LEN, "often64"))
    rng = np.random.default_rng(3)  # every magnitude mixed with raw words: a draw that reads one word too many or too few shifts all later ones
    mixed = [int(rng.integers(1, 1 << int(rng.integers(1, 33)))) if rng.random() < 0.8 else 0 for _ in range(RANGE_LEN)]
    out.append(("mixed32", mixed, None))
    return out


def check_mirror_met(label, ns, want, m):
    """conditions on the INPUT list (is the branch reached?), asserted in the mirror"""
    if want == "never":
        assert m.second_draws == 0, label
    elif want == "often":
        assert m.second_draws >= 1000 and m.carries >= 1 and m.u64_cases == [0, 0, 0], (label, m.second_draws, m.carries)
    elif want == "often64":
        assert m.second_draws >= 1000 and m.carries >= 1 and sum(m.u64_cases) == len(ns) + m.second_draws, (label, m.second_draws, m.carries)
    elif want == "whole_u32":
        assert m.second_draws == 0 and m.u64_cases == [0, 0, 0] and m.refills == len(ns) // 64, label  # one word per draw
    elif want == "u64":
        assert sum(m.u64_cases) >= len(ns), label


# ---- 1. the block function against published vectors ------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", VECTORS, ids=lambda v: v["name"])
def test_chacha_block_of_the_mirror_matches_the_published_vector(v):
    import pyreads
    a = vector_args(v)
    want = _vector_words(v)
    assert len(want) >= 4
    assert pyreads.chacha_block(a["key"], a["counter"], a["stream"], a["rounds"])[:len(want)] == want


def test_the_fixture_holds_the_round_counts_the_generators_are_checked_at():
    assert sorted({v["rounds"] for v in VECTORS}) == [8, 12, 20] and sum(v["rounds"] == 20 for v in VECTORS) >= 2


@pytest.mark.parametrize("v", VECTORS, ids=lambda v: v["name"])
def test_refill_of_the_host_generator_matches_the_published_vector(v):
    # the key is given directly (no seed expansion); sixteen raw words are the first block of StdRng::refill -- the code every draw runs
    want = _vector_words(v)
    assert native_draws([0] * 16, **vector_args(v))[:len(want)] == want


def test_blocks_of_one_refill_are_consecutive_counters():
    # a refill is four blocks, counter .. counter + 3, and the next refill goes on at counter + 4: 160 raw words against single blocks
    import pyreads
    v = VECTORS[0]
    a = vector_args(v)
    want = [w for b in range(10) for w in pyreads.chacha_block(a["key"], a["counter"] + b, a["stream"], a["rounds"])]
    assert native_draws([0] * 160, **a) == want == mirror_draws([0] * 160, **a)[0]


# ---- 2. the word stream: seed expansion, buffer order, next_u64 -------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_raw_words_host_against_mirror(seed):
    want, m = mirror_draws([0] * 1500, seed=seed)
    assert m.refills == 24 and len(set(want)) > 1400
    assert native_draws([0] * 1500, seed=seed) == want


def u64_pattern():
    # from an empty buffer 32 next_u64 use up one refill: the first refills (case 1), 31 find both words (case 0).  One next_u32 shifts
    # the phase: every 32nd next_u64 then finds ONE word left and straddles the refill (case 2).  Then a random mix.
    kinds = [U64] * (32 * 12) + [0] + [U64] * (32 * 12)
    rng = np.random.default_rng(7)
    kinds += [int(x) for x in rng.integers(0, 2, 600)]
    return kinds


@pytest.mark.parametrize("seed", SEEDS)
def test_interleaved_u32_and_u64_reads_host_against_mirror(seed):
    kinds = u64_pattern()
    want, m = mirror_draws([0] * len(kinds), kinds, seed=seed)
    assert all(c >= 10 for c in m.u64_cases), m.u64_cases  # both words there / none left / one left (the straddle)
    assert max(want) >> 32  # (u64 values)
    assert native_draws([0] * len(kinds), kinds, seed=seed) == want


# ---- 3. range draws ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range_lists(), ids=lambda c: c[0])
def test_range_draws_host_against_mirror(case):
    label, ns, want_met = case
    for seed in SEEDS[:1]:
        want, m = mirror_draws(ns, seed=seed)
        check_mirror_met(label, ns, want_met, m)
        assert all(0 <= x < n for x, n in zip(want, ns) if n)
        got = native_draws(ns, seed=seed)
        assert got == want, (label, seed, next(i for i in range(len(ns)) if got[i] != want[i]))


def test_the_32_bit_sampler_is_chosen_by_the_inclusive_bound():
    # random_range(0..n) samples 0 ..= n - 1 and takes the 32-bit sampler when n - 1 <= u32::MAX: n = 2^32 reads ONE word per draw and
    # returns it as it is; n = 2^32 + 1 reads two.  (The host used to test n itself and took the 64-bit sampler for n = 2^32.)
    raw = native_draws([0] * 64)
    assert native_draws([1 << 32] * 64) == raw
    two = native_draws([(1 << 32) + 1] * 32)
    assert two != raw[:32] and two == mirror_draws([(1 << 32) + 1] * 32)[0]


# ---- 4. the reservoir on synthetic BAM files --------------------------------------------------------------------------------------------
_ACGT = bytes.maketrans(bytes(range(4)), b"ACGT")


def _dna(rng, n):
    return bytes(rng.integers(0, 4, n, dtype=np.uint8)).translate(_ACGT).decode()


KEPT, LOW_RQ, SECONDARY, SUPPLEMENTARY, NO_RQ = "k", "q", "s", "u", "n"


def sprinkle(rng, n_kept, rate=0.15):
    """n_kept records that pass the filters (one in eight without an rq tag) with low-rq / secondary / supplementary ones between them"""
    kinds = []
    for _ in range(n_kept):
        while rng.random() < rate:
            kinds.append(str(rng.choice([LOW_RQ, SECONDARY, SUPPLEMENTARY])))
        kinds.append(NO_RQ if rng.random() < 0.125 else KEPT)
    return kinds


def _record(rng, name, pos, kind, length=None, longest=300):
    length = int(rng.integers(100, longest + 1)) if length is None else length
    shape = int(rng.integers(0, 3))
    if shape == 0 or length < 40:
        cigar = [("M", length)]
    elif shape == 1:
        cigar = [("S", 5), ("=", length - 12), ("X", 1), ("=", 6)]
    else:
        cigar = [("=", length // 2), ("I", 3), ("=", length - length // 2 - 3)]
    qlen = sum(n for c, n in cigar if c in "MIS=X")
    tags = {} if kind == NO_RQ else {"rq": ("f", 0.5 if kind == LOW_RQ else 0.999)}
    flag = {SECONDARY: 256, SUPPLEMENTARY: 2048}.get(kind, 0) | (16 if rng.random() < 0.5 else 0)
    return dict(name=name, tid=0, pos=pos, cigar=cigar, seq=_dna(rng, qlen), flag=flag, tags=tags, qual=[int(x) for x in rng.integers(2, 60, qlen)])


def write_data_set(tmp_path, tag, loci, genome_len=9000, block=0x8000, seed=1, extra=(), longest=300):
    """loci: [(start, end, kinds)] -- the records of a locus start in [start - 90, start + 10), in the order of `kinds` (file order: the
    positions never decrease along the list); extra: ready-made records.  Returns (bam, fasta, bed)."""
    rng = np.random.default_rng(seed)
    fa, bed, bam = (str(tmp_path / (tag + e)) for e in (".fa", ".bed", ".bam"))
    write_fasta(fa, [("chr1", _dna(rng, genome_len))])
    with open(bed, "w") as f:
        for i, (a, b, _) in enumerate(loci):
            f.write("chr1\t%d\t%d\tID=D%d;MOTIFS=CAG;STRUC=(CAG)n\n" % (a, b, i))
    recs = list(extra)
    for li, (a, b, kinds) in enumerate(loci):
        for i, kind in enumerate(kinds):
            recs.append(_record(rng, "L%d_%05d%s" % (li, i, kind), a - 90 + (100 * i) // len(kinds), kind, longest=longest))
    recs.sort(key=lambda r: r["pos"])  # (stable: records at one position stay in list order)
    write_bam(bam, [("chr1", genome_len)], recs, block=block)
    return bam, fa, bed


def mirror_expectation(bam, fa, bed, flank_len=250, min_read_qual=0.98, max_depth=250):
    """per locus: names / clipped bases / rq of the kept reads in slot order, reads seen, reads dropped for quality -- by tests/pyreads.py"""
    import pyreads
    loci = pyreads.read_catalog(bed, pyreads.read_fasta(fa), flank_len)
    records = pyreads.read_bam(bam)
    out = []
    for locus in loci:
        reads, n_filt, n_seen = pyreads.extract_reads_seen(locus, records, flank_len, min_read_qual, max_depth)
        region = (locus.start - 2 * flank_len, locus.end + 2 * flank_len)
        kept = [(r.name, pyreads.clip_to_region(r, region), r.rq) for r in reads]
        kept = [k for k in kept if k[1] is not None]
        out.append(dict(names=[k[0] for k in kept], bases=[k[1] for k in kept], rq=[k[2] for k in kept], n_filt=n_filt, n_seen=n_seen))
    return out


def assert_batch_is_the_mirrors(b, exp, label=""):
    assert b["n_loci"] == len(exp), label
    for l, e in enumerate(exp):
        a, z = int(b["locus_read_begin"][l]), int(b["locus_read_begin"][l + 1])
        assert int(b["n_reads_seen"][l]) == e["n_seen"] and int(b["n_quality_filtered"][l]) == e["n_filt"], (label, l)
        assert [b["read_name"][r] for r in range(a, z)] == e["names"], (label, l)
        assert [bytes(b["read_blob"][int(b["read_off"][r]):int(b["read_off"][r]) + int(b["read_len"][r])]) for r in range(a, z)] == e["bases"], (label, l)
        rq = b["read_qual"][a:z]
        want = np.array([np.nan if q is None else q for q in e["rq"]], np.float64)
        assert np.array_equal(rq, want, equal_nan=True), (label, l)


def depths_of(d):
    r = 3 * d
    return [r - 1, r, r + 1, r + 63, r + 64, r + 65, 10 * d]


def single_locus_cases(tmp_path, d):
    """one locus, `depth` reads that pass the filters with other records sprinkled through both phases: (label, files, parameters)"""
    for depth in depths_of(d):
        rng = np.random.default_rng(1000 * d + depth)
        # (reads of 100 .. 300 bases; 100 .. 130 at the default depth, where seven files hold 8 000 records)
        files = write_data_set(tmp_path, "d%d_%d" % (d, depth), [(3000, 3030, sprinkle(rng, depth))], seed=depth, longest=130 if d >= 250 else 300)
        yield "max_depth %d, %d reads" % (d, depth), files, dict(max_depth=d), depth


def multi_locus_cases(tmp_path):
    rng = np.random.default_rng(77)
    # two deep loci whose fetch windows overlap (each sees the other's reads), then a third deep one, then a shallow one
    yield "two overlapping", write_data_set(tmp_path, "two", [(3000, 3030, sprinkle(rng, 40)), (3200, 3240, sprinkle(rng, 25))]), dict(max_depth=2)
    yield "three deep and a shallow", write_data_set(tmp_path, "three", [(2000, 2030, sprinkle(rng, 60)), (2150, 2190, sprinkle(rng, 33)), (5000, 5010, sprinkle(rng, 45)),
                                                                          (7000, 7020, sprinkle(rng, 4))]), dict(max_depth=3)
    yield "deep then shallow, default depth", write_data_set(tmp_path, "ds", [(3000, 3030, sprinkle(rng, 800)), (6000, 6010, sprinkle(rng, 12))]), dict()


def tile_cases(tmp_path):
    """Shapes that matter to walk_kernel (64 records per tile, filtered / secondary records occupy lanes; everything lies in one bin of
    the index, so record i of the file is lane i % 64) -- the host reader goes through them as well."""
    pads = lambda n: [[LOW_RQ, SECONDARY, SUPPLEMENTARY][i % 3] for i in range(n)]
    for lane in (0, 63, 30):  # the first read beyond the reservoir (21) at this lane of its tile
        p = (lane - 21) % 64
        yield "first draw at lane %d" % lane, write_data_set(tmp_path, "lane%d" % lane, [(3000, 3030, pads(p) + [KEPT] * (21 + 100))]), dict(max_depth=7)
    # a first tile that ends with exactly `reservoir` reads (no draw in it), then two tiles in which every lane draws
    yield "full tiles of draws", write_data_set(tmp_path, "full", [(3000, 3030, [KEPT] * 3 + pads(61) + [KEPT] * 128)]), dict(max_depth=1)
    for d in (20, 21, 22):  # reservoirs of 60, 63 and 66 around the tile of 64 (3 * max_depth is a multiple of 3: 64 and 65 do not exist)
        yield "reservoir %d" % (3 * d), write_data_set(tmp_path, "r%d" % d, [(3000, 3030, [KEPT] * (3 * d + 70))]), dict(max_depth=d)
        yield "reservoir %d filled at a tile's end" % (3 * d), write_data_set(tmp_path, "e%d" % d, [(3000, 3030, pads(-3 * d % 64) + [KEPT] * (3 * d + 70))]), dict(max_depth=d)


def chunked_case(tmp_path):
    """A deep locus just behind a 16 kb boundary of the index.  40 long reads start in front of the boundary and reach the locus (bin 585),
    each followed by a short read that ends in front of the boundary (bin 4681, which a query of the locus does not visit): every long
    read is a chunk of its own.  400 reads behind the boundary (bin 4682) are one more chunk.  4 kb BGZF blocks: about 70 of them."""
    rng = np.random.default_rng(5)
    extra = []
    for i in range(40):
        extra.append(_record(rng, "A%02d" % i, 16264 + 2 * i, LOW_RQ if i % 9 == 4 else KEPT, length=300))
        extra.append(_record(rng, "B%02d" % i, 16264 + 2 * i + 1, KEPT, length=30))
    for i in range(400):
        extra.append(_record(rng, "C%03d" % i, 16384 + i // 10, [KEPT, KEPT, KEPT, SECONDARY, KEPT, LOW_RQ, NO_RQ][i % 7], length=200))
    return "chunks and blocks", write_data_set(tmp_path, "chunks", [(16684, 16714, [])], genome_len=20000, block=0x1000, extra=extra), dict(max_depth=10)


def chunks_and_blocks(bam, beg, end):
    """(chunks of the .bai that a query of [beg, end) on the first contig visits, after merging adjacent ones; BGZF blocks with data they lie in)"""
    from bamtools import reg2bin  # noqa: F401  (the bin numbering of the SAM specification, 5.3)
    idx = open(bam + ".bai", "rb").read()
    n_bin = struct.unpack_from("<i", idx, 8)[0]
    p, bins = 12, {}
    for _ in range(n_bin):
        b, n_chunk = struct.unpack_from("<Ii", idx, p)
        bins[b] = [struct.unpack_from("<QQ", idx, p + 8 + 16 * c) for c in range(n_chunk)]
        p += 8 + 16 * n_chunk
    linear = struct.unpack_from("<%dQ" % struct.unpack_from("<i", idx, p)[0], idx, p + 4)
    min_off = linear[min(beg >> 14, len(linear) - 1)]
    want = [0] + [base + k for shift, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)) for k in range(beg >> shift, ((end - 1) >> shift) + 1)]
    chunks = sorted(c for b in want for c in bins.get(b, []) if c[1] > min_off)
    merged = []
    for a, z in chunks:
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], z)
        else:
            merged.append([a, z])
    raw, coffs, o = open(bam, "rb").read(), [], 0
    while o < len(raw):
        coffs.append(o)
        o += struct.unpack_from("<H", raw, o + 16)[0] + 1
    return len(merged), sum(any(a >> 16 <= c <= z >> 16 for a, z in merged) for c in coffs)


def many_loci_case(tmp_path, n=70):
    """n deep loci in one call (one workgroup each on the device; every locus starts a fresh StdRng(42))"""
    rng = np.random.default_rng(6)
    loci = [(1000 + 400 * i, 1000 + 400 * i + 12, sprinkle(rng, 4 + i % 23)) for i in range(n)]
    return "%d deep loci" % n, write_data_set(tmp_path, "many", loci, genome_len=1000 + 400 * n + 1000), dict(max_depth=1, flank_len=50)


def _host_against_mirror(label, files, kw):
    from trgt_amd import ingest
    bam, fa, bed = files
    rd = ingest.Reader(bam, fa)
    b = rd.batch(bed, threads=2, **kw)
    exp = mirror_expectation(bam, fa, bed, **kw)
    assert_batch_is_the_mirrors(b, exp, label)
    rd.close()
    return b, exp


@pytest.mark.parametrize("d", [1, 10, 250])
def test_reservoir_host_against_mirror(tmp_path, d):
    for label, files, kw, depth in single_locus_cases(tmp_path, d):
        b, exp = _host_against_mirror(label, files, kw)
        assert exp[0]["n_seen"] == depth and len(exp[0]["names"]) == min(depth, 3 * d), label
        assert exp[0]["n_filt"] > 0 or depth < 30, label  # (records that must not draw lie between the others)
        if depth > 3 * d + 60:  # later reads did replace earlier ones, and not all of them did
            first = set(mirror_expectation(*files, max_depth=1 << 20)[0]["names"][:3 * d])
            late = [n for n in exp[0]["names"] if n not in first]
            assert len(late) > 0 and (len(late) < len(exp[0]["names"]) or d == 1), label  # (all three slots of max_depth 1 may be replaced)


def test_reservoir_of_several_loci_host_against_mirror(tmp_path):
    for label, files, kw in multi_locus_cases(tmp_path):
        b, exp = _host_against_mirror(label, files, kw)
        assert sum(e["n_seen"] > 3 * kw.get("max_depth", 250) for e in exp) >= 1, label
    # every locus starts the stream again: two loci of the same depth beyond the reservoir keep the same SLOTS
    files = write_data_set(tmp_path, "same", [(2000, 2030, [KEPT] * 50), (6000, 6030, [KEPT] * 50)])
    b, exp = _host_against_mirror("same depth twice", files, dict(max_depth=4))
    assert [n[3:8] for n in exp[0]["names"]] == [n[3:8] for n in exp[1]["names"]] and exp[0]["names"] != exp[1]["names"]


def test_tile_shapes_host_against_mirror(tmp_path):
    for label, files, kw in tile_cases(tmp_path):
        b, exp = _host_against_mirror(label, files, kw)
        assert exp[0]["n_seen"] > 3 * kw["max_depth"], label


def test_chunked_locus_and_many_loci_host_against_mirror(tmp_path):
    label, files, kw = chunked_case(tmp_path)
    n_chunks, n_blocks = chunks_and_blocks(files[0], 16684 - 250, 16714 + 250)
    assert n_chunks >= 30 and n_blocks >= 30, (n_chunks, n_blocks)  # (a condition on the file: the walk goes from chunk to chunk, block to block)
    b, exp = _host_against_mirror(label, files, kw)
    assert exp[0]["n_seen"] > 300 and exp[0]["n_filt"] > 50 and any(n.startswith("A") for n in exp[0]["names"]) and not any(n.startswith("B") for n in exp[0]["names"])
    label, files, kw = many_loci_case(tmp_path)
    b, exp = _host_against_mirror(label, files, kw)
    assert len(exp) == 70 and all(e["n_seen"] > 3 for e in exp)
