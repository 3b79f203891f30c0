"""Device-side read ingestion (trgt_ingest_params.ingest_device, trgt_amd/csrc/ingest_dev.hip: CRC-32 of the inflated BGZF blocks, the record
walk of extract_reads, HiFiRead::from_hts_rec, extract_snps_offset, get_meth and clip_to_region as kernels behind the device inflate)
against the host path of the same library, array by array, on: the reference's example data set, the hand-made records of
tests/test_ingest.py (soft clips, = / X / I / D runs, HP, MM / ML on both strands, secondary / supplementary / low-rq records, a second
contig), synthetic data sets of full-length reads, and the reference's own unit-test vectors for clip_to_region / extract_snps_offset /
get_meth written as BAM records (tests/golden/read_kats.json).  The host path itself is pinned by tests/test_ingest.py and
tests/test_read_helper_kats.py (CPU suite)."""
import json
import os
import re
import threading

import numpy as np
import pytest

from bamtools import write_bam, write_fasta

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
EX = os.path.join(GOLD, "example")
KATS = json.load(open(os.path.join(GOLD, "read_kats.json")))


def _same_batches(x, y):
    assert x["n_loci"] == y["n_loci"] and x["n_reads"] == y["n_reads"]
    for k in x:
        if k in ("read_blob_dev", "read_blob_device", "_native"):
            continue
        if isinstance(x[k], np.ndarray):
            assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, k
            assert np.array_equal(x[k], y[k], equal_nan=True) if x[k].dtype.kind == "f" else np.array_equal(x[k], y[k]), k
        elif isinstance(x[k], list):
            assert x[k] == y[k], k


def _both(rd, bed, **kw):
    host = rd.batch(bed, **kw)
    before = rd.device_stats()
    dev = rd.batch(bed, ingest_device=0, **kw)
    after = rd.device_stats()
    assert after["calls"] == before["calls"] + 1
    return host, dev, after["fallbacks"] - before["fallbacks"], after


def test_example_data_set():
    from trgt_amd import ingest
    rd = ingest.Reader(os.path.join(EX, "sample.bam"), os.path.join(EX, "reference.fasta"))
    host, dev, fell_back, st = _both(rd, os.path.join(EX, "repeat.bed"), keep_bam4=1)
    assert not fell_back and st["blocks"] > 0 and host["n_reads"] == 33
    _same_batches(host, dev)
    assert dev["read_blob_device"] == 0 and dev["read_blob_dev"]


def test_hand_made_records_with_every_kind_of_field(tmp_path):
    from trgt_amd import ingest
    from test_ingest import _synthetic
    bam, fa, bed, recs, genome = _synthetic(tmp_path)
    rd = ingest.Reader(bam, fa)
    host, dev, fell_back, _ = _both(rd, bed, threads=2)
    assert not fell_back and host["n_reads"] >= 5 and host["has_meth"].any() and len(host["mismatch_offsets"]) > 0
    _same_batches(host, dev)
    host, dev, fell_back, _ = _both(rd, bed, min_read_qual=0.1, flank_len=100, keep_bam4=1)
    assert not fell_back
    _same_batches(host, dev)


def test_synthetic_data_set_and_the_reads_left_in_hbm(tmp_path):
    from trgt_amd import _lib, ingest, synth_bam
    ds = synth_bam.write_dataset(str(tmp_path / "ds"), n_loci=60, read_len=3000)
    rd = ingest.Reader(ds["bam"], ds["fasta"])
    host, dev, fell_back, st = _both(rd, ds["bed"], keep_bam4=1, keep_native=True)
    assert not fell_back and st["blocks_by_zlib"] == 0 and host["n_reads"] > 1000
    _same_batches(host, dev)
    # the ASCII reads the batch left in HBM, handed to trgt_locus_batch in place of an upload: same results as from the host blob
    from trgt_amd import locus, shard
    ctx = _lib.Context(0)
    want = locus.run_batch(host, locus.Params(), ctx)
    got = locus.run_batch(dev, locus.Params(), ctx, reads_dev=ingest.device_reads(dev))
    assert shard.result_digest(want, 60) == shard.result_digest(got, 60) and int((want.n_alleles == 2).sum()) > 50
    # a second, partial call on the same reader: slots and slabs are reused
    a, b, fell_back, _ = _both(rd, ds["bed"], first_locus=10, max_loci=25)
    assert not fell_back
    _same_batches(a, b)


def test_calls_from_several_threads_overlap_and_agree(tmp_path):
    from trgt_amd import ingest, synth_bam
    ds = synth_bam.write_dataset(str(tmp_path / "ds"), n_loci=80, read_len=2500)
    rd = ingest.Reader(ds["bam"], ds["fasta"])
    want = [rd.batch(ds["bed"], first_locus=a, max_loci=20) for a in range(0, 80, 20)]
    got, errs = [None] * 8, []

    def run(i):
        try:
            got[i] = rd.batch(ds["bed"], first_locus=20 * (i % 4), max_loci=20, ingest_device=0)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=run, args=(i,)) for i in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(8):
        _same_batches(want[i % 4], got[i])
    assert rd.device_stats()["fallbacks"] == 0


def test_a_locus_deeper_than_the_reservoir_is_down_sampled_like_the_host_path(tmp_path):
    # more reads than 3 * max_depth: every further read replaces a random slot, by the same random stream as the host's StdRng(42)
    from trgt_amd import ingest
    from test_ingest import _synthetic
    bam, fa, bed, recs, genome = _synthetic(tmp_path, deep=200)
    rd = ingest.Reader(bam, fa)
    for depth in (10, 20, 50, 250):   # reservoirs of 30, 60, 150 (all smaller than the 201 reads over the second locus) and 750
        host, dev, fell_back, st = _both(rd, bed, max_depth=depth)
        assert not fell_back, st
        _same_batches(host, dev)
        assert int(host["n_reads_seen"][1]) == 201 and int(host["locus_read_begin"][2] - host["locus_read_begin"][1]) <= 3 * depth


# ---- the reservoir's random stream and deep loci: device = host = the Python mirror (the lists and files of tests/test_reservoir_stream.py) ----
def test_block_function_of_the_kernels_generator_matches_the_published_vectors():
    # DevRng::block through the developer build's one-wave kernel, key given directly; the kernel type has no stream id: the vectors with stream 0
    from test_reservoir_stream import VECTORS, _vector_words, native_draws, vector_args
    done = []
    for v in VECTORS:
        a = vector_args(v)
        if a["stream"] == 0:
            want = _vector_words(v)
            assert native_draws([0] * 16, device=0, **a)[:len(want)] == want, v["name"]
            done.append(v["rounds"])
    assert sorted(done) == [8, 12, 20]


def test_raw_words_of_the_kernels_generator_against_the_mirror():
    from test_reservoir_stream import SEEDS, mirror_draws, native_draws
    for seed in SEEDS:
        want, m = mirror_draws([0] * 1500, seed=seed)
        assert m.refills == 24
        assert native_draws([0] * 1500, seed=seed, device=0) == want, seed


def test_range_draws_of_the_kernels_generator_against_the_mirror():
    # every list of the host test whose ranges fit the kernel's 32-bit type; the mirror's counters say that the second draw (and its carry)
    # was met a thousand times in the lists made for it
    from test_reservoir_stream import check_mirror_met, mirror_draws, native_draws, range_lists
    ran = []
    for label, ns, want_met in range_lists():
        if max(ns) > 0xFFFFFFFF:
            continue
        want, m = mirror_draws(ns, seed=42)
        check_mirror_met(label, ns, want_met, m)
        got = native_draws(ns, seed=42, device=0)
        assert got == want, (label, next(i for i in range(len(ns)) if got[i] != want[i]))
        ran.append(want_met)
    assert ran.count("often") == 3 and ran.count("never") >= 6 and len(ran) >= 13


def _deep_three_ways(label, files, kw, monkeypatch):
    """host = mirror, then device = host array by array, with the inflate kernel's own loop and with the compiler's; no call may go back to
    the host path (the comparison would be the host's with itself), and FB_RESERVOIR (3) is a reason the device never gives"""
    from trgt_amd import ingest
    from test_reservoir_stream import assert_batch_is_the_mirrors, mirror_expectation
    bam, fa, bed = files
    exp = mirror_expectation(bam, fa, bed, **kw)
    rd = ingest.Reader(bam, fa)
    host = rd.batch(bed, **kw)
    assert_batch_is_the_mirrors(host, exp, label)
    for compiler_loop in (False, True):
        if compiler_loop:
            monkeypatch.setenv("TRGT_INFLATE_COMPILER_LOOP", "1")
        else:
            monkeypatch.delenv("TRGT_INFLATE_COMPILER_LOOP", raising=False)
        before = rd.device_stats()
        dev = rd.batch(bed, ingest_device=0, **kw)
        st = rd.device_stats()
        assert st["calls"] == before["calls"] + 1 and st["fallbacks"] == 0 and st["last_reason"] == 0 and st["last_reason"] != 3, (label, st)
        _same_batches(host, dev)
        assert_batch_is_the_mirrors(dev, exp, label)
    monkeypatch.delenv("TRGT_INFLATE_COMPILER_LOOP", raising=False)
    rd.close()
    return exp


@pytest.mark.parametrize("d", [1, 10, 250])
def test_reservoir_device_host_and_mirror(tmp_path, monkeypatch, d):
    from test_reservoir_stream import single_locus_cases
    for label, files, kw, depth in single_locus_cases(tmp_path, d):
        exp = _deep_three_ways(label, files, kw, monkeypatch)
        assert exp[0]["n_seen"] == depth and len(exp[0]["names"]) == min(depth, 3 * d), label


def test_reservoir_of_several_loci_device_host_and_mirror(tmp_path, monkeypatch):
    from test_reservoir_stream import multi_locus_cases
    for label, files, kw in multi_locus_cases(tmp_path):
        exp = _deep_three_ways(label, files, kw, monkeypatch)
        assert sum(e["n_seen"] > 3 * kw.get("max_depth", 250) for e in exp) >= 1, label


def test_reservoir_at_every_place_of_a_tile_device_host_and_mirror(tmp_path, monkeypatch):
    # the first read beyond the reservoir at lane 0 / 63 / 30 of walk_kernel's 64-record tile, tiles in which every lane draws behind a tile
    # that ends with exactly `reservoir` reads, reservoirs of 60 / 63 / 66
    from test_reservoir_stream import tile_cases
    n = 0
    for label, files, kw in tile_cases(tmp_path):
        exp = _deep_three_ways(label, files, kw, monkeypatch)
        assert exp[0]["n_seen"] > 3 * kw["max_depth"], label
        n += 1
    assert n == 10


def test_reservoir_across_chunks_and_blocks_and_in_many_workgroups(tmp_path, monkeypatch):
    from test_reservoir_stream import chunked_case, chunks_and_blocks, many_loci_case
    label, files, kw = chunked_case(tmp_path)
    n_chunks, n_blocks = chunks_and_blocks(files[0], 16684 - 250, 16714 + 250)
    assert n_chunks >= 30 and n_blocks >= 30, (n_chunks, n_blocks)  # (ChunkDesc after ChunkDesc, records across BGZF blocks)
    exp = _deep_three_ways(label, files, kw, monkeypatch)
    assert exp[0]["n_seen"] > 300 and any(n.startswith("A") for n in exp[0]["names"]) and any(n.startswith("C") for n in exp[0]["names"])
    label, files, kw = many_loci_case(tmp_path)
    exp = _deep_three_ways(label, files, kw, monkeypatch)
    assert len(exp) == 70 and all(e["n_seen"] > 3 for e in exp)


def test_a_block_with_a_wrong_crc_is_refused(tmp_path):
    from trgt_amd import _lib, ingest, synth_bam
    ds = synth_bam.write_dataset(str(tmp_path / "ds"), n_loci=12, read_len=2000)
    raw = bytearray(open(ds["bam"], "rb").read())
    # the third block's footer: flip one bit of its CRC-32 (the inflated length still fits)
    off = 0
    for _ in range(2):
        off += (raw[off + 16] | (raw[off + 17] << 8)) + 1
    end = off + (raw[off + 16] | (raw[off + 17] << 8)) + 1
    raw[end - 8] ^= 1
    open(ds["bam"], "wb").write(bytes(raw))
    rd = ingest.Reader(ds["bam"], ds["fasta"])
    with pytest.raises(_lib.TrgtHipError, match="CRC-32"):
        rd.batch(ds["bed"], ingest_device=0)
    st = rd.device_stats()
    assert st["fallbacks"] == 1 and st["last_reason"] == 1
    with pytest.raises(_lib.TrgtHipError, match="CRC-32"):  # the host path refuses it as well (htslib does)
        rd.batch(ds["bed"])


def test_an_unusable_ingest_device_fails_the_call(tmp_path):
    from trgt_amd import _lib, ingest, synth_bam
    ds = synth_bam.write_dataset(str(tmp_path / "ds"), n_loci=12, read_len=2000)
    rd = ingest.Reader(ds["bam"], ds["fasta"])
    with pytest.raises(_lib.TrgtHipError, match="ingest_device 99"):
        rd.batch(ds["bed"], ingest_device=99)
    a, b = rd.batch(ds["bed"]), rd.batch(ds["bed"], ingest_device=0)
    _same_batches(a, b)


# ---- branches of the plan (trgt_amd/csrc/ingest_plan.hpp; its values are pinned by tests/tools/ingest_plan_check.cpp) on the device ---------
@pytest.fixture(scope="module")
def far_apart(tmp_path_factory):
    """chr1 with reads over loci A (3000) and A2 (3400), then 165 random 3 kb reads that no locus wants, then reads over locus B (200000); chr2
    is in the FASTA only.  The filler is about 120 kB of compressed BAM (a quarter of a byte per random base), twice the 64 KiB below which two compressed
    ranges merge, and none of its reads crosses a 16 kb boundary (it would land in a bin that the windows of A and B both look into)."""
    d = tmp_path_factory.mktemp("far")
    rng = np.random.default_rng(23)
    n = 230000
    genome = "".join(rng.choice(list("ACGT"), n))
    fa, bam = str(d / "g.fa"), str(d / "r.bam")
    write_fasta(fa, [("chr1", genome), ("chr2", genome[:20000])])

    def rec(name, pos, length):
        return dict(name=name, tid=0, pos=pos, cigar=[("=", length)], seq="".join(rng.choice(list("ACGT"), length)), tags={"rq": ("f", 0.999)})
    recs = [rec("a%d" % i, 2600 + 10 * i, 1000) for i in range(6)]
    recs += [rec("f%d_%d_%d" % (w, k, c), 16384 * w + 100 + 3200 * k, 3000) for w in range(1, 12) for k in range(5) for c in range(3)]
    recs += [rec("b%d" % i, 199600 + 10 * i, 1000) for i in range(4)]
    write_bam(bam, [("chr1", n)], recs)
    beds = {}
    for tag, lines in (("three", [("chr1", 3000, "A"), ("chr1", 3400, "A2"), ("chr1", 200000, "B")]), ("empty", [("chr2", 1000, "N"), ("chr1", 8000, "E")])):
        beds[tag] = str(d / (tag + ".bed"))
        open(beds[tag], "w").write("".join("%s\t%d\t%d\tID=%s;MOTIFS=CAG;STRUC=(CAG)n\n" % (c, s, s + 30, i) for c, s, i in lines))
    return bam, fa, beds


def test_two_compressed_ranges_in_one_call_and_one_range_for_two_loci(far_apart, monkeypatch, capfd):
    from trgt_amd import ingest
    bam, fa, beds = far_apart
    rd = ingest.Reader(bam, fa)
    monkeypatch.setenv("TRGT_INGEST_TRACE", "1")
    host, dev, fell_back, st = _both(rd, beds["three"], keep_bam4=1)
    monkeypatch.delenv("TRGT_INGEST_TRACE")
    assert not fell_back and st["blocks_by_zlib"] == 0
    _same_batches(host, dev)
    assert [int(v) for v in np.diff(host["locus_read_begin"])] == [6, 6, 4]
    # the call's own account: A and A2 share the first range, the filler is not read, B is the second range
    m = re.search(r"device: (\d+) ranges, (\d+) blocks", capfd.readouterr().err)
    assert m and int(m.group(1)) == 2, m
    raw, off, n_blocks = open(bam, "rb").read(), 0, 0
    while off < len(raw):
        off += (raw[off + 16] | (raw[off + 17] << 8)) + 1
        n_blocks += 1
    assert len(raw) > 2 * 0x10000 and n_blocks >= 12 and int(m.group(2)) <= n_blocks // 2


@pytest.mark.parametrize("keep_bam4", [0, 1])
def test_a_batch_without_any_read(far_apart, keep_bam4):
    # a locus on a contig the BAM header lacks (tid -1: no chunks) and one no record overlaps (its chunk is walked, nothing is kept).  A batch
    # with reads goes first and is freed: the empty one gets that slab back, so what it hands out is what it wrote
    from trgt_amd import ingest
    bam, fa, beds = far_apart
    rd = ingest.Reader(bam, fa)
    assert rd.batch(beds["three"], ingest_device=0, keep_bam4=keep_bam4)["n_reads"] == 16
    host, dev, fell_back, _ = _both(rd, beds["empty"], keep_bam4=keep_bam4)
    assert not fell_back and host["n_loci"] == 2 and host["skipped"] == []
    assert dev["n_reads"] == 0 and host["n_reads"] == 0
    _same_batches(host, dev)
    for k in ("mismatch_off", "meth_off", "cigar_off"):
        assert list(dev[k]) == [0], k
    assert list(dev["locus_read_begin"]) == [0, 0, 0] and list(dev["n_reads_seen"]) == [0, 0]
    assert len(dev["read_blob"]) == len(host["read_blob"]) == 1 and int(dev["read_blob"][0]) == 0   # read_bytes: the one NUL of an empty blob
    assert ("read_bam4" in dev) == bool(keep_bam4)
    if keep_bam4:
        assert list(dev["read_bam4"]) == [0] and list(dev["read_bam4_off"]) == [0]


def test_a_freed_batch_gives_its_slab_to_the_next_one(far_apart):
    from trgt_amd import ingest
    bam, fa, beds = far_apart
    rd = ingest.Reader(bam, fa)
    host = rd.batch(beds["three"])
    first = rd.batch(beds["three"], ingest_device=0, keep_native=True)
    _same_batches(host, first)
    slab = first["read_blob_dev"]
    del first["_native"]   # trgt_ingest_free: the lease returns the slab to the reader's pool
    second = rd.batch(beds["three"], ingest_device=0, keep_native=True)
    _same_batches(host, second)
    assert second["read_blob_dev"] == slab and rd.device_stats()["fallbacks"] == 0   # the same piece of the same slab


# ---- the reference's unit-test vectors as BAM records -----------------------------------------------------------------------------------
def _ops(cigar):
    return [(c, int(n)) for n, c in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]


def _mm_for(bases, meth):
    """MM / ML tags (forward strand) that put meth[i] on the i-th CpG of `bases`"""
    cs = [i for i, ch in enumerate(bases) if ch == "C"]
    cpg = [k for k, i in enumerate(cs) if bases[i:i + 2] == "CG"]
    assert len(cpg) == len(meth)
    deltas, last = [], -1
    for k in cpg:
        deltas.append(k - last - 1)
        last = k
    return "C+m?," + ",".join(map(str, deltas)) + ";", list(meth)


def _one_read_data_set(tmp_path, tag, rec, region, flank_len, genome_len=12000):
    rng = np.random.default_rng(11)
    genome = "".join(rng.choice(list("ACGT"), genome_len))
    fa = str(tmp_path / (tag + ".fa"))
    write_fasta(fa, [("chr1", genome)])
    bed = str(tmp_path / (tag + ".bed"))
    open(bed, "w").write("chr1\t%d\t%d\tID=K;MOTIFS=CAG;STRUC=(CAG)n\n" % region)
    bam = str(tmp_path / (tag + ".bam"))
    write_bam(bam, [("chr1", genome_len)], [rec])
    return bam, fa, bed


@pytest.mark.parametrize("case", [c for c in KATS["clip_to_region"] if c["region_end"] - c["region_start"] >= 5],
                         ids=lambda c: "%s-%d-%d" % (c["test"], c["region_start"], c["region_end"]))
def test_clip_to_region_vectors_through_the_device(tmp_path, case):
    # clip_reads cuts at region -+ 2 * flank_len: flank_len 1 and the locus [start + 2, end - 2) put the cut where the vector has it
    from trgt_amd import ingest
    r = case["read"]
    mm, ml = _mm_for(r["bases"], r["meth"])
    rec = dict(name="kat", tid=0, pos=r["ref_pos"], cigar=_ops(r["cigar"]), seq=r["bases"], qual=[40] * len(r["bases"]),
               tags={"rq": ("f", 0.999), "MM": ("Z", mm), "ML": ("BC", ml)})
    bam, fa, bed = _one_read_data_set(tmp_path, "c", rec, (case["region_start"] + 2, case["region_end"] - 2), 1)
    rd = ingest.Reader(bam, fa)
    host, dev, fell_back, _ = _both(rd, bed, flank_len=1)
    assert not fell_back
    _same_batches(host, dev)
    exp = case["expected"]
    if exp is None:
        assert dev["n_reads"] == 0
        return
    assert dev["n_reads"] == 1
    assert bytes(dev["read_blob"][:int(dev["read_len"][0])]).decode() == exp["bases"]
    assert list(dev["meth"]) == exp["meth"] and int(dev["has_meth"][0]) == 1
    assert [(("MIDNSHP=X"[int(w) & 15]), int(w) >> 4) for w in dev["cigar"]] == _ops(exp["cigar"]) and int(dev["cigar_ref_pos"][0]) == exp["ref_pos"]
    assert bytes(dev["qual_blob"]) == bytes([40]) * len(exp["bases"])


def test_extract_snps_offset_vector_through_the_device(tmp_path):
    from trgt_amd import ingest
    c = KATS["extract_snps_offset"][0]
    ops = _ops(c["cigar"])
    qlen = sum(n for o, n in ops if o in "MIS=X")
    rng = np.random.default_rng(3)
    rec = dict(name="kat", tid=0, pos=c["ref_pos"], cigar=ops, seq="".join(rng.choice(list("ACGT"), qlen)), tags={"rq": ("f", 0.999)})
    ref_end = c["ref_pos"] + sum(n for o, n in ops if o in "MDN=X")
    bam, fa, bed = _one_read_data_set(tmp_path, "s", rec, (c["region"][0], c["region"][1]), 250, genome_len=ref_end + 2000)
    rd = ingest.Reader(bam, fa)
    host, dev, fell_back, _ = _both(rd, bed)
    assert not fell_back and dev["n_reads"] == 1
    _same_batches(host, dev)
    assert list(dev["mismatch_offsets"]) == c["expected"]


@pytest.mark.parametrize("case", KATS["get_meth"], ids=lambda c: c["test"])
def test_get_meth_vectors_through_the_device(tmp_path, case):
    from trgt_amd import ingest
    n = len(case["bases"])
    rec = dict(name="kat", tid=0, pos=1000, cigar=[("=", n)], seq=case["bases"], flag=16 if case["reverse"] else 0,
               tags={"rq": ("f", 0.999), "MM": ("Z", case["mm"]), "ML": ("BC", case["ml"])})
    bam, fa, bed = _one_read_data_set(tmp_path, "m", rec, (1000 + n // 2, 1000 + n // 2 + 1), 250)
    rd = ingest.Reader(bam, fa)
    host, dev, fell_back, _ = _both(rd, bed)
    assert not fell_back and dev["n_reads"] == 1
    _same_batches(host, dev)
    if case["expected"] is None:
        assert int(dev["has_meth"][0]) == 0 and len(dev["meth"]) == 0
    else:
        assert int(dev["has_meth"][0]) == 1 and list(dev["meth"]) == case["expected"]


def test_modification_strings_of_every_shape(tmp_path):
    """MM entries the parser must walk exactly like the host code: several entries, a numeric ChEBI code, two codes per entry (interleaved
    ML values), entries of other bases, '.' / '?' markers, a delta that runs off the read, too few ML values, both strands."""
    from trgt_amd import ingest
    rng = np.random.default_rng(17)
    genome = "".join(rng.choice(list("ACGT"), 9000))
    fa = str(tmp_path / "g.fa")
    write_fasta(fa, [("chr1", genome)])
    bed = str(tmp_path / "c.bed")
    open(bed, "w").write("chr1\t3000\t3060\tID=A;MOTIFS=CAG;STRUC=(CAG)n\n")
    recs = []
    shapes = ["C+m,0,1,0;", "C+76792,0;C+m,0,1;", "C+hm?,0,1,2;", "A+a,0,3;C+m.,1,1;", "C+m,2;C-m,0;G-m,1;C+m,1;", "C+m,0,100000;", "C+m,0,0,0,0,0,0,0,0;", "C+m;", "C+m,5", "N+n,1;C+m?,0;",
              "C+m," + ",".join(["0"] * 60) + ";"]
    for i, mm in enumerate(shapes):
        for flag in (0, 16):
            seq = "".join(rng.choice(list("ACGT"), 900))
            seq = seq[:300] + "CGCGACGTTCGA" * 20 + seq[540:]
            n_ml = mm.count(",") * (2 if "hm" in mm else 1)
            ml = [int(x) for x in rng.integers(1, 255, size=max(0, n_ml - (3 if i == 6 else 0)))]
            recs.append(dict(name="r%d_%d" % (i, flag), tid=0, pos=2600 + i, cigar=[("S", 3), ("=", 890), ("S", 7)], seq=seq, flag=flag,
                             tags={"rq": ("f", 0.999), "MM": ("Z", mm), "ML": ("BC", ml)}))
    recs.sort(key=lambda r: r["pos"])
    bam = str(tmp_path / "m.bam")
    write_bam(bam, [("chr1", 9000)], recs)
    rd = ingest.Reader(bam, fa)
    host, dev, fell_back, _ = _both(rd, bed)
    assert not fell_back and host["n_reads"] == len(recs) and host["has_meth"].sum() >= 8
    _same_batches(host, dev)
    host, dev, fell_back, _ = _both(rd, bed, flank_len=100)  # a narrower cut: the CpGs inside the clipped part only
    assert not fell_back
    _same_batches(host, dev)
