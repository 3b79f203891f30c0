"""trgt_writer_set_records_device (trgt_amd/csrc/bam_records_dev.hip): the spanning-BAM records of device-ingested batches assembled by
kernels from the arrays the ingestion left in HBM.  The yardstick is exact: with the mode on, the VCF and the BAM are the files the same
library writes with the mode off (host formatting of the same batch and results), byte for byte -- for every compression level, with and
without the device deflate, with and without write-behind."""
import os

import numpy as np
import pytest

from bamtools import read_bam_records, write_bam, write_fasta
from writer_results import handmade as _handmade

pytestmark = pytest.mark.gpu



def _fuzz_one_file():
    """one_file of tests/tools/ingest_fuzz.py (a script: it runs its fuzz when imported, so its functions are taken from its text)"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "ingest_fuzz.py")
    src = open(path).read()
    ns = {"__name__": "ingest_fuzz", "__file__": path}
    exec(compile(src[:src.rindex("\nmain()")], path, "exec"), ns)
    return ns["one_file"]


def _write(rd, pairs, tmp_path, tag, records_device, **kw):
    from trgt_amd import writers
    vcf, bam = str(tmp_path / (tag + ".vcf")), str(tmp_path / (tag + ".bam"))
    w = writers.Writer(rd, vcf, bam, records_device=records_device, **kw)
    for b, o in pairs:
        w.write(b, o)
    rs, ds = w.records_stats(), w.device_stats()
    w.close()
    return vcf, bam, rs, ds


def _same_files(a, b):
    assert open(a[0], "rb").read() == open(b[0], "rb").read(), "VCF"
    x, y = open(a[1], "rb").read(), open(b[1], "rb").read()
    if x != y:  # say which record, which field
        (_, _, rx), (_, _, ry) = read_bam_records(a[1]), read_bam_records(b[1])
        assert len(rx) == len(ry), (len(rx), len(ry))
        for i, (p, q) in enumerate(zip(rx, ry)):
            for k in p:
                assert p[k] == q[k], (i, p["name"], k, p[k], q[k])
    assert x == y, "the records agree, the BGZF blocks do not"


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """1 200 synthetic loci ingested on the device in three batches of unequal size (the tail of the BGZF stream carries across them), with
    the results of trgt_locus_batch from the reads left in HBM"""
    from trgt_amd import _lib, ingest, locus, synth_bam
    d = tmp_path_factory.mktemp("ds")
    ds = synth_bam.write_dataset(str(d), n_loci=1200, read_len=2000)
    rd = ingest.Reader(ds["bam"], ds["fasta"])
    ctx = _lib.Context(0)
    pairs = []
    for first, n in ((0, 500), (500, 437), (937, 263)):
        b = rd.batch(ds["bed"], first_locus=first, max_loci=n, keep_native=True, ingest_device=0, threads=4)
        assert b["read_blob_device"] == 0 and b["read_blob_dev"]
        pairs.append((b, locus.run_batch(b, locus.Params(), ctx, reads_dev=ingest.device_reads(b))))
    assert rd.device_stats()["fallbacks"] == 0
    yield ds, rd, pairs
    del pairs
    ctx.close()


@pytest.mark.parametrize("level", [6, 1, 0])
@pytest.mark.parametrize("write_behind", [0, 1])
@pytest.mark.parametrize("deflate_device", [-1, 0])
def test_byte_identity_on_the_synthetic_data_set(synth, tmp_path, deflate_device, write_behind, level):
    ds, rd, pairs = synth
    kw = dict(bam_compress_level=level, deflate_device=deflate_device, write_behind=write_behind, threads=4)
    off = _write(rd, pairs, tmp_path, "off", -1, **kw)
    on = _write(rd, pairs, tmp_path, "on", 0, **kw)
    _same_files(off, on)
    n_rec = len(read_bam_records(on[1])[2])
    assert n_rec > 1200 * 15
    assert off[2] == dict(device_batches=0, host_batches=0, host_reason=0, records=0, bytes=0)
    rs = on[2]
    assert rs["device_batches"] == 3 and rs["host_batches"] == 0 and rs["records"] == n_rec and rs["bytes"] > 100 * n_rec, rs
    if deflate_device == 0:  # (not because everything fell back to zlib)
        assert on[3]["device"] > 0 and off[3]["device"] > 0, (on[3], off[3])
    else:
        assert on[3]["device"] == 0 and on[3]["host"] > 0


@pytest.mark.parametrize("flank_len,output_flank_len,keep_unmapped", [(250, 0, 1), (250, 10, 0), (250, 250, 1), (100, 100, 0)])
def test_output_flank_len_and_the_unmapped_flag(synth, tmp_path, flank_len, output_flank_len, keep_unmapped):
    from trgt_amd import _lib, ingest, locus
    ds, rd, _ = synth
    b = rd.batch(ds["bed"], first_locus=100, max_loci=150, keep_native=True, ingest_device=0, threads=4, flank_len=flank_len)
    ctx = _lib.Context(0)
    o = locus.run_batch(b, locus.Params(search_flank_len=flank_len), ctx, reads_dev=ingest.device_reads(b))
    kw = dict(output_flank_len=output_flank_len, keep_unmapped_flag=keep_unmapped, deflate_device=0)
    off = _write(rd, [(b, o)], tmp_path, "off", -1, **kw)
    on = _write(rd, [(b, o)], tmp_path, "on", 0, **kw)
    _same_files(off, on)
    recs = read_bam_records(on[1])[2]
    assert on[2]["device_batches"] == 1 and on[2]["records"] == len(recs) > 150 * 10
    assert all(r["tags"]["FL"] == ("BI", [output_flank_len] * 2) and r["flag"] & 4 == 4 * keep_unmapped for r in recs)
    ctx.close()


def _hand_made_file(tmp_path):
    """Reads of one locus next to each other: with and without methylation, both strands, a soft clip, = / X / I / D runs, HP, no rq"""
    rng = np.random.default_rng(5)
    genome = "".join(rng.choice(list("ACGT"), 8000))
    fa, bed, bam = str(tmp_path / "h.fa"), str(tmp_path / "h.bed"), str(tmp_path / "h.bam")
    write_fasta(fa, [("chr1", genome)])
    open(bed, "w").write("chr1\t3000\t3060\tID=HM;MOTIFS=CAG;STRUC=(CAG)n\nchr1\t5000\t5030\tID=second_locus;MOTIFS=A;STRUC=(A)n\n")
    recs = []
    for i in range(12):
        cig = [("S", 4), ("=", 300 + i), ("X", 2), ("=", 200), ("I", 3), ("=", 150), ("D", 5), ("=", 400 - i), ("S", 6)] if i % 3 else [("=", 1200)]
        qlen = sum(n for c, n in cig if c in "SI=XM")
        seq = "".join(rng.choice(list("ACGT"), qlen))
        seq = seq[:350] + "CGACGTCG" * 30 + seq[590:]
        tags = {}
        if i != 4:
            tags["rq"] = ("f", 0.999)
        if i % 2:
            tags["HP"] = ("C", 1 + i % 2)
        if i % 4 != 1:  # (reads 1, 5, 9: no methylation, next to reads with it)
            tags["MM"] = ("Z", "C+m," + ",".join(["0"] * 25) + ";")
            tags["ML"] = ("BC", [int(x) for x in rng.integers(1, 255, size=25)])
        recs.append(dict(name="hand_%d" % i, tid=0, pos=2500 + 7 * i, cigar=cig, seq=seq, flag=16 if i % 5 == 2 else 0, mapq=60 - i, tags=tags))
    for i in range(3):
        recs.append(dict(name="two_%d" % i, tid=0, pos=4700 + i, cigar=[("=", 700)], seq="".join(rng.choice(list("ACGT"), 700)), tags={"rq": ("f", 0.995)}))
    recs.sort(key=lambda r: r["pos"])
    write_bam(bam, [("chr1", 8000)], recs)
    return bam, fa, bed


def test_every_kind_of_field(tmp_path):
    """Random BAM files (soft clips, = / X / I / D / N runs, HP, MM / ML on both strands, reverse reads, reads without rq) and a hand-made one,
    with hand-made results that keep most reads: odd and even clipped lengths, cuts inside every kind of operation, a read whose span
    leaves fewer than F flank bases (no record), reads without methylation next to reads with it."""
    one_file = _fuzz_one_file()
    from trgt_amd import ingest
    cases = []
    for seed in (3, 11, 29, 31):
        d = tmp_path / ("f%d" % seed)
        d.mkdir()
        rng = np.random.default_rng(seed)
        bam, fa, bed, flank, _ = one_file(rng, str(d), "z")
        cases.append((bam, fa, bed, flank, seed))
    d = tmp_path / "hand"
    d.mkdir()
    cases.append(_hand_made_file(d) + (250, 0))
    n_rec = n_meth = n_plain = n_odd = n_hp = n_norq = n_rev = 0
    for bam, fa, bed, flank, seed in cases:
        rd = ingest.Reader(bam, fa)
        b = rd.batch(bed, keep_native=True, ingest_device=0, flank_len=flank, min_read_qual=0.9)
        fell_back = rd.device_stats()["fallbacks"]
        assert fell_back == 0, "seed %d: the ingestion went back to the host, pick another" % seed
        for F in (min(flank, 50), 7):
            out, _ = _handmade(b, np.random.default_rng(seed + F), F)
            if seed == 0 and b["n_reads"] > 2:  # the hand-made file: a span that leaves F - 1 bases in front -> skipped by both
                r = int(np.flatnonzero(out.read_rank >= 0)[0])
                out.span_start[r] = F - 1
            d2 = tmp_path / ("o%d_%d" % (seed, F))
            d2.mkdir()
            for dd in (-1, 0):
                off = _write(rd, [(b, out)], d2, "off%d" % dd, -1, output_flank_len=F, deflate_device=dd, bam_compress_level=1)
                on = _write(rd, [(b, out)], d2, "on%d" % dd, 0, output_flank_len=F, deflate_device=dd, bam_compress_level=1)
                _same_files(off, on)
                assert on[2]["host_batches"] == fell_back == 0 and on[2]["device_batches"] == 1, on[2]
            recs = read_bam_records(on[1])[2]
            assert on[2]["records"] == len(recs)
            n_rec += len(recs)
            for r in recs:
                n_meth += "MC" in r["tags"]; n_plain += "MC" not in r["tags"]; n_odd += len(r["seq"]) % 2; n_hp += "HP" in r["tags"]
                n_norq += r["tags"]["rq"][1] == -1.0; n_rev += bool(r["flag"] & 16)
            if seed == 0:
                assert len(recs) == int((out.read_rank >= 0).sum()) - 1
    assert n_rec > 100 and min(n_meth, n_plain, n_odd, n_hp, n_norq, n_rev) > 0, (n_rec, n_meth, n_plain, n_odd, n_hp, n_norq, n_rev)


def test_a_host_ingested_batch_is_formatted_by_the_host_and_counted(synth, tmp_path):
    ds, rd, pairs = synth
    from trgt_amd import _lib, locus
    hb = rd.batch(ds["bed"], first_locus=0, max_loci=120, keep_native=True, threads=4)
    assert not hb.get("read_blob_dev")
    ctx = _lib.Context(0)
    ho = locus.run_batch(hb, locus.Params(), ctx)
    seq = [(hb, ho), pairs[2], (hb, ho)]   # host, device, host: the tail of the stream goes through both paths
    off = _write(rd, seq, tmp_path, "off", -1, deflate_device=0)
    on = _write(rd, seq, tmp_path, "on", 0, deflate_device=0)
    _same_files(off, on)
    assert on[2]["device_batches"] == 1 and on[2]["host_batches"] == 2 and on[2]["host_reason"] == 1 and on[2]["records"] > 0, on[2]
    ctx.close()


def test_results_the_host_path_skips_give_no_record(synth, tmp_path):
    """Hand-made results for a device-ingested batch: span_start < F, span_end + F > read_len, span_end > read_len, loci without alleles.
    The host writes no record for such reads; the size kernel applies the same rules before it touches the read."""
    ds, rd, pairs = synth
    b = pairs[1][0]
    out, n_bad = _handmade(b, np.random.default_rng(77), 50, bad=0.3)
    assert n_bad > 1000 and int((out.n_alleles == 0).sum()) == b["n_loci"]
    off = _write(rd, [(b, out)], tmp_path, "off", -1, deflate_device=0)
    on = _write(rd, [(b, out)], tmp_path, "on", 0, deflate_device=0)
    _same_files(off, on)
    kept = np.flatnonzero(out.read_rank >= 0)
    s, e, n = out.span_start[kept].astype(np.int64), out.span_end[kept].astype(np.int64), b["read_len"][kept].astype(np.int64)
    want = int(((s >= 50) & (n >= e + 50) & (e - s + 100 > 0)).sum())   # write_bam.rs' flank rule and clip_bases' None
    recs = read_bam_records(on[1])[2]
    assert on[2]["device_batches"] == 1 and on[2]["host_batches"] == 0 and on[2]["records"] == len(recs) == want, (on[2], len(recs), want)
    assert 1000 < want < len(kept) - 500


def test_write_behind_reports_a_failed_write(synth, tmp_path):
    from trgt_amd import _lib, writers
    ds, rd, pairs = synth
    if not os.path.exists("/dev/full"):
        pytest.skip("no /dev/full")
    for wb in (0, 1):
        for dd in (-1, 0):
            w = writers.Writer(rd, tmp_path / ("e%d%d.vcf" % (wb, dd + 1)), "/dev/full", write_behind=wb, deflate_device=dd, records_device=0)
            failed = 0
            for b, o in pairs:
                try:
                    w.write(b, o)
                except _lib.TrgtHipError:
                    failed += 1
            try:
                w.close()
            except _lib.TrgtHipError:
                failed += 1
            assert failed >= 1, (wb, dd)
