"""trgt_writer_write_meth (Writer.write(..., allele_meth=, meth_reads=)): the AM field of the VCF from values handed in -- what
trgt_locus_meth_batch returns -- instead of the writer's own scan of every kept read for CpGs.  Host code, no GPU: the small BAM with MM / ML
reads of the writer tests, hand-made genotyping results, and tests/pymeth.py in the kernel's place.  The writer's scan and pymeth are two
readings of tr.rs:198-266, 363-398; each pins the other here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pymeth  # noqa: E402
from test_writers import _synthetic  # noqa: E402  (the builder of the writer tests' BAM, FASTA and catalog)


def _handmade(tmp_path, spans):
    """The batch of the writer tests with two kept reads at locus 0 (spans: name -> (rank, allele, start, end)) and no call at locus 1"""
    from trgt_amd import ingest, locus
    bam, fa, bed, recs, genome = _synthetic(tmp_path)
    rd = ingest.Reader(bam, fa)
    b = rd.batch(bed, keep_native=True)
    out = locus.BatchOutputs(b)
    names = list(b["read_name"])
    for a in (out.span_start, out.span_end, out.read_rank, out.classification):
        a[:] = -1
    seqs = {}
    for name, (rank, cls, s, e) in spans.items():
        r = names.index(name)
        out.span_start[r], out.span_end[r], out.read_rank[r], out.classification[r] = s, e, rank, cls
        o = int(b["read_off"][r])
        seqs[rank] = bytes(b["read_blob"][o + s:o + e])
    out.n_alleles[0] = 2
    for a in (0, 1):
        o = int(out.allele_off[a])
        out.allele_blob[o:o + len(seqs[a])] = np.frombuffer(seqs[a], np.uint8)
        out.allele_len[a] = out.gt_size[a] = len(seqs[a])
        out.num_spanning[a], out.purity[a], out.n_spans[a] = 1, 0.5, 1
        out.spans3[3 * int(out.span_off[a]):3 * int(out.span_off[a]) + 3] = [a, 0, len(seqs[a])]
    lens = [len(seqs[0]), len(seqs[1])]
    out.ci[:4] = [min(lens), max(lens)] * 2
    return rd, b, out


def _pymeth_of(b, out):
    """tests/pymeth.py over the arrays the writer reads: (allele_meth, meth_reads), two per locus in output order"""
    am, n = [], []
    for l in range(int(b["n_loci"])):
        r0, r1 = int(b["locus_read_begin"][l]), int(b["locus_read_begin"][l + 1])
        reads = []
        for r in range(r0, r1):
            o = int(b["read_off"][r])
            calls = bytes(b["meth"][int(b["meth_off"][r]):int(b["meth_off"][r + 1])]) if b["has_meth"][r] else None
            reads.append((bytes(b["read_blob"][o:o + int(b["read_len"][r])]), calls))
        a, c, _ = pymeth.locus_meth(int(out.n_alleles[l]), [int(v) for v in out.gt_size[2 * l:2 * l + 2]], [int(v) for v in out.ci[4 * l:4 * l + 4]],
                                    int(out.flipped[l]), reads, [(int(out.span_start[r]), int(out.span_end[r])) for r in range(r0, r1)],
                                    [int(out.read_rank[r]) for r in range(r0, r1)])
        am += a; n += c
    return np.array(am, np.float64), np.array(n, np.int32)


def _am_fields(path):
    return [l.split("\t")[9].split(":")[7] for l in open(path).read().splitlines() if not l.startswith("#")]


PICKS = {"spans_all": (0, 0, 500, 562), "rev_meth": (1, 1, 500, 560)}


@pytest.mark.parametrize("flipped", [0, 1])
def test_given_values_write_the_same_vcf_as_the_host_scan(tmp_path, flipped):
    from trgt_amd import writers
    rd, b, out = _handmade(tmp_path, PICKS)
    out.flipped[0] = flipped
    am, n = _pymeth_of(b, out)
    assert not np.isnan(am[:2]).any() and list(n[:2]) == [1, 1] and np.isnan(am[2:]).all()   # both alleles of locus 0 have a level: the field is not empty
    files = {}
    for wb in (0, 1):
        for given in (0, 1):
            vcf, bam = tmp_path / ("o%d%d.vcf" % (wb, given)), tmp_path / ("o%d%d.bam" % (wb, given))
            w = writers.Writer(rd, vcf, bam, output_flank_len=40, sample_name="S1", command_line="cmd", write_behind=wb, threads=2)
            for _ in range(2):
                if given:
                    w.write(b, out, allele_meth=am, meth_reads=n)
                else:
                    w.write(b, out)
            w.close()
            files[wb, given] = (open(vcf, "rb").read(), open(bam, "rb").read())
    assert files[0, 0] == files[0, 1] == files[1, 0] == files[1, 1]
    # the two readings pin each other: pymeth's %.2f is the AM text of the writer's own scan
    got = _am_fields(tmp_path / "o00.vcf")
    assert got[0] == ",".join(pymeth.fmt_am(v) for v in am[:2]) and got[1] == "." and "." not in got[0].split(",")
    assert (am[0] != am[1]) and got[0].split(",")[0] != got[0].split(",")[1]   # (so a swapped pair would show)


def test_given_values_are_printed_and_the_scan_is_skipped(tmp_path):
    from trgt_amd import writers
    rd, b, out = _handmade(tmp_path, PICKS)
    nl = int(b["n_loci"])
    am, n = np.full(2 * nl, np.nan), np.zeros(2 * nl, np.int32)
    am[0], am[1], n[0], n[1] = 0.777, 0.125, 5, 6    # nothing the reads would give; 0.125 -> "0.12" (round-half-even of the exact binary value)
    w = writers.Writer(rd, tmp_path / "c.vcf", None, sample_name="S1")
    w.write(b, out, allele_meth=am, meth_reads=n)
    w.close()
    assert _am_fields(tmp_path / "c.vcf") == ["0.78,0.12", "."]
    am[1] = np.nan                                    # NaN = None -> "."
    w = writers.Writer(rd, tmp_path / "d.vcf", None, sample_name="S1")
    w.write(b, out, allele_meth=am, meth_reads=n)
    w.close()
    assert _am_fields(tmp_path / "d.vcf") == ["0.78,.", "."]


def test_both_arrays_are_required(tmp_path):
    import ctypes as C
    from trgt_amd import _lib, writers
    rd, b, out = _handmade(tmp_path, PICKS)
    am, n = np.zeros(2 * int(b["n_loci"])), np.zeros(2 * int(b["n_loci"]), np.int32)
    w = writers.Writer(rd, tmp_path / "g.vcf", None, sample_name="S1")
    with pytest.raises(ValueError):
        w.write(b, out, allele_meth=am)
    L = _lib.lib()
    L.trgt_writer_write_meth.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for a, c in ((None, _lib.ptr(n)), (_lib.ptr(am), None)):
        assert L.trgt_writer_write_meth(w.handle, C.addressof(b["_native"].handle.contents), C.addressof(out.c_out), a, c) == -1
        assert b"required" in L.trgt_writer_last_error(w.handle)
    w.close()
    assert _am_fields(tmp_path / "g.vcf") == []   # nothing was written by the refused calls
