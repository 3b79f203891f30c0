"""Call time of trgt_locus_meth_batch and what it takes off the writer.

Part 1 -- the entry point on a flagship-sized chunk: 1 000 loci of 30 reads of 6 000 random bases, every read kept and with a call on every CpG
(about 375 per read), repeat spans of 60 to 600 bases around the middle of the read, two alleles per locus; reads and calls resident in HBM.
Blocking calls on one context; reported per read encoding: the call (host clock around the synchronous call) and its two kernels (HIP events
inside the library, trgt_locus_meth_kernel_ms), median (min .. max) of REPEATS calls after WARMUP calls, the bytes tr_meth_kernel streams and
the rate that makes, and whether ASCII and 4-bit reads give the same bits.

Part 2 -- Writer.write on a batch that carries methylation: a BAM written here (LOCI loci, 30 forward reads of 2 400 bases each with MM / ML
calls on every CpG, (CGG)20 repeats), ingested, genotyped by trgt_locus_batch, then written three ways, alternating call by call: write()
-- the host scan, the code path of the commit before this entry point existed --, write(allele_meth=, meth_reads=) with the values of
trgt_locus_meth_batch, and, when LOCUS_METH_TIMING_PARENT_LIB names a libtrgt_hip.so built from that commit, its trgt_writer_write on the
same native batch.  VCF and spanning BAM, default writer settings.  Reported: median (min .. max) per arm, whether the files are the same
byte for byte, and whether the ranges overlap.

The lines are also written to the file named by the first argument (default: profiles/locus_meth_timing.txt).
LOCUS_METH_TIMING_LOCI=<n>: loci of part 1 (default 1000).  LOCUS_METH_TIMING_WRITER_LOCI=<n>: loci of part 2 (default 200).
LOCUS_METH_TIMING_REPEATS=<n>: calls per arm (default 9, at least 5)."""
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from trgt_amd import _lib, ingest, locus, writers  # noqa: E402

WARMUP = 3


def med(t):
    return "median %8.3f ms  (min %.3f .. max %.3f of %d)" % (statistics.median(t), min(t), max(t), len(t))


def flagship_chunk(rng, n_loci, reads_per_locus=30, read_len=6000):
    """the arrays trgt_locus_meth_batch reads, made directly: no genotyping run is needed to time it"""
    nr = n_loci * reads_per_locus
    blob = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=nr * read_len)]
    cg = (blob[:-1] == ord("C")) & (blob[1:] == ord("G"))
    cg[read_len - 1::read_len] = False   # (no CpG across two reads)
    per_read = np.add.reduceat(np.concatenate([cg, [False]]).astype(np.int64), np.arange(0, nr * read_len, read_len))
    meth_off = np.zeros(nr + 1, np.uint64)
    meth_off[1:] = np.cumsum(per_read)
    span_len = rng.integers(60, 601, size=nr).astype(np.int32)
    start = (read_len // 2 - span_len // 2 + rng.integers(-100, 101, size=nr)).astype(np.int32)
    a = dict(n_loci=n_loci, n_reads=nr, read_encoding=0, flank_blob=np.zeros(1, np.uint8), read_blob=blob,
             locus_read_begin=np.arange(0, nr + 1, reads_per_locus, dtype=np.uint64), read_off=np.arange(0, nr * read_len, read_len, dtype=np.uint64),
             read_len=np.full(nr, read_len, np.uint32), meth=rng.integers(0, 256, size=int(meth_off[-1]), dtype=np.uint8), meth_off=meth_off,
             has_meth=np.ones(nr, np.uint8))
    for k in ("lf_off", "lf_len", "rf_off", "rf_len", "tr_blob", "tr_off", "tr_len", "motif_blob", "motif_off", "set_motif_begin", "ploidy"):
        a[k] = np.zeros(n_loci + 1, np.uint64)   # (not read by trgt_locus_meth_batch: the struct only needs an address)

    class Out:   # the fields of trgt_locus_batch_out the entry point reads
        pass
    out = Out()
    out.span_start, out.span_end = start, start + span_len
    out.read_rank = np.tile(rng.permutation(reads_per_locus).astype(np.int32), n_loci)
    out.n_alleles = np.full(n_loci, 2, np.int32)
    out.allele_len = np.tile(np.array([200, 460], np.uint32), n_loci)
    out.gt_size = out.allele_len.astype(np.int32)
    out.ci = np.tile(np.array([60, 330, 331, 600], np.int32), n_loci)
    out.flipped = (rng.random(n_loci) < 0.3).astype(np.uint8)
    out.c_out = _lib.LocusBatchOut()
    for k in ("span_start", "span_end", "read_rank", "n_alleles", "allele_len", "gt_size", "ci", "flipped"):
        setattr(out.c_out, k, _lib.ptr(getattr(out, k)).value)
    return a, out


def part1(say, repeats):
    import torch
    n_loci = int(os.environ.get("LOCUS_METH_TIMING_LOCI", "1000"))
    rng = np.random.default_rng(20251020)
    a, out = flagship_chunk(rng, n_loci)
    a4 = locus.pack_bam4(a)
    nr = a["n_reads"]
    say("part 1: %d loci x 30 reads x 6000 bases, %d reads, %.1f MB of bases (%.1f MB as 4-bit codes), %d calls (%.1f per read); spans of 60-600 bases; reads and calls resident in HBM" % (
        n_loci, nr, a["read_blob"].nbytes / 1e6, a4["read_blob"].nbytes / 1e6, int(a["meth_off"][-1]), float(a["meth_off"][-1]) / nr))
    streamed = int(np.minimum(a["read_len"].astype(np.int64), out.span_end.astype(np.int64) + 1).sum())
    say("tr_meth_kernel streams bases[0 .. span_end + 1) of every read: %.1f MB of ASCII bases, %.1f MB of 4-bit codes" % (streamed / 1e6, streamed / 2e6))
    ctx = _lib.Context(0)
    ctx.timing_enable(True)
    meth_dev = torch.from_numpy(a["meth"]).cuda()
    got = {}
    for name, b, nbytes in (("ASCII", a, streamed), ("BAM4", a4, streamed / 2)):
        reads_dev = torch.from_numpy(b["read_blob"]).cuda()
        call, k0, k1 = [], [], []
        ms = (C.c_double * 2)()
        for i in range(WARMUP + repeats):
            t0 = time.perf_counter()
            res = locus.allele_meth(b, out, ctx, reads_dev=reads_dev, meth_dev=meth_dev)   # (blocking: returns with the results on the host)
            t = (time.perf_counter() - t0) * 1e3
            _lib.lib().trgt_locus_meth_kernel_ms(ctx.handle, ms)
            if i >= WARMUP:
                call.append(t); k0.append(ms[0]); k1.append(ms[1])
        got[name] = res
        say("%-5s trgt_locus_meth_batch  %s" % (name, med(call)))
        say("%-5s   tr_meth_kernel       %s   %.0f GB/s of bases" % (name, med(k0), nbytes / 1e6 / statistics.median(k0)))
        say("%-5s   allele_meth_kernel   %s" % (name, med(k1)))
        del reads_dev
    same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got["ASCII"], got["BAM4"]))
    say("ASCII and 4-bit reads give the same bits: %s; alleles with a level: %d of %d" % (same, int(np.isfinite(got["ASCII"][0]).sum()), 2 * n_loci))
    ctx.close()
    return same


def meth_bam(tmp, n_loci, rng):
    from bamtools import write_bam, write_fasta
    pitch, rlen = 4000, 2400
    g = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n_loci * pitch)].copy()
    bed = []
    for i in range(n_loci):
        s = i * pitch + 1970
        g[s:s + 60] = np.frombuffer(b"CGG" * 20, np.uint8)
        bed.append("chr1\t%d\t%d\tID=L%d;MOTIFS=CGG;STRUC=(CGG)n\n" % (s, s + 60, i))
    genome = g.tobytes().decode()
    fa, bam, cat = os.path.join(tmp, "g.fa"), os.path.join(tmp, "s.bam"), os.path.join(tmp, "cat.bed")
    write_fasta(fa, [("chr1", genome)])
    open(cat, "w").write("".join(bed))
    recs = []
    for i in range(n_loci):
        pos = i * pitch + 800
        seq = genome[pos:pos + rlen]
        cs = [k for k, ch in enumerate(seq) if ch == "C"]
        deltas, last = [], -1
        for k, p in enumerate(cs):
            if seq[p:p + 2] == "CG":
                deltas.append(k - last - 1)
                last = k
        mm = "C+m?," + ",".join(map(str, deltas)) + ";"
        for r in range(30):
            recs.append(dict(name="r%d_%d" % (i, r), tid=0, pos=pos, cigar=[("=", rlen)], seq=seq, flag=0, qual=[30] * rlen,
                             tags={"rq": ("f", 0.999), "MM": ("Z", mm), "ML": ("BC", [int(v) for v in rng.integers(0, 256, size=len(deltas))])}))
    write_bam(bam, [("chr1", len(genome))], recs)
    return bam, fa, cat


def part2(say, repeats):
    n_loci = int(os.environ.get("LOCUS_METH_TIMING_WRITER_LOCI", "200"))
    parent = os.environ.get("LOCUS_METH_TIMING_PARENT_LIB")
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as tmp:
        bam, fa, cat = meth_bam(tmp, n_loci, rng)
        rd = ingest.Reader(bam, fa)
        b = rd.batch(cat, keep_native=True)
        ctx = _lib.Context(0)
        out = locus.run_batch(b, ctx=ctx)
        am, n, _ = locus.allele_meth(b, out, ctx)
        say("part 2: %d loci, %d clipped reads, %.1f MB of bases, %d calls; %d loci genotyped, %d alleles with a level" % (
            int(b["n_loci"]), int(b["n_reads"]), float(b["read_len"].sum()) / 1e6, int(b["meth_off"][-1]), int((out.n_alleles > 0).sum()), int(np.isfinite(am).sum())))
        arms = {"write() [host scan]": lambda w: w.write(b, out), "write(allele_meth=, meth_reads=)": lambda w: w.write(b, out, allele_meth=am, meth_reads=n)}
        ws = {k: writers.Writer(rd, os.path.join(tmp, "o%d.vcf" % i), os.path.join(tmp, "o%d.bam" % i)) for i, k in enumerate(arms)}
        P = None
        if parent:
            P = C.CDLL(parent)
            P.trgt_writer_open.argtypes = [C.c_void_p, C.POINTER(writers.WriterParams), C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
            P.trgt_writer_write.argtypes = [C.c_void_p, C.POINTER(ingest.IngestBatch), C.c_void_p]
            P.trgt_writer_close.argtypes = [C.c_void_p]
            wp = writers.WriterParams(50, b"sample", b"trgt", b"3.0.0", b"", 1, 0, 6, -1, 0)
            ph = C.c_void_p()
            assert P.trgt_writer_open(rd.handle, C.byref(wp), os.path.join(tmp, "p.vcf").encode(), os.path.join(tmp, "p.bam").encode(), C.byref(ph)) == 0

            def parent_write(_):
                assert P.trgt_writer_write(ph, b["_native"].handle, C.addressof(out.c_out)) == 0
            arms["parent library's trgt_writer_write"] = parent_write
            ws["parent library's trgt_writer_write"] = None
        times = {k: [] for k in arms}
        for i in range(WARMUP + repeats):
            for k, f in arms.items():
                t0 = time.perf_counter()
                f(ws[k])
                t = (time.perf_counter() - t0) * 1e3
                if i >= WARMUP:
                    times[k].append(t)
        for w in ws.values():
            if w is not None:
                w.close()
        if P is not None:
            P.trgt_writer_close(ph)
        for k in arms:
            say("%-36s %s" % (k, med(times[k])))
        files = [open(os.path.join(tmp, f), "rb").read() for f in ("o0.vcf", "o1.vcf", "o0.bam", "o1.bam")]
        same = files[0] == files[1] and files[2] == files[3]
        if P is not None:
            same = same and open(os.path.join(tmp, "p.vcf"), "rb").read() == files[0] and open(os.path.join(tmp, "p.bam"), "rb").read() == files[2]
        say("all arms write the same VCF and spanning BAM, byte for byte: %s" % same)
        base = times["parent library's trgt_writer_write"] if P is not None else times["write() [host scan]"]
        new = times["write(allele_meth=, meth_reads=)"]
        apart = max(new) < min(base) or max(base) < min(new)
        say("given values against the %s: the ranges %s" % ("parent library" if P is not None else "host scan of this library (no parent library was named)",
                                                             "do not overlap" if apart else "overlap: no difference is claimed"))
        ctx.close()
        return same


def main():
    import torch
    repeats = max(5, int(os.environ.get("LOCUS_METH_TIMING_REPEATS", "9")))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "locus_meth_timing.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("python tools/locus_meth_timing.py -- device: %s; %d calls per arm after %d warm-up calls" % (torch.cuda.get_device_name(0), repeats, WARMUP))
    ok = part1(say, repeats)
    ok = part2(say, repeats) and ok
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
