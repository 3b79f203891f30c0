"""Hand-made genotyping results for the writer tests (tests/test_writers.py on the CPU, tests/test_writer_records_device_gpu.py on the
GPU): what a caller may hand to trgt_writer_write without having run trgt_locus_batch."""


def handmade(b, rng, F, keep=0.85, bad=0.0):
    """Results as a caller may hand them over: per locus a random subset of the reads ranked in random order, spans that leave F bases on
    both sides; a share `bad` of them gets a span the host path skips (span_start < F, span_end + F > read_len, span_end > read_len)."""
    from trgt_amd import locus
    out = locus.BatchOutputs(b)
    out.span_start[:] = -1; out.span_end[:] = -1; out.read_rank[:] = -1; out.classification[:] = -1
    lrb = b["locus_read_begin"]
    n_bad = 0
    for l in range(b["n_loci"]):
        rs = [r for r in range(int(lrb[l]), int(lrb[l + 1])) if rng.random() < keep]
        rng.shuffle(rs)
        for rank, r in enumerate(rs):
            n = int(b["read_len"][r])
            s = int(rng.integers(F, max(F, n - F) + 1))
            e = int(rng.integers(s, max(s, n - F) + 1))
            if rng.random() < bad:
                n_bad += 1
                kind = int(rng.integers(0, 3))
                if kind == 0 and F > 0:
                    s = int(rng.integers(0, F))
                elif kind == 1:
                    e = max(s, n - F + 1 + int(rng.integers(0, max(1, F))))
                else:
                    e = n + 1 + int(rng.integers(0, 5000))
            out.span_start[r], out.span_end[r], out.read_rank[r], out.classification[r] = s, e, rank, int(rng.integers(0, 2))
    return out, n_bad


def two_alleles(b, out):
    """Every locus of `out` gets two alleles cut from its first two reads (20 + 3 l + 7 a bases from base 200 on), with the fields the VCF shows"""
    lrb = b["locus_read_begin"]
    for l in range(int(b["n_loci"])):
        r0 = int(lrb[l])
        assert int(lrb[l + 1]) - r0 >= 2
        out.n_alleles[l] = 2
        for a in (0, 1):
            n = 20 + 3 * l + 7 * a
            o, k = int(b["read_off"][r0 + a]) + 200, 2 * l + a
            out.allele_blob[int(out.allele_off[k]):int(out.allele_off[k]) + n] = b["read_blob"][o:o + n]
            out.allele_len[k] = out.gt_size[k] = n
            out.ci[2 * k:2 * k + 2] = [n - 1, n + 1]
            out.num_spanning[k], out.purity[k], out.n_spans[k] = 3 + a, 0.9, 1
            out.spans3[3 * int(out.span_off[k]):3 * int(out.span_off[k]) + 3] = [0, 0, n]
