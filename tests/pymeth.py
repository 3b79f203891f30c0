"""Plain-Python restatement of the reference's per-allele methylation, from src/trgt/workflows/tr.rs alone:

  get_tr_meth  tr.rs:363-398   the mean call over the CpGs whose C lies inside the repeat span of one read
  assign_read  tr.rs:239-266   which allele(s) of the genotype a read of that span length counts for
  get_meth     tr.rs:198-230   per allele, the mean of the levels of its reads

Python floats are IEEE doubles and `+`, `/` round like Rust's f64, so the bits are the reference's.  Every sum is an explicit `t += x`
loop: the builtin sum() is compensated from Python 3.12 on and would give other bits.
"""
import math

FIRST, SECOND, BOTH, NONE = "first", "second", "both", "none"


class Malformed(Exception):
    """get_tr_meth's "Read {} has malformed methylation profile" (tr.rs:381-384: the reference logs it and exits)"""


def get_tr_meth(bases, meth, span, order="forward"):
    """bases: bytes; meth: None or a sequence of calls (0..255); span: (start, end).  Returns the level or None.
    order: "forward" is the reference; "reversed" and "pairwise" are WRONG-ORDER mutants for the tests that show the cases tell them apart."""
    if meth is None or len(meth) == 0:
        return None
    vals = []
    cpg_index = 0
    for pos in range(len(bases) - 1):
        if bases[pos:pos + 2] == b"CG":
            if span[0] <= pos < span[1]:
                if cpg_index >= len(meth):
                    raise Malformed(cpg_index)
                vals.append(meth[cpg_index] / 255.0)
            cpg_index += 1
    if not vals:
        return None
    return ordered_sum(vals, order) / len(vals)


def ordered_sum(vals, order="forward"):
    if order == "forward":
        t = 0.0
        for v in vals:
            t += v
        return t
    if order == "reversed":
        t = 0.0
        for v in reversed(vals):
            t += v
        return t
    if order == "pairwise":  # a tree reduction: neighbours first
        vals = list(vals)
        while len(vals) > 1:
            nxt = []
            for i in range(0, len(vals) - 1, 2):
                nxt.append(vals[i] + vals[i + 1])
            if len(vals) % 2:
                nxt.append(vals[-1])
            vals = nxt
        return vals[0] if vals else 0.0
    raise ValueError(order)


def assign_read(gt, tr_len):
    """gt: list of (size, (ci_lo, ci_hi)) in the genotype's OWN order (before "reference allele first")"""
    if len(gt) == 1:
        return FIRST
    (size_1, ci_1), (size_2, ci_2) = gt
    spans_1 = ci_1[0] <= tr_len <= ci_1[1]
    spans_2 = ci_2[0] <= tr_len <= ci_2[1]
    dist_1, dist_2 = abs(tr_len - size_1), abs(tr_len - size_2)
    if dist_1 < dist_2 and spans_1:
        return FIRST
    if dist_2 < dist_1 and spans_2:
        return SECOND
    if size_1 == size_2 and spans_1:
        return BOTH
    return NONE


def get_meth(gt, reads, spans, order="forward", allele_order=None):
    """reads: [(bases, meth or None)] in LocusResult.reads order, spans: [(start, end)].  Returns (levels per allele (None = no read),
    number of reads per allele), in the genotype's own order.  order: of the per-read sums; allele_order: of the per-allele sums (default: the same)."""
    allele_order = allele_order or order
    meths = [[], []]
    for (bases, meth), span in zip(reads, spans):
        level = get_tr_meth(bases, meth, span, order) if meth is not None else None
        if level is None:
            continue
        a = assign_read(gt, span[1] - span[0])
        if a in (FIRST, BOTH):
            meths[0].append(level)
        if a in (SECOND, BOTH):
            meths[1].append(level)
    out = [ordered_sum(m, allele_order) / len(m) if m else None for m in meths[:len(gt)]]
    return out, [len(m) for m in meths[:len(gt)]]


def locus_meth(n_alleles, gt_size, ci, flipped, reads, spans, ranks, order="forward", allele_order=None):
    """What trgt_locus_meth_batch returns for one locus, from the arrays of trgt_locus_batch_out: gt_size [2] and ci [4] in OUTPUT order,
    flipped, the input reads [(bases, meth or None)] with spans and ranks (-1 = not kept).
    Returns (allele_meth [2] in output order, NaN = None; meth_reads [2]; read_meth per input read, NaN = None)."""
    nan = float("nan")
    read_meth = []
    for (bases, meth), span, rank in zip(reads, spans, ranks):
        lv = get_tr_meth(bases, meth, span, order) if rank >= 0 and meth is not None else None
        read_meth.append(nan if lv is None else lv)
    kept = sorted((rank, i) for i, rank in enumerate(ranks) if rank >= 0)
    swap = bool(flipped) and n_alleles == 2
    pre = (lambda a: 1 - a) if swap else (lambda a: a)  # allele of the genotype's own order -> output slot
    gt = [(gt_size[pre(a)], (ci[2 * pre(a)], ci[2 * pre(a) + 1])) for a in range(n_alleles)]
    allele_meth, meth_reads = [nan, nan], [0, 0]
    if n_alleles:
        levels, counts = get_meth(gt, [reads[i] for _, i in kept], [spans[i] for _, i in kept], order, allele_order)
        for a in range(n_alleles):
            allele_meth[pre(a)] = nan if levels[a] is None else levels[a]
            meth_reads[pre(a)] = counts[a]
    return allele_meth, meth_reads, read_meth


def fmt_am(v):
    """write_vcf.rs: "{:.2}" of the level, "." for None"""
    return "." if v is None or (isinstance(v, float) and math.isnan(v)) else "%.2f" % v
