"""merge_exact (src/merge/strategy/exact.rs:6-88) restated in plain Python from that file alone, with sets, dicts and sorted: the
expectation of the merge path's tests.  Nothing here knows the library's layout, its hash or its kernels.

Genotype values are GenotypeAllele as tuples: ("U", i) Unphased(i), ("P", i) Phased(i), ("U", None) / ("P", None) the two missing values.
"""


class MergeError(ValueError):
    """The reference's Err(String); .status is the library's site_status for it"""

    def __init__(self, status, msg):
        ValueError.__init__(self, msg)
        self.status = status


def merge_exact(vcf_gts, sample_alleles):
    """-> (out_gts, sorted_alleles), or MergeError with the reference's message.  vcf_gts[i][sample] = [GenotypeAllele tuples]"""
    ref_allele = None
    all_alleles = set()
    for sample_allele in sample_alleles:                      # :13-31
        if len(sample_allele) != 0:
            if ref_allele is not None:
                if ref_allele != sample_allele[0]:
                    raise MergeError(1, "Reference alleles do not match: '%s' and '%s'" % (
                        ref_allele.decode("utf-8", "replace"), sample_allele[0].decode("utf-8", "replace")))
            else:
                ref_allele = sample_allele[0]
            for allele in sample_allele[1:]:
                all_alleles.add(allele)
    if ref_allele is None:                                    # :32
        raise MergeError(2, "No reference allele found")
    sorted_alleles = sorted(all_alleles, key=lambda a: (len(a), a))   # :34-38: by length, then a.cmp(b) on &[u8] (bytes compare unsigned)
    sorted_alleles.insert(0, ref_allele)                      # :39
    allele_to_index = {}                                      # :41-45: collect() into a HashMap, a later equal key overwrites an earlier one
    for idx, allele in enumerate(sorted_alleles):
        allele_to_index[allele] = idx
    out_sample_gts = []
    for i, vcf_gt in enumerate(vcf_gts):                      # :47-86
        out_gt = []
        for sample_gt in vcf_gt:
            s_gt = []
            for kind, pos in sample_gt:
                if pos is None:
                    s_gt.append((kind, None))
                    continue
                if pos < 0:
                    raise MergeError(3, "Index out of range: %d" % pos)
                if pos >= len(sample_alleles[i]) or sample_alleles[i][pos] not in allele_to_index:
                    raise MergeError(3, "Index out of bounds or allele not found in index: None")
                s_gt.append((kind, allele_to_index[sample_alleles[i][pos]]))
            out_gt.append(s_gt)
        out_sample_gts.append(out_gt)
    return out_sample_gts, sorted_alleles


def site_arrays(entries_alleles, entries_gts, first_allele=0):
    """The library's per-site outputs from the restatement, for a site whose entries hold flat lists of BCF-encoded genotype values:
    (status, src, allele_map, gt_out) -- src the input indices (site-local + first_allele) in output order, the LOWEST index among equals
    (status 1: the two REFs; otherwise [] with a status); allele_map / gt_out None with a status."""
    from trgt_amd.merge import VECTOR_END, gt_decode, gt_encode
    alleles = [[bytes(a) for a in al] for al in entries_alleles]
    base, k = [], first_allele
    for al in alleles:
        base.append(k)
        k += len(al)
    gts = [[[gt_decode(v) for v in g if v != VECTOR_END]] for g in entries_gts]
    try:
        out_gts, merged = merge_exact(gts, alleles)
    except MergeError as e:
        if e.status == 1:
            non_empty = [i for i, al in enumerate(alleles) if al]
            bad = next(i for i in non_empty[1:] if alleles[i][0] != alleles[non_empty[0]][0])
            return 1, [base[non_empty[0]], base[bad]], None, None
        return e.status, [], None, None
    first = {}
    for i, al in enumerate(alleles):
        for j, a in enumerate(al[1:], 1):
            first.setdefault(a, base[i] + j)
    src = [base[next(i for i, al in enumerate(alleles) if al)]] + [first[a] for a in merged[1:]]
    index = {}
    for idx, a in enumerate(merged):
        index[a] = idx
    amap = [index[a] for al in alleles for a in al]
    gt_out = []
    for g, og in zip(entries_gts, out_gts):
        it = iter(og[0])
        gt_out.append([v if v == VECTOR_END else gt_encode(next(it)) for v in g])
    return 0, src, amap, gt_out
