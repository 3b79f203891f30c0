"""merge_variants / merge_variant (src/merge/vcf_processor.rs:237-299, 350-415, 452-532, 570-656) restated in plain Python from that file
alone: the heap over positions kept literally (heapq, one record per file in it), add_padding_base, process_record,
process_missing_record, process_am_field, flatten_genotypes, and merge_exact from tests/pymerge.py at the end.  The expectation of the
tests of trgt_merge_sites_batch; nothing here knows the library's layout, its sort or its kernels, and nothing is imported from it
(the BCF encoding of GenotypeAllele is restated below).

Input: the `files` of trgt_amd.merge.pack_sites -- per file n_samples, pre_v1, am_is_int and records; a record has pos, alleles, pad_base
and the per-sample lists gt, AL, SD, AP, AM.  A per-sample list is what BCF stores for the sample without the filling: the slice of
format(..).integer() / .float() / genotypes().get(i), read as CUT AT THE FIRST VECTOR-END VALUE (the reading the header documents).
Float values are kept as 32-bit patterns (ints): NaN payloads are data.
"""
import heapq
import struct

import pymerge

MISSING_INTEGER = -2 ** 31            # :24-27
VECTOR_END_INTEGER = -2 ** 31 + 1
MISSING_FLOAT = 0x7F800001
VECTOR_END_FLOAT = 0x7F800002
RAGGED = 4                            # the library's stage status for what the reference cannot write


class Ragged(Exception):
    """a present record has a sample with no value in GT or a numeric field: ragged arrays that htslib refuses, or the padding's unwrap"""


def bits(x):
    """a float as its float32 pattern; an int is a pattern already"""
    if isinstance(x, int):
        return x & 0xFFFFFFFF
    return struct.unpack("<I", struct.pack("<f", x))[0]


def f32_div_255(i):
    """i as f32 / 255.0 (:645) as a pattern: the int rounded to float32, the quotient rounded to float32.  Both are exact in double
    arithmetic followed by one rounding: float32(i) has 24 bits, 255 has 8, and a double quotient of such operands rounds to float32 as
    the exact quotient does (53 >= 2 * 24 + 2)."""
    a = struct.unpack("<f", struct.pack("<f", float(i)))[0]
    return struct.unpack("<I", struct.pack("<f", a / 255.0))[0]


def gt_decode(v):
    """i32 -> GenotypeAllele (rust-htslib's From<i32>): 0 UnphasedMissing, 1 PhasedMissing, else (v >> 1) - 1 with bit 0 the phase"""
    return ("P" if v & 1 else "U", None if v < 2 else (v >> 1) - 1)


def gt_encode(g):
    """GenotypeAllele -> i32 (From<GenotypeAllele>): (index + 1) << 1 | phase, missing is index -1"""
    kind, i = g
    return ((-1 if i is None else i) + 1) << 1 | (1 if kind == "P" else 0)


def cut(values, end):
    out = []
    for v in values:
        if v == end:
            break
        out.append(v)
    return out


def int_slice(values):
    return cut([int(v) for v in values], VECTOR_END_INTEGER)


def float_slice(values):
    return cut([bits(v) for v in values], VECTOR_END_FLOAT)


def heap_sites(files):
    """merge_variants, :242-285 -> [(min_pos, sample_records)], sample_records[i] the index of file i's record at the site or None"""
    cur = [0] * len(files)           # the next record a reader's advance() yields
    heap, seq = [], 0

    def advance_and_push(i):
        nonlocal seq
        if cur[i] < len(files[i]["records"]):
            heapq.heappush(heap, (files[i]["records"][cur[i]]["pos"], seq, i, cur[i]))   # Ord looks at pos alone; seq only keeps tuples comparable
            cur[i] += 1
            seq += 1
    for i in range(len(files)):      # init_heap
        advance_and_push(i)
    sites = []
    while heap:
        min_pos, _, i, r = heapq.heappop(heap)
        sample_records = [None] * len(files)
        sample_records[i] = r
        while heap and heap[0][0] == min_pos:
            _, _, i, r = heapq.heappop(heap)
            sample_records[i] = r
        sites.append((min_pos, sample_records))
        for i, r in enumerate(sample_records):   # update_heap
            if r is not None:
                advance_and_push(i)
    return sites


def key_sites(files):
    """the same sites for files whose positions never decrease: the distinct keys (pos, k) in increasing order, k the record's rank among
    the records of its own file at that position"""
    keyed = {}
    for i, f in enumerate(files):
        rank = {}
        for r, rec in enumerate(f["records"]):
            k = rank.get(rec["pos"], 0)
            rank[rec["pos"]] = k + 1
            keyed.setdefault((rec["pos"], k), [None] * len(files))[i] = r
    return [(key[0], keyed[key]) for key in sorted(keyed)]


def _b(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def padded_alleles(f, rec):
    """add_padding_base, :350-388, for one present record -> (alleles, padded)"""
    alleles = [_b(a) for a in rec["alleles"]]
    if not f["pre_v1"]:
        return alleles, False
    first = int_slice(rec["AL"][0])
    if not first:
        raise Ragged("min() of an empty slice: unwrap panics")
    if min(first) == 0:              # "Skip zero-length allele records"
        return alleles, False
    pb = rec["pad_base"]
    base = bytes([pb]) if isinstance(pb, int) else _b(pb)
    return [base + a for a in alleles], True


def merge_variant(files, min_pos, sample_records):
    """merge_variant, :390-415, with merge_and_write_data's merge_exact and flatten_genotypes -> what is written for the site: a dict of
    pos, template (file, record), status, alleles, gt, AL, SD, AP, AM, strings ((file, record, sample) or None per column), padded (files)"""
    template = next((i, r) for i, r in enumerate(sample_records) if r is not None)   # get_template_record
    als, sds, aps, ams, strings, gt_vecs, alleles, padded = [], [], [], [], [], [], [], []
    raw_gt = []                      # per file the genotype values as read, a one-value sample followed by vector end
    n_columns = sum(f["n_samples"] for f in files)
    out = dict(pos=min_pos, template=template, status=0, alleles=None, gt=None, AL=None, SD=None, AP=None, AM=None, strings=None, padded=None)
    try:
        for i, r in enumerate(sample_records):
            f = files[i]
            if r is None:            # process_missing_record, :464-484
                alleles.append([])
                gt_vecs.append([[("U", None)] for _ in range(f["n_samples"])])
                raw_gt.append([0, VECTOR_END_INTEGER] * f["n_samples"])   # i32::from(UnphasedMissing) is 0
                for _ in range(f["n_samples"]):
                    als.extend([MISSING_INTEGER, VECTOR_END_INTEGER])
                    sds.extend([MISSING_INTEGER, VECTOR_END_INTEGER])
                    aps.extend([MISSING_FLOAT, VECTOR_END_FLOAT])
                    ams.extend([MISSING_FLOAT, VECTOR_END_FLOAT])
                    strings.append(None)
                continue
            rec = f["records"][r]
            al, was_padded = padded_alleles(f, rec)
            if was_padded:
                padded.append(i)
            alleles.append(al)       # process_record, :452-462
            gt_vecs.append([[gt_decode(v) for v in int_slice(s)] for s in rec["gt"]])
            raw_gt.append([v for s in rec["gt"] for v in (int_slice(s) + [VECTOR_END_INTEGER] * (len(int_slice(s)) == 1))])
            for dst, name in ((als, "AL"), (sds, "SD")):   # process_integer_field, :586-599
                for s in rec[name]:
                    v = int_slice(s)
                    dst.extend(v)
                    if len(v) <= 1:
                        dst.append(VECTOR_END_INTEGER)
            for s in rec["AP"]:      # process_float_field, :601-614
                v = float_slice(s)
                aps.extend(v)
                if len(v) <= 1:
                    aps.append(VECTOR_END_FLOAT)
            for s in rec["AM"]:      # process_am_field, :628-656
                if f["am_is_int"]:
                    v = [MISSING_FLOAT if x == MISSING_INTEGER else f32_div_255(x) for x in int_slice(s)]
                else:
                    v = float_slice(s)
                ams.extend(v)
                if len(v) <= 1:
                    ams.append(VECTOR_END_FLOAT)
            strings.extend((i, r, k) for k in range(f["n_samples"]))
        if any(len(row) != 2 * n_columns for row in (als, sds, aps, ams)) or any(len(g) == 0 for e in gt_vecs for g in e):
            raise Ragged("rows of different lengths per sample")
    except Ragged:
        out["status"] = RAGGED
        return out
    # what merge_and_write_data is handed (:412): the stage the sites call stops at, genotypes in the two-value form of flatten_genotypes
    out.update(AL=als, SD=sds, AP=aps, AM=ams, strings=strings, padded=padded, entry_alleles=alleles,
               entry_gt=raw_gt)
    try:
        out_gts, merged = pymerge.merge_exact(gt_vecs, alleles)
    except pymerge.MergeError as e:
        out["status"] = e.status
        return out
    gts_new = []                  # flatten_genotypes, :519-532
    for file_gts in out_gts:
        for sample_gt in file_gts:
            conv = [gt_encode(g) for g in sample_gt]
            if len(conv) == 1:
                conv.append(VECTOR_END_INTEGER)
            gts_new.extend(conv)
    out.update(alleles=merged, gt=gts_new)
    return out


def merge_variants(files):
    return [merge_variant(files, pos, recs) for pos, recs in heap_sites(files)]
