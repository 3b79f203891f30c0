"""Designed cases for trgt_locus_meth_batch (get_meth / assign_read / get_tr_meth, tr.rs:198-266, 363-398), as plain data.

A case is a list of loci; a locus is the slice of trgt_locus_batch_out the entry point reads (n_alleles, allele_len, gt_size, ci, flipped, all in
OUTPUT order) and its input reads (bases, calls or None, span, rank).  build() lays a case out as the ABI's arrays, expected() is tests/pymeth.py
applied to it.  CASES maps a name to (loci, notes); notes: gt_size_null, error ("malformed", read index), order ("read" / "allele": the case
must give other bits when the sums run in another order -- tests/test_pymeth.py holds it to that).
"""
import random

import numpy as np

import pymeth

BAM4 = "=ACMGRSVTWYHKDBN"


def rd(bases, meth, span, rank):
    return dict(bases=bases if isinstance(bases, bytes) else bases.encode(), meth=None if meth is None else bytes(meth), span=span, rank=rank)


def locus(n_alleles, allele_len, ci, reads, flipped=0, gt_size=None):
    return dict(n_alleles=n_alleles, allele_len=list(allele_len), gt_size=list(gt_size if gt_size is not None else allele_len), ci=list(ci),
                flipped=flipped, reads=reads)


def one(reads):
    """one allele that takes every read"""
    return locus(1, (10, 0), (0, 1000, 0, 0), reads)


def rand_bases(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def n_cpg(bases):
    b = bases if isinstance(bases, bytes) else bases.encode()
    return sum(1 for i in range(len(b) - 1) if b[i:i + 2] == b"CG")


def calls_for(rng, bases):
    return bytes(rng.randrange(256) for _ in range(n_cpg(bases)))


# seeds for which the forward sum differs from the reversed one AND from a pairwise tree, per read and per allele (test_pymeth checks)
SEED_MANY_CPG = 3
SEED_MANY_READS = 2
SEED_TWO_ALLELES = 7


def _boundaries():
    """CG across bases 63 | 64, 255 | 256 and 511 | 512 (lane, step and 4-bit step boundaries when the read starts aligned), nothing else"""
    b = ["A"] * 600
    for c in (63, 255, 511):
        b[c], b[c + 1] = "C", "G"
    return "".join(b)


def _many_cpg(seed):
    rng = random.Random(seed)
    bases = "TTA" + "CG" * 35 + "ACGT" * 35 + "GG"   # 70 CpGs inside the span (3, 3 + 70 + 140)
    return bases, bytes(rng.randrange(256) for _ in range(n_cpg(bases)))


def _many_reads(seed, n, two_alleles):
    """n kept reads, every one with its own level, ranks a permutation of input order"""
    rng = random.Random(seed)
    ranks = list(range(n))
    rng.shuffle(ranks)
    reads = []
    for i in range(n):
        length = (20 if i % 2 else 30) if two_alleles else 24
        bases = rand_bases(rng, 5, "AT") + ("CGA" * 10)[:length] + rand_bases(rng, 4, "AT")
        reads.append(rd(bases, calls_for(rng, bases), (5, 5 + length), ranks[i]))
    if two_alleles:
        return locus(2, (30, 20), (28, 32, 18, 22), reads, flipped=1)
    return one(reads)


def _cases():
    rng = random.Random(11)
    C = {}
    cg5 = "TTCGACGTTACGAT"   # CpGs at 2, 5, 10
    C["has_meth_0"] = ([one([rd(cg5, None, (0, 14), 0)])], {})
    C["empty_range"] = ([one([rd(cg5, b"", (0, 14), 0), rd(cg5, [10, 20, 30], (0, 14), 1)])], {})
    C["no_cpg_in_span"] = ([one([rd(cg5, [10, 20, 30], (6, 10), 0)])], {})
    C["c_before_span"] = ([one([rd(cg5, [10, 20, 30], (3, 9), 0)])], {})            # the CG at 2 is out, the one at 5 (index 1) is in
    C["c_last_of_span"] = ([one([rd(cg5, [10, 20, 30], (3, 6), 0)])], {})           # C at span_end - 1, its G outside: counts
    C["cg_ends_read"] = ([one([rd("AATTCG", [77], (1, 6), 0), rd("CG", [5], (0, 2), 1), rd("ACG", [200], (0, 1), 2)])], {})
    bd = _boundaries()
    C["boundaries"] = ([one([rd(bd, [1, 1, 32], (0, 600), 0), rd(bd, [9, 200, 31], (64, 512), 1), rd(bd, [9, 200, 31], (63, 256), 2),
                              rd("T" + bd, [1, 2, 3], (0, 601), 3), rd("TT" + bd, [1, 2, 3], (0, 602), 4), rd("TTT" + bd, [255, 254, 253], (257, 520), 5)])], {})
    C["unaligned_start"] = ([one([rd("A", None, (0, 1), 0), rd(cg5, [10, 20, 30], (0, 14), 1), rd("AC", None, (0, 0), 2), rd(cg5 * 3, [1, 1, 32] * 3, (1, 40), 3),
                                   rd("ACG", [3], (0, 3), 4), rd(cg5 * 40, calls_for(rng, cg5 * 40), (100, 500), 5)])], {})
    mb, mc = _many_cpg(SEED_MANY_CPG)
    C["many_cpg"] = ([one([rd(mb, mc, (3, 213), 0)])], {"order": "read"})
    C["anchor"] = ([one([rd("ACGTCGCG", [255, 0, 51], (2, 7), 0)])], {})
    C["sum_order_triple"] = ([one([rd("CGCGCG", [1, 1, 32], (0, 6), 0)])], {})   # (left-to-right differs from right-to-left; a tree of three does not)
    C["empty_span"] = ([one([rd(cg5, [10, 20, 30], (5, 5), 0), rd(cg5, [10], (0, 0), 1), rd(cg5, [10, 20, 30], (14, 14), 2)])], {})
    C["malformed_in_span"] = ([one([rd(cg5, [10, 20, 30], (0, 14), 0), rd(cg5, [10, 20], (0, 11), 1), rd(cg5, [10], (0, 14), 2)])], {"error": ("malformed", 1)})
    C["short_calls_beyond_span"] = ([one([rd(cg5, [10, 20], (0, 10), 0), rd(cg5, [10], (0, 5), 1), rd(cg5 * 30, [7] * 4, (3, 14), 2)])], {})
    two = lambda reads, **kw: locus(2, (10, 20), (8, 12, 18, 22), reads, **kw)
    span_of = lambda n: rd("AT" + ("CGT" * 20)[:n] + "AT", [40 + n] * 21, (2, 2 + n), None)
    def ranked(reads):
        for i, r in enumerate(reads):
            r["rank"] = i
        return reads
    C["one_allele"] = ([one(ranked([span_of(3), span_of(30)]))], {})
    C["two_alleles"] = ([two(ranked([span_of(10), span_of(11), span_of(19), span_of(22), span_of(15)]))], {})
    C["nearer_outside_interval"] = ([two(ranked([span_of(13), span_of(7), span_of(17), span_of(23), span_of(12)]))], {})
    C["equal_sizes_both"] = ([locus(2, (12, 12), (10, 14, 12, 12), ranked([span_of(12), span_of(13), span_of(15)]))], {})
    C["equal_distance_unequal_sizes"] = ([locus(2, (10, 14), (8, 14, 10, 16), ranked([span_of(12), span_of(11), span_of(13)]))], {})
    C["flipped"] = ([two(ranked([span_of(10), span_of(11), span_of(19), span_of(12)]), flipped=1),
                     locus(1, (10, 0), (8, 12, 0, 0), ranked([span_of(10)]), flipped=1)], {})   # (flipped is ignored unless n_alleles == 2)
    C["gt_size_differs"] = ([locus(2, (10, 20), (0, 40, 0, 40), ranked([span_of(14), span_of(16), span_of(9)]), gt_size=(10, 16)),
                             locus(2, (10, 20), (0, 40, 0, 40), ranked([span_of(14), span_of(16), span_of(9)]), gt_size=(18, 20), flipped=1)], {})
    C["gt_size_null"] = ([locus(2, (10, 20), (0, 40, 0, 40), ranked([span_of(14), span_of(16), span_of(9)]), gt_size=(10, 16)),
                          two(ranked([span_of(10), span_of(19)]), flipped=1)], {"gt_size_null": True})
    C["no_alleles"] = ([locus(0, (0, 0), (0, 0, 0, 0), [rd(cg5, [10, 20, 30], (0, 14), -1), rd(cg5, None, (-1, -1), -1)])], {})
    C["no_kept_reads"] = ([two([rd(cg5, [10, 20, 30], (0, 14), -1)]), locus(1, (10, 0), (8, 12, 0, 0), []), two(ranked([span_of(10), span_of(19)]))], {})
    C["many_reads"] = ([_many_reads(SEED_MANY_READS, 70, False)], {"order": "allele"})
    C["many_reads_two_alleles"] = ([_many_reads(SEED_TWO_ALLELES, 150, True)], {"order": "allele"})
    # unkept reads between kept ones, spans that would be invalid on a kept read, several loci in one call
    C["mixed"] = ([two([rd(cg5, [1, 2, 3], (-1, -1), -1), rd(cg5, [10, 20, 30], (2, 12), 1), rd(cg5, None, (0, 99), -1), rd(cg5 * 2, [9] * 6, (0, 20), 0)]),
                   one([rd(mb, mc, (3, 213), 0)]), C["boundaries"][0][0], _many_reads(5, 9, True)], {})
    return C


CASES = _cases()


def expected(loci, order="forward", gt_size_null=False, allele_order=None):
    """(allele_meth [2 per locus], meth_reads [2 per locus], read_meth [per read]) by tests/pymeth.py; gt_size_null: sizes from allele_len"""
    am, n, rm = [], [], []
    for L in loci:
        a, c, r = pymeth.locus_meth(L["n_alleles"], L["allele_len"] if gt_size_null else L["gt_size"], L["ci"], L["flipped"], [(x["bases"], x["meth"]) for x in L["reads"]],
                                    [x["span"] for x in L["reads"]], [x["rank"] for x in L["reads"]], order, allele_order)
        am += a; n += c; rm += r
    return np.array(am, np.float64), np.array(n, np.int32), np.array(rm, np.float64)


def pack_bam4(bases):
    codes = [BAM4.index(chr(b)) for b in bases] + [0]
    return bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(bases), 2))


def build(loci, encoding=0, lead=0, gt_size_null=False):
    """The ABI arrays of a case.  encoding 1: TRGT_READS_BAM4.  lead: bytes in front of the first read (moves every read's alignment)."""
    blob = bytearray(b"\x11" * lead)
    lrb, off, length, s0, s1, rank, calls, coff, has = [0], [], [], [], [], [], bytearray(), [0], []
    for L in loci:
        for x in L["reads"]:
            off.append(len(blob)); length.append(len(x["bases"]))
            blob += pack_bam4(x["bases"]) if encoding else x["bases"]
            s0.append(x["span"][0]); s1.append(x["span"][1]); rank.append(x["rank"])
            has.append(0 if x["meth"] is None else 1)
            calls += x["meth"] or b""
            coff.append(len(calls))
        lrb.append(len(off))
    nl = len(loci)
    arr = lambda v, t: np.array(list(v) or [0], t)
    return dict(n_loci=nl, n_reads=len(off), read_encoding=encoding, locus_read_begin=np.array(lrb, np.uint64), read_blob=arr(blob, np.uint8),
                read_off=arr(off, np.uint64), read_len=arr(length, np.uint32), span_start=arr(s0, np.int32), span_end=arr(s1, np.int32),
                read_rank=arr(rank, np.int32), n_alleles=arr((L["n_alleles"] for L in loci), np.int32),
                ci=arr((v for L in loci for v in L["ci"]), np.int32), allele_len=arr((v for L in loci for v in L["allele_len"]), np.uint32),
                gt_size=None if gt_size_null else arr((v for L in loci for v in L["gt_size"]), np.int32),
                flipped=arr((L["flipped"] for L in loci), np.uint8), meth=arr(calls, np.uint8), meth_off=np.array(coff, np.uint64), has_meth=arr(has, np.uint8))
