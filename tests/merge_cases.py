"""Designed sites for the merge path (trgt_merge_exact_batch / trgt_merge_exact_host), the smallest at which each step can go wrong, and
a seeded generator of random small sites.  A site is (entries_alleles, entries_gts) as trgt_amd.merge.pack takes it: per entry the alleles
(REF first, [] for a file without a record) and the flat genotype values in BCF encoding.  The expectation comes from tests/pymerge.py.
"""
import random

from trgt_amd.merge import VECTOR_END

REF = b"CAGCAGCAGCAG"
PAD = (0, 1, 2, 3, 1, 0, 3, 2, 2, 2, 1)   # filler bytes in front of allele k (cycled): equal sequences land at different offsets modulo 4


def U(i):
    return (i + 1) << 1


def P(i):
    return ((i + 1) << 1) | 1


U_MISSING, P_MISSING = 0, 1


def _pair(a, b, ref=REF):
    """two entries whose one ALT each is a / b, a third that repeats both the other way round"""
    return ([[ref, a], [ref, b], [ref, b, a]], [[U(0), U(1)], [U(1), U(1)], [U(1), P(2)]])


def _differ_at(n, k, lo=b"A", hi=b"C", fill=b"G"):
    """two sequences of n bytes that differ only in byte k"""
    return fill * k + lo + fill * (n - k - 1), fill * k + hi + fill * (n - k - 1)


def _wide(n_alleles, length=8, seed=3, n_distinct=None):
    """a site of exactly n_alleles input alleles: entries of a REF and two ALTs of `length` bases (the last entry takes the rest)"""
    rng = random.Random(seed * 7919 + n_alleles)
    ref = b"T" * length
    pool = [bytes(rng.choice(b"ACGT") for _ in range(length)) for _ in range(n_distinct or max(4, n_alleles // 3))]
    alleles, gts, left = [], [], n_alleles
    while left > 0:
        k = min(3, left) if left != 4 else 2
        alleles.append([ref] + [rng.choice(pool) for _ in range(k - 1)])
        gts.append([U(rng.randrange(k)), P(rng.randrange(k))])
        left -= k
    assert sum(len(a) for a in alleles) == n_alleles
    return (alleles, gts)


def designed(limit):
    """[(name, site)]; limit = trgt_merge_site_alleles_limit()"""
    c = []
    x, y = _differ_at(12, 11)
    c.append(("last_byte", _pair(y, x)))
    for k in (3, 4, 7, 8):
        x, y = _differ_at(13, k)
        c.append(("byte_%d" % k, _pair(y, x)))
    for k in (255, 256):
        x, y = _differ_at(300, k)
        c.append(("byte_%d" % k, _pair(y, x)))
    x, y = _differ_at(1500, 1203)
    c.append(("long_ref_and_alts", _pair(y, x, ref=b"ACGT" * 300)))
    c.append(("AAAB_BAAA", _pair(b"BAAA", b"AAAB")))
    c.append(("AAAB_BAAA_behind_key", _pair(b"GGGGGGGGBAAA", b"GGGGGGGGAAAB")))
    c.append(("0x7F_0x80", _pair(b"AC\x80GT", b"AC\x7fGT")))
    c.append(("0x7F_0x80_behind_key", _pair(b"ACGTACGTAC\x80", b"ACGTACGTAC\x7f")))
    c.append(("prefix", _pair(b"CAGCAGCAGA", b"CAGCAGCAG")))
    c.append(("prefix_same_length_order", ([[REF, b"CAGCAGCAGCA", b"CAGCAGCAGC", b"CAGCAGCAGCAGCAG"]], [[U(3), U(1), U(2)]])))
    c.append(("length_0", ([[REF, b"", b"A"], [REF, b"A", b""], [REF, b""]], [[U(1), U(2)], [U(1), U(2)], [P(1), P(0)]])))
    c.append(("length_0_ref", ([[b"", b"A"], [b"", b""]], [[U(0), U(1)], [U(1), U(0)]])))
    c.append(("equal_at_other_offsets", ([[REF, b"CAGCAGCAGCAGCAGCAGT"], [REF, b"CAGCAGCAGCAGCAGCAGT"], [REF, b"CAGCAGCAGCAGCAGCAGT", b"CAGCAGCAGCAGCAGCAGA"],
                                          [REF, b"CAGCAGCAGCAGCAGCAGA"], [REF, b"CAGCAGCAGCAGCAGCAGT"]],
                                         [[U(1), U(0)], [U(1), U(1)], [U(1), U(2)], [U(1), U(0)], [P(1), P(1)]])))
    c.append(("duplicates_in_one_entry", ([[REF, b"CAG", b"CAGCAG", b"CAG", b"CAG"], [REF, b"CAGCAG", b"CAGCAG"]], [[U(1), U(2), U(3), U(4)], [U(2), U(1)]])))
    c.append(("alt_equals_ref", ([[REF, b"CAG", REF], [REF, b"CAGCAGCAGCAGCAG"], [REF]], [[U(0), U(2)], [U(0), U(1)], [U(0), P(0)]])))
    c.append(("first_entries_empty", ([[], [], [REF, b"CAG"], [], [REF, b"CA"]], [[U_MISSING, U_MISSING], [], [U(1), U(0)], [P_MISSING, VECTOR_END], [U(1), U(1)]])))
    c.append(("all_entries_empty", ([[], [], []], [[U_MISSING, U_MISSING], [U_MISSING], []])))
    c.append(("no_entries", ([], [])))
    c.append(("ref_mismatch_last", ([[REF, b"CAG"], [], [REF, b"CA"], [REF[:-1] + b"T", b"CAG"]], [[U(1), U(0)], [], [U(1), U(1)], [U(0), U(1)]])))
    c.append(("ref_mismatch_first_of_two", ([[REF], [REF + b"A"], [REF + b"C"]], [[U(0)], [U(0)], [U(0)]])))
    c.append(("ref_mismatch_long", ([[b"ACGT" * 300], [b"ACGT" * 300], [b"ACGT" * 299 + b"ACGA"]], [[U(0)], [U(0)], [U(0)]])))
    c.append(("ref_mismatch_and_bad_gt", ([[REF, b"CAG"], [REF + b"G", b"CA"]], [[U(2), U(0)], [U(1), U(5)]])))
    c.append(("gt_equal_to_count", ([[REF, b"CAG"], [REF, b"CA"]], [[U(1), U(0)], [U(1), U(2)]])))
    c.append(("gt_in_empty_entry", ([[REF, b"CAG"], []], [[U(1), U(0)], [U(0)]])))
    c.append(("haploid_vector_end", ([[REF, b"CAG"], [REF, b"CA", b"CAG"]], [[U(1), VECTOR_END, U(0), U(1)], [P(2), VECTOR_END, U(1), VECTOR_END]])))
    c.append(("phased_and_missing", ([[REF, b"CAG"], [REF, b"CA"]], [[P(1), P(0), U_MISSING, P_MISSING], [P_MISSING, P(1), U(1), U_MISSING]])))
    for n in (64, 65, 256, 257):
        c.append(("alleles_%d" % n, _wide(n)))
    c.append(("alleles_300_all_distinct", _wide(300, length=11, n_distinct=4000)))
    c.append(("alleles_at_limit", _wide(limit, n_distinct=600)))
    c.append(("alleles_limit_plus_1", _wide(limit + 1, n_distinct=600)))
    return c


def has_hbm_tie(site):
    """two distinct ALTs of equal length and equal first 8 bytes: the ranking must go to the bytes"""
    alts = set(a for al in site[0] for a in al[1:] if len(a) > 8)
    keys = {}
    for a in alts:
        keys.setdefault((len(a), a[:8]), set()).add(a)
    return any(len(v) > 1 for v in keys.values())


def random_sites(n, seed):
    """small sites over a 2-letter alphabet and lengths 0-9 (now and then 8 bases more in front, so ties reach beyond the prefix key): equal
    sequences and key ties are the rule; statuses 1 to 3 appear now and then"""
    rng = random.Random(seed)
    sites = []
    for _ in range(n):
        stem = b"AC" * 4 if rng.random() < 0.75 else b""
        seq = lambda: stem + bytes(rng.choice(b"AC") for _ in range(rng.randrange(10)))  # noqa: E731
        ref = seq()
        alleles, gts = [], []
        for _e in range(rng.randrange(0, 8)):
            if rng.random() < 0.15:
                alleles.append([])
                gts.append([rng.choice((U_MISSING, P_MISSING)) for _g in range(rng.randrange(3))])
                continue
            al = [ref if rng.random() > 0.03 else seq()] + [seq() for _a in range(rng.randrange(0, 6))]
            g = []
            for _g in range(rng.randrange(0, 5)):
                r = rng.random()
                g.append(U_MISSING if r < 0.05 else P_MISSING if r < 0.1 else VECTOR_END if r < 0.15 else
                         rng.choice((U, P))(rng.randrange(len(al) + (1 if rng.random() < 0.03 else 0))))
            alleles.append(al)
            gts.append(g)
        sites.append((alleles, gts))
    return sites


RANDOM = random_sites(2000, 20261021)
# self-check: the generator does what it is for
assert sum(has_hbm_tie(s) for s in RANDOM) * 3 >= len(RANDOM), sum(has_hbm_tie(s) for s in RANDOM)

_EXPECTED = {}


def expected(sites):
    """per site (status, src, allele_map, gt_out) from tests/pymerge.py, input indices counted over the whole list; computed once per list"""
    key = id(sites)
    if key not in _EXPECTED:
        import pymerge
        out, first = [], 0
        for alleles, gts in sites:
            out.append(pymerge.site_arrays(alleles, gts, first))
            first += sum(len(a) for a in alleles)
        _EXPECTED[key] = (sites, out)
    return _EXPECTED[key][1]


def check_outputs(b, outs, sites, label=""):
    """every output array of a packed batch (trgt_amd.merge.pack / alloc_outputs, read back to the host) against the restatement"""
    seb, eab, egb, slot = b["site_entry_begin"], b["entry_allele_begin"], b["entry_gt_begin"], b["out_allele_begin"]
    for s, (status, src, amap, gt_out) in enumerate(expected(sites)):
        where = "%s site %d" % (label, s)
        assert int(outs["site_status"][s]) == status, where
        assert int(outs["out_n_alleles"][s]) == (len(src) if status == 0 else 0), where
        at = int(slot[s])
        assert [int(v) for v in outs["out_allele_src"][at:at + len(src)]] == src, where
        if status == 0:
            a0, a1 = int(eab[int(seb[s])]), int(eab[int(seb[s + 1])])
            g0, g1 = int(egb[int(seb[s])]), int(egb[int(seb[s + 1])])
            assert [int(v) for v in outs["allele_map"][a0:a1]] == amap, where
            assert [int(v) for v in outs["gt_out"][g0:g1]] == [v for g in gt_out for v in g], where
