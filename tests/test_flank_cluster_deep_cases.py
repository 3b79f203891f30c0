"""What the cases of tests/flank_cluster_deep_cases.py are meant to exercise, asserted from the oracle's results and the restatement of
the tag rule: a case that no longer meets its condition would let tests/test_flank_cluster_deep_gpu.py pass without running the code it
was built for.  No GPU, and nothing here comes from the library.  The oracle's results are computed once per case and shared."""
import functools

import pytest

import flank_cluster_deep_cases as fc
from test_flank_device_gpu import _ref, _tag_rule
from test_repair_needs import group_needs


def _params(kw):
    from trgt_amd import locus
    return locus.Params(**kw)


_CACHE = {}


def _results(oracle, name, loci, kw, full=False):
    """(plain results, routes[, results with read metadata]) of a case, computed once"""
    key = (name, tuple(sorted(kw.items())), full)
    if key not in _CACHE:
        params = _params(kw)
        plain = fc.plain_results(oracle, loci, params)
        routes = [fc.route(L, q) for L, q in zip(loci, plain)]
        _CACHE[key] = (plain, routes, [_ref(oracle, L, params) for L in loci] if full else None)
    return _CACHE[key]


def test_depths_keep_the_counts_they_claim(oracle):
    (one, kw1), (many, kw2) = fc.case_depths()
    plain, routes, _ = _results(oracle, "depths 1", one, kw1)
    assert len(one[0]["reads"]) == 257 and len(plain[0]["kept_read"]) == 250 and routes[0] is not None
    plain, routes, _ = _results(oracle, "depths 2", many, kw2)
    assert [len(q["kept_read"]) for q in plain] == [257, 300, 513, 1025]
    assert all(r is not None and min(r[1]) == 1.0 for r in routes)
    assert all(abs(len(q["alleles"][0]) - len(q["alleles"][1])) <= 10 for q in plain)
    assert fc.expected_stats(many, plain) == (4, 0, 0)


def test_the_ceiling_locus_keeps_2048_reads(oracle):
    loci = fc.case_ceiling()
    plain, routes, _ = _results(oracle, "ceiling", loci, fc.DEEP)
    assert len(plain[0]["kept_read"]) == fc.CEILING == 2048 and routes[0] is not None and routes[0][1] == [1.0, 1.0]
    assert sorted(len(a) for a in plain[0]["alleles"]) == [60, 63]


def test_tags_against_the_clusters_change_the_genotype(oracle):
    loci = fc.case_tags_against_clusters()
    plain, routes, full = _results(oracle, "against", loci, fc.DEEP, full=True)
    assert routes[0] is not None and routes[0][1] == [0.5, 0.5]
    assert [len(a) for a in full[0]["alleles"]] == [60, 60] and [tuple(int(v) for v in c) for c in full[0]["gt_ci"]] == [(60, 63), (60, 63)]
    assert full[0]["alleles"] != plain[0]["alleles"]


def test_homozygous_loci_take_the_route(oracle):
    loci = fc.case_homozygous()
    plain, routes, _ = _results(oracle, "homozygous", loci, fc.DEEP)
    assert all(r is not None for r in routes)
    assert plain[0]["alleles"] == [fc.CAG20.decode()] * 2
    cls = [int(v) for v in plain[0]["classification"]]
    assert all(cls[i] != cls[i + 1] for i in range(len(cls) - 1))  # the even / odd split of a homozygous locus
    assert abs(len(plain[1]["alleles"][0]) - len(plain[1]["alleles"][1])) <= 10
    assert plain[1]["stats"]["n_wfa_cons"] == 2 * len(plain[1]["kept_read"])  # small_group_is_outlier: a second round over all kept reads
    assert fc.expected_stats(loci, plain) == (2, 0, 0)


def test_acceptance_threshold_on_either_side_and_an_empty_group(oracle):
    assert 182.0 / 260.0 >= 0.7 and not 181.0 / 260.0 >= 0.7
    loci = fc.case_threshold()
    plain, routes, _ = _results(oracle, "threshold", loci, fc.DEEP)
    assert all(len(q["kept_read"]) == 260 for q in plain)
    assert routes[0] is not None and routes[1] is None and routes[2] is None
    assert [sum(h in (1, 2) for h in fc.kept_tags(L, q)) for L, q in zip(loci, plain)] == [182, 181, 260]
    assert set(_tag_rule(fc.kept_tags(loci[2], plain[2]))[0]) == {0}
    assert all(not any(L["mismatch_offsets"]) for L in loci)


def test_untagged_reads_on_both_sides_of_the_round_boundary(oracle):
    loci = fc.case_boundary()
    plain, routes, full = _results(oracle, "boundary", loci, fc.DEEP, full=True)
    L, q = loci[0], plain[0]
    tags = fc.kept_tags(L, q)
    assert [i for i, h in enumerate(tags) if h is None] == [10, 70, 100, 260] and len(tags) == 368
    assert routes[0] is not None
    asg = routes[0][0]
    c = fc.group_counts(L, q, asg, 0)
    assert c[fc.X60] == c[fc.Y60] == 133  # the tie the case is built for: the first in byte order wins
    assert full[0]["alleles"] == [fc.X60.decode(), fc.W63.decode()]
    wrong = fc.group_counts(L, q, fc.tag_rule_restart(tags, 256), 0)  # a count that starts again with the second round of the workgroup
    assert wrong[fc.Y60] == 134 and wrong[fc.X60] == 133


def test_ties(oracle):
    loci = fc.case_ties()
    plain, routes, full = _results(oracle, "ties", loci, fc.DEEP, full=True)
    assert all(r is not None for r in routes)
    assert all(abs(len(q["alleles"][0]) - len(q["alleles"][1])) <= 10 for q in plain)
    counts = [fc.group_counts(L, q, r[0], 0) for L, q, r in zip(loci, plain, routes)]
    for k in (0, 1):  # equal counts, equal lengths: the first in byte order, in both read orders
        assert counts[k] == {fc.CAG20: 65, fc.CAA_CAG19: 65} and fc.CAA_CAG19 < fc.CAG20
        assert fc.CAA_CAG19.decode() in full[k]["alleles"] and fc.CAG20.decode() not in full[k]["alleles"]
    # median (60 + 62) / 2 = 61: both at distance 1
    assert counts[2] == {fc.CAG20: 65, fc.CAG20_CA: 65} and fc.CAG20_CA.startswith(fc.CAG20)
    assert fc.CAG20.decode() in full[2]["alleles"] and fc.CAG20_CA.decode() not in full[2]["alleles"]  # a proper prefix comes first
    assert counts[3] == {fc.CAG20: 65, fc.AAG_CAG19_CA: 65} and fc.AAG_CAG19_CA < fc.CAG20 and len(fc.AAG_CAG19_CA) == 62
    assert fc.AAG_CAG19_CA.decode() in full[3]["alleles"] and fc.CAG20.decode() not in full[3]["alleles"]  # not the first in kept order
    segs3 = fc.kept_segments(loci[3], plain[3])
    assert segs3.index(fc.CAG20) < segs3.index(fc.AAG_CAG19_CA)
    # median ties: even and odd group sizes
    assert sum(counts[4].values()) == 130 and sum(counts[5].values()) == 131
    for k in (4, 5):
        assert counts[k][fc.CAG20] == counts[k][b"CAG" * 22] == 52 and routes[k][1][0] < 0.5
        assert full[k]["stats"]["n_wfa_cons"] > plain[k]["stats"]["n_wfa_cons"]  # the group is repaired from a60: a third round
    assert counts[6] == {b"AAG" + fc.CAG20: 65, fc.CAG20: 65} and fc.CAG20.decode() in full[6]["alleles"]
    assert fc.expected_stats(loci, plain) == (7, 2, 0)


def test_repair_cases_align_in_a_third_round(oracle):
    loci = fc.case_repair()
    plain, routes, full = _results(oracle, "repair", loci, fc.DEEP, full=True)
    assert routes[0] is not None and routes[0][1][0] == 0.2 and routes[0][1][1] == 1.0
    assert routes[1] is not None and max(routes[1][1]) == 0.2
    for q, f in zip(plain, full):
        assert f["stats"]["n_wfa_cons"] > q["stats"]["n_wfa_cons"] > 0
    assert fc.expected_stats(loci, plain) == (2, 2, 0)


def test_reference_first_cases_swap_and_flip(oracle):
    loci = fc.case_reference_first()
    plain, routes, full = _results(oracle, "reference", loci, fc.DEEP, full=True)
    assert all(r is not None for r in routes)
    assert full[0]["alleles"] == [fc.CAG20.decode(), fc.CAG21.decode()] and full[1]["alleles"] == [fc.CAG21.decode(), fc.CAG20.decode()]
    # tag 1 carries the longer allele: after the swap its reads are allele 1; with the reference allele moved to the front, allele 0 again
    for f, L, want in zip(full, loci, (1, 0)):
        assert all(int(c) == (want if L["hp_tag"][int(r)] == 1 else 1 - want) for r, c in zip(f["kept_read"], f["classification"]))


@pytest.mark.parametrize("kw", [fc.PURITY, dict(fc.PURITY, **fc.DEEP)])
def test_purity_case_keeps_the_route(oracle, kw):
    loci = fc.case_purity()
    plain, routes, _ = _results(oracle, "purity", loci, kw)
    assert all(r is not None for r in routes) and all(len(L["reads"]) > 256 for L in loci)
    assert all(len(q["kept_read"]) < min(len(L["reads"]), kw.get("max_depth", 250)) + 1 for L, q in zip(loci, plain))
    assert any(len(q["kept_read"]) < min(len(L["reads"]), kw.get("max_depth", 250)) for L, q in zip(loci, plain))  # the filter dropped reads


def test_mixed_batch(oracle):
    import flank_cluster_cases as shallow
    loci = fc.case_mixed()
    plain, routes, _ = _results(oracle, "mixed", loci, fc.DEEP)
    assert [L["genotyper"] for L in loci] == ["size", "cluster", "cluster", "cluster", "cluster", "size", "cluster"]
    assert [len(L["reads"]) for L in loci] == [24, 24, 300, 100, 280, 18, 270]
    assert [r is not None for r in routes] == [False, False, True, False, False, False, False]
    assert plain[4]["n_alleles"] == 1 and sorted(len(a) for a in plain[6]["alleles"]) == [60, 90]
    assert fc.expected_stats(loci, plain) == (1, 0, 0)
    assert shallow.expected_stats(loci, plain) == (2, 0, 0)  # the one-wave route's loci: [1] and [3]
    # ... and again beside a 300-read and a 301-read locus, at cluster_max_reads = 300: every deep locus of the batch is within the setting
    more = loci + fc.case_setting_300()
    plain2, _, _ = _results(oracle, "mixed + setting", more, fc.DEEP)
    assert max(len(L["reads"]) for L in loci) == 300 and [len(L["reads"]) for L in more[-2:]] == [300, 301]
    assert fc.expected_stats(more, plain2, 300) == (2, 0, 0) and fc.expected_stats(more, plain2) == (3, 0, 0)
    assert sum(L["genotyper"] == "cluster" and len(L["reads"]) <= 300 for L in more) == 6


def test_setting_300(oracle):
    loci = fc.case_setting_300()
    plain, _, _ = _results(oracle, "setting", loci, fc.DEEP)
    assert [len(L["reads"]) for L in loci] == [300, 301]
    assert fc.expected_stats(loci, plain, 300) == (1, 0, 0) and fc.expected_stats(loci, plain) == (2, 0, 0)


def test_entry_point_case(oracle):
    loci = fc.case_entry_points()
    plain, _, _ = _results(oracle, "entry", loci, fc.DEEP)
    assert fc.expected_stats(loci, plain) == (4, 1, 0)


@functools.lru_cache(maxsize=None)
def no_room_arithmetic():
    """TRGT_CLUSTER_ARENA_KB = kb caps each arena of the deep chain (CIGAR: 256 kb words, results: 1 024 kb bytes, scratch: 256 kb words)
    and the deep pair budget (65 536 kb bytes, 60 bytes per pair: an alignment job of 48, a score, a matrix entry).  The arenas are not rolled
    back between the rounds.  For fc.case_no_room -- 257 kept reads, 129 segments of 54 and 128 of 57 bases, round 1 with every read a
    member of one of two groups, no second round -- round 1 takes between r1_min and r1_max whatever the grouping and the backbones,
    round 3 (tag group 0: the 129 reads of 54 bases, group 1: the 128 of 57) exactly r3 CIGAR words.  Returns the kb that admits the locus,
    fits round 1 and does not fit round 3."""
    n, lo, hi = fc.NO_ROOM_READS, fc.NO_ROOM_LO, fc.NO_ROOM_HI
    n_lo, n_hi = (n + 1) // 2, n // 2
    mbytes = n_lo * lo + n_hi * hi
    r1_min = n * (lo + 1) + mbytes                       # CIGAR words: one slot of bb + len + 1 per member
    r1_max = (n * (hi + 1) + mbytes, mbytes + 2 * (hi + 16 + 15), 3 * n)  # CIGAR words, result bytes, scratch words
    r3 = group_needs(lo, n_lo, n_lo * lo)[0] + group_needs(hi, n_hi, n_hi * hi)[0]
    kb = -(-r1_max[0] // 256)
    assert r1_max[0] <= kb * 256 < r1_min + r3 and r1_max[1] <= kb * 1024 and r1_max[2] <= kb * 256
    assert n * (n - 1) // 2 * 60 <= kb << 16  # the pair budget admits the locus
    return kb


def test_no_room_case_fits_round_1_and_not_round_3(oracle):
    loci = fc.case_no_room()
    plain, routes, full = _results(oracle, "no room", loci, fc.DEEP, full=True)
    q = plain[0]
    n = fc.NO_ROOM_READS
    segs = fc.kept_segments(loci[0], q)
    assert len(segs) == n and len(set(segs)) == n
    assert sorted(len(s) for s in segs) == [fc.NO_ROOM_LO] * ((n + 1) // 2) + [fc.NO_ROOM_HI] * (n // 2)
    assert q["stats"]["n_wfa_cons"] == n  # one round, every kept read a member of one group: nothing for a second round
    assert sorted(len(a) for a in q["alleles"]) == [fc.NO_ROOM_LO, fc.NO_ROOM_HI]
    assert routes[0] is not None and max(routes[0][1]) < 0.5
    asg = routes[0][0]
    assert all((len(s) == fc.NO_ROOM_LO) == (a == 0) for s, a in zip(segs, asg))  # the tag groups are the alleles
    assert full[0]["stats"]["n_wfa_cons"] == 2 * n  # the third round: every read against the backbone of its tag group
    assert 31 <= no_room_arithmetic() <= 218
