"""What the cases of tests/snv_cluster_deep_cases.py are meant to exercise, asserted from the oracle's results and the restatement of
get_trs_with_clustering: the cluster genotyper keeps and orders reads on its own, so a case taken over from the deep size route could
stop meeting its condition and let tests/test_snv_cluster_deep_gpu.py pass without running the code it was built for.  No GPU, and
nothing here comes from the library.  The oracle's results are computed once per case and shared."""
import pytest

import snv_cluster_deep_cases as sc
from test_flank_cluster_deep_cases import no_room_arithmetic as tag_no_room_arithmetic
from test_flank_device_gpu import _ref
from test_repair_needs import group_needs

_CACHE = {}


def _results(oracle, name, full=False):
    """(loci, plain results, traces[, results with read metadata]) of a case of all_cases(), computed once"""
    from trgt_amd import locus
    if (name, full) not in _CACHE:
        loci, kw = next((loci, kw) for n, loci, kw in sc.all_cases() if n == name)
        params = locus.Params(**kw)
        plain = sc.plain_results(oracle, loci, params)
        _CACHE[(name, full)] = (loci, plain, [sc.route(L, q) for L, q in zip(loci, plain)], [_ref(oracle, L, params) for L in loci] if full else None)
    return _CACHE[(name, full)]


def _settled(t):
    return t is not None and not sc.over_a_cap(t) and not sc.undecided(t) and t["split"] is not None


def test_every_margin_is_far_from_the_rule(oracle):
    """the device decides at 2^-30 (1 + |M|): every search of every case but the 2 048-read one is undecided by far or decided by far"""
    for name, _, _ in sc.all_cases():
        if name == "offset cap":
            continue
        for t in _results(oracle, name)[2]:
            if t is not None and t["margin"] is not None and not sc.over_a_cap(t):
                assert t["margin"] <= sc.UNDECIDED or t["margin"] >= sc.DECIDED, (name, t["margin"])


def test_default_depth_keeps_250_of_257(oracle):
    loci, plain, tr, _ = _results(oracle, "default depth")
    assert len(loci[0]["reads"]) == 257 and len(plain[0]["kept_read"]) == 250 and _settled(tr[0])
    assert sc.expected_stats(loci, plain) == (1, 0, 0, 0)


def test_depths_keep_every_read_and_split(oracle):
    loci, plain, tr, _ = _results(oracle, "depths")
    assert [len(q["kept_read"]) for q in plain] == [257, 513, 1025, 256, 30]
    assert all(_settled(t) and not any(sc.lacks_majority(L, q, t)) for L, q, t in list(zip(loci, plain, tr))[:3])
    assert tr[3] is None and tr[4] is None  # the one-wave chain's
    assert all(sc.close_alleles(q) for q in plain)
    assert sc.expected_stats(loci, plain) == (3, 0, 0, 0)


@pytest.mark.parametrize("n", sorted(sc.SKIPS))
def test_skip_cases_sit_on_the_rounding_and_on_the_edges(oracle, n):
    loci, plain, tr, _ = _results(oracle, "skip %d" % n)
    assert sc.case_skip(n)[1] == sc.SKIPS[n] and n * (1.0 - 0.85) > sc.SKIPS[n] - 0.5 > n * 0.15 - 1e-9
    for t in tr:
        assert t["n"] == n and t["skip"] == sc.SKIPS[n] and t["region"] == (-300, 300)
    # the site exactly on either edge is called and splits the reads, one base outside there is no SNV at all
    assert [len(t["snvs"]) for t in tr] == [1, 0, 1, 0] and [_settled(t) for t in tr] == [True, False, True, False]
    # repeated values on both sides of the selected rank
    for L, t in zip(loci, tr):
        eo = sorted(L["end_offset"][r] for r in t["kept"])
        k = sc.SKIPS[n]
        assert eo[k - 2] == eo[k - 1] < eo[k] < eo[k + 1] == eo[k + 2]
    assert sc.expected_stats(loci, plain) == (2, 0, 0, 0)


def test_ties_alternate_across_the_round_boundary_and_cause_the_repair(oracle):
    loci, plain, tr, full = _results(oracle, "ties", full=True)
    t = tr[0]
    asg, mem, _ = t["split"]
    ties = [i for i, m in enumerate(mem) if len(m) == 2]
    assert ties == list(range(sc.TIE_FIRST, sc.TIE_FIRST + sc.N_TIES)) == [253, 254, 255, 256, 257]  # kept positions, on both sides of 256
    assert [asg[i] for i in ties] == [0, 1, 0, 1, 0]
    segs = sc.kept_segments(loci[0], plain[0], t["kept"])
    carriers = [i for i, m in enumerate(mem) if m == {0}]
    assert len(carriers) == 70 and sum(segs[i] == sc.sd.W63 for i in carriers) == 36  # 36 of 70 by assignment alone ...
    assert sum(1 for m in mem if 0 in m) == 75 and sc.lacks_majority(loci[0], plain[0], t) == (True, False)  # ... 36 of 75 with the tied reads
    assert full[0]["stats"]["n_wfa_cons"] - plain[0]["stats"]["n_wfa_cons"] == 75  # a tied read is a job of the round although it is assigned elsewhere
    assert sc.expected_stats(loci, plain) == (1, 1, 0, 0)


def test_margins(oracle):
    loci, plain, tr, _ = _results(oracle, "margin")
    assert 0 <= tr[0]["margin"] <= sc.UNDECIDED and 0 <= tr[1]["margin"] <= sc.UNDECIDED and tr[2]["margin"] >= 0.5
    assert sc.expected_stats(loci, plain) == (1, 0, 0, 2)


def test_repair_cases(oracle):
    loci, plain, tr, full = _results(oracle, "repair", full=True)
    lacks = [sc.lacks_majority(L, q, t) for L, q, t in list(zip(loci, plain, tr))[:4]]
    assert lacks[0] == (True, True) and sorted(lacks[1]) == [False, True] and lacks[2] == lacks[3] == (False, False)
    # [1]: the noisy group is the carriers', group 0, and its repaired allele is the longer one: swap, and the assignment flips
    assert lacks[1] == (True, False) and len(full[1]["alleles"][0]) < len(full[1]["alleles"][1])
    # [2] / [3]: the carriers (group 0) have the longer allele; the reference allele is first either way
    assert full[2]["alleles"] == [sc.CAG20.decode(), sc.CAG21.decode()] and full[3]["alleles"] == [sc.CAG21.decode(), sc.CAG20.decode()]
    # [4]: one SNV carried by every read: one profile, one candidate, no split -- and the host agrees
    assert len(tr[4]["snvs"]) == 1 and tr[4]["split"] is None and full[4]["alleles"] == plain[4]["alleles"]
    assert all(r["stats"]["n_wfa_cons"] > q["stats"]["n_wfa_cons"] for r, q in list(zip(full, plain))[:2])
    assert sc.expected_stats(loci, plain) == (4, 2, 0, 0)


def test_limits(oracle):
    loci, plain, tr, _ = _results(oracle, "snv cap")
    assert [len(t["snvs"]) for t in tr] == [sc.MAX_SNVS, sc.MAX_SNVS + 1] and sc.expected_stats(loci, plain) == (1, 0, 1, 0)
    loci, plain, tr, _ = _results(oracle, "hap cap")
    assert [len(t["haps"]) for t in tr] == [sc.MAX_HAPS, sc.MAX_HAPS + 1] and sc.expected_stats(loci, plain) == (1, 0, 1, 0)


def test_offset_cap_at_the_ceiling(oracle):
    loci, plain, tr, _ = _results(oracle, "offset cap")
    assert len(plain[0]["kept_read"]) == sc.CEILING == 2048 and [t["in_region"] for t in tr] == [sc.OFFS_CAP, sc.OFFS_CAP + 1] == [16384, 16385]
    assert _settled(tr[0]) and tr[0]["margin"] >= sc.DECIDED and len(tr[1]["snvs"]) == 1 and len(tr[1]["haps"]) <= sc.MAX_HAPS
    assert sc.expected_stats(loci, plain) == (1, 0, 1, 0)


def test_tags_and_snvs(oracle):
    loci, plain, tr, _ = _results(oracle, "tags and snvs")
    assert sc.tags_split(loci[0], plain[0]) and tr[0] is None
    assert loci[1]["hp_tag"] is not None and not sc.tags_split(loci[1], plain[1]) and _settled(tr[1]) and loci[2]["hp_tag"] is None and _settled(tr[2])
    assert sc.expected_stats(loci, plain) == (2, 0, 0, 0) and sc.tag_stats(loci, plain) == (1, 0, 0)
    loci, plain, tr, _ = _results(oracle, "tags and snvs repaired")
    assert tr[0] is None and sc.lacks_majority(loci[1], plain[1], tr[1]) == (True, True)
    assert sc.expected_stats(loci, plain) == (1, 1, 0, 0) and sc.tag_stats(loci, plain) == (1, 1, 0)


def no_room_arithmetic():
    """The SNV groups of sc.case_no_room are the tag groups of flank_cluster_deep_cases.case_no_room (129 reads of 54 bases, 128 of 57, no
    read in both), so the arithmetic of the tag route's test holds: the kb that admits the locus, fits round 1 and does not fit round 3.
    (With the route the lists have four parts; under TRGT_CLUSTER_ARENA_KB the arenas are capped by kb whatever the parts.)"""
    return tag_no_room_arithmetic()


def test_no_room_case_fits_round_1_and_not_round_3(oracle):
    loci, plain, tr, full = _results(oracle, "no room", full=True)
    n, q, t = sc.NO_ROOM_READS, plain[0], tr[0]
    segs = sc.kept_segments(loci[0], q, t["kept"])
    assert len(segs) == n and len(set(segs)) == n and q["stats"]["n_wfa_cons"] == n
    asg, mem, _ = t["split"]
    assert all(len(m) == 1 for m in mem) and sc.lacks_majority(loci[0], q, t) == (True, True)
    by_len = {g: sorted({len(s) for s, a in zip(segs, asg) if a == g}) for g in (0, 1)}
    assert sorted(by_len.values()) == [[sc.NO_ROOM_LO], [sc.NO_ROOM_HI]]  # the SNV groups are the alleles
    assert sorted(asg.count(g) for g in (0, 1)) == [n // 2, (n + 1) // 2]
    assert full[0]["stats"]["n_wfa_cons"] == 2 * n  # the third round: every read against the backbone of its group
    r3 = group_needs(sc.NO_ROOM_LO, (n + 1) // 2, (n + 1) // 2 * sc.NO_ROOM_LO)[0] + group_needs(sc.NO_ROOM_HI, n // 2, n // 2 * sc.NO_ROOM_HI)[0]
    kb = no_room_arithmetic()
    assert 31 <= kb <= 218 and r3 > 0
    assert sc.expected_stats(loci, plain, handed=(0,)) == (0, 0, 1, 0) and sc.expected_stats(loci, plain) == (1, 1, 0, 0)


def test_allele_cap_case(oracle):
    loci, plain, tr, full = _results(oracle, "allele cap", full=True)
    assert [len(a) for a in plain[0]["alleles"]] == [60, 60] and max(len(a) for a in full[0]["alleles"]) == 63 > sc.ALLELE_CAP >= 60
    assert _settled(tr[0]) and not any(sc.lacks_majority(loci[0], plain[0], tr[0]))


def test_purity_case_drops_reads_and_keeps_the_route(oracle):
    loci, plain, tr, _ = _results(oracle, "purity")
    assert all(sc.SHALLOW < len(q["kept_read"]) < len(L["reads"]) or len(L["reads"]) == 260 for L, q in zip(loci, plain))
    assert [len(q["kept_read"]) < len(L["reads"]) for L, q in zip(loci, plain)] == [True, True] and all(_settled(t) for t in tr)
    assert sc.expected_stats(loci, plain) == (2, 0, 0, 0)


def test_mixed_batch(oracle):
    loci, plain, tr, _ = _results(oracle, "mixed")
    assert [t is not None for t in tr] == [False, False, False, True, False, True, True]
    assert _settled(tr[3]) and tr[5]["split"] is None and plain[4]["n_alleles"] == 1
    assert sc.expected_stats(loci, plain, sc.MIXED_SETTING) == (1, 0, 0, 0) and sc.expected_stats(loci, plain) == (2, 0, 0, 0)


def test_six_routes_case(oracle):
    loci, plain, tr, _ = _results(oracle, "six routes")
    assert [t is not None for t in tr] == [False] * 5 + [True] and _settled(tr[5])
    assert sc.tag_stats(loci, plain) == (1, 0, 0) and sc.expected_stats(loci, plain) == (1, 0, 0, 0)
    assert all(sc.close_alleles(q) for q in plain)


def test_random_case_mostly_settles_on_the_device(oracle):
    """by the restatement, at least half of the loci that reach the search are settled on the device (not undecided, not over a limit):
    a property of the seed and the reference alone"""
    loci, plain, tr, _ = _results(oracle, "random")
    assert all(sc.SHALLOW < len(L["reads"]) <= 600 for L in loci) and len(loci) == 24
    reach = [t for t in tr if t is not None and t["margin"] is not None]
    settled = [t for t in reach if not sc.over_a_cap(t) and not sc.undecided(t)]
    assert len(reach) >= 4 and 2 * len(settled) >= len(reach), (len(reach), len(settled))
    done, _, room, und = sc.expected_stats(loci, plain)
    assert done >= 1 and done + room + und <= len(reach)
