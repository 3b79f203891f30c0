"""The conditions that the cases of tests/test_flank_deep_gpu.py claim, checked with the oracle and the restatement of the tag rule alone
(flank_deep_cases.py): no GPU, and no library under test beyond trgt_amd.locus.Params."""
import flank_deep_cases as fc
from test_flank_device_gpu import _tag_rule
from trgt_amd.locus import Params


def _pair(oracle, loci, kw):
    return fc.oracle_pair(oracle, loci, Params(**kw))


def _changed(r, q):
    return sum(int(a) != int(b) for a, b in zip(r["classification"], q["classification"]))


def test_kept_counts_per_case(oracle):
    (one, kw1), (many, kw2) = fc.case_depths()
    assert [len(q["kept_read"]) for q in _pair(oracle, one, kw1)[1]] == [250]
    assert [len(q["kept_read"]) for q in _pair(oracle, many, kw2)[1]] == [257, 300, 513, 256, 30]
    assert [len(L["reads"]) for L in one + many] == [257, 257, 300, 513, 256, 30]
    assert [len(q["kept_read"]) for q in _pair(oracle, fc.case_ceiling(), fc.DEEP)[1]] == [fc.CEILING]
    assert [len(q["kept_read"]) for q in _pair(oracle, fc.case_threshold(), fc.DEEP)[1]] == [260] * 5
    assert all(len(q["kept_read"]) > 256 for q in _pair(oracle, fc.case_purity(), dict(fc.PURITY, **fc.DEEP))[1][1:])
    for case in (fc.case_ties, fc.case_repair, fc.case_reference_first, fc.case_hand_back, fc.case_boundary, fc.case_tags_against_lengths):
        assert all(256 < len(L["reads"]) <= fc.CEILING for L in case())


def test_tags_against_lengths_changes_classifications(oracle):
    loci = fc.case_tags_against_lengths()
    for kw in ({}, fc.DEEP):
        (r,), (q,) = _pair(oracle, loci, kw)
        assert r["alleles"] == q["alleles"] and _changed(r, q) >= 60
    assert _changed(*[p[0] for p in _pair(oracle, loci, fc.DEEP)]) == 100


def test_threshold_pair(oracle):
    loci = fc.case_threshold()
    _, plain = _pair(oracle, loci, fc.DEEP)
    assert 182.0 / 260.0 >= 0.7 and not 181.0 / 260.0 >= 0.7
    assert [fc.on_route(L, q, fc.CEILING) is not None for L, q in zip(loci, plain)] == [True, False, False, True, False]
    assert [sum(h in (1, 2) for h in fc.kept_tags(L, q)) for L, q in zip(loci, plain)] == [182, 181, 260, 182, 181]
    assert all(not any(L["mismatch_offsets"]) for L in loci)  # the refused ones stay on the device with the length genotype


def test_boundary_condition(oracle):
    (L,) = fc.case_boundary()
    (r,), (q,) = _pair(oracle, [L], fc.DEEP)
    tags = fc.kept_tags(L, q)
    lens = [len(s) for s in fc.kept_segments(L, q)]
    assert len(tags) >= 261 and len(set(lens[:261])) == 1
    assert [i for i, h in enumerate(tags) if h is None] == [10, 70, 100, 260]
    right, ok = _tag_rule(tags)
    assert ok and [right[i] for i in (10, 70, 100, 260)] == [0, 1, 0, 1]
    top = lambda asg: sorted(fc.group_counts(L, q, asg, 0).items(), key=lambda kv: (-kv[1], kv[0]))[0][0]
    without = [a if h is not None else -1 for a, h in zip(right, tags)]
    c = fc.group_counts(L, q, without, 0)
    assert c[fc.X60] == c[fc.Y60] == max(c.values())  # tied without the untagged reads
    assert top(right) == fc.X60 and top(fc.tag_rule_restart(tags, 64)) == fc.Y60 and top(fc.tag_rule_restart(tags, 256)) == fc.Y60
    assert r["alleles"][0] == fc.X60.decode()


def test_tie_cases_pick_what_they_claim(oracle):
    loci = fc.case_ties()
    refs, plain = _pair(oracle, loci, fc.DEEP)
    for L, q in zip(loci, plain):
        asg, repaired = fc.on_route(L, q, fc.CEILING)
        c = fc.group_counts(L, q, asg, 0)
        assert asg.count(0) > 128 and sorted(c.values())[-1] == sorted(c.values())[-2]  # equal multiplicity at the top
    assert [fc.on_route(L, q, fc.CEILING)[1] for L, q in zip(loci, plain)] == [True, False, False]
    assert refs[0]["stats"]["n_wfa_cons"] > 0 and refs[0]["alleles"][0] == fc.CAG20.decode()  # repaired from a60: the vote restores it
    assert refs[1]["alleles"][0] == fc.CAG20.decode() and refs[2]["alleles"][0] == fc.CAG20.decode()
    med = sorted(len(s) for s, a in zip(fc.kept_segments(loci[2], plain[2]), fc.on_route(loci[2], plain[2], fc.CEILING)[0]) if a == 0)
    assert len(med) % 2 == 0 and (med[len(med) // 2 - 1] + med[len(med) // 2]) % 2 == 1  # the median is x.5 and truncates


def test_repair_cases_align_and_swap(oracle):
    loci = fc.case_repair()
    refs, plain = _pair(oracle, loci, fc.DEEP)
    assert all(r["stats"]["n_wfa_cons"] > 0 for r in refs)
    assert [fc.on_route(L, q, fc.CEILING)[1] for L, q in zip(loci, plain)] == [True, True, True]
    sw = refs[2]
    assert [int(v) for v in sw["classification"]] == [1 - (loci[2]["hp_tag"][int(r)] - 1) for r in sw["kept_read"]]
    assert len(sw["alleles"][0]) < len(sw["alleles"][1])
    (r,), (q,) = _pair(oracle, fc.case_ceiling(noisy=True), fc.DEEP)
    assert r["stats"]["n_wfa_cons"] > 0 and fc.on_route(fc.case_ceiling(noisy=True)[0], q, fc.CEILING)[1]
    hb = fc.case_hand_back()
    refs, plain = _pair(oracle, hb, fc.DEEP)
    assert [fc.on_route(L, q, fc.CEILING)[1] for L, q in zip(hb, plain)] == [True, False] and refs[0]["stats"]["n_wfa_cons"] > 0
    assert max(len(s) for s in fc.kept_segments(hb[0], plain[0])) > 60


def test_reference_first(oracle):
    refs, _ = _pair(oracle, fc.case_reference_first(), fc.DEEP)
    assert refs[0]["alleles"] == [fc.CAG20.decode(), fc.CAG21.decode()] and refs[1]["alleles"] == [fc.CAG21.decode(), fc.CAG20.decode()]


def test_mixed_and_entry_point_statistics(oracle):
    loci, snv = fc.case_mixed()
    for kw in ({}, fc.DEEP):
        _, plain = _pair(oracle, loci, kw)
        assert fc.expected_stats(loci, plain, fc.CEILING, snv) == ((3, 0, 2, 2), (5, 0, 0, 0))
        assert fc.expected_stats(loci, plain, fc.SHALLOW, snv)[0] == (1, 0, 0, 0)  # the flank setting alone: deep loci are the host's from the start
    two = fc.case_setting_300()
    assert fc.expected_stats(two, _pair(oracle, two, fc.DEEP)[1], 300) == ((1, 0, 0, 1), (1, 0, 0, 0))


def test_random_floors(oracle):
    routed = repaired = 0
    for loci, kw in fc.case_random():
        assert all(257 <= len(L["reads"]) <= 400 for L in loci)
        stats, _ = fc.expected_stats(loci, _pair(oracle, loci, kw)[1], fc.CEILING)
        routed += stats[0]; repaired += stats[1]
    assert routed >= 5 and repaired >= 2
