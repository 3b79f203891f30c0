"""The conditions the cases of snv_cluster_cases.py claim, checked on the CPU with the oracle and the plain-Python restatement of the SNV
branch: what test_snv_cluster_gpu.py compares on the device is then what its docstrings say, and every count is predictable whatever
the device's exp and log round to."""
import pytest

import snv_cluster_cases as cc
import snv_split_cases as sc
from test_flank_device_gpu import _ref


def _params(kw):
    from trgt_amd import locus
    return locus.Params(**kw)


def _same(r, q):
    return r["alleles"] == q["alleles"] and list(r["classification"]) == list(q["classification"])


@pytest.fixture(scope="module")
def cases(oracle):
    out = {}
    for name, loci, kw in cc.all_cases():
        p = _params(kw)
        refs, plain = [_ref(oracle, L, p) for L in loci], [_ref(oracle, L, p, meta=False) for L in loci]
        out[name] = (loci, refs, plain, [cc.cluster_trace(L, q) for L, q in zip(loci, plain)])
    return out


def test_every_margin_is_tiny_or_wide_and_the_rule_predicts_the_oracle(cases):
    for name, (loci, refs, plain, traces) in cases.items():
        for l, (L, r, q, t) in enumerate(zip(loci, refs, plain, traces)):
            if t is None:
                continue
            if t["margin"] is not None:
                assert t["margin"] <= cc.UNDECIDED or t["margin"] >= cc.DECIDED, (name, l, t["margin"])
                if t["margin"] <= cc.UNDECIDED:
                    continue  # the host's own last bits decide
            if t["split"] is None:
                assert _same(r, q), (name, l)
                continue
            asg, mem, _ = t["split"]
            cls = [int(v) for v in r["classification"]]
            assert [int(v) for v in r["kept_read"]] == t["kept"] and cls in (asg, [1 - a for a in asg]), (name, l)
            lens = [int(q["span_end"][k]) - int(q["span_start"][k]) for k in t["kept"]]
            ivs = sorted((min(x for x, m in zip(lens, mem) if g in m), max(x for x, m in zip(lens, mem) if g in m)) for g in (0, 1))
            assert sorted(tuple(int(v) for v in c) for c in r["gt_ci"]) == ivs, (name, l)


def test_every_close_diploid_locus_is_on_the_route(cases):
    """every diploid cluster locus of at most 256 reads with mismatch lists, other than the ones meant to be far apart (and the tagged
    ones), has two cluster alleles at most 10 apart: the search runs for it"""
    for name, (loci, refs, plain, traces) in cases.items():
        if name == "random":  # (generated: motifs of up to 6 bases, up to 4 repeats apart)
            continue
        for l, (L, q, t) in enumerate(zip(loci, plain, traces)):
            if L.get("genotyper") != "cluster" or L.get("ploidy", 2) != 2 or len(L["reads"]) > 256 or L.get("mismatch_offsets") is None:
                assert t is None, (name, l)
                continue
            if (name, l) in cc.FAR_APART or (name, l) == ("mixed batch", 6):
                assert t is None and q["n_alleles"] == 2 and abs(len(q["alleles"][0]) - len(q["alleles"][1])) > 10, (name, l)
                continue
            if L.get("hp_tag") is not None and cc._tag_rule([L["hp_tag"][r] for r in q["kept_read"]])[1]:
                assert t is None, (name, l)
                continue
            assert t is not None, (name, l)


def test_reference_vectors(cases):
    loci, refs, plain, traces = cases["kats"]
    assert [int(v) for v in refs[0]["classification"]] == [0, 0, 0, 1, 1, 1] and traces[0]["split"] is not None
    assert traces[1] is not None and traces[1]["split"] is None and _same(refs[1], plain[1])
    assert cc.expected_stats(loci, plain) == (1, 0, 0, 0)


def test_plain_split_and_far_alleles(cases):
    loci, refs, plain, traces = cases["plain"]
    assert traces[0]["split"] is not None and traces[1] is None
    st = cc.expected_stats(loci, plain)
    assert st[0] == 1 and st[2:] == (0, 0)


@pytest.mark.parametrize("n", [3, 10, 30])
def test_skip_rounding(cases, n):
    loci, refs, plain, traces = cases["skip %d" % n]
    skip = cc.case_skip(n)[1]
    assert [t["skip"] for t in traces] == [skip] * 4
    assert [len(t["snvs"]) for t in traces] == [1, 0, 1, 0] and [t["split"] is not None for t in traces] == [True, False, True, False]
    assert cc.expected_stats(loci, plain) == (2, 0, 0, 0)


def test_call_threshold_and_fewest_fully_observed_reads(cases):
    loci, refs, plain, traces = cases["call threshold"]
    assert traces[0]["snvs"] == [-120, 85] and traces[0]["split"] is not None
    t = cases["least full"][3][0]
    assert t["n"] == 20 and t["skip"] == 3 and t["full"] == 14 and len(t["snvs"]) == 2 and t["split"] is not None
    assert cc.expected_stats(loci + cases["least full"][0], plain + cases["least full"][2]) == (2, 0, 0, 0)


def test_ties_join_both_groups(cases):
    loci, refs, plain, traces = cases["ties"]
    asg, mem, _ = traces[0]["split"]
    assert sum(m == {0, 1} for m in mem) == 2 and [asg[i] for i, m in enumerate(mem) if m == {0, 1}] == [0, 1]
    r = refs[0]
    assert sorted(r["alleles"]) == sorted([sc.Y60.decode(), sc.CAG21.decode()])          # by assignment alone: X60
    assert sorted(tuple(int(v) for v in c) for c in r["gt_ci"]) == [(60, 66), (60, 66)]  # ... (60, 63) and (60, 66)
    assert [list(r["classification"]).count(g) for g in (0, 1)] == [5, 5] and [sum(g in m for m in mem) for g in (0, 1)] == [6, 6]
    assert cc.expected_stats(loci, plain) == (1, 0, 0, 0)


def test_margins(cases):
    loci, refs, plain, traces = cases["margin"]
    assert traces[0]["margin"] <= cc.UNDECIDED and traces[1]["margin"] <= cc.UNDECIDED and traces[2]["margin"] >= cc.DECIDED
    assert cc.expected_stats(loci[:2], plain[:2]) == (0, 0, 0, 2) and cc.expected_stats(loci, plain) == (1, 0, 0, 2)


def test_repair_and_tail(cases):
    loci, refs, plain, traces = cases["repair"]
    assert cc.expected_stats(loci, plain) == (4, 2, 0, 0)
    assert all(r["stats"]["n_wfa_cons"] > 0 for r in refs[:2])
    carriers = lambda L, t: [1 if L["mismatch_offsets"][k] and -120 in L["mismatch_offsets"][k] else 0 for k in t["kept"]]
    for l in (1, 2, 3):  # the carriers are group 0 and hold the longer allele: the swap flips the assignment
        assert traces[l]["split"][0] == [1 - c for c in carriers(loci[l], traces[l])]
    assert [int(v) for v in refs[1]["classification"]] == carriers(loci[1], traces[1])
    assert refs[2]["alleles"] == [sc.CAG20.decode(), sc.CAG21.decode()] and refs[3]["alleles"] == [sc.CAG21.decode(), sc.CAG20.decode()]


def test_no_room_and_allele_cap(cases):
    loci, refs, plain, traces = cases["no room"]
    asg, mem, _ = traces[0]["split"]
    lens = sorted({int(plain[0]["span_end"][k]) - int(plain[0]["span_start"][k]) for k in traces[0]["kept"]})
    assert lens == [54, 57] and [sum(g in m for m in mem) for g in (0, 1)] == [12, 12] and all(len(m) == 1 for m in mem)
    assert cc.expected_stats(loci, plain) == (1, 1, 0, 0) and cc.expected_stats(loci, plain, handed=(0,)) == (0, 0, 1, 0)
    loci, refs, plain, traces = cases["allele cap"]
    assert [len(a) for a in plain[0]["alleles"]] == [60, 60] and max(len(a) for a in refs[0]["alleles"]) == 63
    assert 60 <= cc.ALLELE_CAP < 63 and traces[0]["split"] is not None
    assert cc.expected_stats(loci, plain, handed=(0,)) == (0, 0, 1, 0)


def test_forms_and_limits(cases):
    for name, want in (("forms", (3, 0, 0, 0)), ("beyond lds small", (1, 0, 0, 0)), ("beyond lds big", (2, 0, 0, 0)), ("purity", (3, 0, 0, 0)),
                       ("snv cap", (1, 0, 1, 0)), ("hap cap", (1, 0, 1, 0)), ("offset cap small", (1, 0, 1, 0)), ("offset cap big", (1, 0, 1, 0))):
        loci, refs, plain, traces = cases[name]
        assert cc.expected_stats(loci, plain) == want, name
    assert [len(t["snvs"]) for t in cases["snv cap"][3]] == [64, 65]
    assert [len(t["haps"]) for t in cases["hap cap"][3]] == [16, 17]
    assert [t["in_region"] for t in cases["offset cap small"][3]] == [512, 513] and [t["in_region"] for t in cases["offset cap big"][3]] == [2048, 2049]


def test_tags_and_snvs(cases):
    loci, refs, plain, traces = cases["tags and snvs"]
    assert traces[0] is None and traces[1]["split"] is not None and cc.expected_stats(loci, plain) == (1, 0, 0, 0)
    loci, refs, plain, traces = cases["tags and snvs repaired"]
    assert traces[0] is None and cc.expected_stats(loci, plain) == (1, 1, 0, 0)
    import flank_cluster_cases as fc
    assert fc.expected_stats(loci, plain) == (1, 1, 0)  # the tagged one, by the tag route's restatement


def test_mixed_batch(cases):
    loci, refs, plain, traces = cases["mixed batch"]
    assert [t is not None for t in traces] == [False, True, False, False, True, False, False]
    assert traces[4]["split"] is None and cc.expected_stats(loci, plain) == (1, 0, 0, 0)
    assert sc.expected_stats(loci, plain) == (2, 0, 0, 0)  # the size route's restatement: the two size loci


def test_random_loci_are_all_decided(cases):
    loci, refs, plain, traces = cases["random"]
    st = cc.expected_stats(loci, plain)
    assert st[3] == 0 and st[2] == 0 and st[0] >= 5, st
