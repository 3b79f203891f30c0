"""The conditions the cases of snv_deep_cases.py claim, checked on the CPU with the oracle and the plain-Python restatement of the SNV
branch alone: what test_snv_deep_gpu.py compares on the device is then what the docstrings say, and every count is predictable whatever
the device's exp and log round to."""
import pytest

import flank_deep_cases as fc
import snv_deep_cases as dc
import snv_split_cases as sc


def _params(kw):
    from trgt_amd import locus
    return locus.Params(**kw)


def _same(r, q):
    return r["alleles"] == q["alleles"] and list(r["classification"]) == list(q["classification"])


@pytest.fixture(scope="module")
def cases(oracle):
    out = {}
    for name, loci, kw in dc.all_cases():
        refs, plain = fc.oracle_pair(oracle, loci, _params(kw))
        out[name] = (loci, refs, plain, [dc.locus_trace(L, q) for L, q in zip(loci, plain)])
    return out


def test_every_margin_is_tiny_or_wide_and_the_rule_predicts_the_oracle(cases):
    for name, (loci, refs, plain, traces) in cases.items():
        for l, (L, r, q, t) in enumerate(zip(loci, refs, plain, traces)):
            if t is None:
                continue
            assert dc.SHALLOW < len(L["reads"]) <= dc.CEILING
            if t["margin"] is not None:
                assert t["margin"] <= dc.UNDECIDED or t["margin"] >= dc.DECIDED, (name, l, t["margin"])
                if t["margin"] <= dc.UNDECIDED:
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


def test_depths(cases):
    loci, refs, plain, traces = cases["depths"]
    assert [len(L["reads"]) for L in loci] == [257, 513, 256, 30] and [t is not None for t in traces] == [True, True, False, False]
    assert [t["n"] for t in traces[:2]] == [257, 513] and all(t["split"] is not None for t in traces[:2])
    assert sc.locus_trace(loci[2], plain[2])["split"] is not None  # the 256-read locus is the one-wave route's
    assert dc.expected_stats(loci, plain) == ((4, 0, 0, 0), (2, 0, 0, 2))
    assert dc.expected_stats(loci, plain, max_reads=dc.SHALLOW) == (sc.expected_stats(loci, plain), (0, 0, 0, 0))


@pytest.mark.parametrize("n", sorted(dc.SKIPS))
def test_skip_rounding_and_repeated_values_around_the_rank(cases, n):
    assert 270 * (1.0 - 0.85) > 40.5 and 290 * (1.0 - 0.85) > 43.5 and 270 * 0.15 == 40.5 and 290 * 0.15 == 43.5
    loci, refs, plain, traces = cases["skip %d" % n]
    skip = dc.case_skip(n)[1]
    assert [t["skip"] for t in traces] == [skip] * 4 and [t["region"] for t in traces] == [(-300, 300)] * 4
    assert [len(t["snvs"]) for t in traces] == [1, 0, 1, 0] and [t["split"] is not None for t in traces] == [True, False, True, False]
    for L, t in zip(loci, traces):
        so, eo = sorted(L["start_offset"][k] for k in t["kept"]), sorted(L["end_offset"][k] for k in t["kept"])
        # one less or one more selects another value, and the values next to the selected one are repeated
        assert eo[skip - 2:skip + 3] == [290, 290, 300, 310, 310] and so[n - 3 - skip:n + 2 - skip] == [-310, -310, -300, -290, -290]
        assert L["start_offset"] != sorted(L["start_offset"]) and L["end_offset"] != sorted(L["end_offset"])
    assert dc.expected_stats(loci, plain) == ((2, 0, 0, 0), (4, 0, 0, 2))


def test_call_threshold(cases):
    loci, refs, plain, traces = cases["call threshold"]
    assert 52.0 / 260.0 >= 0.20 and not 51.0 / 260.0 >= 0.20
    assert traces[0]["n"] == 260 and traces[0]["snvs"] == [-150, -120, 85] and traces[0]["split"] is not None
    assert traces[1]["in_region"] == 153 and traces[1]["snvs"] == [] and traces[1]["split"] is None
    assert dc.expected_stats(loci, plain) == ((1, 0, 0, 0), (2, 0, 0, 1))


def test_fully_observed_reads_at_their_fewest(cases):
    t = cases["least full"][3][0]
    assert t["n"] == 260 and t["skip"] == 39 and t["full"] == 260 - 2 * 39 and t["full"] / t["n"] >= 0.40 and len(t["snvs"]) == 2 and t["split"] is not None


def test_ties_cross_the_round_boundary_and_cause_the_repair(cases):
    loci, refs, plain, traces = cases["ties"]
    L, q, t = loci[0], plain[0], traces[0]
    asg, mem, _ = t["split"]
    tied = [i for i, m in enumerate(mem) if m == {0, 1}]
    assert tied == list(range(dc.TIE_FIRST, dc.TIE_FIRST + dc.N_TIES)) and tied[0] < 256 <= tied[-1]
    assert [asg[i] for i in tied] == [0, 1, 0, 1, 0]
    restarted = [k % 2 for k in range(256 - tied[0])] + [k % 2 for k in range(tied[-1] - 255)]
    assert restarted != [asg[i] for i in tied]  # a count that starts again at the boundary is visible in the classification
    assert dc.needs_repair(L, q, t) == (True, False)
    # by assignment alone group 0 has its majority sequence
    from collections import Counter
    segs = dc.kept_segments(L, q, t["kept"])
    own = [s for s, m in zip(segs, mem) if m == {0}]
    assert max(Counter(own).values()) / len(own) >= 0.5 and refs[0]["stats"]["n_wfa_cons"] > 0
    assert dc.expected_stats(loci, plain) == ((1, 1, 0, 0), (1, 1, 0, 1))


def test_margins(cases):
    loci, refs, plain, traces = cases["margin"]
    assert traces[0]["margin"] <= dc.UNDECIDED and traces[1]["margin"] <= dc.UNDECIDED and traces[2]["margin"] >= dc.DECIDED
    assert len(traces[0]["haps"]) == 4 and len(traces[2]["haps"]) == 3 and traces[2]["split"] is not None
    assert dc.expected_stats(loci, plain) == ((1, 0, 0, 2), (1, 0, 2, 1))


def test_repair_and_tail(cases):
    loci, refs, plain, traces = cases["repair"]
    assert dc.expected_stats(loci, plain) == ((4, 2, 0, 0), (4, 2, 0, 4))
    assert [dc.needs_repair(L, q, t) for L, q, t in zip(loci, plain, traces)] == [(True, True), (True, False), (False, False), (False, False)]
    assert all(r["stats"]["n_wfa_cons"] > 0 for r in refs[:2])
    carriers = lambda L, t: [1 if -120 in L["mismatch_offsets"][k] else 0 for k in t["kept"]]
    for l in (1, 2, 3):  # the carriers are group 0 and hold the longer allele: the swap flips the assignment
        assert traces[l]["split"][0] == [1 - c for c in carriers(loci[l], traces[l])]
    assert [int(v) for v in refs[1]["classification"]] == carriers(loci[1], traces[1])
    assert refs[2]["alleles"] == [dc.CAG20.decode(), dc.CAG21.decode()] and refs[3]["alleles"] == [dc.CAG21.decode(), dc.CAG20.decode()]
    loci, refs, plain, traces = cases["hand back"]
    assert dc.expected_stats(loci, plain) == ((2, 1, 0, 0), (2, 1, 0, 2)) and dc.expected_stats(loci, plain, handed=(0,)) == ((1, 0, 1, 0), (1, 0, 1, 1))
    assert max(int(plain[0]["span_end"][k]) - int(plain[0]["span_start"][k]) for k in traces[0]["kept"]) > 60
    assert dc.needs_repair(loci[0], plain[0], traces[0]) == (True, False) and traces[1]["split"] is not None


def test_limits(cases):
    for name in ("snv cap", "hap cap", "offset cap"):
        loci, refs, plain, traces = cases[name]
        assert dc.expected_stats(loci, plain) == ((1, 0, 1, 0), (1, 0, 1, 1)), name
        assert [dc.over_a_cap(t) for t in traces] == [False, True] and all(t["split"] is not None for t in traces), name
    assert [len(t["snvs"]) for t in cases["snv cap"][3]] == [64, 65]
    assert [len(t["haps"]) for t in cases["hap cap"][3]] == [16, 17]
    assert [t["in_region"] for t in cases["offset cap"][3]] == [dc.OFFS_CAP, dc.OFFS_CAP + 1] == [16384, 16385]
    assert [t["n"] for t in cases["offset cap"][3]] == [dc.CEILING] * 2


def test_tags_and_snvs(cases):
    loci, refs, plain, traces = cases["tags and snvs"]
    assert traces[0] is None and dc.tags_split(loci[0], plain[0]) and not dc.tags_split(loci[1], plain[1]) and loci[2]["hp_tag"] is None
    assert traces[1]["split"] is not None and traces[2]["split"] is not None
    assert dc.expected_stats(loci, plain) == ((2, 0, 0, 0), (3, 0, 0, 2)) == dc.expected_stats(loci, plain, flank_device=True)
    assert dc.tag_route_stats(loci, plain) == (1, 0, 1)


def test_mixed_batch(cases):
    loci, refs, plain, traces = cases["mixed"]
    assert [t is not None for t in traces] == [False, False, True, False, True, True, True]
    assert traces[5]["split"] is None and len(loci[6]["reads"]) == dc.MIXED_SETTING + 1
    assert dc.expected_stats(loci, plain) == ((4, 0, 0, 0), (5, 0, 0, 3))
    assert dc.expected_stats(loci, plain, max_reads=dc.MIXED_SETTING) == ((3, 0, 0, 0), (4, 0, 0, 2))


def test_purity_and_random(cases):
    loci, refs, plain, traces = cases["purity"]
    assert [t["n"] for t in traces] == [len(q["kept_read"]) for q in plain] and all(t["n"] < len(L["reads"]) for t, L in zip(traces, loci))
    assert dc.expected_stats(loci, plain) == ((2, 0, 0, 0), (2, 0, 0, 2))
    loci, refs, plain, traces = cases["random"]
    assert len(loci) == 24 and all(256 < len(L["reads"]) <= 600 for L in loci)
    snv, deep = dc.expected_stats(loci, plain)
    assert snv[0] >= 10 and snv[1] >= 3 and snv[2:] == (0, 0) and deep[0] == 24 and deep[3] == snv[0], (snv, deep)
