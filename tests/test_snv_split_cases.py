"""The conditions the cases of snv_split_cases.py claim, checked on the CPU with the oracle and the plain-Python restatement of the SNV
branch: what test_snv_split_gpu.py compares on the device is then what its docstrings say, and every count is predictable whatever the
device's exp and log round to."""
import pytest

import snv_split_cases as sc
from test_flank_device_gpu import _ref


def _params(kw):
    from trgt_amd import locus
    return locus.Params(**kw)


def _both(oracle, loci, kw=None):
    p = _params(kw or {})
    return [_ref(oracle, L, p) for L in loci], [_ref(oracle, L, p, meta=False) for L in loci]


def _same(r, q):
    return r["alleles"] == q["alleles"] and list(r["classification"]) == list(q["classification"])


@pytest.fixture(scope="module")
def cases(oracle):
    out = {}
    for name, loci, kw in sc.all_cases():
        refs, plain = _both(oracle, loci, kw)
        out[name] = (loci, refs, plain, [sc.locus_trace(L, q) for L, q in zip(loci, plain)])
    return out


def test_every_margin_is_tiny_or_wide_and_the_rule_predicts_the_oracle(cases):
    for name, (loci, refs, plain, traces) in cases.items():
        for l, (L, r, q, t) in enumerate(zip(loci, refs, plain, traces)):
            if t is None:
                continue
            if t["margin"] is not None:
                assert t["margin"] <= sc.UNDECIDED or t["margin"] >= sc.DECIDED, (name, l, t["margin"])
                if t["margin"] <= sc.UNDECIDED:
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


def test_reference_vectors(cases):
    loci, refs, plain, traces = cases["kats"]
    assert [int(v) for v in refs[0]["classification"]] == [0, 0, 0, 1, 1, 1] and traces[0]["split"] is not None
    assert traces[1] is not None and traces[1]["split"] is None and _same(refs[1], plain[1])
    assert sc.expected_stats(loci, plain) == (1, 0, 0, 0)


def test_plain_split_and_far_alleles(cases):
    loci, refs, plain, traces = cases["plain"]
    assert traces[0]["split"] is not None and traces[1] is None
    st = sc.expected_stats(loci, plain)
    assert st[0] == 1 and st[2:] == (0, 0)


@pytest.mark.parametrize("n", [3, 10, 30])
def test_skip_rounding(cases, n):
    assert round(10 * (1.0 - 0.85), 16) != 1.5 and 10 * (1.0 - 0.85) > 1.5  # 1.5000000000000002: 2 under any rounding of the half
    loci, refs, plain, traces = cases["skip %d" % n]
    skip = sc.case_skip(n)[1]
    assert [t["skip"] for t in traces] == [skip] * 4
    assert [len(t["snvs"]) for t in traces] == [1, 0, 1, 0] and [t["split"] is not None for t in traces] == [True, False, True, False]
    # one less loses the sites at the edges, one more gains the sites outside
    for t, L, (lo, hi) in zip(traces, loci, [(1, 0)] * 4):
        so, eo = sorted(L["start_offset"][k] for k in t["kept"]), sorted(L["end_offset"][k] for k in t["kept"])
        site = [o for m in L["mismatch_offsets"] for o in m][0]
        inside = lambda s: s < n and so[n - 1 - s] <= site <= eo[s]
        assert inside(skip) == bool(t["snvs"])
        if skip > 0:
            assert inside(skip - 1) is False or not t["snvs"]
        assert inside(skip + 1) is True or bool(t["snvs"]) or skip + 1 >= n
    assert sc.expected_stats(loci, plain) == (2, 0, 0, 0)


def test_call_threshold(cases):
    loci, refs, plain, traces = cases["call threshold"]
    assert 4.0 / 20.0 >= 0.20 and not 3.0 / 20.0 >= 0.20
    assert traces[0]["snvs"] == [-120, 85] and traces[0]["split"] is not None


def test_fully_observed_reads_at_their_fewest(cases):
    loci, refs, plain, traces = cases["least full"]
    t = traces[0]
    assert t["n"] == 20 and t["skip"] == 3 and t["full"] == 14 and len(t["snvs"]) == 2 and t["split"] is not None


def test_ties_join_both_groups(cases):
    loci, refs, plain, traces = cases["ties"]
    asg, mem, _ = traces[0]["split"]
    assert sum(m == {0, 1} for m in mem) == 2 and [asg[i] for i, m in enumerate(mem) if m == {0, 1}] == [0, 1]
    r = refs[0]
    assert sorted(r["alleles"]) == sorted([sc.Y60.decode(), sc.CAG21.decode()])          # by assignment alone: X60
    assert sorted(tuple(int(v) for v in c) for c in r["gt_ci"]) == [(60, 66), (60, 66)]  # ... (60, 63) and (60, 66)
    assert [list(r["classification"]).count(g) for g in (0, 1)] == [5, 5] and [sum(g in m for m in mem) for g in (0, 1)] == [6, 6]


def test_margins(cases):
    loci, refs, plain, traces = cases["margin"]
    assert traces[0]["margin"] <= sc.UNDECIDED and traces[1]["margin"] <= sc.UNDECIDED and traces[2]["margin"] >= sc.DECIDED
    assert len(traces[2]["haps"]) == 3 and traces[2]["split"] is not None
    assert sc.expected_stats(loci[:2], plain[:2]) == (0, 0, 0, 2) and sc.expected_stats(loci, plain) == (1, 0, 0, 2)


def test_repair_and_tail(cases):
    loci, refs, plain, traces = cases["repair"]
    assert sc.expected_stats(loci, plain) == (4, 2, 0, 0)
    assert all(r["stats"]["n_wfa_cons"] > 0 for r in refs[:2])
    carriers = lambda L, t: [1 if L["mismatch_offsets"][k] and -120 in L["mismatch_offsets"][k] else 0 for k in t["kept"]]
    for l in (1, 2, 3):  # the carriers are group 0 and hold the longer allele: the swap flips the assignment
        assert traces[l]["split"][0] == [1 - c for c in carriers(loci[l], traces[l])]
    assert [int(v) for v in refs[1]["classification"]] == carriers(loci[1], traces[1])
    assert refs[2]["alleles"] == [sc.CAG20.decode(), sc.CAG21.decode()] and refs[3]["alleles"] == [sc.CAG21.decode(), sc.CAG20.decode()]
    loci, refs, plain, traces = cases["hand back"]
    assert sc.expected_stats(loci, plain) == (2, 1, 0, 0) and sc.expected_stats(loci, plain, handed=(0,)) == (1, 0, 1, 0)
    assert max(int(plain[0]["span_end"][k]) - int(plain[0]["span_start"][k]) for k in traces[0]["kept"]) > 60


def test_forms_and_limits(cases):
    for name, want in (("forms", (3, 0, 0, 0)), ("beyond lds small", (1, 0, 0, 0)), ("beyond lds big", (2, 0, 0, 0)), ("purity", (3, 0, 0, 0)),
                       ("snv cap", (1, 0, 1, 0)), ("hap cap", (1, 0, 1, 0)), ("offset cap small", (1, 0, 1, 0)), ("offset cap big", (1, 0, 1, 0))):
        loci, refs, plain, traces = cases[name]
        assert sc.expected_stats(loci, plain) == want, name
    assert [len(t["snvs"]) for t in cases["snv cap"][3]] == [64, 65]
    assert [len(t["haps"]) for t in cases["hap cap"][3]] == [16, 17]
    assert [t["in_region"] for t in cases["offset cap small"][3]] == [512, 513] and [t["in_region"] for t in cases["offset cap big"][3]] == [2048, 2049]
    assert 20 * len(sc.L167) > 8192 and 40 * len(sc.L167) > 16384


def test_tags_and_snvs(cases):
    loci, refs, plain, traces = cases["tags and snvs"]
    assert traces[0] is None and traces[1]["split"] is not None and sc.expected_stats(loci, plain) == (1, 0, 0, 0)


def test_mixed_batch(cases):
    loci, refs, plain, traces = cases["mixed"]
    assert [t is not None for t in traces] == [True, False, False, False, True, True, True]
    st = sc.expected_stats(loci, plain)
    assert traces[6]["split"] is None and st[0] == 3 and st[2:] == (0, 0)


def test_random_loci_hand_back_at_most_two(cases):
    loci, refs, plain, traces = cases["random"]
    st = sc.expected_stats(loci, plain)
    assert st[3] <= 2 and st[2] == 0 and st[0] >= 5, st
