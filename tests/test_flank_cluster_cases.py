"""What the cases of tests/flank_cluster_cases.py are meant to exercise, asserted from the oracle's plain result (no read metadata) and
the restatement of the tag rule: a case that no longer meets its condition would let tests/test_flank_cluster_gpu.py pass without
running the code it was built for.  No GPU, and nothing here comes from the library."""
import pytest

import flank_cluster_cases as fc
from test_flank_device_gpu import _ref


@pytest.fixture(scope="module")
def params():
    from trgt_amd import locus
    return locus.Params()


def _routes(oracle, loci, params):
    plain = fc.plain_results(oracle, loci, params)
    return plain, [fc.route(L, q) for L, q in zip(loci, plain)]


def test_het_is_settled_without_repair_and_unchanged(oracle, params):
    loci = fc.case_het()
    plain, routes = _routes(oracle, loci, params)
    assert all(r is not None and min(r[1]) == 1.0 for r in routes)
    for L, q in zip(loci, plain):
        full = _ref(oracle, L, params)
        assert full["alleles"] == q["alleles"] and list(full["classification"]) == list(q["classification"])
    assert plain[0]["alleles"] == [fc.CAG20.decode(), fc.CAG21.decode()]
    assert plain[1]["alleles"] == [fc.CAG21.decode(), fc.CAG20.decode()]  # reference allele first: the flip is taken


def test_tags_against_the_clusters_change_the_genotype(oracle, params):
    loci = fc.case_tags_against_clusters()
    plain, routes = _routes(oracle, loci, params)
    assert routes[0] is not None and routes[0][1] == [0.5, 0.5]
    full = _ref(oracle, loci[0], params)
    assert [len(a) for a in full["alleles"]] == [60, 60] and [tuple(int(v) for v in c) for c in full["gt_ci"]] == [(60, 63), (60, 63)]
    assert full["alleles"] != plain[0]["alleles"]


def test_homozygous_loci_take_the_route(oracle, params):
    loci = fc.case_homozygous()
    plain, routes = _routes(oracle, loci, params)
    assert all(r is not None for r in routes)
    assert plain[0]["alleles"] == [fc.CAG20.decode()] * 2
    assert abs(len(plain[1]["alleles"][0]) - len(plain[1]["alleles"][1])) < 10
    assert fc.expected_stats(loci, plain)[0] == 2


def test_acceptance_threshold(oracle, params):
    assert 14.0 / 20.0 >= 0.7 and not 12.0 / 20.0 >= 0.7
    loci = fc.case_threshold()
    _, routes = _routes(oracle, loci, params)
    assert routes[0] is not None and routes[1] is None and routes[2] is None
    assert all(not any(L["mismatch_offsets"]) for L in loci)


def test_loci_outside_the_route(oracle, params):
    loci = fc.case_no_route()
    plain, routes = _routes(oracle, loci, params)
    assert [r is not None for r in routes] == [False, False, False, True]
    assert [len(a) for a in plain[0]["alleles"]] == [60, 90] and plain[1]["n_alleles"] == 1
    assert plain[2]["n_alleles"] == 2 and plain[2]["alleles"][0] == plain[2]["alleles"][1]


def test_lexicographic_tie_in_both_read_orders(oracle, params):
    loci = fc.case_lex_tie()
    _, routes = _routes(oracle, loci, params)
    for L, r in zip(loci, routes):
        assert r is not None and r[1] == [0.5, 1.0]
        assert fc.CAA_CAG19.decode() in _ref(oracle, L, params)["alleles"] and fc.CAG20.decode() not in _ref(oracle, L, params)["alleles"]


def test_median_tie_repairs_group_0(oracle, params):
    loci = fc.case_median_tie()
    _, routes = _routes(oracle, loci, params)
    assert routes[0] is not None and routes[0][1] == [0.25, 0.5]
    assert _ref(oracle, loci[0], params)["stats"]["n_wfa_cons"] > 0


@pytest.mark.parametrize("seed", [400, 401, 402, 403, 404])
def test_noisy_groups_are_both_repaired(oracle, params, seed):
    loci = fc.case_noisy(seed)
    _, routes = _routes(oracle, loci, params)
    assert routes[0] is not None and max(routes[0][1]) <= 0.17


def test_no_room_case_has_two_segment_lengths_and_repairs_both_groups(oracle, params):
    loci = fc.case_no_room()
    plain, routes = _routes(oracle, loci, params)
    q = plain[0]
    assert {int(q["span_end"][r]) - int(q["span_start"][r]) for r in q["kept_read"]} == {54, 57} and len(q["kept_read"]) == 24
    assert routes[0] is not None and max(routes[0][1]) < 0.5


def test_deeper_loci(oracle, params):
    for loci, reads, kept in ((fc.case_100_reads(), 100, 100), (fc.case_256_reads(), 256, 250)):
        plain, routes = _routes(oracle, loci, params)
        assert len(loci[0]["reads"]) == reads and len(plain[0]["kept_read"]) == kept and routes[0] is not None


def test_long_segments_are_repaired(oracle, params):
    loci = fc.case_long_segments()
    plain, routes = _routes(oracle, loci, params)
    assert routes[0] is not None and max(routes[0][1]) < 0.5
    assert min(len(a) for a in plain[0]["alleles"]) > 1100


def test_purity_case_keeps_the_route(oracle):
    from trgt_amd import locus
    p = locus.Params(min_read_qual=0.5)
    loci = fc.case_purity()
    _, routes = _routes(oracle, loci, p)
    assert all(r is not None for r in routes) and len(loci[2]["reads"]) > 64


def test_random_list_has_enough_settled_and_repaired_loci(oracle, params):
    loci = fc.case_random()
    plain = fc.plain_results(oracle, loci, params)
    done, repaired, _ = fc.expected_stats(loci, plain)
    print("random list, seed", fc.RANDOM_SEED, "settled", done, "repaired", repaired)
    assert done >= 10 and repaired >= 5


def test_mixed_batch(oracle, params):
    loci = fc.case_mixed()
    plain, routes = _routes(oracle, loci, params)
    assert [L["genotyper"] for L in loci] == ["size", "cluster", "size", "cluster", "cluster", "cluster", "size"]
    assert [r is not None for r in routes] == [False, True, False, False, True, False, False]
    assert loci[3]["hp_tag"] is None and any(loci[3]["mismatch_offsets"]) and len(loci[5]["reads"]) == 300
    assert fc.expected_stats(loci, plain) == (2, 0, 0)
