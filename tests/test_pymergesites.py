"""tests/pymergesites.py, the plain-Python restatement of merge_variants / merge_variant (src/merge/vcf_processor.rs), held to values written
out by hand from that file.  No library, no GPU."""
import random

import numpy as np

import merge_sites_cases
import pymergesites as ps

VE, MI, MF, VF = ps.VECTOR_END_INTEGER, ps.MISSING_INTEGER, ps.MISSING_FLOAT, ps.VECTOR_END_FLOAT
HALF, ONE = 0x3F000000, 0x3F800000


def rec(pos, alleles=("A", "AC"), gt=((2, 4),), AL=((1, 2),), SD=((7, 8),), AP=((0.5, 1.0),), AM=((1.0,),), pad_base="G"):
    return dict(pos=pos, alleles=list(alleles), pad_base=pad_base, gt=[list(x) for x in gt], AL=[list(x) for x in AL], SD=[list(x) for x in SD],
                AP=[list(x) for x in AP], AM=[list(x) for x in AM])


def one_sample_file(records, pre_v1=False, am_is_int=False):
    return dict(n_samples=1, pre_v1=pre_v1, am_is_int=am_is_int, records=records)


def test_the_references_heap_test():
    # vcf_processor.rs:667-723: positions 100, 2000, 50, 99 of readers 0, 1, 2, 3 come out smallest first
    files = [one_sample_file([rec(p)]) for p in (100, 2000, 50, 99)]
    assert ps.heap_sites(files) == [(50, [None, None, 0, None]), (99, [None, None, None, 0]), (100, [0, None, None, None]), (2000, [None, 0, None, None])]


def test_a_duplicate_position_inside_one_file_gives_two_sites():
    files = [one_sample_file([rec(7), rec(7), rec(9)]), one_sample_file([rec(7), rec(9)])]
    assert ps.heap_sites(files) == [(7, [0, 0]), (7, [1, None]), (9, [2, 1])]


def test_a_padded_and_an_unpadded_file_meet_with_equal_alleles():
    files = [one_sample_file([rec(5, alleles=("A", "ACC"), gt=((2, 4),))], pre_v1=True), one_sample_file([rec(5, alleles=("GA", "GAC", "GACC"), gt=((4, 6),), AM=((0.5,),))])]
    (site,) = ps.merge_variants(files)
    assert site["status"] == 0 and site["padded"] == [0] and site["template"] == (0, 0)
    assert site["entry_alleles"] == [[b"GA", b"GACC"], [b"GA", b"GAC", b"GACC"]]
    assert site["alleles"] == [b"GA", b"GAC", b"GACC"]
    assert site["gt"] == [2, 6, 4, 6]            # file 0's ALT 1 is the merged ALT 2
    assert site["AL"] == [1, 2, 1, 2] and site["SD"] == [7, 8, 7, 8]
    assert site["AP"] == [HALF, ONE, HALF, ONE] and site["AM"] == [ONE, VF, HALF, VF]
    assert site["strings"] == [(0, 0, 0), (1, 0, 0)]


def test_al_zero_is_not_padded():
    files = [one_sample_file([rec(5, AL=((0, 9),))], pre_v1=True), one_sample_file([rec(5, AL=((9, 9),))], pre_v1=True)]
    (site,) = ps.merge_variants(files)
    assert site["padded"] == [1] and site["entry_alleles"] == [[b"A", b"AC"], [b"GA", b"GAC"]]
    assert site["status"] == 1                    # "Reference alleles do not match"


def test_the_documented_haploid_zero_in_a_width_two_record_is_not_padded():
    # the first sample is haploid with AL 0; BCF fills its second value with vector end.  Cut at vector end the slice is [0]: minimum 0.
    f = dict(n_samples=2, pre_v1=True, am_is_int=False, records=[rec(5, gt=((2,), (2, 4)), AL=((0, VE), (3, 4)), SD=((1,), (2, 3)), AP=((1.0,), (0.5, 0.5)), AM=((1.0,), (1.0, 1.0)))])
    (site,) = ps.merge_variants([f])
    assert site["padded"] == [] and site["status"] == 0
    assert site["AL"] == [0, VE, 3, 4] and site["gt"] == [2, VE, 2, 4] and site["SD"] == [1, VE, 2, 3]


def test_an_absent_record_is_missing_and_vector_end():
    files = [one_sample_file([rec(5)]), dict(n_samples=2, pre_v1=False, am_is_int=False, records=[])]
    (site,) = ps.merge_variants(files)
    assert site["gt"] == [2, 4, 0, VE, 0, VE] and site["AL"] == [1, 2, MI, VE, MI, VE] and site["AP"] == [HALF, ONE, MF, VF, MF, VF]
    assert site["strings"] == [(0, 0, 0), None, None]


def test_legacy_integer_am():
    files = [one_sample_file([rec(5, AM=((MI, 0),)), rec(6, AM=((255, 128),)), rec(7, AM=((128,),))], am_is_int=True)]
    a, b, c = ps.merge_variants(files)
    assert a["AM"] == [MF, 0] and b["AM"] == [ONE, 0x3F008081] and c["AM"] == [0x3F008081, VF]   # 128 / 255 = 0.50196081...
    want = (np.array([128, 16777217, -1, 2 ** 31 - 1], np.int32).astype(np.float32) / np.float32(255.0)).view(np.uint32)
    assert [ps.f32_div_255(v) for v in (128, 16777217, -1, 2 ** 31 - 1)] == [int(v) for v in want]


def test_a_sample_without_a_value_is_ragged():
    files = [one_sample_file([rec(5, SD=((),))])]
    assert ps.merge_variants(files)[0]["status"] == ps.RAGGED
    files = [one_sample_file([rec(5, AL=((VE, 3),))], pre_v1=True)]
    assert ps.merge_variants(files)[0]["status"] == ps.RAGGED


def test_the_heap_yields_the_pos_rank_grouping_on_200_random_sorted_inputs():
    for k, files in enumerate(merge_sites_cases.random_contigs(200, seed=99)):
        assert ps.heap_sites(files) == ps.key_sites(files), k
    rng = random.Random(3)
    files = [one_sample_file([rec(p) for p in sorted(rng.choice((1, 2, 3)) for _ in range(6))]) for _ in range(9)]
    assert ps.heap_sites(files) == ps.key_sites(files)


def test_the_designed_cases_hold_their_conditions():
    names = [n for n, _, _ in merge_sites_cases.designed()]
    assert len(names) == len(set(names)) and len(names) >= 30
