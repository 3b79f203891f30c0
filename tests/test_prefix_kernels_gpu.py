"""allele_prefix_kernel (locus.hip) and hmm_span_prefix_kernel (hmm.hip): the exclusive prefix sums that place every allele and every
span list in the packed result arrays, one workgroup of 16 waves each (block_prefix_u32 of common.hpp: a piece of whole 64-element tiles
per wave, one LDS hop over the 16 wave totals).

Batches of 1, 2, 511, 512, 513 and 1 025 loci, so that both kernels scan counts of 2, 4, 1 022, 1 024, 1 026 and 2 050 elements -- below
one tile, around the 1 024 elements at which every wave owns exactly one tile, and beyond -- with loci of 0, 1 and 2 alleles and alleles
of length 0 among them.  A wrong offset moves an allele or a span list: alleles, kept reads, classification, intervals and AL / ALLR / SD /
MC / MS / AP of every locus are compared with the CPU oracle, whose results are computed once for the largest batch and shared."""
import pytest

from test_size_gt_parallel_gpu import F, Maker, _against_oracle, _oracle, _params

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 511, 512, 513, 1025)


@pytest.fixture(scope="module")
def locus():
    from trgt_amd import locus
    return locus


@pytest.fixture(scope="module")
def cases(oracle, locus):
    """1 025 small loci in a fixed order and the oracle's result of each; a batch of n loci is a prefix of the list"""
    mk = Maker(77)
    seg = lambda n: (b"CAG" * 12)[:n]
    kinds = [
        lambda: mk.locus([seg(9)] * 2 + [seg(15)] * 2),           # two alleles
        lambda: mk.locus([seg(12)] * 3, ploidy=1),                # one allele
        lambda: mk.locus([seg(12)] * 2, ploidy=0),                # none: Ploidy::Zero
        lambda: mk.locus([seg(0)] * 3, tr=b"CAG"),                # two alleles of length 0
        lambda: mk.locus([seg(0)] * 2 + [seg(6)] * 2, tr=b"CAG"),  # a 0-length allele in front of a longer one
        lambda: mk.locus([seg(7)] * 2, unkept=(0, 1)),            # none: no read kept
        lambda: mk.locus([seg(21)] * 3),                          # homozygous
    ]
    loci = [kinds[int(k)]() for k in mk.rng.integers(0, len(kinds), size=max(SIZES))]
    params = _params(locus)
    return loci, [_oracle(oracle, L, params) for L in loci], params


@pytest.mark.parametrize("n", SIZES)
def test_offsets_place_every_allele_and_span_list(locus, cases, n):
    loci, refs, params = cases
    b = locus.pack(loci[:n])
    out = locus.run_batch(b, params)
    _against_oracle(locus, b, out, refs[:n], n)
    for l, ref in enumerate(refs[:n]):
        if ref["n_alleles"]:
            f = locus.locus_result(b, out, l).vcf_fields()
            for k in ("AL", "ALLR", "SD", "MC", "MS", "AP"):
                assert f[k] == ref[k], (n, l, k)
    assert F == params.search_flank_len and len(out.allele_len) == 2 * n
