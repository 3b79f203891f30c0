"""The haplotype-tag branch of genotype_flank (get_trs_with_hp, src/trgt/genotype/genotype_flank.rs:43-76, with simple_consensus :147-170;
applied by analyze at tr.rs:69-75) inside the device genotyper: the FLANK forms of locus_gt.hpp, opt-in per context through
trgt_hip_set_flank_device.

Every case compares alleles, kept reads and their order, classification, intervals, the sizes of the genotype and AL / ALLR / SD / MC / MS /
AP with the oracle's restatement of analyze_tr, for three contexts -- setting on, setting off (the default), TRGT_HOST_GENOTYPER=1 -- and
with the reads on the host and resident in HBM; `flipped`, which the oracle does not report, must agree between the three.  What
trgt_hip_flank_stats must report is computed here from the oracle's plain result (no read metadata: n_alleles, gt_size, kept_read) and a
restatement of the tag rule, never taken from the library.  Loci are small: 250-base flanks, 6 to 40 reads unless a case says otherwise."""
from collections import Counter

import numpy as np
import pytest

from helpers import mutate, rand_dna
from test_flank_gpu import _oracle, _phased_locus

pytestmark = pytest.mark.gpu

CAG20, CAG21 = b"CAG" * 20, b"CAG" * 21


@pytest.fixture(scope="module")
def locus():
    from trgt_amd import locus
    return locus


@pytest.fixture(scope="module")
def ctxs():
    """(name, context): the setting on, off (a context as it is created), every locus on the host glue"""
    from trgt_amd import _lib
    on, off, host = _lib.Context(0), _lib.Context(0), _lib.context_with_env(TRGT_HOST_GENOTYPER=1)
    on.set_flank_device(True)
    yield [("on", on), ("off", off), ("host genotyper", host)]
    for c in (on, off, host):
        c.close()


def _tagged_locus(rng, segs, hp, tr=CAG20, motifs=(b"CAG",), **kw):
    """reads = pad + left flank + segment + right flank + pad with exact segments, start_offset / end_offset set, no mismatches"""
    lf, rf = rand_dna(rng, 250), rand_dna(rng, 250)
    reads, so, eo = [], [], []
    for s in segs:
        lc, rc = int(rng.integers(260, 400)), int(rng.integers(260, 400))
        reads.append(rand_dna(rng, lc - 250) + lf + s + rf + rand_dna(rng, rc - 250))
        so.append(-lc); eo.append(rc)
    return dict(dict(left_flank=lf, right_flank=rf, tr=tr, motifs=list(motifs), ploidy=2, reads=reads, genotyper="size", hp_tag=list(hp),
                     start_offset=so, end_offset=eo, mismatch_offsets=[[] for _ in segs]), **kw)


def _het(rng, n, a=CAG20, b=CAG21, hp=None, **kw):
    """every other read carries a / b; hp: the tags (default: all tagged by allele)"""
    return _tagged_locus(rng, [a if i % 2 == 0 else b for i in range(n)], hp if hp is not None else [i % 2 + 1 for i in range(n)], **kw)


def _ref(oracle, L, params, meta=True):
    if meta and L.get("read_qual") is None:
        return _oracle(oracle, L, params)
    m = dict(hp_tag=L.get("hp_tag"), start_offset=L["start_offset"], end_offset=L["end_offset"], mismatch_offsets=L["mismatch_offsets"]) if meta else None
    return oracle.locus_analyze(L["left_flank"], L["right_flank"], L["tr"], L["motifs"], L["reads"], flank_len=params.search_flank_len,
                                min_flank_id_frac=params.min_flank_id_frac, max_depth=params.max_depth, scoring=params.aln_scoring,
                                ploidy=L.get("ploidy", 2), genotyper=1 if L.get("genotyper") == "cluster" else 0,
                                min_read_qual=params.min_read_qual, read_qual=L.get("read_qual"), meta=m)


def _tag_rule(tags):
    """get_trs_with_hp: tag 1 -> 0, tag 2 -> 1, the k-th other read (k from 0) -> k % 2; accepted with both groups and 70 % tagged"""
    asg, k = [], 0
    for h in tags:
        if h in (1, 2):
            asg.append(h - 1)
        else:
            asg.append(k % 2)
            k += 1
    return asg, bool(asg) and 0 in asg and 1 in asg and (len(asg) - k) / len(asg) >= 0.7


def _expected_stats(loci, plain, sent=0, handed=()):
    """trgt_hip_flank_stats after a call with the setting on.  plain: the oracle's results without read metadata.  sent: loci the test
    built for the SNV branch; handed: loci on the route that the case makes the device hand back."""
    done = repaired = 0
    for l, (L, q) in enumerate(zip(loci, plain)):
        if L.get("genotyper", "size") != "size" or len(L["reads"]) > 256 or L.get("hp_tag") is None:
            continue
        if q["n_alleles"] != 2 or abs(int(q["gt_size"][0]) - int(q["gt_size"][1])) > 10:
            continue
        kept = [int(r) for r in q["kept_read"]]
        asg, ok = _tag_rule([L["hp_tag"][r] for r in kept])
        if not ok or l in handed:
            continue
        done += 1
        segs = [L["reads"][r][int(q["span_start"][r]):int(q["span_end"][r])] for r in kept]
        repaired += any(max(Counter(s for s, a in zip(segs, asg) if a == g).values()) / asg.count(g) < 0.5 for g in (0, 1))
    return (done, repaired, sent + len(handed), 0)


def _compare(locus, b, out, refs, how):
    for l, ref in enumerate(refs):
        got = locus.locus_result(b, out, l)
        na = ref["n_alleles"]
        assert [a.seq.decode() for a in got.genotype] == ref["alleles"], (how, l)
        assert got.reads == [int(v) for v in ref["kept_read"]] and got.classification == [int(v) for v in ref["classification"]], (how, l)
        assert [a.ci for a in got.genotype] == [tuple(int(v) for v in c) for c in ref["gt_ci"]], (how, l)
        assert [int(v) for v in out.gt_size[2 * l:2 * l + na]] == [int(v) for v in ref["gt_size"]], (how, l)
        if na:
            f = got.vcf_fields()
            for k in ("AL", "ALLR", "SD", "MC", "MS", "AP"):
                assert f[k] == ref[k], (how, l, k)


def _runs(locus, b, params, ctx):
    import torch
    yield "host reads", locus.run_batch(b, params, ctx=ctx)
    yield "HBM reads", locus.run_batch(b, params, ctx=ctx, flank_dev=torch.from_numpy(b["flank_blob"]).cuda(), reads_dev=torch.from_numpy(b["read_blob"]).cuda())


def _check(oracle, locus, ctxs, loci, params=None, sent=0, handed=(), want=None, on_ctx=None):
    """want: what the case itself expects of the statistics (checked against the restatement before any GPU run)"""
    params = params or locus.Params()
    b = locus.pack(loci)
    refs = [_ref(oracle, L, params) for L in loci]
    plain = [_ref(oracle, L, params, meta=False) for L in loci]
    stats = _expected_stats(loci, plain, sent, handed)
    if want is not None:
        assert stats == want
    flipped = []
    for name, ctx in ([("on", on_ctx)] if on_ctx is not None else ctxs):
        for how, out in _runs(locus, b, params, ctx):
            _compare(locus, b, out, refs, (name, how))
            flipped.append(out.flipped.copy())
            if name != "host genotyper":
                print(name, how, "flank_stats", ctx.flank_stats(), "expected", stats if name == "on" else (0, 0, 0, 0))
                assert ctx.flank_stats() == (stats if name == "on" else (0, 0, 0, 0)), (name, how)
    assert all(np.array_equal(f, flipped[0]) for f in flipped)
    return b, refs, stats


# ---- the cases (builders, so that their conditions can be checked on the CPU with the oracle alone)

def case_tags_decide():
    rng = np.random.default_rng(101)
    return [_het(rng, 24), _het(rng, 24, a=CAG20, b=CAG20)]


def case_threshold():
    rng = np.random.default_rng(102)
    t = lambda n, tags: _het(rng, n, hp=tags)
    return [t(10, [1, 2, 1, 2, 1, 2, 1, None, None, None]),           # 7 of 10: 7.0 / 10.0 >= 0.7 holds in f64
            t(13, [1, 2] * 4 + [1] + [None] * 4),                       # 9 of 13: refused
            t(12, [1] * 12),                                            # one group is empty: refused
            t(10, [1, 2, 1, 2, 1, 2, 1, 0, 3, 0]),                      # tags 0 and 3 are untagged: 7 of 10, accepted
            t(10, [1, 2, 1, 2, 1, 2, 0, 3, 0, 3])]                      # ... 6 of 10: refused


X60, Y60, W63 = CAG20, b"CAG" * 19 + b"CAT", CAG21


def case_alternation(drop_untagged=False):
    """12 reads of which 9 are tagged.  Kept order: the seven 60-base reads in input order, then the 63-base ones.  Group 0 holds X, X, Y, Y
    by tag -- a tie that the lexicographically first, X, wins -- and the first and third untagged read, both Y: Y wins 4 : 2.  The second
    untagged read joins group 1 (five W) and changes nothing there."""
    rng = np.random.default_rng(103)
    segs = [X60, Y60, X60, Y60, Y60, Y60, Y60] + [W63] * 5
    hp = [1, None, 1, 1, None, 1, None] + [2] * 5
    if drop_untagged:
        segs, hp = [s for s, h in zip(segs, hp) if h], [h for h in hp if h]
    return [_tagged_locus(rng, segs, hp, tr=b"CAG" * 10)]


def case_ties():
    rng = np.random.default_rng(104)
    a60, b66, c61, d63 = CAG20, b"CAG" * 22, b"CAG" * 20 + b"C", CAG21
    e60 = b"CAG" * 19 + b"CAT"
    f63 = b"AAG" + CAG20  # lexicographically before CAG20
    other = [d63] * 5
    mk = lambda g0: _tagged_locus(rng, g0 + other, [1] * len(g0) + [2] * 5, tr=b"CAG" * 10)
    return [mk([a60, a60, b66, b66, c61]),  # equal multiplicity, median 61: |60 - 61| < |66 - 61| (40 %: this group is repaired from a60)
            mk([e60, a60, e60, a60]),       # equal multiplicity, equal delta: the lexicographically first, a60
            mk([f63, a60, f63, a60])]       # median 61.5 -> 61: a60 (delta 1) beats f63 (delta 2), which sorts first


def _noisy_group(seed, base):
    """8 reads, 5 distinct sequences (multiplicities 2, 2, 2, 1, 1: no sequence reaches 50 %): `base` with 3 % errors"""
    rng = np.random.default_rng(seed)
    v = []
    while len(v) < 5:
        m = mutate(rng, base, 0.03, 0.015, 0.015)
        if m != base and m not in v:
            v.append(m)
    return [v[0], v[1], v[0], v[2], v[3], v[1], v[2], v[4]]


CCG18, CCG19 = b"CCG" * 18, b"CCG" * 19
SEED_G18, SEED_G19, SEED_SWAP = 3, 11, 5  # checked on the CPU with the oracle: every locus of case_repair aligns (n_wfa_cons > 0), the third swaps


def case_repair():
    """[0] group 0 repaired, [1] both, [2] group 0 (tag 1) is the noisy longer one: its repaired allele is longer than allele 1, so the
    alleles swap and the assignment flips (the oracle's classification is 1 - (tag - 1) for every read; tr matches neither allele)"""
    rng = np.random.default_rng(105)
    g18, g19, gsw = _noisy_group(SEED_G18, CCG18), _noisy_group(SEED_G19, CCG19), _noisy_group(SEED_SWAP, CCG19)
    kw = dict(tr=b"CCG" * 10, motifs=(b"CCG",))
    return [_tagged_locus(rng, g18 + [CCG19] * 8, [1] * 8 + [2] * 8, **kw),
            _tagged_locus(rng, g18 + g19, [1] * 8 + [2] * 8, **kw),
            _tagged_locus(rng, gsw + [CCG18] * 8, [1] * 8 + [2] * 8, **kw)]


def case_reference_first():
    """group 0 (tag 1) carries the longer allele: swap.  tr = the allele of group 1 (tag 2), first after the swap: no flip; tr = the allele
    of group 0, second after the swap: the reference allele moves to the front after all"""
    rng = np.random.default_rng(106)
    return [_het(rng, 12, a=CAG21, b=CAG20, tr=CAG20), _het(rng, 12, a=CAG21, b=CAG20, tr=CAG21)]


def case_small_form():
    rng = np.random.default_rng(107)
    return [_het(rng, 64), _het(rng, 9), _het(rng, 40, a=CAG20, b=b"CAG" * 22)]


def case_large_form():
    rng = np.random.default_rng(108)
    return [_het(rng, 65), _het(rng, 256), _het(rng, 257), _het(rng, 30)]


L167, L168 = b"CAG" * 167, b"CAG" * 168


def case_segments_beyond_lds(n, big):
    rng = np.random.default_rng(109)
    return [_het(rng, n, a=L167, b=L168)] + ([_het(rng, 65)] if big else [])


def case_purity():
    """min_read_qual = 0.5: every tenth read has rq 0.7 and a degraded repeat (scored and possibly dropped by filter_impure_trs)"""
    rng = np.random.default_rng(110)
    loci = []
    for n in (20, 30, 40):
        segs = [(CAG20 if i % 2 == 0 else CAG21) if i % 10 != 3 else rand_dna(rng, 20) + b"CAG" * 13 for i in range(n)]
        loci.append(_tagged_locus(rng, segs, [i % 2 + 1 for i in range(n)], read_qual=[0.7 if i % 10 == 3 else 0.99 for i in range(n)]))
    return loci


def case_mixed():
    rng = np.random.default_rng(111)
    loci = [_het(rng, 24), _phased_locus(rng, b"CAG", 20, 21, hp_frac=0.0, snv=True), _phased_locus(rng, b"CAG", 12, 30, snv=True),
            _het(rng, 12, ploidy=1), _phased_locus(rng, b"AT", 25, 27, hp_frac=0.0, genotyper="cluster"),
            _phased_locus(rng, b"CAG", 20, 22, hp_frac=0.0, snv=True), _het(rng, 18, a=CAG20, b=CAG20)]
    return loci, 2  # the two SNV loci with close alleles


def case_hand_back():
    """a repair locus whose segments (about 70 bases) are beyond a 60-base repair envelope, next to one that needs no repair"""
    rng = np.random.default_rng(112)
    base = b"CCG" * 23 + b"C"
    g = _noisy_group(7, base)
    return [_tagged_locus(rng, g + [b"CCG" * 24] * 8, [1] * 8 + [2] * 8, tr=b"CCG" * 10, motifs=(b"CCG",)), _het(rng, 16)]


def case_random():
    rng = np.random.default_rng(21)
    loci = []
    for _ in range(40):
        m = rand_dna(rng, int(rng.integers(2, 7)))
        c1 = int(rng.integers(5, 40))
        c2 = max(3, c1 + int(rng.integers(-4, 5)))
        loci.append(_phased_locus(rng, m, c1, c2, n=int(rng.integers(6, 40)), hp_frac=float(rng.choice([0.6, 0.75, 0.9, 1.0])),
                                  snv=bool(rng.integers(0, 2)), err=float(rng.choice([0.002, 0.01, 0.03]))))
    return loci


# ---- the tests

def test_tags_decide(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, case_tags_decide(), want=(2, 0, 0, 0))


def test_acceptance_threshold(oracle, locus, ctxs):
    assert 7.0 / 10.0 >= 0.7 and not 9.0 / 13.0 >= 0.7
    _check(oracle, locus, ctxs, case_threshold(), want=(2, 0, 0, 0))  # refused loci carry no mismatches: they stay on the device


def test_untagged_reads_alternate(oracle, locus, ctxs):
    params = locus.Params()
    with_u, without = case_alternation()[0], case_alternation(drop_untagged=True)[0]
    assert _ref(oracle, with_u, params)["alleles"] != _ref(oracle, without, params)["alleles"]
    _check(oracle, locus, ctxs, [with_u], want=(1, 0, 0, 0))


def test_consensus_ties(oracle, locus, ctxs):
    _, refs, _ = _check(oracle, locus, ctxs, case_ties(), want=(3, 1, 0, 0))
    assert CAG20.decode() in refs[1]["alleles"] and CAG20.decode() in refs[2]["alleles"]


def test_repair_one_group_both_groups_and_swap(oracle, locus, ctxs):
    loci = case_repair()
    _, refs, _ = _check(oracle, locus, ctxs, loci, want=(3, 3, 0, 0))
    assert all(r["stats"]["n_wfa_cons"] > 0 for r in refs)
    sw = refs[2]
    assert [int(v) for v in sw["classification"]] == [1 - (loci[2]["hp_tag"][int(r)] - 1) for r in sw["kept_read"]]


def test_reference_allele_first_after_the_swap(oracle, locus, ctxs):
    _, refs, _ = _check(oracle, locus, ctxs, case_reference_first(), want=(2, 0, 0, 0))
    assert refs[0]["alleles"] == [CAG20.decode(), CAG21.decode()] and refs[1]["alleles"] == [CAG21.decode(), CAG20.decode()]


def test_small_and_large_instantiation(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, case_small_form(), want=(3, 0, 0, 0))
    _check(oracle, locus, ctxs, case_large_form(), want=(3, 0, 0, 0))  # the 257-read locus is the host path's from the start


@pytest.mark.parametrize("n,big", [(20, False), (40, True)])
def test_segments_that_do_not_fit_the_lds(oracle, locus, ctxs, n, big):
    assert n * len(L167) > (16384 if big else 8192)
    _check(oracle, locus, ctxs, case_segments_beyond_lds(n, big), want=(2 if big else 1, 0, 0, 0))


def test_purity_filter_on(oracle, locus, ctxs):
    _check(oracle, locus, ctxs, case_purity(), params=locus.Params(min_read_qual=0.5), want=(3, 0, 0, 0))


def test_mixed_call(oracle, locus, ctxs):
    loci, snv = case_mixed()
    _check(oracle, locus, ctxs, loci, sent=snv, want=(2, 0, 2, 0))


@pytest.mark.parametrize("env", [dict(TRGT_REPAIR_MAX_SEG=60), dict(TRGT_HOST_REPAIR=1)])
def test_handing_back(oracle, locus, ctxs, env):
    from trgt_amd import _lib
    ctx = _lib.context_with_env(**env)
    try:
        ctx.set_flank_device(True)
        _check(oracle, locus, ctxs, case_hand_back(), handed=(0,), want=(1, 0, 1, 0), on_ctx=ctx)
    finally:
        ctx.close()


def test_other_entry_points(oracle, locus, ctxs):
    import torch
    from trgt_amd import _lib
    from trgt_amd.driver import split_batch
    on = ctxs[0][1]
    loci = case_tags_decide() + case_repair()[:1] + case_reference_first()
    b, refs, stats = _check(oracle, locus, ctxs, loci, on_ctx=on)
    recs = lambda bb, out: [(locus.locus_result(bb, out, l).genotype, locus.locus_result(bb, out, l).classification, int(out.flipped[l])) for l in range(int(bb["n_loci"]))]
    want = recs(b, locus.run_batch(b, ctx=on))
    assert recs(b, locus.submit_batch(b, ctx=on).wait()) == want and on.flank_stats() == stats
    pk = locus.pack_bam4(b)
    assert recs(pk, locus.run_batch(pk, ctx=on)) == want and on.flank_stats() == stats
    got, total = [], [0, 0, 0, 0]
    for c in split_batch(b, 2):
        got += recs(c, locus.run_batch(c, ctx=on))
        total = [x + y for x, y in zip(total, on.flank_stats())]
    assert got == want and tuple(total) == stats
    pool = _lib.Pool([0, 0], flank_device=True)
    try:
        chunks = split_batch(b, 3)
        outs, _ = locus.run_many(pool, chunks)
        assert [r for c, o in zip(chunks, outs) for r in recs(c, o)] == want
    finally:
        pool.close()
    # the setting on a batch without hp_tag: nothing to do, nothing counted
    plain = {k: v for k, v in b.items() if k not in ("hp_tag", "start_offset", "end_offset", "mismatch_offsets", "mismatch_off", "_cin")}
    ref_plain = [_ref(oracle, L, locus.Params(), meta=False) for L in loci]
    _compare(locus, plain, locus.run_batch(plain, ctx=on, reads_dev=torch.from_numpy(plain["read_blob"]).cuda()), ref_plain, "no hp_tag")
    assert on.flank_stats() == (0, 0, 0, 0)


def test_random_loci(oracle, locus, ctxs):
    """A condition, not a measurement: at least 15 of the 40 loci must go down the route by the restatement above, or the test could
    pass without exercising it.  stats[2] depends on the SNV branch, which has no few-line restatement: bounded, not pinned."""
    loci = case_random()
    params = locus.Params()
    b = locus.pack(loci)
    refs = [_ref(oracle, L, params) for L in loci]
    stats = _expected_stats(loci, [_ref(oracle, L, params, meta=False) for L in loci])
    assert stats[0] >= 15
    for name, ctx in ctxs:
        for how, out in _runs(locus, b, params, ctx):
            _compare(locus, b, out, refs, (name, how))
            if name == "on":
                got = ctx.flank_stats()
                print("random", how, got, "expected", stats[:2])
                assert got[:2] == stats[:2] and 0 <= got[2] <= 40 - got[0] and got[3] == 0
            elif name == "off":
                assert ctx.flank_stats() == (0, 0, 0, 0)
