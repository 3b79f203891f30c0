"""The common-subsequence rule on the device (trgt_amd/csrc/spans.hip, lcs_below in settled_sibling_kernel): an expensive fallback job
without seeds never meets the pre-filter when its piece has no common subsequence of min_matches bases with the part of the read beside
a sibling whose span is known -- found exactly by the scan, or settled by a shortcut of the front seed search.  Hand-made loci aim at
the kernel's edges: regions of exactly min_matches bases, of exactly the cap and of one more; a region at the very start and at the very
end of the read blob; a stump of min_matches clean bases (kept) and of one less with errors; an N in the piece and in the text; a sibling
that is neither exact nor settled (windowed: the job stays); a degraded copy of the missed piece on the wrong side of the sibling; and
pieces of 254 and of 100 bases, whose top dword of the bit vector is partial (the rule runs over the pre-filter's list: 254 bases is
the longest piece the pre-filter takes, and below 96 the seed search that builds the list does not run).  Spans, alleles and VCF fields must be the oracle's; every output must be the
same with the rule switched off (TRGT_NO_LCS_RULE, developer build) and with every sibling rule off (TRGT_NO_SIBLING_RULE); the rule's
tally (debug line) must be the count of the Python restatement (tools/sibling_census.py), the settled-sibling rule's tally must not
move, and with the rule on the pre-filter computes strictly fewer offsets (stats[17]) for the same flank alignments reported (stats[0])."""
import math

import numpy as np
import pytest

from helpers import rand_dna
from test_span_lcs_rule import LCS_MAX_ADM, spoil
from test_span_settled_sibling_gpu import _settled_line, _sub3
from test_span_settled_sibling_rule import front_search, seed_plan, settled_rule_drops, sibling_variant
from test_span_sibling_gpu import OUTPUTS
from test_span_sibling_rule import degrade

import sibling_census as sc  # (tools/: on the path through test_span_lcs_rule)

pytestmark = pytest.mark.gpu

FRAC = 0.7
TR = b"CAG" * 20


def _rep(n):
    return b"A" * n  # (shares with a piece no more than the piece's own A's: the long regions stay below min_matches)


def _locus(rng, l, F):
    """a dozen reads; read 0 is a missed left piece (its region starts the locus' reads), read 11 a missed right piece (its region ends
    them): in the first and the last locus these are the two ends of the read blob"""
    mm = int(math.ceil(F * FRAC))
    cap = LCS_MAX_ADM
    lf, rf = rand_dna(rng, F), rand_dna(rng, F)
    if l == 5:  # an N in the right piece, inside the stump the cut reads hold
        rf = rf[:30] + b"N" + rf[31:]
    v = lambda piece, variant: sibling_variant(rng, piece, variant) if F == 250 else piece  # (sibling_variant is written for 250 bases)
    ctx = lambda n: rand_dna(rng, n)
    k, k2 = F * 2 // 5 + 5 * l, F // 4  # stumps well below min_matches
    reads = [
        lf[F - (mm - len(TR)):] + TR + rf + ctx(150),                                   # left missed, region of exactly min_matches bases
        ctx(150) + lf + TR + rf[:mm - len(TR)],                                         # right missed, the same
        ctx(140) + lf + _rep(cap - k2) + rf[:k2],                                       # region of exactly the cap
        lf[F - k2:] + _rep(cap + 1 - k2) + rf + ctx(140),                               # ... and of one base more: not the rule's
        ctx(150) + v(lf, ("sub_inner", "sub_two", "ins", "del", "sub_first", "sub_last")[l]) + TR + rf[:k + 20],   # beside a settled sibling
        lf[F - k - 20:] + TR + v(rf, ("del", "ins", "sub_last", "sub_inner", "sub_two", "sub_first")[l]) + ctx(150),
        ctx(150) + lf + TR + rf[:mm],                                                   # a clean stump of min_matches bases: kept
        spoil(rng, lf[F - (mm - 1):], 4) + TR + rf + ctx(150),                          # one base less, and a few errors
        ctx(150) + (_sub3(lf) if F == 250 else lf[:5] + ctx(3) + lf[8:]) + TR + rf[:k],  # a sibling with seeds that no shortcut settles (F = 250: windowed)
        ctx(40) + degrade(rng, rf.replace(b"N", b"A"), 0.80 + 0.03 * l) + ctx(30) + lf + TR + rf[:k - 10],   # a degraded copy on the wrong side
        ctx(300) + lf + TR + rf + ctx(300),                                             # complete: the locus' longest read
        ctx(130) + lf + TR + rf[:k - 30] + b"N" + rf[k - 29:k + 10],                    # an N in the text; the region ends the locus' reads
    ]
    assert len(reads) == 12
    return dict(left_flank=lf, right_flank=rf, tr=TR, motifs=[b"CAG"], ploidy=2, reads=reads)


def restated(loci, F, scoring):
    """what the device tallies, read by read: (jobs the common-subsequence rule drops, by kind of sibling; jobs the settled-sibling rule
    drops) among the expensive jobs (read shorter than the locus' longest minus 1.2 F, piece missed by the exact scan and not dropped
    by the scan's rule) that the front seed search leaves without seeds"""
    mm, plan = int(math.ceil(F * FRAC)), seed_plan(F, *scoring)
    lcs, settled = dict(exact=0, settled=0), 0
    for d in loci:
        pieces = (d["left_flank"][-F:], d["right_flank"][:F])
        heavy_len = max(max(len(r) for r in d["reads"]) - (F + F // 5), 0)
        for read in d["reads"]:
            if len(read) >= heavy_len:
                continue
            pos = [read.find(p) for p in pieces]
            for side in (0, 1):
                sib = pos[side ^ 1]
                if pos[side] >= 0 or (sib >= 0 and (len(read) - sib - F if side else sib) < mm):
                    continue
                if front_search(read, pieces[side], plan) != ("noseed",):
                    continue
                if sib < 0 and settled_rule_drops(read, pieces, side, plan, mm):
                    settled += 1
                    continue
                kind = sc.lcs_rule_job_drops(read, pieces, side, plan, mm)
                if kind:
                    lcs[kind] += 1
    return lcs, settled


def _lcs_line(err):
    line = [l for l in err.splitlines() if l.startswith("[spans+] common-subsequence rule")][-1]
    return line.split()[3].rstrip(":"), int(line.split()[4])


_BATCHES = {}


def _batch(F):
    """packed once per piece length and shared, unchanged, by the tests"""
    if F not in _BATCHES:
        from trgt_amd import locus
        rng = np.random.default_rng(20261020 + F)
        loci = [_locus(rng, l, F) for l in range(6)]
        _BATCHES[F] = (locus.pack(loci), loci)
    return _BATCHES[F]


def test_restatement_covers_the_edges():
    """(no device work) the hand-made reads are what they are meant to be: the rule fires beside both kinds of sibling, the edge regions
    are there, the job beside a windowed sibling is none of the rule's"""
    _, loci = _batch(250)
    lcs, settled = restated(loci, 250, (2, 5, 1))
    assert lcs["exact"] >= 12 and lcs["settled"] >= 6 and settled == 0, (lcs, settled)
    assert restated(loci, 250, (1, 0, 1))[0]["settled"] == 0  # (no shortcut under 1,0,1: nothing is settled)
    plan = seed_plan(250, 2, 5, 1)
    for d in loci:
        pieces, r = (d["left_flank"], d["right_flank"]), d["reads"]
        assert r[0].find(pieces[1]) == 175 and len(r[1]) - r[1].find(pieces[0]) - 250 == 175
        assert len(r[2]) - r[2].find(pieces[0]) - 250 == LCS_MAX_ADM and r[3].find(pieces[1]) == LCS_MAX_ADM + 1
        assert sc.lcs_rule_job_drops(r[2], pieces, 1, plan, 175) == "exact" and sc.lcs_rule_job_drops(r[3], pieces, 0, plan, 175) is None
        assert sc.lcs_rule_job_drops(r[6], pieces, 1, plan, 175) is None
        assert front_search(r[8], pieces[0], plan) == ("window",) and sc.known_sibling_span(r[8], pieces, 1, plan) == (None, None)


def _run_three(oracle, F, scoring, capfd):
    import torch
    from trgt_amd import _lib, locus
    from test_locus_gpu import _compare
    b, loci = _batch(F)
    p = locus.Params(aln_scoring=scoring, search_flank_len=F)
    dev = dict(flank_dev=torch.from_numpy(b["flank_blob"]).cuda(), reads_dev=torch.from_numpy(b["read_blob"]).cuda())
    ctxs = [_lib.context_with_env(TRGT_WFA_DEBUG=1), _lib.context_with_env(TRGT_WFA_DEBUG=1, TRGT_NO_LCS_RULE=1),
            _lib.context_with_env(TRGT_WFA_DEBUG=1, TRGT_NO_SIBLING_RULE=1)]
    outs, errs = [], []
    try:
        for ctx in ctxs:
            capfd.readouterr()
            outs.append(locus.run_batch(b, p, ctx=ctx, **dev))
            errs.append(capfd.readouterr().err)
    finally:
        for ctx in ctxs:
            ctx.close()
    for out in outs:
        _compare(oracle, locus, b, out, p, range(int(b["n_loci"])))
    on, lcs_off, all_off = outs
    for name in OUTPUTS:
        assert np.array_equal(getattr(on, name), getattr(lcs_off, name)), name
        assert np.array_equal(getattr(on, name), getattr(all_off, name)), name
    print("F = %d, stats[0] on / lcs off / all off: %d / %d / %d, stats[14]: %d / %d / %d, stats[17]: %d / %d / %d" % ((F,) + tuple(
        int(o.stats[i]) for i in (0, 14, 17) for o in outs)))
    print("debug lines:", [_lcs_line(e) for e in errs], [_settled_line(e) for e in errs])
    for i in (0, 14):
        assert int(on.stats[i]) == int(lcs_off.stats[i]) == int(all_off.stats[i]), i
    lcs, settled = restated(loci, F, scoring)
    dropped = lcs["exact"] + lcs["settled"]
    assert dropped > 0
    assert 0 < int(on.stats[17]) < int(lcs_off.stats[17]) <= int(all_off.stats[17])
    # the rule's own tally: exactly the jobs the Python restatement drops, and none with either switch set
    assert _lcs_line(errs[0]) == ("on", dropped), errs[0]
    assert _lcs_line(errs[1]) == ("off", 0), errs[1]
    assert _lcs_line(errs[2]) == ("off", 0), errs[2]
    # ... and the settled-sibling rule's is what it is without the new rule
    assert _settled_line(errs[0]) == _settled_line(errs[1]) == ("on" if scoring == (2, 5, 1) else "off", settled), (errs[0], errs[1])
    return lcs


@pytest.mark.parametrize("scoring", [(2, 5, 1), (1, 0, 1)])
def test_rule_on_and_off_match_the_oracle(oracle, scoring, capfd):
    lcs = _run_three(oracle, 250, scoring, capfd)
    assert lcs["exact"] >= 12 and (lcs["settled"] >= 6) == (scoring == (2, 5, 1))


@pytest.mark.parametrize("F", [254, 100])
def test_partial_top_dword(oracle, F, capfd):
    _run_three(oracle, F, (2, 5, 1), capfd)


def test_stand_alone_entry_keeps_the_hit_bytes(oracle, capfd):
    """trgt_find_spans_batch hands out lf_hit / rf_hit: with both pointers given the rule stays off (the hit byte of a dropped piece
    would read 0 where its alignment makes it 2) and spans and bytes are what they are with every sibling rule switched off"""
    from trgt_amd import _lib, locus
    b, _ = _batch(250)
    on = _lib.context_with_env(TRGT_WFA_DEBUG=1)
    off = _lib.context_with_env(TRGT_WFA_DEBUG=1, TRGT_NO_SIBLING_RULE=1)
    try:
        capfd.readouterr()
        got_on = locus.find_tr_spans_batch(b, ctx=on)
        err = capfd.readouterr().err
        got_off = locus.find_tr_spans_batch(b, ctx=off)
    finally:
        on.close()
        off.close()
    assert _lcs_line(err) == ("off", 0), err
    for x, y in zip(got_on, got_off):
        assert x.tobytes() == y.tobytes()
    # the degraded copy beyond the sibling (read 9) is an alignment hit, though the read has no span
    lrb = b["locus_read_begin"]
    assert any(got_on[3][int(lrb[l]) + 9] == 2 and got_on[0][int(lrb[l]) + 9] < 0 for l in range(6))
