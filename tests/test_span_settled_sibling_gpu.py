"""The settled-sibling rule on the device (trgt_amd/csrc/spans.hip, settled_sibling_kernel): an expensive fallback job without seeds never
meets the pre-filter when the other flank piece of its read was settled by a shortcut of the front seed search -- one or two
substitutions, one inserted or deleted base -- and leaves it fewer than min_matches = 175 bases of the read.  Hand-made loci aim at the
edges: regions of 174 / 175 / 176 bases on either side of every kind of settled sibling, a sibling with three substitutions (seeded, not
settled: windowed) and one with a substitution and a gap (windowed too), whose jobs must stay, both pieces without seeds, a degraded
copy of the missed piece on the wrong side of the sibling.  Spans, alleles and VCF fields must be the oracle's; every output must be
the same with the rule switched off (TRGT_NO_SETTLED_SIBLING_RULE, developer build) and with both sibling rules off
(TRGT_NO_SIBLING_RULE); the rule's own tally (debug line) must be the count of the Python restatement (tools/sibling_census.py), and
with the rule on the pre-filter computes strictly fewer offsets (stats[17]) for the same flank alignments reported (stats[0])."""
import numpy as np
import pytest

from helpers import rand_dna
from test_span_sibling_gpu import OUTPUTS, _no_seed_copy
from test_span_sibling_rule import F, MIN_MATCHES, degrade
from test_span_settled_sibling_rule import PLAN, front_search, seed_plan, settled_rule_drops, sibling_variant

pytestmark = pytest.mark.gpu

REGIONS = (174, 175, 176)
TR = b"CAG" * 20


def _sub3(piece):
    a = bytearray(piece)
    for i in (20, 110, 200):
        a[i] = b"ACGT"[(b"ACGT".index(a[i]) + 1) % 4]
    return bytes(a)


def _sub_and_gap(piece):
    a = bytearray(piece)
    a[60] = b"ACGT"[(b"ACGT".index(a[60]) + 1) % 4]
    return bytes(a[:150]) + bytes([b"ACGT"[(b"ACGT".index(a[150]) + 1) % 4]]) + bytes(a[150:])


def _locus(rng, l):
    lf, rf = rand_dna(rng, F), rand_dna(rng, F)
    reg, reg2 = REGIONS[l % 3], REGIONS[(l + 1) % 3]
    k, k2 = reg - len(TR), reg2 - len(TR)  # bases of the missed piece a cut read still holds behind / in front of the repeat
    v = lambda piece, variant: sibling_variant(rng, piece, variant)
    reads = [
        rand_dna(rng, 150) + v(lf, ("sub_inner", "sub_first", "sub_last")[l % 3]) + TR + rf[:k],   # right piece missed beside a left one with a substitution
        lf[F - k:] + TR + v(rf, "sub_two") + rand_dna(rng, 150),                                   # left piece missed, two substitutions in the right one
        rand_dna(rng, 150) + v(lf, "ins") + TR + rf[:k],                                           # one inserted base: the sibling spans F + 1 bases
        lf[F - k:] + TR + v(rf, "del") + rand_dna(rng, 150),                                       # one deleted base
        lf[F - k2:] + TR + v(rf, ("sub_last", "sub_inner", "sub_first")[l % 3]) + rand_dna(rng, 140),
        rand_dna(rng, 140) + v(lf, "del") + TR + rf[:k2],
        # siblings with seeds that no shortcut settles (they join the windowed launch): the job beside them stays, whatever room it has
        rand_dna(rng, 150) + _sub3(lf) + TR + rf[:174 - len(TR)],
        lf[F - (174 - len(TR)):] + TR + _sub_and_gap(rf) + rand_dna(rng, 150),
        # a degraded copy of the missed piece on the wrong side of the settled sibling: an alignment hit the rule never computes
        rand_dna(rng, 40) + degrade(rng, rf, 0.80 + 0.03 * l) + rand_dna(rng, 30) + v(lf, "sub_two") + TR + rf[:60 + 10 * l],
        rand_dna(rng, 100) + _no_seed_copy(lf) + TR + _no_seed_copy(rf)[:200],                     # both pieces without seeds
        # complete reads: they make the locus' longest read, so that the cut ones are the expensive alignments
        rand_dna(rng, 300) + lf + TR + rf + rand_dna(rng, 300),
        rand_dna(rng, 290) + lf + TR + rf + rand_dna(rng, 310),
    ]
    assert len(reads) == 12
    assert front_search(reads[6], lf, PLAN) == ("window",) and front_search(reads[7], rf, PLAN) == ("window",)
    assert front_search(reads[9], lf, PLAN) == ("noseed",) and front_search(reads[9], rf, PLAN) == ("noseed",)
    return dict(left_flank=lf, right_flank=rf, tr=TR, motifs=[b"CAG"], ploidy=2, reads=reads)


def restated_drops(loci, plan):
    """what settled_sibling_kernel drops, read by read: the expensive jobs (read shorter than the locus' longest minus 1.2 F, piece missed by
    the exact scan, no exactly found sibling short of room) that the front seed search leaves without seeds, beside a settled sibling"""
    n = 0
    for d in loci:
        pieces = (d["left_flank"], d["right_flank"])
        heavy_len = max(max(len(r) for r in d["reads"]) - (F + F // 5), 0)
        for read in d["reads"]:
            if len(read) >= heavy_len or any(read.find(p) >= 0 for p in pieces):
                continue  # (an exact hit: the sibling is not one the seed search sees)
            n += sum(front_search(read, pieces[side], plan) == ("noseed",) and settled_rule_drops(read, pieces, side, plan, MIN_MATCHES) for side in (0, 1))
    return n


@pytest.fixture(scope="module")
def batch():
    from trgt_amd import locus
    rng = np.random.default_rng(20261019)
    loci = [_locus(rng, l) for l in range(6)]
    dropped = restated_drops(loci, PLAN)
    # per locus the degraded-copy read, and every cut read whose region is 174 bases: four in two loci, two in two others, none in the rest
    assert dropped == 6 + 2 * 4 + 2 * 2, dropped
    assert restated_drops(loci, seed_plan(F, 1, 0, 1)) == 0
    return locus.pack(loci), dropped


def _settled_line(err):
    line = [l for l in err.splitlines() if l.startswith("[spans+] settled-sibling rule")][-1]
    return line.split()[3].rstrip(":"), int(line.split()[4])


@pytest.mark.parametrize("scoring", [(2, 5, 1), (1, 0, 1)])
def test_rule_on_and_off_match_the_oracle(oracle, batch, scoring, capfd):
    import torch
    from trgt_amd import _lib, locus
    from test_locus_gpu import _compare
    b, dropped = batch
    if scoring != (2, 5, 1):
        dropped = 0  # (no shortcut under 1,0,1: the rule is inert)
    p = locus.Params(aln_scoring=scoring)
    dev = dict(flank_dev=torch.from_numpy(b["flank_blob"]).cuda(), reads_dev=torch.from_numpy(b["read_blob"]).cuda())
    ctxs = [_lib.context_with_env(TRGT_WFA_DEBUG=1), _lib.context_with_env(TRGT_WFA_DEBUG=1, TRGT_NO_SETTLED_SIBLING_RULE=1),
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
    on, switch, both_off = outs
    for out in outs:
        _compare(oracle, locus, b, out, p, range(int(b["n_loci"])))
    for name in OUTPUTS:
        assert np.array_equal(getattr(on, name), getattr(switch, name)), name
        assert np.array_equal(getattr(on, name), getattr(both_off, name)), name
    print("stats[0] on / switch / both off: %d / %d / %d, stats[14]: %d / %d / %d, stats[17]: %d / %d / %d" % tuple(
        int(o.stats[i]) for i in (0, 14, 17) for o in outs))
    print("debug lines:", [_settled_line(e) for e in errs])
    for i in (0, 14):
        assert int(on.stats[i]) == int(switch.stats[i]) == int(both_off.stats[i]), i
    # the rule's own tally: exactly the jobs the Python restatement drops, and none with either switch set
    assert _settled_line(errs[0]) == ("on" if dropped else "off", dropped), errs[0]
    assert _settled_line(errs[1]) == ("off", 0), errs[1]
    assert _settled_line(errs[2]) == ("off", 0), errs[2]
    if dropped:
        assert 0 < int(on.stats[17]) < int(switch.stats[17]) <= int(both_off.stats[17])


def test_stand_alone_entry_keeps_the_hit_bytes(oracle, batch, capfd):
    """trgt_find_spans_batch hands out lf_hit / rf_hit: with the pointers given both sibling rules stay off (the hit byte of a dropped
    piece would read 0 where its alignment makes it 2) and the bytes are what they are without the rule; spans are the same either way."""
    from trgt_amd import _lib, locus
    b, _ = batch
    ss, se, lh, rh = locus.find_tr_spans_batch(b)
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
    assert _settled_line(err) == ("off", 0), err
    for a, x, y in zip((ss, se, lh, rh), got_on, got_off):
        assert np.array_equal(a, x) and np.array_equal(a, y)
    # the degraded copy beyond the settled sibling (read 8) is an alignment hit, though the read has no span
    lrb = b["locus_read_begin"]
    assert any(rh[int(lrb[l]) + 8] == 2 and ss[int(lrb[l]) + 8] < 0 for l in range(6))
