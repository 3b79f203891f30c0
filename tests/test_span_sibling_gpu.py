"""The sibling rule of the flank scan on the device (trgt_amd/csrc/spans.hip, ScanArgs::min_matches): a missed flank piece whose exactly
found sibling leaves it fewer than min_matches = 175 bases of the read gets no fallback alignment.  Hand-made loci aim at the rule's
edges -- regions of 174 / 175 / 176 and 249 / 250 / 251 bases on either side, a read shorter than the flank, both pieces missed, a
second copy of the missed piece (exact, and at 80-95 % identity) on the wrong side of the sibling, a missed flank at 75 % identity
without a single intact seed -- under both penalty presets that have a pre-filter.  Spans, alleles and VCF fields must be the oracle's,
every output must be the same with the rule switched off (TRGT_NO_SIBLING_RULE, developer build), and with the rule on the pre-filter
computes strictly fewer offsets (stats[17]) for the same number of flank alignments reported (stats[0])."""
import numpy as np
import pytest

from helpers import rand_dna
from test_span_sibling_rule import F, MIN_MATCHES, degrade, rule_drops

pytestmark = pytest.mark.gpu

REGIONS = (174, 175, 176, 249, 250, 251)


def _no_seed_copy(seq):
    """about 75 % identity, a substitution in every fourth base: no twelve-base seed survives, 187 of 250 bases still match"""
    b = bytearray(seq)
    for i in range(1, len(b), 4):
        b[i] = b"ACGT"[(b"ACGT".index(b[i]) + 1 + i % 3) % 4]
    return bytes(b)


def _locus(rng, l):
    lf, rf = rand_dna(rng, F), rand_dna(rng, F)
    tr = b"CAG" * 20
    reg = REGIONS[l % len(REGIONS)]
    k = reg - len(tr)  # bases of the missed piece a cut read still holds behind / in front of the repeat
    reads = [
        rand_dna(rng, 150) + lf + tr + rf[:k],                                   # right piece missed, region of `reg` bases
        lf[F - k:] + tr + rf + rand_dna(rng, 150),                               # left piece missed, region of `reg` bases
        rand_dna(rng, 150) + lf + rf[:reg] if reg < F else rand_dna(rng, 150) + lf + tr * 2 + rf[:reg - 2 * len(tr)],   # ... with as much of the piece as the region holds
        lf[F - reg:] + rf + rand_dna(rng, 150) if reg < F else lf[F - (reg - 2 * len(tr)):] + tr * 2 + rf + rand_dna(rng, 150),
        # a second copy of the missed piece on the wrong side of the sibling: exact in the even loci (then the scan finds it: discordant
        # exact hits), degraded in the odd ones (the alignment would find it: a hit the rule never computes)
        rand_dna(rng, 40) + (rf if l % 2 == 0 else degrade(rng, rf, 0.80 + 0.03 * l)) + rand_dna(rng, 30) + lf + tr + rf[:60 + 10 * l],
        lf[F - 60 - 10 * l:] + tr + rf + rand_dna(rng, 30) + (lf if l % 2 == 0 else degrade(rng, lf, 0.95 - 0.03 * l)) + rand_dna(rng, 40),
        [lf[:200], rf[30:F - 1], tr * 3][l % 3],                                 # shorter than the flank
        rand_dna(rng, 120) + _no_seed_copy(lf) + tr + _no_seed_copy(rf) + rand_dna(rng, 120),   # both pieces missed
        rand_dna(rng, 200) + lf + tr + _no_seed_copy(rf),                        # 75 % identity, no seeds: kept by the pre-filter and back-traced
        _no_seed_copy(lf) + tr + rf + rand_dna(rng, 200),
        # complete reads: they make the locus' longest read, so that the cut ones are the expensive alignments
        rand_dna(rng, 300) + lf + tr + rf + rand_dna(rng, 300),
        rand_dna(rng, 290) + lf + tr + rf + rand_dna(rng, 310),
    ]
    assert len(reads) == 12
    return dict(left_flank=lf, right_flank=rf, tr=tr, motifs=[b"CAG"], ploidy=2, reads=reads)


@pytest.fixture(scope="module")
def batch():
    from trgt_amd import locus
    rng = np.random.default_rng(20260118)
    loci = [_locus(rng, l) for l in range(6)]
    dropped = sum(rule_drops(r, d["left_flank"], d["right_flank"], F, MIN_MATCHES) for d in loci for r in d["reads"])
    # the regions of 174 bases on either side and the cut reads with a degraded copy beyond the sibling (an exact copy is found by the scan)
    assert dropped >= 8, dropped
    return locus.pack(loci), dropped


OUTPUTS = ("span_start", "span_end", "n_alleles", "allele_blob", "allele_len", "ci", "num_spanning", "classification", "read_rank", "spans3",
           "n_spans", "motif_counts", "purity", "gt_size", "flipped")


def _drop_line(err):
    line = [l for l in err.splitlines() if l.startswith("[spans+] sibling rule")][-1]
    return line.split()[3].rstrip(":"), int(line.split()[4])


@pytest.mark.parametrize("scoring", [(2, 5, 1), (1, 0, 1)])
def test_rule_on_and_off_match_the_oracle(oracle, batch, scoring, capfd):
    import torch
    from trgt_amd import _lib, locus
    from test_locus_gpu import _compare
    b, dropped = batch
    p = locus.Params(aln_scoring=scoring)
    dev = dict(flank_dev=torch.from_numpy(b["flank_blob"]).cuda(), reads_dev=torch.from_numpy(b["read_blob"]).cuda())
    on = _lib.context_with_env(TRGT_WFA_DEBUG=1)
    off = _lib.context_with_env(TRGT_WFA_DEBUG=1, TRGT_NO_SIBLING_RULE=1)
    try:
        capfd.readouterr()
        out_on = locus.run_batch(b, p, ctx=on, **dev)
        err_on = capfd.readouterr().err
        out_off = locus.run_batch(b, p, ctx=off, **dev)
        err_off = capfd.readouterr().err
        out_host = locus.run_batch(b, p, ctx=on)  # (reads uploaded by the call)
    finally:
        on.close()
        off.close()
    for out in (out_on, out_off, out_host):
        _compare(oracle, locus, b, out, p, range(int(b["n_loci"])))
    for name in OUTPUTS:
        assert np.array_equal(getattr(out_on, name), getattr(out_off, name)), name
        assert np.array_equal(getattr(out_on, name), getattr(out_host, name)), name
    print("stats[0] on / off: %d / %d, stats[14]: %d / %d, stats[16]: %d / %d, stats[17]: %d / %d" % tuple(
        int(v) for i in (0, 14, 16, 17) for v in (out_on.stats[i], out_off.stats[i])))
    assert int(out_on.stats[0]) == int(out_off.stats[0]) and int(out_on.stats[14]) == int(out_off.stats[14])
    assert 0 < int(out_on.stats[17]) < int(out_off.stats[17])
    # the scan's own tally (debug line): exactly the reads the rule as restated in Python drops, and none with the switch set
    assert _drop_line(err_on) == ("on", dropped), err_on
    assert _drop_line(err_off) == ("off", 0), err_off


def test_stand_alone_entry_keeps_the_hit_bytes(oracle, batch):
    """trgt_find_spans_batch hands out lf_hit / rf_hit ("2 = WFA"): with the pointers given the rule stays off and a discordant alignment
    still reports 2; without them (spans only) the rule is on.  Spans are the same either way."""
    import ctypes as C
    from trgt_amd import _lib, locus
    b, _ = batch
    ss, se, lh, rh = locus.find_tr_spans_batch(b)
    ctx, p = _lib.context(), _lib.ptr
    sp = _lib.SpanParams(F, 0.7, 2, 5, 1)
    n = int(b["n_reads"])
    ss2, se2 = np.zeros(n, np.int32), np.zeros(n, np.int32)
    ctx.check(_lib.lib().trgt_find_spans_batch(ctx.handle, C.byref(sp), int(b["n_loci"]), p(b["flank_blob"]), p(b["lf_off"]), p(b["lf_len"]), p(b["rf_off"]),
                                               p(b["rf_len"]), p(b["locus_read_begin"]), p(b["read_blob"]), p(b["read_off"]), p(b["read_len"]), p(ss2), p(se2), None, None))
    assert np.array_equal(ss, ss2) and np.array_equal(se, se2)
    # the degraded copy beyond the sibling (reads 4 and 5 of the odd loci) is an alignment hit, though the read has no span
    lrb = b["locus_read_begin"]
    assert any(rh[int(lrb[l]) + 4] == 2 and ss[int(lrb[l]) + 4] < 0 for l in (1, 3, 5))
    assert any(lh[int(lrb[l]) + 5] == 2 and ss[int(lrb[l]) + 5] < 0 for l in (1, 3, 5))
