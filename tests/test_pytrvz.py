"""tests/pytrvz.py -- the restatement trgt_plot_align_batch is judged by -- held to values written out by hand from a reading of
PacificBiosciences/trgt v3.0.0 src/trvz/{align_consensus,align_reads,read,waterfall_plot}.rs.  Events, motif spans and alignment
operations are given by hand here, so no aligner and no HMM stands between the Rust text and the expected values; one leg runs the whole
chain on tests/pyhmm.py, and the last tests run the self-checks of the designed cases (tests/plot_cases.py).  No GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plot_cases as pc  # noqa: E402
import pytrvz as tz  # noqa: E402
from pytrvz import DEL, INS, LEFT_FLANK as LFT, MATCH, RIGHT_FLANK as RFT, SUBST  # noqa: E402

EV = {c: i for i, c in enumerate("MXIDTS[]")}   # HmmEvent numbers by the letters used below: [ MotifStart, ] MotifEnd, T Trans, S Skip


def given(events, spans):
    return lambda motifs, seq: ([EV[c] for c in events], spans)


def test_event_numbers_are_the_reference_enum():
    # events.rs:5-15: Match, Mismatch, Ins, Del, Trans, Skip, MotifStart, MotifEnd
    assert (tz.EV_MATCH, tz.EV_MISMATCH, tz.EV_INS, tz.EV_DEL, tz.EV_TRANS, tz.EV_SKIP, tz.EV_MOTIF_START, tz.EV_MOTIF_END) == tuple(range(8))
    assert (MATCH, SUBST, INS, DEL) == (0, 1, 2, 3)   # align.rs:18-24


def test_align_motifs_perfect_run_merges_across_copies():
    # MotifStart / MotifEnd / Trans emit nothing (:64-69); the final merge joins the Match groups they separated (:108-119)
    hmm = given("TT[MMM]TT[MMM]TT", [(0, 0, 3), (0, 3, 6)])
    assert tz.align_motifs(["CAG"], "CAGCAG", hmm) == [(6, MATCH, 0)]


def test_align_motifs_mismatch_insertion_deletion():
    # HMM Ins (a base the motif does not have) -> AlignOp::Del with its width (:75-79); HMM Del -> a width-0 AlignOp::Ins (:70-74);
    # Mismatch -> Subst (:85-89).  7 + 8 + 6 bases of one motif of 7.
    hmm = given("TT[MMMMXMM]TT[MMMIMMMM]TT[MMMDMMM]TT", [(0, 0, 7), (0, 7, 15), (0, 15, 21)])
    assert tz.align_motifs(["CAGCAGT"], "C" * 21, hmm) == [(4, MATCH, 0), (1, SUBST, 0), (5, MATCH, 0), (1, DEL, 0), (7, MATCH, 0), (0, INS, 0), (3, MATCH, 0)]


def test_align_motifs_implied_leading_deletions():
    # get_events puts path[j + 1] - s - 1 Del events behind a MotifStart (events.rs:36-44): ONE group, one width-0 Ins segment, of the type
    # of the base that follows
    hmm = given("TT[DDMMMMM]TT[MMMMMMM]TT", [(0, 0, 5), (0, 5, 12)])
    assert tz.align_motifs(["CAGCAGT"], "G" * 12, hmm) == [(0, INS, 0), (12, MATCH, 0)]


def test_closing_deletion_takes_the_next_copys_type():
    # base_pos is not advanced by Del (:100-103): behind the last base of a copy, motif_by_base[base_pos] is the NEXT copy's motif
    hmm = given("TT[MMMMMMD]TT[MMMMMMM]TT", [(0, 0, 6), (1, 6, 13)])
    assert tz.align_motifs(["CAGCAGT", "GGCCTTA"], "A" * 13, hmm) == [(6, MATCH, 0), (0, INS, 1), (7, MATCH, 1)]


def test_closing_deletion_at_the_very_end_takes_the_last_bases_type():
    # base_pos == motif_by_base.len(): motif_by_base[base_pos - 1] (:57-60)
    hmm = given("TT[MMMMMMM]TT[MMMMMDD]TT", [(1, 0, 7), (0, 7, 12)])
    assert tz.align_motifs(["CAGCAGT", "GGCCTTA"], "A" * 12, hmm) == [(7, MATCH, 1), (5, MATCH, 0), (0, INS, 0)]


def test_dropped_imperfect_copy_is_unsegmented():
    # after remove_imperfect_motifs the copy is MotifStart, Skip x bases, MotifEnd of the skip block: Match segments of Tr(motifs.len()) (:90-97)
    hmm = given("TT[MMM]TT[SSS]TT[MMM]TT", [(0, 0, 3), (1, 3, 6), (0, 6, 9)])
    assert tz.align_motifs(["CAG"], "CAGCTGCAG", hmm) == [(3, MATCH, 0), (3, MATCH, 1), (3, MATCH, 0)]
    # ... and the whole chain on the oracle-free restatement of the HMM: CTG is an imperfect copy of a 3-base motif
    assert tz.align_motifs(["CAG"], "CAGCTGCAG", pc.hmm_pyhmm) == [(3, MATCH, 0), (3, MATCH, 1), (3, MATCH, 0)]
    # a copy of a 7-base motif is kept with its mismatch (max_motif_len 6, operations.rs:45)
    assert tz.align_motifs(["CAGCAGT"], "CAGCAGTCAGCTGTCAGCAGT", pc.hmm_pyhmm) == [(11, MATCH, 0), (1, SUBST, 0), (9, MATCH, 0)]


def test_empty_tr():
    def never(motifs, seq):
        raise AssertionError("an empty sequence is not labelled (:36-38)")
    assert tz.align_motifs(["CAG"], "", never) == []
    assert tz.align_consensus(["CAG"], "ACGT", "TTG", "ACGTTTG", never) == [(4, MATCH, LFT), (3, MATCH, RFT)]


def test_align_consensus_puts_the_flanks_around():
    hmm = given("TT[MMM]TT", [(0, 0, 3)])
    assert tz.align_consensus(["CAG"], "AC", "GTA", "ACCAGGTA", hmm) == [(2, MATCH, LFT), (3, MATCH, 0), (3, MATCH, RFT)]


CONS = [(3, MATCH, LFT), (2, MATCH, 0), (0, INS, 0), (1, SUBST, 0), (1, DEL, 0), (2, MATCH, 1), (2, MATCH, RFT)]   # 3 | 4 of type 0 | 2 of type 1 | 2


def test_convert_cuts_runs_at_seg_type_boundaries_only():
    # seg_type_by_ref (:35-42): Del / Match / Subst segments give their width, Ins segments nothing: LLL0000 11RR.  One match run over
    # everything is cut where the TYPE changes, not where the consensus's own op does.
    assert tz.convert_reads(CONS, "M" * 11, 11, 11) == [(3, MATCH, LFT), (4, MATCH, 0), (2, MATCH, 1), (2, MATCH, RFT)]
    # a deletion run and a mismatch run lying across a boundary are cut too
    assert tz.convert_reads(CONS, "MMDDMXXMMMM", 11, 9) == [(2, MATCH, LFT), (1, DEL, LFT), (1, DEL, 0), (1, MATCH, 0), (2, SUBST, 0), (2, MATCH, 1), (2, MATCH, RFT)]
    assert tz.convert_reads(CONS, "MMMMMMXXMMM", 11, 11) == [(3, MATCH, LFT), (3, MATCH, 0), (1, SUBST, 0), (1, SUBST, 1), (1, MATCH, 1), (2, MATCH, RFT)]


def test_convert_insertions_take_the_next_reference_bases_type():
    # an insertion exactly at a boundary: the type of the NEXT reference base (:47-53), width 0 (:84-88)
    assert tz.convert_reads(CONS, "MMMIIMMMMMMMM", 11, 13) == [(3, MATCH, LFT), (0, INS, 0), (4, MATCH, 0), (2, MATCH, 1), (2, MATCH, RFT)]
    # a leading insertion, and the trailing one, which takes the type of the LAST base
    assert tz.convert_reads(CONS, "I" + "M" * 11 + "II", 11, 14) == [(0, INS, LFT), (3, MATCH, LFT), (4, MATCH, 0), (2, MATCH, 1), (2, MATCH, RFT), (0, INS, RFT)]


def test_convert_flank_has_one_type():
    assert tz.convert_flank("MMXMDDMII", RFT, 7, 7) == [(2, MATCH, RFT), (1, SUBST, RFT), (1, MATCH, RFT), (2, DEL, RFT), (1, MATCH, RFT), (0, INS, RFT)]


def test_project_betas_by_hand():
    v = lambda p: 0.1 * p
    # read positions 0 1 | 2 (mismatch) | 3 4 (inserted) | 5 6; two reference bases deleted between read 1 and 2
    ops = "MMDDXIIMM"
    betas = [(p, v(p)) for p in range(7)]
    # 0 -> 0, 1 -> 1; 2 sits right behind the deletion: the loop meets it at the FIRST deletion operation, where seq_pos == 2 already and
    # the operation is not visible: consumed, dropped (read.rs:34-45); 3, 4 inside the insertion: dropped; 5 -> 5, 6 -> 6
    assert tz.project_betas(ops, betas) == [(0, v(0)), (1, v(1)), (5, v(5)), (6, v(6))]
    # without the deletion the beta on the mismatch is kept
    assert tz.project_betas("MMXIIMM", betas) == [(0, v(0)), (1, v(1)), (2, v(2)), (3, v(5)), (4, v(6))]
    # a deletion at the very start drops the beta on the first base
    assert tz.project_betas("DMM", [(0, 1.0), (1, 2.0)]) == [(2, 2.0)]
    assert tz.project_betas("MMM", []) == []


def test_align_reads_sorts_by_length_then_higher_score_first_stably():
    scores = {b"AAAA": -4, b"CCCC": 0, b"GGGG": -4, b"TT": -9, b"ACGT": 0}
    wfa = lambda pattern, text: ("M" * len(text) + "D" * (4 - len(text)), scores[bytes(text)])
    reads = [dict(seq=s) for s in ("AAAA", "CCCC", "GGGG", "TT", "ACGT")]
    aligned, order, got_scores = tz.align_reads("ACGT", [(4, MATCH, 0)], reads, wfa)
    assert order == [3, 1, 4, 0, 2]   # the short read; score 0 in input order; score -4 in input order
    assert got_scores == [-4, 0, -4, -9, 0]
    assert aligned[0] == ([(2, MATCH, 0), (2, DEL, 0)], [])


def test_waterfall_by_hand():
    lf, rf, motifs = "ACGT", "TTGA", ["CAG"]
    r0 = dict(seq="ACGT" + "CAGCAG" + "TTGA", betas=[(4, 0.5)])
    r1 = dict(seq="ACCT" + "CAG" + "TGAA", betas=[(p, 0.01 * p) for p in (0, 2, 4, 6, 7, 8, 10)])
    table = {(b"ACGT", b"ACGT"): ("MMMM", 0), (b"TTGA", b"TTGA"): ("MMMM", 0), (b"ACGT", b"ACCT"): ("MMXM", -2), (b"TTGA", b"TGAA"): ("MDMMI", -12)}
    wfa = lambda p, t: table[(bytes(p), bytes(t))]
    hmm = lambda m, s: ([EV[c] for c in "TT" + "[MMM]TT" * (len(s) // 3)], [(0, 3 * i, 3 * i + 3) for i in range(len(s) // 3)])
    got = tz.waterfall_align(motifs, lf, rf, [r0, r1], hmm, wfa)
    assert got["order"] == [1, 0]   # sorted by length (waterfall_plot.rs:28-31); the longest read came first
    a1, b1 = got["reads"][0]
    # left flank | repeat | the deletion that lines up the right flanks, longest_read - len = 14 - 11 (:60-69) | right flank
    assert a1 == [(2, MATCH, LFT), (1, SUBST, LFT), (1, MATCH, LFT), (3, MATCH, 0), (3, DEL, RFT), (1, MATCH, RFT), (1, DEL, RFT), (2, MATCH, RFT), (0, INS, RFT)]
    # betas: 0, 2 through the left alignment; 4, 6 keep their position; 7, 8, 10 are 0, 1, 3 of the right flank: 0 projects to 0 and moves
    # by lf + tr + longest - len = 4 + 3 + 3; 1 sits right behind the deletion and 3 in the insertion: dropped (:74-115)
    assert b1 == [(0, 0.01 * 0), (2, 0.01 * 2), (4, 0.01 * 4), (6, 0.01 * 6), (10, 0.01 * 7)]
    a0, b0 = got["reads"][1]
    assert a0 == [(4, MATCH, LFT), (6, MATCH, 0), (4, MATCH, RFT)] and b0 == [(4, 0.5)]   # no padding segment of width 0 (:62-63)


def test_a_read_shorter_than_its_flanks_is_refused():
    with pytest.raises(AssertionError):
        tz.waterfall_align_read(["CAG"], "ACGT", "TTGA", 7, dict(seq="ACGTTTG"), None, None)


def test_oracle_and_pyhmm_give_the_restatement_the_same(oracle):
    for name in ("perfect", "edits", "leading_dels", "closing_del_mid", "closing_del_end", "dropped6_kept7", "skip_bases", "run_ends_on_63"):
        _, motifs, seq, _ = pc.TR_BY_NAME[name]
        assert pc.hmm_oracle(motifs, seq) == tuple(pc.hmm_pyhmm(motifs, seq)), name


def test_designed_cases_realise_their_conditions(oracle):
    seen = pc.self_check()
    assert pc.REQUIRED <= seen


def test_designed_cases_expected_values_are_well_formed(oracle):
    for case in pc.cases():
        p, exp = case["panel"], pc.expected(case)
        assert sorted(exp["order"]) == list(range(len(p["reads"])))
        for k, (align, betas) in zip(exp["order"], exp["reads"]):
            seq = p["reads"][k]["seq"]
            assert sum(w for w, op, _ in align if op in (MATCH, SUBST)) <= len(seq)
            assert len(betas) <= len(p["reads"][k]["betas"])
            assert all(w == 0 if op == INS else w > 0 for w, op, _ in align)   # width 0 is what marks an insertion, and nothing else has it
