"""The CPU oracle's aligner (oracle/wfa.cpp) against tests/pywfa.py -- a restatement written from the textbook recurrences and the
reference wrapper's text, without looking at the oracle or the kernels -- on the lists of tests/wfa_cases.py, and pywfa against itself:
its numpy form against its plain form, its checker against damaged results, and the counters that say the lists are what their
docstrings promise.  No GPU.  tests/test_wfa_independent_gpu.py puts the same lists through the kernels.

Exact where the aligner is exact (Heuristic::None): the penalty of the returned operations IS the plain-DP optimum.  With the default
heuristic only ">= the optimum" is claimed (what wfadaptive drops is defined by WFA2-lib alone), and nowhere is anything claimed about
WHICH of several co-optimal alignments comes back."""
import numpy as np
import pytest

import pywfa
import wfa_cases as C
from helpers import rand_dna


def oracle_params(orc, cfg):
    pen = dict(zip(("x", "e1"), cfg.pen)) if cfg.metric == "linear" else dict(zip(("x", "o1", "e1", "o2", "e2"), cfg.pen))
    return orc.wfa_params(metric=cfg.metric, span=cfg.span, pbf=cfg.free[0], pef=cfg.free[1], tbf=cfg.free[2], tef=cfg.free[3],
                          scope=cfg.scope, memory=cfg.memory, heuristic=cfg.heuristic, min_score=cfg.min_score, min_length=cfg.min_length, **pen)


def oracle_batch(orc, cfg, pairs):
    pats, txts = [p for p, _ in pairs], [t for _, t in pairs]
    n = len(pairs)
    plen = np.array([len(x) for x in pats], np.uint32)
    tlen = np.array([len(x) for x in txts], np.uint32)
    blob = b"".join(pats) + b"".join(txts)
    pat_off = np.zeros(n, np.uint64)
    pat_off[1:] = np.cumsum(plen[:-1], dtype=np.uint64)
    txt_off = np.zeros(n, np.uint64)
    txt_off[1:] = np.cumsum(tlen[:-1], dtype=np.uint64)
    txt_off += np.uint64(int(plen.sum()))
    coff = np.zeros(n + 1, np.uint64)
    coff[1:] = np.cumsum(plen.astype(np.uint64) + tlen.astype(np.uint64) + 1, dtype=np.uint64)
    batch = dict(seqs=np.frombuffer(blob, np.uint8).copy() if blob else np.zeros(1, np.uint8), pat_off=pat_off, pat_len=plen,
                 txt_off=txt_off, txt_len=tlen, cigar_off=coff, ops_off=coff)
    res = orc.wfa_batch(oracle_params(orc, cfg), batch, n_threads=8, want_ops=cfg.want_ops)
    res["cigar_off"] = coff
    return res


def run(orc, name, cfg):
    return C.verify(name, cfg, oracle_batch(orc, cfg, C.pairs(name)), "oracle")


# ---------------------------------------------------------------------------------------------------------- pywfa against itself
def test_the_numpy_form_equals_the_plain_form():
    """240 pairs of up to 45 x 75 bases, every penalty set and span in turn -- the row form's prefix minimum is exact"""
    rng = np.random.default_rng(31)
    n = 0
    for k in range(240):
        metric, pen = C.PENALTY_SETS[k % len(C.PENALTY_SETS)]
        span, free = C.SPANS[(k // len(C.PENALTY_SETS) + k) % len(C.SPANS)]
        a = rand_dna(rng, int(rng.integers(0, 46)))
        b = [rand_dna(rng, int(rng.integers(0, 30))), b""][k % 2] + C.noisy(rng, a, 0.15) + rand_dna(rng, int(rng.integers(0, 30)))
        if k % 7 == 0:
            a, b = b, a
        if k % 11 == 0:
            a, b = (b"AT" * 9)[:len(a)], (b"TA" * 20)[:len(b)]
        plain, rows = pywfa.optimum(a, b, metric, pen, span, *free), pywfa.optimum_rows(a, b, metric, pen, span, *free)
        assert plain == rows, (k, metric, pen, span, free, a, b, plain, rows)
        n += 1
    assert n >= 200
    # the combined key of match_bracket on the plain form's terms: the optimum it reports is the optimum
    for k in range(40):
        a = rand_dna(rng, 30)
        b = rand_dna(rng, 15) + C.noisy(rng, a, 0.2) + rand_dna(rng, 15)
        cost, lo, hi = pywfa.match_bracket(a, b)
        assert cost == pywfa.optimum(a, b, "affine", (2, 5, 1), "endsfree", 0, 0, -1, -1) and 0 <= lo <= hi <= 30
        assert pywfa.end_positions(a, b)[0] == cost


def _hand_made():
    """a correct result built by hand (no aligner involved): text-free (2,5,1); six free text bases, ten matches, a substitution, nine
    matches, an insertion of two, twenty matches, four free text bases"""
    rng = np.random.default_rng(5)
    while True:
        core = b"A" + rand_dna(rng, 39)
        mid = bytes([b"ACGT"[(b"ACGT".index(core[10]) + 1) % 4]])
        ins = rand_dna(rng, 2)
        text = rand_dna(rng, 5) + b"A" + core[:10] + mid + core[11:20] + ins + core[20:] + rand_dna(rng, 4)
        ops = "I" * 6 + "M" * 10 + "X" + "M" * 9 + "II" + "M" * 20 + "I" * 4
        res = dict(score=-9, n_match=39, span4=[0, 40, 6, 48], cigar=pywfa.run_length_cigar(ops), ops=ops)
        if pywfa.optimum(core, text, "affine", (2, 5, 1), "endsfree", 0, 0, -1, -1) == 9:
            return core, text, res


def test_the_checker_rejects_every_damaged_result():
    """A checker that accepted everything would go unnoticed: a correct result, then the same result damaged in each way the checker is
    there to catch; it must name the clause."""
    p, t, good = _hand_made()
    args = ("affine", (2, 5, 1), "endsfree", (0, 0, -1, -1))

    def check(res, exact=True, cigar_only=False):
        res = dict(res)
        if cigar_only:
            res["ops"] = None
        return pywfa.check_alignment(p, t, *args, res, exact, 9)

    assert check(good) == 9 and check(good, cigar_only=True) == 9

    def damaged(clause, cigar_only=False, **change):
        res = dict(good, **change)
        if "ops" in change and "cigar" not in change:
            res["cigar"] = pywfa.run_length_cigar(change["ops"])
        with pytest.raises(pywfa.Rejected) as e:
            check(res, cigar_only=cigar_only)
        assert e.value.clause == clause, (clause, str(e.value))

    ops = good["ops"]
    for both in (False, True):
        damaged("bases", both, ops=ops[:8] + "X" + ops[9:])                                   # one M turned into X
        damaged("consumes", both, ops=ops[:30] + ops[31:])                                    # one operation dropped
        damaged("consumes", both, ops=ops + "M")
        # a leading I moved behind the first M (the text has A A there: the bases still fit, but the moved base is now a paid gap)
        damaged("score", both, ops="I" * 5 + "M" + "I" + ops[7:], span4=[0, 40, 5, 48])
        for k in range(4):                                                                    # span4 shifted by one, each entry
            for d in (-1, 1):
                damaged("span", both, span4=[v + d * (i == k) for i, v in enumerate(good["span4"])])
        damaged("score", both, score=-10)
        damaged("score", both, score=-8)
        damaged("sign", both, score=9)
        damaged("n_match", both, n_match=38)
        damaged("n_match", both, n_match=40)
        w = good["cigar"][1]
        damaged("cigar", both, cigar=good["cigar"][:1] + [(4 << 4) | 7, (6 << 4) | 7] + good["cigar"][2:])   # a run split in two
        damaged("cigar", both, cigar=good["cigar"][:1] + [w, 7] + good["cigar"][2:])                          # an empty run
    damaged("cigar", ops=ops, cigar=good["cigar"][:-1])                                      # (with operations: the two must agree)
    # an alignment one penalty unit worse than the optimum, consistent in itself: rejected exactly when the aligner claims to be exact
    a, b = b"ACGTACGT", b"ACGAACGT"
    worse = dict(score=2, n_match=7, span4=[0, 8, 0, 8], ops="MMMIDMMMM", cigar=pywfa.run_length_cigar("MMMIDMMMM"))
    assert pywfa.optimum(a, b, "edit") == 1
    assert pywfa.check_alignment(a, b, "edit", (), "end2end", (0, 0, 0, 0), worse, False, 1) == 2
    with pytest.raises(pywfa.Rejected) as e:
        pywfa.check_alignment(a, b, "edit", (), "end2end", (0, 0, 0, 0), worse, True, 1)
    assert e.value.clause == "optimum"
    with pytest.raises(pywfa.Rejected) as e:   # ... and a substitution is no operation of the indel metric
        pywfa.check_alignment(a, b, "indel", (), "end2end", (0, 0, 0, 0), dict(worse, ops="MMMXMMMM", cigar=pywfa.run_length_cigar("MMMXMMMM"), score=1), True, 2)
    assert e.value.clause == "bases"
    # score-only scope
    pywfa.check_score(-9, "affine", True, 9)
    pywfa.check_score(-11, "affine", False, 9)
    for score, metric, exact, clause in ((9, "affine", True, "sign"), (-1, "edit", True, "sign"), (-10, "affine", True, "optimum"),
                                         (-8, "affine", False, "optimum"), (3, "edit", True, "optimum")):
        with pytest.raises(pywfa.Rejected) as e:
            pywfa.check_score(score, metric, exact, 9 if metric == "affine" else 2)
        assert e.value.clause == clause


SHARE_EXACT = dict(too_long_for_lds=14 / 15)  # every other list: all of it


def test_the_lists_are_what_they_say():
    for name in C.LISTS:
        assert len(C.pairs(name)) == C.N_PAIRS[name]
        assert C.share_exact(name) == SHARE_EXACT.get(name, 1.0), name
    # the boundaries of the register-resident tiers, as wfa_lean.hip's set_window has them
    for name, limit in (("lean_tier1", 55), ("lean_tier2", 119), ("lean_tier3", 247)):
        d = [abs(len(t) - len(p)) for p, t in C.pairs(name)]
        assert {limit - 1, limit, limit + 1, limit + 2} <= set(d), (name, d)
    assert {(len(p), len(t)) for p, t in C.pairs("lean_lengths")} == {(a, b) for a in (99, 100, 101) for b in (99, 100, 101)}
    # gaps of 9, 10 and 11 bases: the second two-piece set changes piece exactly there
    two = C.PENALTY_SETS[-1][1]
    assert [pywfa.gap_cost("affine2p", two, n) for n in (9, 10, 11)] == [29, 31, 33] and 2 + 3 * 9 == 29 and 11 + 2 * 10 == 31 < 2 + 3 * 10
    ends = wide = 0
    for name in C.TIE_LISTS:
        e, w = C.tie_counts(name)
        print("%s: %d pairs, %d with several optimal end positions, %d with a bracket of more than one value" % (name, C.N_PAIRS[name], e, w))
        ends += e
        wide += w
    assert ends >= 100 and wide >= 100, (ends, wide)


# ------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("metric,pen", C.PENALTY_SETS, ids=["%s%s" % (m, "-".join(map(str, p))) for m, p in C.PENALTY_SETS])
def test_oracle_every_metric_and_span(oracle, metric, pen):
    n = 0
    for name, cfg in C.METRIC_PLAN:
        if (cfg.metric, cfg.pen) == (metric, tuple(pen)):
            done = run(oracle, name, cfg)
            assert cfg.heuristic != "none" or done == C.N_PAIRS[name]
            n += 1
    assert n >= 8


@pytest.mark.parametrize("want_ops", [False, True])
def test_oracle_biwfa_lists(oracle, want_ops):
    for cfg in C.lean_configs(want_ops):
        for name in C.LEAN_LISTS:
            run(oracle, name, cfg)
    assert run(oracle, "lean_deep", C.DEEP_CONFIG._replace(want_ops=want_ops)) == 3
    assert run(oracle, "lean_deep", C.DEEP_CONFIG._replace(want_ops=want_ops, heuristic="default")) >= 1
    print("BiWFA under the heuristic, score != cost of the CIGAR:", sorted(set(C.PROMISES_NOT_KEPT)))


def test_oracle_flank_shape_ties_and_a_long_pair(oracle):
    flank = C.config("affine", (2, 5, 1), C.TEXT_FREE)
    for name in ("flank_shape",) + C.TIE_LISTS:
        assert run(oracle, name, flank) == C.N_PAIRS[name]
        assert run(oracle, name, flank._replace(want_ops=False)) == C.N_PAIRS[name]
    for cfg in (C.config("affine", (2, 5, 1)), C.config("affine", (4, 6, 2)), flank):
        assert run(oracle, "too_long_for_lds", cfg) == 15   # (the long pair: validity, cost = score, span)


# ------------------------------------------------------------------------------------------------------------ flank location
def oracle_spans(orc, loci, flank_len, frac):
    """find_tr_spans (span_locater.rs:32-68) from the oracle's find_spans; per piece also (start, end, aligned) of what it found"""
    ss, se, lh, rh, found = [], [], [], [], []
    thr = float(flank_len) * frac
    for L in loci:
        ls, le, lu, _ = orc.find_spans(L["left_flank"][-flank_len:], L["reads"], 2, 5, 1, threshold=thr)
        rs, re_, ru, _ = orc.find_spans(L["right_flank"][:flank_len], L["reads"], 2, 5, 1, threshold=thr)
        for i in range(len(L["reads"])):
            hl = 0 if ls[i] < 0 else (2 if lu[i] else 1)
            hr = 0 if rs[i] < 0 else (2 if ru[i] else 1)
            both = hl and hr and le[i] <= rs[i]
            ss.append(int(le[i]) if both else -1)
            se.append(int(rs[i]) if both else -1)
            lh.append(hl)
            rh.append(hr)
            found.append(((int(ls[i]), int(le[i])), (int(rs[i]), int(re_[i]))))
    return ss, se, lh, rh, found


@pytest.mark.parametrize("flank_len", [250, 40])
def test_oracle_flank_location(oracle, flank_len):
    loci, jobs = C.flank_loci(flank_len)
    ss, se, lh, rh, found = oracle_spans(oracle, loci, flank_len, 0.7)
    n_found, n_missed, n_undecided = C.verify_flank(flank_len, 0.7, ss, se, lh, rh, "oracle")
    print("flank_len %d: %d found, %d missed, %d undecided of %d" % (flank_len, n_found, n_missed, n_undecided, len(jobs)))
    assert 10 * n_undecided <= len(jobs) and n_found >= 20 and n_missed >= 5  # (at most one in ten undecided; both verdicts well represented)
    # both ends of what the oracle aligned (the stand-alone entry of the product shows one end per read)
    for (l, side, k), a in zip(jobs, C.flank_answers(flank_len)):
        (ts, te) = found[2 * l][0 if side == "left" else 1]
        if ts >= 0:
            L = loci[l]
            piece = L["left_flank"] if side == "left" else L["right_flank"]
            assert pywfa.placement_is_optimal(piece, L["reads"][0], ts, te), (flank_len, l, side, ts, te, a)
