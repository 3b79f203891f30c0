"""The designed cases of the plot path (trgt_plot_align_batch, tests/test_plot_align_gpu.py; the restatement tests/pytrvz.py), each with
the conditions it was built to realise, and a self-check that ASSERTS every condition from what the oracle answers -- its state paths,
events and alignment operations -- not from how a case was put together: where the aligner places a gap or the HMM a copy is its
decision, and a case that no longer realises its condition must fail here, not pass silently on the GPU.

A case is dict(name=, mode=, panel=dict(motifs=, lf=, rf=, ref=, reads=[dict(seq=, betas=[(pos, value)])]), want={condition, ...}).
expected(case) is what pytrvz computes for it from the oracle's answers, computed once and shared.
"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytrvz  # noqa: E402

EVN = "MXIDTS[]"  # one letter per HmmEvent number (pytrvz.EV_*)


# ------------------------------------------------------------------------------------------------------ the two inputs from below
def _s(x):
    return x.decode() if isinstance(x, (bytes, bytearray)) else x


_HMM_CACHE, _WFA_CACHE = {}, {}


def hmm_paths(motifs, seq):
    """-> (path of Hmm::label, path after remove_imperfect_motifs(.., 6)) from the oracle"""
    from oracle import binding as orc
    motifs, seq = [_s(m) for m in motifs], _s(seq)
    key = (tuple(motifs), seq)
    if key not in _HMM_CACHE:
        path = orc.hmm_label(motifs, seq)
        _HMM_CACHE[key] = (path, orc.hmm_remove_imperfect(motifs, path, seq, 6))
    return _HMM_CACHE[key]


def hmm_oracle(motifs, seq):
    """the `hmm` parameter of pytrvz from the oracle: (events, motif spans) of the path after remove_imperfect_motifs"""
    from oracle import binding as orc
    motifs, seq = [_s(m) for m in motifs], _s(seq)
    _, kept = hmm_paths(motifs, seq)
    return [int(e) for e in orc.hmm_events(motifs, kept, seq)], [tuple(int(v) for v in sp) for sp in orc.hmm_label_motifs(motifs, kept)]


def hmm_pyhmm(motifs, seq):
    """the same from tests/pyhmm.py (oracle-free; slow on large models)"""
    import pyhmm
    model = pyhmm.build(motifs)
    kept = pyhmm.remove_imperfect_motifs(model, pyhmm.label(model, seq).path, seq, 6)
    return pyhmm.events(model, kept, seq), pyhmm.label_motifs(model, kept)


def wfa_oracle(pattern, text):
    """the `wfa` parameter of pytrvz: WFAligner::builder(Alignment, MemoryHigh).affine(2, 5, 1).build().align_end_to_end from the oracle"""
    from oracle import binding as orc
    key = (bytes(pattern), bytes(text))
    if key not in _WFA_CACHE:
        r = orc.wfa_align(orc.wfa_params("affine", x=2, o1=5, e1=1, span="end2end", scope="alignment", memory="high", heuristic="default"), key[0], key[1])
        assert r["status"] == 0, r["status"]
        _WFA_CACHE[key] = (r["ops"], r["score"])
    return _WFA_CACHE[key]


# -------------------------------------------------------------------------------------------------------------------- sequences
def rand_seq(rng, n, avoid=""):
    out = []
    for _ in range(n):
        prev = out[-1] if out else avoid
        out.append(rng.choice([c for c in "ACGT" if c != prev]))  # no homopolymer runs: a gap has one place to go
    return "".join(out)


_R = random.Random(20240611)
A, B = "CAGCAGT", "GGCCTTA"            # two motifs of 7 bases: their imperfect copies are kept (remove_imperfect_motifs drops up to 6)
LF, RF = "TGACTACGATCTAGTCATGCATGTCAGTACTGACATGATCGTACGTATCA", "ATCGTATGCTAGTCATACGTAGCTGATGTCATGCATACGTGACTGTACAG"  # 50 + 50
LF200, RF200 = rand_seq(_R, 200), rand_seq(_R, 200)
M35 = [rand_seq(_R, 35), rand_seq(_R, 35)]                 # 7 + 2 * 106 = 219 states on four waves: no position-per-lane fill
M120 = [rand_seq(_R, 120) for _ in range(3)]               # 7 + 3 * 361 = 1090 states: hmm_viterbi_big_kernel
assert len(LF) == 50 and len(RF) == 50


def sub(seq, pos, shift=1):
    """the base at pos replaced by another one"""
    return seq[:pos] + "ACGT"[("ACGT".index(seq[pos]) + shift) % 4] + seq[pos + 1:]


def spaced_mismatches(seq, k, first=3, step=7):
    for i in range(k):
        seq = sub(seq, first + i * step)
    return seq


# the repeat parts: (name, motifs, sequence, conditions)
TRS = [
    ("perfect", [A, B], A * 5, {"perfect"}),
    ("edits", [A, B], A * 2 + "CAGCTGT" + A + "CAGACAGT" + A + "CAGAGT" + A, {"mismatch", "insertion", "deletion_state", "kept_copy_of_7"}),
    ("leading_dels", [A, B], "GCAGT" + A * 2 + "GCAGT" + A, {"implied_leading_dels"}),
    ("closing_del_mid", [A, B], A * 2 + "CAGCAG" + B * 2, {"closing_del_takes_next_type"}),
    ("closing_del_end", [A, B], B * 2 + "CAGCAG", {"closing_del_at_end"}),
    ("closing_del2_end", [A, B], A * 2 + "CAGCA", {"closing_del_at_end"}),
    ("dropped6_kept7", ["CAGCAG", A], "CAGCAG" * 2 + "CAGCTG" + "CAGCAG" + A + "CAGCTGT" + A, {"dropped_copy_le_6", "kept_copy_of_7"}),
    ("skip_bases", [A, B], A * 2 + "TTTTTTTTT" + B * 2, {"skip_bases"}),
    ("empty", [A, B], "", {"empty_tr"}),
    ("path63", ["CAG", B], "CAG" * 4 + B * 3, {"path_63"}),
    ("path64", ["CAG", B], "CAG" + B * 5, {"path_64"}),
    ("path65", ["CAG", B], "CAG" * 9, {"path_65"}),
    ("path198", ["CAG", B], "CAG" * 28, {"path_about_200", "run_crosses_64"}),
    ("run_ends_on_63", ["CAG", B], "CAG" * 2 + B * 4 + "CAG" + B * 2, {"run_ends_on_63"}),
    ("one_motif_of_three", ["CAG", "CCG", "A"], "CAG" * 3 + "CCG" * 2 + "AAAA" + "CAG", {"perfect"}),
    ("multi_wave", M35, M35[0] + sub(M35[1], 10) + M35[0][:20] + M35[0][22:] + M35[1][:12] + "T" + M35[1][12:], {"model_multi_wave", "mismatch", "deletion_state", "insertion"}),
    ("big_model", M120, M120[0] + sub(M120[1], 40)[:100] + M120[1][102:] + M120[2][5:60], {"model_big"}),
]
TR_BY_NAME = {t[0]: t for t in TRS}


def designed_betas(ref, seq, extra=()):
    """Betas at the positions the issue names, found in the oracle's alignment of seq against ref: the first and the last base, the first
    mismatch, the middle of the first insertion, and the read position right behind EVERY deletion run.  Values: 0.01 * position."""
    ops, _ = wfa_oracle(ref.encode(), seq.encode())
    pos = {0, len(seq) - 1} | set(extra)
    sp, seen_x, seen_i, i = 0, False, False, 0
    while i < len(ops):
        j = i
        while j < len(ops) and ops[j] == ops[i]:
            j += 1
        if ops[i] == "X" and not seen_x:
            pos.add(sp)
            seen_x = True
        if ops[i] == "I" and not seen_i:
            pos.add(sp + (j - i) // 2)
            seen_i = True
        if ops[i] == "D" and sp < len(seq):
            pos.add(sp)
        sp += (j - i) if ops[i] in "MXI" else 0
        i = j
    return [(p, round(0.01 * p, 4)) for p in sorted(p for p in pos if 0 <= p < len(seq))]


def _read(ref, seq, betas="designed", extra=()):
    if betas == "designed":
        return dict(seq=seq, betas=designed_betas(ref, seq, extra))
    return dict(seq=seq, betas=list(betas or []))


def _build():
    cases = []
    # ---- mode 0: every repeat part as the allele of a consensus, with an identical read and one with a mismatch in each flank
    for name, motifs, tr, want in TRS:
        ref = LF + tr + RF
        reads = [_read(ref, ref, None), _read(ref, sub(sub(ref, 10), len(ref) - 7))]
        cases.append(dict(name="allele_" + name, mode=0, panel=dict(motifs=motifs, lf=LF, rf=RF, ref=ref, reads=reads), want=set(want) | {"read_identical", "betas_none"}))
    # ---- mode 0: conversion
    tr = A * 3 + B * 2
    ref = LF + tr + RF
    lf, e = len(LF), len(LF) + len(tr)
    conv = [
        ("del_across_lf_tr", ref[:lf - 2] + ref[lf + 2:]), ("del_across_tr_rf", ref[:e - 2] + ref[e + 3:]),
        ("subst_across_lf_tr", sub(sub(ref, lf - 1), lf)), ("subst_across_tr_rf", sub(sub(ref, e - 1), e)),
        ("ins_at_lf_tr", ref[:lf] + "TT" + ref[lf:]), ("ins_at_tr_rf", ref[:e] + "CC" + ref[e:]),
        ("leading_trailing_ins", "GG" + ref + "CC"),
        ("ins_and_del", ref[:20] + "ACA" + ref[20:70] + ref[73:120] + ref[122:]),
    ]
    cases.append(dict(name="convert_boundaries", mode=0, panel=dict(motifs=[A, B], lf=LF, rf=RF, ref=ref, reads=[_read(ref, s) for _, s in conv] + [_read(ref, ref)]),
                      want={c for c, _ in conv[:6]} | {"match_across_lf_tr", "match_across_tr_rf", "leading_ins", "trailing_ins", "beta_first", "beta_last", "beta_on_mismatch_kept",
                                                       "beta_in_insertion_dropped", "beta_behind_every_deletion_dropped"}))
    tr = A + "CAGAGT" + "CAGCTGT" + "CAGACAGT" + A
    ref = LF + tr + RF
    cases.append(dict(name="convert_mixed_consensus", mode=0, panel=dict(motifs=[A, B], lf=LF, rf=RF, ref=ref, reads=[_read(ref, ref), _read(ref, sub(ref, len(LF) + 9))]),
                      want={"consensus_ops_inside_one_type"}))
    # reads with 63 / 64 / 65 and at least 130 CIGAR runs, and as many segments: k mismatches give 2 k + 1 runs, a trailing insertion one more
    ref = LF200 + "CAG" * 20 + RF200
    many = []
    for k, tail in ((30, ""), (30, "A"), (31, ""), (31, "A"), (32, ""), (32, "A"), (65, ""), (66, "A")):
        many.append(_read(ref, spaced_mismatches(ref, k) + tail, None))
    many.append(dict(seq=ref, betas=[(p, 0.5) for p in range(0, len(ref), 3)]))
    many.append(_read(ref, spaced_mismatches(ref[:150] + ref[153:], 12, 5, 11) + "", "designed"))
    cases.append(dict(name="convert_many_runs", mode=0, panel=dict(motifs=["CAG"], lf=LF200, rf=RF200, ref=ref, reads=many),
                      want={"runs_63", "runs_64", "runs_65", "runs_130", "segs_63", "segs_64", "segs_65", "segs_130", "betas_gt_64"}))
    # ---- mode 0: order
    tr = A * 4
    ref = LF + tr + RF
    reads = [_read(ref, sub(sub(ref, 5), 80), None), _read(ref, sub(ref, 30), None), _read(ref, ref, None), _read(ref, sub(ref, 30), None), _read(ref, ref[:60] + ref[61:], None),
             _read(ref, ref, None), _read(ref, sub(ref, 31), None)]
    cases.append(dict(name="order_scores", mode=0, panel=dict(motifs=[A], lf=LF, rf=RF, ref=ref, reads=reads), want={"order_equal_len_diff_score", "order_equal_len_equal_score"}))
    # ---- mode 1: every repeat part inside reads whose flanks are exact, carry a mismatch, or lost / gained a base
    for group, names in (("a", ["perfect", "edits", "leading_dels", "empty", "closing_del_mid"]), ("b", ["closing_del_end", "closing_del2_end", "skip_bases"]), ("g", ["dropped6_kept7"]),
                         ("c", ["path63", "path64", "path65", "run_ends_on_63", "path198"]), ("d", ["one_motif_of_three"]), ("e", ["multi_wave"]), ("f", ["big_model"])):
        motifs = TR_BY_NAME[names[0]][1]
        reads, want = [], {"mode1"}
        for i, n in enumerate(names):
            assert TR_BY_NAME[n][1] == motifs
            t = TR_BY_NAME[n][2]
            want |= TR_BY_NAME[n][3]
            indel = bool(t) and group in "ab"   # (elsewhere the repeat part must stay what its name says: the read is cut by length)
            lfv = [LF, sub(LF, 17), LF[:30] + LF[31:] if indel else LF][i % 3]   # exact, a mismatch, a base lost (the repeat's first base moves into the read's first 50)
            rfv = [RF, sub(sub(RF, 3), 4), RF[:12] + "G" + RF[12:] if indel else RF][(i + 1) % 3]
            seq = lfv + t + rfv
            cuts = {len(LF) - 1, len(LF), len(seq) - len(RF) - 1, len(seq) - len(RF)}
            reads.append(dict(seq=seq, betas=[(p, round(0.001 * p, 4)) for p in sorted({0, 5, 18, 31, len(seq) - 45, len(seq) - 1} | cuts) if 0 <= p < len(seq)]))
        if group == "a":
            want |= {"longest_not_last", "beta_both_sides_of_both_boundaries", "flank_with_indel"}
        cases.append(dict(name="waterfall_" + group, mode=1, panel=dict(motifs=motifs, lf=LF, rf=RF, ref=LF + RF, reads=reads), want=want))
    return cases


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


_EXPECTED = {}


def expected(case):
    """what pytrvz computes for the case from the oracle's answers: dict(seq=, reads=, order=, scores=) (mode 1: seq None, scores None)"""
    if case["name"] not in _EXPECTED:
        p = case["panel"]
        if case["mode"] == 0:
            _EXPECTED[case["name"]] = pytrvz.get_allele_align(p["motifs"], p["lf"], p["rf"], p["ref"], p["reads"], hmm_oracle, wfa_oracle)
        else:
            r = pytrvz.waterfall_align(p["motifs"], p["lf"], p["rf"], p["reads"], hmm_oracle, wfa_oracle)
            _EXPECTED[case["name"]] = dict(seq=None, reads=r["reads"], order=r["order"], scores=None)
    return _EXPECTED[case["name"]]


# -------------------------------------------------------------------------------------------------------------------- self-check
def _runs(ops):
    out, i, ref, sp = [], 0, 0, 0
    while i < len(ops):
        j = i
        while j < len(ops) and ops[j] == ops[i]:
            j += 1
        out.append((ops[i], j - i, ref, sp))  # (op, length, first reference position, first read position)
        ref += (j - i) if ops[i] in "MXD" else 0
        sp += (j - i) if ops[i] in "MXI" else 0
        i = j
    return out


def _hmm_conditions(motifs, seq):
    """the conditions a repeat part realises, read off the oracle's paths and events"""
    got = set()
    if not seq:
        return {"empty_tr"}
    from oracle import binding as orc
    import pyhmm
    path, kept = hmm_paths(motifs, seq)
    ev0 = "".join(EVN[e] for e in orc.hmm_events(motifs, path, seq))
    events, spans = hmm_oracle(motifs, seq)
    ev = "".join(EVN[e] for e in events)
    segs = pytrvz.align_motifs(motifs, seq, hmm_oracle)
    n_states = 7 + sum(3 * len(m) + 1 for m in motifs)
    if n_states > 1024:
        got.add("model_big")        # hmm_set_class: more than 16 waves
    elif n_states > 64 and sum(len(m) for m in motifs) + 1 > 64:
        got.add("model_multi_wave")  # layout_set: n_lanes != 0 above 64 states, ppl_lanes == 0 beyond 64 motif positions
    if set(ev) <= set("MT[]"):
        got.add("perfect")
    if "X" in ev:
        got.add("mismatch")
    if "I" in ev:
        got.add("insertion")
    if "[D" in ev:
        got.add("implied_leading_dels")
    if any(ev[i] == "D" and ev[i - 1] in "MXI" for i in range(1, len(ev))):
        got.add("deletion_state")
    if "S" in ev0:
        got.add("skip_bases")
    if ev.rstrip("T").endswith("D]"):
        got.add("closing_del_at_end")
        assert segs[-1][:2] == (0, pytrvz.INS) and segs[-1][2] == segs[-2][2]  # ... and takes the type of the last base
    # a deletion that closes a copy in front of ANOTHER motif's copy: its width-0 Ins segment has the next copy's type
    for i in range(1, len(segs) - 1):
        if segs[i][:2] == (0, pytrvz.INS) and segs[i][2] == segs[i + 1][2] != segs[i - 1][2] and "D]" in ev:
            got.add("closing_del_takes_next_type")
    # visits: (motif index, events of the visit) before and after remove_imperfect_motifs
    v0, v1 = ev0.replace("T", "").split("]")[:-1], ev.replace("T", "").split("]")[:-1]
    assert len(v0) == len(v1) == len(spans)
    for a, b, sp in zip(v0, v1, spans):
        if a != b:
            assert set(b) <= set("[S") and sp[0] == len(motifs)
            got.add("dropped_copy_le_6")
        elif sp[0] < len(motifs) and len(motifs[sp[0]]) == 7 and set(b) & set("XID"):
            got.add("kept_copy_of_7")
    n = len(path)
    got |= {"path_%d" % n} if n in (63, 64, 65) else set()
    if 190 <= n <= 210:
        got.add("path_about_200")
    # path entry of every base (the emitting entries of Hmm::label's path, in order), then the entries of every segment's bases
    model = pyhmm.build(motifs)
    entry_of_base = [j for j, s in enumerate(path) if model.emits_base(int(s))]
    assert len(entry_of_base) == len(seq)
    at = 0
    for k, (width, op, _) in enumerate(segs):
        if op == pytrvz.INS:
            continue
        first, last = entry_of_base[at], entry_of_base[at + width - 1]
        if first < 64 <= last:
            got.add("run_crosses_64")
        nxt = entry_of_base[at + width] if at + width < len(seq) else None
        if last == 63 and nxt is not None and nxt > 64:
            got.add("run_ends_on_63")
        at += width
    assert at == len(seq)
    return got


def conditions(case):
    """every condition the case realises, as the oracle's answers show it"""
    p, got = case["panel"], set()
    lf, rf = len(p["lf"]), len(p["rf"])
    exp = expected(case)
    if case["mode"] == 1:
        got.add("mode1")
        lens = [len(r["seq"]) for r in p["reads"]]
        if lens.index(max(lens)) != len(lens) - 1 and len(set(lens)) > 1:
            got.add("longest_not_last")
        for r in p["reads"]:
            tr = r["seq"][lf:len(r["seq"]) - rf]
            got |= _hmm_conditions(p["motifs"], tr)
            pos = {b[0] for b in r["betas"]}
            if tr and {lf - 1, lf, lf + len(tr) - 1, lf + len(tr)} <= pos:
                got.add("beta_both_sides_of_both_boundaries")
            for flank, part in ((p["lf"], r["seq"][:lf]), (p["rf"], r["seq"][len(r["seq"]) - rf:])):
                if set(wfa_oracle(flank.encode(), part.encode())[0]) & set("ID"):
                    got.add("flank_with_indel")
        return got
    tr = p["ref"][lf:len(p["ref"]) - rf]
    got |= _hmm_conditions(p["motifs"], tr)
    e = lf + len(tr)
    # consensus: Ins (width 0), Subst and Del segments inside one seg type, under one read segment
    by_type = {}
    for width, op, t in exp["seq"]:
        by_type.setdefault(t, set()).add(op)
    mixed = [t for t, ops in by_type.items() if {pytrvz.INS, pytrvz.SUBST, pytrvz.DEL} <= ops]
    scores, lens = exp["scores"], [len(r["seq"]) for r in p["reads"]]
    for i in range(len(lens)):
        for j in range(i + 1, len(lens)):
            if lens[i] == lens[j]:
                got.add("order_equal_len_equal_score" if scores[i] == scores[j] else "order_equal_len_diff_score")
    for k, r in enumerate(p["reads"]):
        ops, _ = wfa_oracle(p["ref"].encode(), r["seq"].encode())
        runs = _runs(ops)
        align, kept = exp["reads"][exp["order"].index(k)]
        if set(ops) == {"M"}:
            got.add("read_identical")
            if mixed and sum(1 for s in align if s[2] in mixed) == len(mixed):
                got.add("consensus_ops_inside_one_type")
        for n in (63, 64, 65):
            if len(runs) == n:
                got.add("runs_%d" % n)
            if len(align) == n:
                got.add("segs_%d" % n)
        if len(runs) >= 130:
            got.add("runs_130")
        if len(align) >= 130:
            got.add("segs_130")
        for op, n, r0, s0 in runs:
            for name, cut in (("lf_tr", lf), ("tr_rf", e)):
                if op != "I" and r0 < cut < r0 + n:
                    got.add({"M": "match", "X": "subst", "D": "del"}[op] + "_across_" + name)
                if op == "I" and r0 == cut:
                    got.add("ins_at_" + name)
        if ops[0] == "I":
            got.add("leading_ins")
        if ops[-1] == "I":
            got.add("trailing_ins")
        betas = {b[0] for b in r["betas"]}
        kept_at = {b[0] for b in kept}
        got.add("betas_none" if not betas else "betas_some")
        if len(betas) > 64:
            got.add("betas_gt_64")
        if 0 in betas:
            got.add("beta_first")
        if len(r["seq"]) - 1 in betas:
            got.add("beta_last")
        dels = [(r0, s0) for op, n, r0, s0 in runs if op == "D" and s0 < len(r["seq"])]
        if dels and all(s0 in betas for _, s0 in dels):
            # the beta right behind a deletion run is dropped: no kept beta sits where that base projects to
            first_ref_behind = {r0 + n for op, n, r0, s0 in runs if op == "D"}
            if len(kept) < len(betas) and not (first_ref_behind & kept_at):
                got.add("beta_behind_every_deletion_dropped")
        for op, n, r0, s0 in runs:
            if op == "X" and s0 in betas and r0 in kept_at:
                got.add("beta_on_mismatch_kept")
            if op == "I" and any(s0 <= b < s0 + n for b in betas) and len(kept) < len(betas):
                got.add("beta_in_insertion_dropped")
    return got


REQUIRED = {
    "perfect", "mismatch", "insertion", "deletion_state", "implied_leading_dels", "closing_del_takes_next_type", "closing_del_at_end", "dropped_copy_le_6", "kept_copy_of_7",
    "skip_bases", "empty_tr", "path_63", "path_64", "path_65", "path_about_200", "run_crosses_64", "run_ends_on_63", "model_multi_wave", "model_big",
    "read_identical", "match_across_lf_tr", "match_across_tr_rf", "del_across_lf_tr", "del_across_tr_rf", "subst_across_lf_tr", "subst_across_tr_rf", "ins_at_lf_tr",
    "ins_at_tr_rf", "leading_ins", "trailing_ins", "consensus_ops_inside_one_type", "runs_63", "runs_64", "runs_65", "runs_130", "segs_63", "segs_64", "segs_65", "segs_130",
    "betas_none", "beta_first", "beta_last", "beta_on_mismatch_kept", "beta_in_insertion_dropped", "beta_behind_every_deletion_dropped", "betas_gt_64",
    "beta_both_sides_of_both_boundaries", "order_equal_len_diff_score", "order_equal_len_equal_score", "longest_not_last", "mode1", "flank_with_indel",
}


def self_check():
    """every case realises what it was built for, and together they realise everything the kernels have to get right"""
    seen = set()
    for case in cases():
        got = conditions(case)
        assert case["want"] <= got, (case["name"], sorted(case["want"] - got))
        seen |= got
    assert REQUIRED <= seen, sorted(REQUIRED - seen)
    return seen
