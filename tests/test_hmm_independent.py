"""The motif HMM held to something other than the oracle: tests/pyhmm.py, a generic restatement written from the reference's
src/hmm/*.rs alone (states, in-edge lists, ln tables, the order of order_states; no blocks, positions or lanes).

  reference vectors -> pyhmm        the eleven KATs of tests/golden/hmm_kats.json, directly
  oracle == pyhmm, bit for bit      every field the reference defines, on the shape lists of tests/hmm_cases.py (the lists
                                    tests/test_hmm_independent_gpu.py runs through the kernels)
  ties on purpose                   pyhmm counts the cells where two predecessors score EQUAL in f64 -- the first strict maximum in
                                    list order decides there; every list made for ties holds >= 100 of them
  exact optimality                  a path is a walk along existing edges over the whole query, and its exact score (Fraction over the
                                    f64 tables) is within a derived bound of the exact optimum
  ln tables                         math.log of every probability the builder takes ln of is within 1 ulp of the correctly rounded value
  sensitivity                       >= for >, silent states in index order: each breaks the oracle comparison on a listed case

No GPU."""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_cases as HC
import pyhmm

KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hmm_kats.json")))["kats"]


def _summary(spans):  # `summarize` of the reference's tests, builder.rs:191-206: runs of one motif index, (first start, last end, index)
    out = []
    for m, s, e in spans:
        if out and out[-1][2] == m:
            out[-1][1] = e
        else:
            out.append([s, e, m])
    return out


@pytest.mark.parametrize("kat", KATS, ids=[k["id"] for k in KATS])
def test_reference_vectors(kat):
    model = pyhmm.build(kat["motifs"])
    if "summary" in kat:
        for mode in ("f64", "f64-scalar", "exact"):
            path = pyhmm.label(model, kat["query"], mode).path
            if kat["remove_imperfect"]:
                path = pyhmm.remove_imperfect_motifs(model, path, kat["query"], 6)
            assert _summary(pyhmm.label_motifs(model, path)) == kat["summary"], mode
    elif "purity" in kat:
        pur, edit, most = pyhmm.purity(model, pyhmm.label(model, kat["query"]).path, kat["query"])
        if kat["purity"] is None:
            assert math.isnan(pur) and pyhmm.label_with_hmm(kat["motifs"], [kat["query"]])[0]["spans"] == []
        else:
            assert pur == kat["purity"][0] / kat["purity"][1] and (most - edit) * kat["purity"][1] == most * kat["purity"][0]
    else:
        assert chr(pyhmm.base_match(model, kat["state"])) == kat["base_match"]


@pytest.mark.parametrize("name", HC.GROUPS)
def test_oracle_equals_restatement(oracle, name):
    from trgt_amd import hmm as H  # (host-side packing only)
    sets, jobs = HC.group(name)
    refs = HC.reference(name)
    batch = H.pack_hmm_batch([list(s) for s in sets], list(jobs))
    out = oracle.hmm_batch(batch, n_threads=4)
    HC.check_batch(batch, out, refs, name)
    if name in ("ppl", "ties_rotations"):  # ... and the pieces one by one, as the reference composes them (tr.rs:464-470)
        for (s, _), r in zip(jobs, refs):
            if not r["seq"]:
                continue
            motifs, q = [m.decode() for m in pyhmm.clean_motifs(sets[s])], r["seq"].decode()
            path = oracle.hmm_label(motifs, q).tolist()
            assert path == r["path"]
            assert oracle.hmm_events(motifs, path, q).tolist() == pyhmm.events(r["model"], path, q)
            pur, edit, most = oracle.hmm_purity(motifs, path, q)
            assert (np.float64(pur).view(np.uint64), edit, most) == (np.float64(r["purity"]).view(np.uint64), r["edit"], r["maxd"])
            kept = oracle.hmm_remove_imperfect(motifs, path, q, 6).tolist()
            assert kept == pyhmm.remove_imperfect_motifs(r["model"], path, q, 6)
            assert [tuple(x) for x in oracle.hmm_label_motifs(motifs, kept).tolist()] == pyhmm.label_motifs(r["model"], kept)


@pytest.mark.parametrize("name", HC.TIE_GROUPS)
def test_tie_lists_hit_exact_ties(name):
    # a condition on the INPUTS: without equal f64 sums "first strict maximum in list order" decides nothing.  Where the list's
    # structure makes the tie decide the winning path itself (duplicates, rotations, one-base motifs), so many on the path too.
    refs = HC.reference(name)
    assert sum(r["labelling"].ties for r in refs) >= 100
    if name in ("ties_duplicates", "ties_rotations", "ties_homopolymer"):
        assert sum(r["labelling"].path_ties for r in refs) >= 100
    else:
        assert sum(r["labelling"].path_ties for r in refs) >= 1


@pytest.mark.parametrize("name", HC.GROUPS)
def test_paths_are_exact_optima_of_the_f64_tables(name):
    # 0 <= S* - exact(path) <= 8 len(path) 2^-53 |S*| (hmm_cases.path_bound); beyond it the f64 recursion took a worse path
    held = 0
    for j, r in enumerate(HC.reference(name)):
        if r["optimum"] is not None:
            HC.check_optimal(r, r["path"], (name, j))
            held += 1
    assert held >= 1


def test_exact_path_score_refuses_what_is_no_path():
    model = pyhmm.build(["CAG", "A"])
    q = b"CAGCAGA"
    good = pyhmm.label(model, q).path
    assert pyhmm.exact_path_score(model, q, good) == pyhmm.label(model, q, "exact").score
    bad = list(good)
    i = next(i for i, s in enumerate(good) if model.emits_base(s))
    for wrong in (good[:-1], good[1:], bad[:i] + bad[i + 1:], bad[:i] + [bad[i]] + bad[i:]):  # cut short, no start, a state dropped, doubled
        with pytest.raises(AssertionError):
            pyhmm.exact_path_score(model, q, wrong)
    with pytest.raises(AssertionError):
        pyhmm.exact_path_score(model, q + b"A", good)  # consumes less than the query


@pytest.mark.parametrize("name", ("multiwave",) + HC.TIE_GROUPS)
def test_both_f64_fills_of_the_restatement_agree(name):
    # the column-at-a-time fill (numpy over the emitting states) and the cell-by-cell one: same paths, same tie counts
    for r in HC.reference(name):
        if r["seq"]:
            a = pyhmm.label(r["model"], r["seq"], "f64-scalar")
            lab = r["labelling"]
            assert (a.path, a.score, a.ties, a.path_ties) == (lab.path, lab.score, lab.ties, lab.path_ties)


def _differs_somewhere(oracle, **wrong):
    for name in HC.TIE_GROUPS:
        sets, jobs = HC.group(name)
        for (s, _), r in zip(jobs, HC.reference(name)):
            if r["seq"]:
                m = r["model"]
                order = m.visiting_order(by_index=True) if wrong.get("by_index") else None
                got = pyhmm.label(m, r["seq"], "f64-scalar", order=order, strict=not wrong.get("loose", False)).path
                if got != oracle.hmm_label([x.decode() for x in pyhmm.clean_motifs(sets[s])], r["seq"].decode()).tolist():
                    return True
    return False


def test_misreadings_of_the_restatement_do_not_pass(oracle):
    # the last of equal predecessors instead of the first; silent states by index instead of order_states: the tie lists see both
    assert _differs_somewhere(oracle, loose=True)
    assert _differs_somewhere(oracle, by_index=True)


def _ulps(a, b):
    ia, ib = (int(np.float64(x).view(np.int64)) for x in (a, b))
    return abs(ia - ib)


def test_ln_of_every_probability_the_builder_uses():
    """math.log against mpmath at 200 bits rounded to f64: the fixed constants of builder.rs (collected from built models) and
    mismatch_seed_prob * k (builder.rs:93-111) for motifs of 2 to 1 362 bases, the longest under the 4 096-state ceiling.  Within 1 ulp
    everywhere; what is not CORRECTLY rounded is the residue DESIGN.md section 2 lists (f64::ln of the reference could differ there)."""
    mpmath = pytest.importorskip("mpmath")
    from mpmath import libmp
    args = set()
    for motifs in (["A"], ["CAG", "GCN"], ["AC"]):
        args |= pyhmm.build(motifs).ln_args
    n_fixed = len(args)
    for length in range(2, 1363):
        seed = pyhmm.mismatch_seed(length)
        args.update(seed * float(length - i) for i in range(1, length))
    args.discard(0.0)
    assert {0.1, 0.5, 0.9, 0.03, 0.25, 0.75, 1.0, (1.00 - 0.90) / 2.00} <= args and n_fixed < 20 and len(args) > 500_000
    off = []
    for p in sorted(args):
        exact = libmp.to_float(libmp.mpf_log(libmp.from_float(p), 200, "n"), rnd="n")  # (mpmath.log without the context's overhead)
        got = math.log(p)
        if got != exact:
            assert _ulps(got, exact) <= 1, (p, got, exact)
            off.append(p)
    assert float(mpmath.mpf(libmp.mpf_log(libmp.from_float(0.5), 200, "n"))) == math.log(0.5)
    print("ln: %d distinct probabilities, %d not correctly rounded: %s" % (len(args), len(off), " ".join(p.hex() for p in off)))
