"""The settled-sibling rule of flank location (trgt_amd/csrc/spans.hip, settled_sibling_kernel), restated in Python next to rule_drops of
test_span_sibling_rule.py and held against the oracle's span location on hand-made reads.  No GPU.

The scan's rule (ScanArgs::min_matches) looks at a sibling that was found EXACTLY.  This one looks at a sibling the exact scan missed but
the front seed search settled by a shortcut -- one or two substitutions on one diagonal, one inserted or one deleted base -- whose text
span [st, en) is therefore known without an alignment.  A missed right piece can count only inside Adm = [en, n), a missed left piece
only inside Adm = [0, st): with |Adm| < min_matches the read has no span whatever the missed piece's alignment is.  Checked here: every
read the rule drops has span None in the oracle, under both penalty presets -- siblings with a substitution in the first, the last or an
inner base, with two, with one inserted base (text span F + 1: the edge moves by one) and with one deleted base, |Adm| on 173 .. 177 on
either side, and a copy of the missed piece at 80-95 % identity inside the inadmissible part of the read.  The shortcut conditions
themselves are the host restatement of tools/sibling_census.py (front_search), the one the device's debug count is held against.
"""
import os
import sys

import numpy as np
import pytest

from test_span_sibling_rule import F, MIN_MATCHES, degrade, oracle_spans, rnd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from sibling_census import front_search, seed_plan, settled_rule_drops  # noqa: E402

PRESETS = ((2, 5, 1), (1, 0, 1))
PLAN = seed_plan(F, 2, 5, 1)  # the preset whose shortcuts exist
VARIANTS = ("sub_first", "sub_last", "sub_inner", "sub_two", "ins", "del")
ADMS = tuple(range(MIN_MATCHES - 2, MIN_MATCHES + 3))  # 173 .. 177


def _other(base):
    return b"ACGT"[(b"ACGT".index(base) + 1) % 4]


def sibling_variant(rng, piece, variant):
    """the flank piece as the read holds it: what the shortcuts settle (and the exact scan misses)"""
    a = bytearray(piece)
    if variant == "ins":
        i = int(rng.integers(40, 200))
        return bytes(a[:i]) + bytes([_other(a[i])]) + bytes(a[i:])
    if variant == "del":
        i = int(rng.integers(40, 200))
        return bytes(a[:i]) + bytes(a[i + 1:])
    where = dict(sub_first=[0], sub_last=[F - 1], sub_inner=[int(rng.integers(1, F - 1))], sub_two=[int(rng.integers(1, 120)), int(rng.integers(130, F - 1))])[variant]
    for i in where:
        a[i] = _other(a[i])
    return bytes(a)


def cut_read(rng, lf, rf, side, variant, adm, tr_len, adv):
    """a read cut `adm` bases beyond the sibling: the missed piece is `side` (1 right, 0 left), the other one is there as `variant`;
    adv: a degraded copy of the missed piece on the wrong side of the sibling"""
    tr = rnd(rng, tr_len)
    k = adm - tr_len  # bases of the missed piece the read still holds
    copy = degrade(rng, rf if side else lf, float(rng.uniform(0.80, 0.95))) if adv else b""
    if side:
        return rnd(rng, int(rng.integers(20, 80))) + copy + rnd(rng, int(rng.integers(5, 30))) + sibling_variant(rng, lf, variant) + tr + rf[:k]
    return lf[F - k:] + tr + sibling_variant(rng, rf, variant) + rnd(rng, int(rng.integers(5, 30))) + copy + rnd(rng, int(rng.integers(20, 80)))


def make_locus_reads(rng, lf, rf):
    reads, meta = [], []  # meta: (side, variant, adm, kind)
    for side in (0, 1):
        for variant in VARIANTS:
            for adm in ADMS:
                for kind in ("bare", "tr", "adv"):  # bare: no repeat between the flanks, the most matches the region can give
                    tr_len = 0 if kind == "bare" else int(rng.integers(1, 40))
                    reads.append(cut_read(rng, lf, rf, side, variant, adm, tr_len, kind == "adv"))
                    meta.append((side, variant, adm, kind))
    return reads, meta


def rule_drops(read, lf, rf, plan, min_matches):
    """the settled-sibling rule over a read: some piece the exact scan missed, its sibling missed too but settled by a shortcut, and fewer
    than min_matches bases of the read left beside that sibling's text span"""
    if read.find(lf) >= 0 or read.find(rf) >= 0:
        return False  # (an exactly found piece: the scan's rule, test_span_sibling_rule.py)
    return any(settled_rule_drops(read, (lf, rf), side, plan, min_matches) for side in (0, 1))


N_LOCI = 16  # 16 x 180 reads, the presets in turn


@pytest.fixture(scope="module")
def census():
    rng = np.random.default_rng(20261019)
    rows = []  # (dropped, span is None, side, variant, adm, kind, scoring)
    for l in range(N_LOCI):
        lf, rf = rnd(rng, F), rnd(rng, F)
        reads, meta = make_locus_reads(rng, lf, rf)
        scoring = PRESETS[l % 2]
        ss, _ = oracle_spans(lf, rf, reads, scoring)
        for read, m, s in zip(reads, meta, ss):
            rows.append((rule_drops(read, lf, rf, PLAN, MIN_MATCHES), int(s) < 0) + m + (scoring,))
    return rows


def test_dropped_reads_have_no_span(census):
    assert len(census) == N_LOCI * 180
    bad = [r for r in census if r[0] and not r[1]]
    assert not bad, bad[:5]


def test_rule_is_not_vacuous(census):
    """the shortcuts settle the hand-made siblings, so the rule drops exactly the reads with |Adm| < min_matches -- every variant, either
    side, both presets' oracles, with and without the copy beyond the sibling"""
    dropped = sum(1 for r in census if r[0])
    print("dropped %d of %d cut reads" % (dropped, len(census)))
    for scoring in PRESETS:
        for side in (0, 1):
            for variant in VARIANTS:
                for adm in ADMS:
                    hit = [r for r in census if r[2:5] == (side, variant, adm) and r[6] == scoring]
                    assert len(hit) >= 3 and {r[5] for r in hit} == {"bare", "tr", "adv"}
                    assert all(r[0] == (adm < MIN_MATCHES) for r in hit), (scoring, side, variant, adm, hit)


def test_bound_is_tight(census):
    """at |Adm| = min_matches the oracle does find spans, for every sibling variant on either side: the rule could not ask for less"""
    for scoring in PRESETS:
        for side in (0, 1):
            for variant in VARIANTS:
                assert any(not r[1] for r in census if r[2:5] == (side, variant, MIN_MATCHES) and r[5] == "bare" and r[6] == scoring), (scoring, side, variant)


def test_inserted_base_moves_the_edge():
    """the sibling with one inserted base spans F + 1 bases of the read: the region is counted from that edge, not from start + F"""
    rng = np.random.default_rng(7)
    lf, rf = rnd(rng, F), rnd(rng, F)
    for side in (0, 1):
        read = cut_read(rng, lf, rf, side, "ins", MIN_MATCHES, 0, False)
        sib = front_search(read, rf if side == 0 else lf, PLAN)
        assert sib[0] == "settled" and sib[2] - sib[1] == F + 1
        assert (len(read) - sib[2] if side else sib[1]) == MIN_MATCHES
        assert not rule_drops(read, lf, rf, PLAN, MIN_MATCHES)
        # one base less of the read beyond the sibling and the rule drops it
        shorter = read[:-1] if side else read[1:]
        assert rule_drops(shorter, lf, rf, PLAN, MIN_MATCHES)


def test_rule_is_inert_without_shortcuts():
    """preset 1,0,1 has no shortcut (hamming_max = 0): nothing is settled, nothing dropped"""
    plan = seed_plan(F, 1, 0, 1)
    assert plan["hamming_max"] == 0 and not plan["indel_ok"]
    rng = np.random.default_rng(8)
    lf, rf = rnd(rng, F), rnd(rng, F)
    reads, _ = make_locus_reads(rng, lf, rf)
    assert not any(rule_drops(r, lf, rf, plan, MIN_MATCHES) for r in reads[::7])
