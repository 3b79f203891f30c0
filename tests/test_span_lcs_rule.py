"""The common-subsequence rule of flank location (trgt_amd/csrc/spans.hip, lcs_below in settled_sibling_kernel), restated in Python
(tools/sibling_census.py: lcs_bound, lcs_rule_drops) and held against the oracle's span location on hand-made cut reads.  No GPU.

A missed flank piece P beside a sibling whose text span [st, en) is known -- found exactly, or settled by a shortcut of the front seed
search -- can count only inside Adm = [en, n) (right piece) or [0, st) (left piece).  An alignment that stays inside Adm has
count_matches() <= LCS(P, T[Adm]), one that leaves it is discordant: with LCS < min_matches the read has no span.  The reads here put
into T[Adm] a repeat of 0 to 200 bases and a stump of the piece of 0 to 180 bases (dense around 165 .. 180, clean and with a few errors),
beside a sibling that is exact or settled by each kind of shortcut, on either side, under both penalty presets; some carry a degraded
copy of the missed piece on the wrong side of the sibling, some an N in the piece and in the text.  Checked: no dropped read has a span
in the oracle; a stump of min_matches clean bases is never dropped; the bit-parallel LCS is the plain quadratic one on every case.  The
share of reads the rule leaves to the pre-filter although the oracle rejects them is printed only: the rule is a certificate, not a
decision.
"""
import os
import sys

import numpy as np
import pytest

from test_span_sibling_rule import F, MIN_MATCHES, degrade, oracle_spans, rnd
from test_span_settled_sibling_rule import PRESETS, VARIANTS, sibling_variant

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from sibling_census import LCS_MAX_ADM, admissible, known_sibling_span, lcs_bound, lcs_rule_drops, seed_plan  # noqa: E402

SIBLINGS = ("exact",) + VARIANTS
STUMPS = (0, 60, 120, 150, 160, 165, 168, 170, 172, 173, 174, 175, 176, 178, 180)
REPEATS = (0, 30, 100, 200)
MOTIFS = (b"CAG", b"AAAG", b"GGCCCC", b"AT")
ACGT = np.frombuffer(b"ACGT", np.uint8)


def lcs_plain(a, b):
    """the quadratic recurrence, row by row: cur[j + 1] = prev[j] + 1 on a match, else max(prev[j + 1], cur[j]) -- the running maximum
    of a row is that second term (on a match prev[j] + 1 is the largest of the three); bytes outside ACGT match everything"""
    a, b = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    wild_b = ~np.isin(b, ACGT)
    prev = np.zeros(len(b) + 1, np.int64)
    for x in a:
        match = wild_b | (b == x) if x in ACGT else np.ones(len(b), bool)
        prev = np.concatenate(([0], np.maximum.accumulate(np.where(match, prev[:-1] + 1, prev[1:]))))
    return int(prev[-1])


def spoil(rng, seq, n_err):
    """a few substitutions and one-base gaps in the stump"""
    a = bytearray(seq)
    for i in sorted((int(v) for v in rng.choice(len(a), size=min(n_err, len(a)), replace=False)), reverse=True):
        kind = int(rng.integers(0, 3))
        if kind == 0:
            a[i] = b"ACGT"[(b"ACGTN".index(a[i]) + 1 + int(rng.integers(0, 3))) % 4]
        elif kind == 1:
            del a[i]
        else:
            a.insert(i, b"ACGT"[int(rng.integers(0, 4))])
    return bytes(a)


def cut_read(rng, lf, rf, side, sibling, rep_len, stump, n_err=0, adv=False, n_in_text=False):
    """a read cut behind `stump` bases of the missed piece `side` (1 right, 0 left): the sibling is there exactly or as the variant a
    shortcut settles, a repeat of rep_len bases lies between the two; adv: a degraded copy of the missed piece on the wrong side"""
    motif = MOTIFS[int(rng.integers(0, len(MOTIFS)))]
    tr = (motif * (rep_len // len(motif) + 1))[:rep_len]
    piece, other = (rf, lf) if side else (lf, rf)
    held = piece[:stump] if side else piece[F - stump:]
    if n_err and held:
        held = spoil(rng, held, n_err)
    if n_in_text and len(held) > 20:
        i = int(rng.integers(5, len(held) - 5))
        held = held[:i] + b"N" + held[i + 1:]
    sib = other
    while sibling != "exact" and sib == other:
        try:
            sib = sibling_variant(rng, other, sibling)
        except ValueError:  # (the position drawn was the piece's N: draw again)
            pass
    copy = degrade(rng, piece.replace(b"N", b"A"), float(rng.uniform(0.80, 0.95))) if adv else b""
    if side:
        return rnd(rng, int(rng.integers(20, 80))) + copy + rnd(rng, int(rng.integers(5, 30))) + sib + tr + held
    return held + tr + sib + rnd(rng, int(rng.integers(5, 30))) + copy + rnd(rng, int(rng.integers(20, 80)))


def make_locus_reads(rng, lf, rf, l):
    """every (side, sibling kind, stump) once per locus; repeat length, errors, the copy beyond the sibling and the N in the text rotate
    with the locus, so that the loci together hold every combination"""
    reads, meta = [], []  # meta: (side, sibling, rep_len, stump, n_err, adv, n_in_text)
    i = l
    for side in (0, 1):
        for sibling in SIBLINGS:
            for stump in STUMPS:
                i += 1
                m = (side, sibling, REPEATS[i % 4], stump, (0, 0, 3, 6)[(i // 4) % 4], (i // 16) % 3 == 2, (i // 5) % 4 == 3)
                reads.append(cut_read(rng, lf, rf, *m))
                meta.append(m)
    return reads, meta


def rule_drops(read, pieces, plan):
    """the rule over a read: some piece the exact scan missed, the other one's span known (exact, or settled under this preset's
    shortcuts), and no common subsequence of min_matches bases beside it"""
    for side in (0, 1):
        if read.find(pieces[side]) >= 0:
            continue
        span, _ = known_sibling_span(read, pieces, side, plan)
        if span is not None and lcs_rule_drops(read, pieces[side], side, span, MIN_MATCHES):
            return True
    return False


N_LOCI = 12  # 12 x 210 reads, the presets in turn; loci 4 and 5 with an N in both pieces


@pytest.fixture(scope="module")
def census():
    rng = np.random.default_rng(20261020)
    rows = []  # (dropped, span is None, scoring, read, pieces) + meta
    for l in range(N_LOCI):
        lf, rf = rnd(rng, F), rnd(rng, F)
        if l in (4, 5):  # an N in either piece, inside the part a cut read holds
            lf, rf = lf[:F - 40] + b"N" + lf[F - 39:], rf[:40] + b"N" + rf[41:]
        reads, meta = make_locus_reads(rng, lf, rf, l)
        scoring = PRESETS[l % 2]
        plan = seed_plan(F, *scoring)
        ss, _ = oracle_spans(lf, rf, reads, scoring)
        for read, m, s in zip(reads, meta, ss):
            rows.append((rule_drops(read, (lf, rf), plan), int(s) < 0, scoring, read, (lf, rf)) + m)
    return rows


def test_dropped_reads_have_no_span(census):
    assert len(census) == N_LOCI * 2 * len(SIBLINGS) * len(STUMPS)
    bad = [r[:3] + r[5:] for r in census if r[0] and not r[1]]
    assert not bad, bad[:5]
    left = sum(1 for r in census if r[1] and not r[0])
    print("dropped %d of %d cut reads; %d (%.1f %%) without a span in the oracle are left to the pre-filter" % (
        sum(1 for r in census if r[0]), len(census), left, 100.0 * left / len(census)))


def test_rule_is_not_vacuous(census):
    """it fires on either side, under both presets, beside an exact sibling and (under 2,5,1, where shortcuts exist) beside every kind of
    settled one, on reads with the copy beyond the sibling and on reads with an N; and only where min_matches <= |Adm| <= the cap"""
    for scoring in PRESETS:
        for side in (0, 1):
            kinds = SIBLINGS if scoring == (2, 5, 1) else ("exact",)
            for sibling in kinds:
                assert any(r[0] for r in census if r[2] == scoring and r[5] == side and r[6] == sibling), (scoring, side, sibling)
    assert any(r[0] and r[10] for r in census) and any(r[0] and r[11] for r in census)
    assert any(r[0] and b"N" in r[4][0] for r in census)
    plan = seed_plan(F, 2, 5, 1)
    for r in census:
        if r[0] and r[2] == (2, 5, 1):
            rooms = [len(admissible(r[3], side, known_sibling_span(r[3], r[4], side, plan)[0])) for side in (0, 1)
                     if r[3].find(r[4][side]) < 0 and known_sibling_span(r[3], r[4], side, plan)[0] is not None]
            assert any(MIN_MATCHES <= room <= LCS_MAX_ADM for room in rooms), r[5:]


def test_clean_stump_of_min_matches_is_kept(census):
    """a read that still holds min_matches clean bases of the missed piece has a common subsequence of that length: never dropped, and
    the oracle does find spans among them (the bound could not ask for more)"""
    clean = [r for r in census if r[8] >= MIN_MATCHES and r[9] == 0 and not r[11]]
    assert len(clean) >= 100
    assert not any(r[0] for r in clean)
    assert any(not r[1] for r in clean)


def test_bit_parallel_lcs_is_the_plain_one(census):
    """on T[Adm] of every read, either side, capped or not -- and on a few short and odd lengths where the top word of V is partial"""
    n = 0
    for r in census:
        read, pieces, side = r[3], r[4], r[5]
        adm = read[len(read) - (r[7] + r[8]) - 8:] if side else read[:r[7] + r[8] + 8]  # (a few bases of the sibling with it)
        assert lcs_bound(pieces[side], adm) == lcs_plain(pieces[side], adm), r[5:]
        n += 1
    rng = np.random.default_rng(3)
    for flen in (1, 31, 32, 33, 40, 64, 255, 256):
        for tlen in (0, 1, 15, 16, 17, 175, 352):
            a, b = rnd(rng, flen), rnd(rng, tlen)
            if flen > 8 and tlen > 8:
                a, b = a[:3] + b"N" + a[4:], b[:6] + b"n" + b[7:]
            assert lcs_bound(a, b) == lcs_plain(a, b), (flen, tlen)
    assert n == len(census)


def test_cap_and_threshold_edges():
    """|Adm| below min_matches and above the cap are not the rule's (the scan's rule owns the first, the pre-filter the second)"""
    rng = np.random.default_rng(5)
    lf, rf = rnd(rng, F), rnd(rng, F)
    for room, expect in ((MIN_MATCHES - 1, False), (MIN_MATCHES, True), (LCS_MAX_ADM, True), (LCS_MAX_ADM + 1, False)):
        read = rnd(rng, 40) + lf + (b"AT" * room)[:room]  # (a repeat: two random sequences of these lengths can share 175 bases)
        assert lcs_rule_drops(read, rf, 1, (40, 40 + F), MIN_MATCHES) == expect, room
        read = (b"AT" * room)[:room] + rf + rnd(rng, 40)
        assert lcs_rule_drops(read, lf, 0, (room, room + F), MIN_MATCHES) == expect, room
