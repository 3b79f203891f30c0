"""The pair lists of the independent aligner checks (tests/test_wfa_independent.py holds the CPU oracle to tests/pywfa.py on them,
tests/test_wfa_independent_gpu.py the kernels), the configurations each list runs under, their pywfa answers -- computed once per
process and shared, never changed -- and the one comparison both files use.  Seeded; reads no file.

A list is made for a path of the launcher (trgt_amd/csrc/wfa.hip: wfa_launch; wfa_lean.hip: wfa_lean_launch, set_window); the
numbers in the docstrings are the launcher's:
  * a register-resident tier of 64 NS diagonals takes a pair only when | |t| - |p| | <= 64 NS - 9: 55, 119 and 247 for the tiers of
    64, 128 and 256 diagonals; what the last tier does not take goes to the generic kernel
  * the lean kernels keep at most RLE_CAP = 80 CIGAR runs and a split stack of STACK = 12 entries
  * end to end a batch runs one wave per alignment (64 threads), ends-free four; exact gap-affine batches that are not BiWFA run on the
    dedicated kernel while 26 (|p| + |t|) bytes or so fit its LDS ((2,5,1): sums up to about 3 700)

Every pair whose exact answer is asserted lies within EXACT_BUDGET cells; within PLAIN_BUDGET the answer comes from pywfa.optimum
(the definition), above it from pywfa.optimum_rows (the test file holds the two to each other).  Lists may hold larger pairs for the
checks that need no optimum (validity, cost = score, span); share_exact() says how many of a list are inside."""
import functools
from collections import namedtuple

import numpy as np

import pywfa
from helpers import mutate, rand_dna, repeat_allele

PLAIN_BUDGET = 3_000       # cells up to which the plain-Python form answers
EXACT_BUDGET = 250 * 900   # cells up to which an exact answer is asserted at all
AFFINE7 = [(1, 0, 1), (1, 3, 1), (3, 2, 2), (4, 6, 2), (2, 5, 1), (5, 1, 3), (7, 9, 1)]  # test_dedicated_affine_kernel_penalties_and_shapes
# two-piece sets: the library's example, and one whose second piece is the cheaper one exactly for gaps of ten bases and more
# (2 + 3 n > 11 + 2 n  <=>  n >= 10)
PENALTY_SETS = ([("indel", ()), ("edit", ()), ("linear", (6, 2)), ("affine", (6, 4, 2))] + [("affine", p) for p in AFFINE7] +
                [("affine2p", (8, 4, 2, 24, 1)), ("affine2p", (4, 2, 3, 11, 2))])
E2E = ("end2end", (0, 0, 0, 0))
TEXT_FREE = ("endsfree", (0, 0, -1, -1))
FIXED_SPANS = [("endsfree", (3, 5, 40, 7)), ("endsfree", (2, 0, 0, 9)), ("endsfree", (0, 4, 11, 0))]
SPANS = [E2E, TEXT_FREE] + FIXED_SPANS

Config = namedtuple("Config", "metric pen span free heuristic memory scope min_length min_score want_ops")


def config(metric, pen=(), span=E2E, heuristic="none", memory="high", scope="alignment", min_length=100, min_score=250, want_ops=True):
    return Config(metric, tuple(pen), span[0], tuple(span[1]), heuristic, memory, scope, min_length, min_score, want_ops)


def _sub(rng, seq, positions):
    b = bytearray(seq)
    for p in positions:
        b[p] = int(rng.choice([c for c in b"ACGT" if c != b[p]]))
    return bytes(b)


def _pad(rng, pairs):
    """fixed free-end lengths must not exceed the sequences (the reference's library refuses such a call)"""
    return [(a + rand_dna(rng, 6) if len(a) < 6 else a, b + rand_dna(rng, 41) if len(b) < 41 else b) for a, b in pairs]


# ------------------------------------------------------------------------------------------------------------------ the lists
def _shapes(rng):
    """every metric and span: random pairs of 8 to 70 bases with substitutions and gaps, lengths 0 and 1, a pattern longer than its text,
    identical sequences, nothing in common, a homopolymer run of 130 against 129 + 1 + 40 (many windows per extension), and gaps of
    9, 10 and 11 bases (either side of where the second piece of a two-piece gap takes over)"""
    pairs = []
    for i in range(14):
        a = rand_dna(rng, int(rng.integers(8, 71)))
        pairs.append((a, rand_dna(rng, int(rng.integers(0, 12))) + mutate(rng, a, 0.06, 0.03, 0.03) + rand_dna(rng, int(rng.integers(0, 12)))))
    pairs += [(b"", b""), (b"", b"A"), (b"A", b""), (b"A", b"A"), (b"A", b"C"), (b"", rand_dna(rng, 9)), (rand_dna(rng, 9), b""), (b"ACGTACGTAC", b"T")]
    for i in range(3):
        b = rand_dna(rng, int(rng.integers(10, 40)))
        pairs.append((rand_dna(rng, 9) + mutate(rng, b, 0.05, 0.02, 0.02) + rand_dna(rng, 14), b))
    a = rand_dna(rng, 30)
    pairs += [(a, a), (rand_dna(rng, 1) * 70,) * 2, (b"A" * 20, b"C" * 25), (b"AC" * 10, b"GT" * 12)]
    pairs.append((b"G" * 130, b"G" * 129 + b"C" + b"G" * 40))
    for g in (9, 10, 11):
        a = rand_dna(rng, 60)
        pairs += [(a, a[:30] + rand_dna(rng, g) + a[30:]), (a[:25] + rand_dna(rng, g) + a[25:], a), (_sub(rng, a, [7, 50]), a[:20] + a[20 + g:])]
    return pairs


def _shapes_padded(rng):
    """_shapes for the spans with fixed free-end lengths: every pattern at least 6, every text at least 41 bases"""
    return _pad(rng, _shapes(rng))


def _free_limit(rng):
    """free ends at their limit, for the spans (3,5,40,7), (2,0,0,9), (0,4,11,0) and the fully free text: the best placement needs exactly
    pbf / pef / tbf / tef free bases, and one more than that (the surplus has to be paid as a gap); a piece that hangs over either end
    of the text by 1, 5 and 12 bases"""
    pairs = []
    for _ in range(2):
        core = rand_dna(rng, 60)
        for n in (2, 3, 4):           # pattern begin free 2 / 3
            pairs.append((rand_dna(rng, n) + core, core + rand_dna(rng, 7)))
        for n in (4, 5, 6):           # pattern end free 4 / 5
            pairs.append((core + rand_dna(rng, n), rand_dna(rng, 11) + core))
        for n in (11, 12, 40, 41):    # text begin free 11 / 40
            pairs.append((core, rand_dna(rng, n) + core))
        for n in (7, 8, 9, 10):       # text end free 7 / 9
            pairs.append((core, core + rand_dna(rng, n)))
        for n in (1, 5, 12):
            pairs += [(core, core[n:] + rand_dna(rng, 30)), (core, rand_dna(rng, 30) + core[:-n])]
    return _pad(rng, pairs)


def _insert(rng, a, d):
    """a against a with |d| bases inserted in the middle (d < 0: the other way round) and one substitution: |t| - |p| = d.  (d = 0: three
    substitutions -- after a lone one a front of the BiWFA breakpoint search reaches the far end before the two overlap, and whether
    cigar.score is set then is the library's choice: DESIGN.md, the unpinned list)"""
    b = _sub(rng, a, [len(a) // 4] if d else [len(a) // 4, len(a) // 2, len(a) - 9])
    b = b[:len(a) // 2] + rand_dna(rng, abs(d)) + b[len(a) // 2:]
    return (a, b) if d >= 0 else (b, a)


LEAN_D1 = (0, 20, 40, 50, 54, 55, -55, 56, -56, 57, 60, 63, 64, 65, 70)
LEAN_D2 = (118, 119, -119, 120, -120, 121)
LEAN_D3 = (246, 247, -247, 248, -248, 249, 250, 255, 256, 257)


def _lean_lengths(rng):
    """register-resident BiWFA: lengths 99 / 100 / 101 on either side (bialign_min_length = 100: the longer sequence decides whether the
    recursion begins with a split), with a few substitutions and the gap the two lengths ask for"""
    pairs = []
    for pl in (99, 100, 101):
        for tl in (99, 100, 101):
            for _ in range(2):
                a = rand_dna(rng, pl)
                b = _sub(rng, a, [10, 77])
                b = b[:40] + rand_dna(rng, tl - pl) + b[40:] if tl >= pl else b[:40] + b[40 + pl - tl:]
                assert len(b) == tl
                pairs.append((a, b))
    return pairs


def _lean_tier1(rng):
    """|t| - |p| from 0 to 70 around the first tier's limit of 55 (both signs at the limit): 140 bases with one substitution and one gap"""
    return [_insert(rng, rand_dna(rng, 140), d) for d in LEAN_D1]


def _lean_tier2(rng):
    """... around 119, the limit of the optional tier of 128 diagonals"""
    return [_insert(rng, rand_dna(rng, 140), d) for d in LEAN_D2]


def _lean_tier3(rng):
    """... around 247, the limit of the tier of 256 diagonals: one past it the generic kernel redoes the pair"""
    return [_insert(rng, rand_dna(rng, 140), d) for d in LEAN_D3]


def _lean_runs(rng):
    """alignments of more than RLE_CAP = 80 CIGAR runs: a substitution on every third or fourth base of 130 to 260"""
    pairs = []
    for n, step in ((130, 3), (200, 3), (260, 4), (260, 3)):
        a = rand_dna(rng, n)
        pairs.append((a, _sub(rng, a, range(1, n, step))))
    a = rand_dna(rng, 240)
    pairs.append((a, _sub(rng, a, range(2, 240, 24))))  # (twenty-one runs: stays)
    return pairs


def _lean_deep(rng):
    """a split recursion deeper than the lean kernel's stack: bialign_min_score = 2 and bialign_min_length = 0 (the configuration this list
    runs under) split down to single differences, and 70 to 130 differences spread evenly make the splits even"""
    pairs = []
    for n, step in ((420, 6), (470, 4), (390, 3)):
        a = rand_dna(rng, n)
        pairs.append((a, _sub(rng, a, range(2, n, step))))
    return pairs


def _biwfa_alleles(rng):
    """the consensus configuration's own inputs (repeat alleles with stutter), as the oracle-free test of tests/test_wfa_gpu.py had them:
    BiWFA gap-affine (2,5,1) with and without the heuristic, with and without expanded operations"""
    pairs = []
    for i in range(60):
        motif = [rand_dna(rng, int(rng.integers(2, 7)))]
        backbone = repeat_allele(rng, motif, int(rng.integers(10, 330)), err=0.0)
        read = mutate(rng, backbone, 0.02, 0.015, 0.015)
        if i % 4 == 0:
            k = len(motif[0]) * int(rng.integers(1, 5))
            read = read[:len(read) // 3] + (motif[0] * 5)[:k] + read[len(read) // 3:] if i % 8 else read[k:]
        if backbone == read and len(read) > 100:
            read = _sub(rng, read, [len(read) // 2])  # (identical pairs beyond 100 bases: DESIGN.md, the unpinned list)
        pairs.append((backbone, read))
    return pairs


def _biwfa_high(rng):
    """BiWFA with a penalty above bialign_min_score = 250: unrelated and half-related sequences of 250 to 330 bases"""
    pairs = []
    for n in (250, 300, 330):
        a = rand_dna(rng, n)
        pairs += [(a, rand_dna(rng, n - 20)), (a, mutate(rng, a, 0.3, 0.1, 0.1))]
    return pairs


def _too_long_for_lds(rng):
    """the dedicated kernel sizes its LDS by the batch's longest pair: with one pair of 2 000 + 2 000 bases in it (beyond every exact
    budget: validity only) a gap-affine batch takes the generic kernel -- the short pairs with it"""
    a = rand_dna(rng, 2000)
    return _shapes(rng)[:14] + [(a, mutate(rng, a, 0.01, 0.005, 0.005))]


def _flank_shape(rng):
    """the 256-thread flank specialisation through trgt_wfa_batch: 250-base pieces in reads of up to 850 bases, noise from 0 to 30 %,
    (2,5,1), pattern global and text free"""
    pairs = []
    for i in range(12):
        f = rand_dna(rng, 250)
        pairs.append((f, rand_dna(rng, int(rng.integers(0, 300))) + noisy(rng, f, 0.3 * i / 11) + rand_dna(rng, int(rng.integers(0, 300)))))
    return pairs


def noisy(rng, seq, rate):
    """substitutions (half of the edits), insertions and deletions of one to three bases, `rate` edits per base"""
    out = bytearray(seq)
    for p in sorted((int(v) for v in rng.choice(len(seq), int(rng.binomial(len(seq), rate)), replace=False)), reverse=True):
        kind = int(rng.integers(0, 4))
        if kind < 2:
            out[p] = b"ACGT"[(b"ACGT".index(out[p]) + 1 + int(rng.integers(0, 3))) % 4]
        elif kind == 2:
            out[p:p] = rand_dna(rng, 1 if rng.random() < 0.8 else int(rng.integers(2, 4)))
        else:
            del out[p:p + (1 if rng.random() < 0.8 else int(rng.integers(2, 4)))]
    return bytes(out)


def _ties_periodic(rng):
    """tie list: periodic pieces (CAG n, AT n, with one base changed now and then) in periodic reads, and pieces that occur twice in
    their read -- more than one text position at which an optimal alignment can end"""
    pairs = []
    for i in range(60):
        unit = (b"CAG", b"AT")[i % 2]
        n = int(rng.integers(8, 16))
        piece = unit * n
        if i % 3:
            piece = _sub(rng, piece, [int(rng.integers(0, len(piece)))])
        pairs.append((piece, rand_dna(rng, int(rng.integers(0, 20))) + unit * (n + int(rng.integers(2, 12))) + rand_dna(rng, int(rng.integers(0, 20)))))
    for i in range(60):
        piece = rand_dna(rng, int(rng.integers(30, 50)))
        seen = noisy(rng, piece, 0.05 * (i % 3))
        pairs.append((piece, rand_dna(rng, int(rng.integers(0, 30))) + seen + rand_dna(rng, int(rng.integers(5, 30))) + seen + rand_dna(rng, int(rng.integers(0, 30)))))
    return pairs


def _ties_bracket(rng):
    """tie list: minimum-cost alignments that differ in their number of matches.  Under (2,5,1) an inserted base (6) costs what three
    substitutions do: one extra base k bases before the end of the piece's copy, chosen so that the shifted tail has exactly three
    unequal bases, leaves the choice between a gap with k matches behind it and three substitutions with k - 3; likewise at the start"""
    pairs = []
    while len(pairs) < 130:
        piece = rand_dna(rng, int(rng.integers(36, 56)))
        k = int(rng.integers(4, 9))
        at_end = len(pairs) % 2 == 0
        extra = rand_dna(rng, 1)
        mine = piece[-k:] if at_end else piece[:k]
        shifted = (extra + mine)[:k] if at_end else (mine + extra)[1:]
        if sum(x != y for x, y in zip(shifted, mine)) != 3:
            continue
        copy = piece[:-k] + extra + piece[-k:] if at_end else piece[:k] + extra + piece[k:]
        pairs.append((piece, rand_dna(rng, int(rng.integers(3, 25))) + copy + rand_dna(rng, int(rng.integers(3, 25)))))
    return pairs


_BUILDERS = dict(shapes=_shapes, shapes_padded=_shapes_padded, free_limit=_free_limit, lean_lengths=_lean_lengths, lean_tier1=_lean_tier1,
                 lean_tier2=_lean_tier2, lean_tier3=_lean_tier3, lean_runs=_lean_runs, lean_deep=_lean_deep, biwfa_alleles=_biwfa_alleles,
                 biwfa_high=_biwfa_high, too_long_for_lds=_too_long_for_lds, flank_shape=_flank_shape, ties_periodic=_ties_periodic,
                 ties_bracket=_ties_bracket)
LISTS = tuple(_BUILDERS)
TIE_LISTS = ("ties_periodic", "ties_bracket")
N_PAIRS = dict(shapes=39, shapes_padded=39, free_limit=40, lean_lengths=18, lean_tier1=15, lean_tier2=6, lean_tier3=10, lean_runs=5,
               lean_deep=3, biwfa_alleles=60, biwfa_high=6, too_long_for_lds=15, flank_shape=12, ties_periodic=120, ties_bracket=130)


@functools.lru_cache(maxsize=None)
def pairs(name):
    out = [(bytes(a), bytes(b)) for a, b in _BUILDERS[name](np.random.default_rng(20261019 + LISTS.index(name)))]
    assert len(out) == N_PAIRS[name], (name, len(out))
    return tuple(out)


def cells(pair):
    return (len(pair[0]) + 1) * (len(pair[1]) + 1)


def share_exact(name):
    p = pairs(name)
    return sum(cells(x) <= EXACT_BUDGET for x in p) / len(p)


@functools.lru_cache(maxsize=None)
def answers(name, metric, pen, span, free):
    """pywfa's least penalty of every pair of the list under this metric and span (None beyond the budget)"""
    out = []
    for a, b in pairs(name):
        c = cells((a, b))
        if c > EXACT_BUDGET:
            out.append(None)
        else:
            out.append((pywfa.optimum if c <= PLAIN_BUDGET else pywfa.optimum_rows)(a, b, metric, pen, span, *free))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tie_counts(name):
    """(pairs with more than one optimal end position, pairs whose bracket of match counts holds more than one value) of a tie list,
    flank configuration"""
    ends = wide = 0
    for piece, read in pairs(name):
        ends += pywfa.end_positions(piece, read)[1] > 1
        _, lo, hi = pywfa.match_bracket(piece, read)
        wide += hi > lo
    return ends, wide


# ------------------------------------------------------------------------------------------------- which list runs under what
def _metric_plan():
    plan = []
    for metric, pen in PENALTY_SETS:
        for span in SPANS:
            for name in (("shapes",) if span in (E2E, TEXT_FREE) else ("shapes_padded",)) + (("free_limit",) if span != E2E else ()):
                plan.append((name, config(metric, pen, span)))
    for metric, pen in PENALTY_SETS[:4] + [("affine", (2, 5, 1)), PENALTY_SETS[-2]]:
        plan.append(("shapes", config(metric, pen, heuristic="default")))                 # what wfadaptive drops is the library's: >= optimum
        plan.append(("shapes", config(metric, pen, scope="score")))
        plan.append(("shapes", config(metric, pen, scope="score", heuristic="default")))
    return plan


METRIC_PLAN = _metric_plan()
LEAN_LISTS = ("lean_lengths", "lean_tier1", "lean_tier2", "lean_tier3", "lean_runs", "biwfa_alleles", "biwfa_high", "shapes")


def lean_configs(want_ops=False):
    """the register-resident kernels' configurations: BiWFA, edit (alignment and score-only) and gap-affine (2,5,1), with the default
    heuristic and without, bialign_min_length 100 and 0"""
    out = []
    for heuristic in ("none", "default"):
        for min_length in (100, 0):
            out.append(config("affine", (2, 5, 1), heuristic=heuristic, memory="ultralow", min_length=min_length, want_ops=want_ops))
            out.append(config("edit", heuristic=heuristic, memory="ultralow", min_length=min_length, want_ops=want_ops))
        out.append(config("edit", heuristic=heuristic, memory="ultralow", scope="score", want_ops=want_ops))
    return out


DEEP_CONFIG = config("affine", (2, 5, 1), memory="ultralow", min_length=0, min_score=2, want_ops=False)


# ------------------------------------------------------------------------------------------------------------ the comparison
PROMISES_NOT_KEPT = []  # (who, list, pair, bialign_min_length, score, cost of the CIGAR, optimum): BiWFA under the heuristic, for the record


def verify(name, cfg, res, who):
    """Hold one batch result -- the arrays of trgt_wfa_batch / orc_wfa_batch: status, score, n_match, span4, cigar, cigar_off, cigar_len,
    ops, ops_len -- to pywfa.  Returns the number of jobs that completed."""
    ps = pairs(name)
    best = answers(name, cfg.metric, cfg.pen, cfg.span, cfg.free)
    exact = cfg.heuristic == "none"
    biwfa = cfg.memory == "ultralow"
    done = 0
    for j, (p, t) in enumerate(ps):
        st = int(res["status"][j])
        where = (who, name, j, cfg)
        if exact:
            assert st == 0, ("an exact alignment must complete", st) + where
        if st != 0:
            continue
        done += 1
        try:
            if cfg.scope == "score":
                assert best[j] is not None, where
                pywfa.check_score(res["score"][j], cfg.metric, exact, best[j])
                continue
            o, n = int(res["cigar_off"][j]), int(res["cigar_len"][j])
            r = dict(score=res["score"][j], n_match=res["n_match"][j], span4=res["span4"][j], cigar=res["cigar"][o:o + n],
                     ops=bytes(res["ops"][o:o + int(res["ops_len"][j])]) if cfg.want_ops else None)
            # the one documented exception: a BiWFA alignment that took the unidirectional base case never sets cigar.score (INT32_MIN)
            unset = biwfa and max(len(p), len(t)) <= 100 and int(r["score"]) == pywfa.I32_MIN
            # ... and one thing only WFA2-lib defines: under a heuristic BiWFA reports what its top-level breakpoint promised, which the
            # halves -- aligned again, pruned again -- need not keep (the unpinned list)
            cost = pywfa.check_alignment(p, t, cfg.metric, cfg.pen, cfg.span, cfg.free, r, exact, best[j], score_may_be_unset=unset,
                                         score_is_a_bound=biwfa and not exact)
            if biwfa and not exact and not unset and abs(int(r["score"])) != cost:
                PROMISES_NOT_KEPT.append((who, name, j, cfg.min_length, int(r["score"]), cost, best[j]))
        except pywfa.Rejected as e:
            raise AssertionError("%s: %s" % (where, e)) from e
    return done


# -------------------------------------------------------------------------------------------------------------- flank location
FlankCase = namedtuple("FlankCase", "piece damaged rate")


@functools.lru_cache(maxsize=None)
def flank_cases(flank_len):
    """damaged copies of a piece of flank_len bases, noise swept from 0 to 30 %: the acceptance threshold (0.7 flank_len matches) falls
    inside the sweep, so that pieces are found, missed and -- rarely -- undecided"""
    rng = np.random.default_rng(777 + flank_len)
    n = 48
    out = []
    for i in range(n):
        piece = rand_dna(rng, flank_len)
        rate = 0.30 * i / (n - 1)
        damaged = noisy(rng, piece, rate)
        if damaged == piece:
            damaged = _sub(rng, piece, [flank_len // 2])
        out.append(FlankCase(piece, damaged, rate))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def flank_loci(flank_len):
    """test_window_reg_gpu.py's construction: every damaged piece once as the LEFT piece of a read whose right piece is exact (the end of
    its alignment shows as the start of the repeat span) and once as the RIGHT piece of a read whose left piece is exact (its start
    shows as the end of the span); a second read per locus has both pieces exact.  Returns (loci, jobs): jobs[k] = (locus, side, case)"""
    rng = np.random.default_rng(778 + flank_len)
    loci, jobs = [], []
    tr = b"CAG" * 20
    for k, c in enumerate(flank_cases(flank_len)):
        other = rand_dna(rng, flank_len)
        head, tail = rand_dna(rng, int(rng.integers(40, 150))), rand_dna(rng, int(rng.integers(40, 150)))
        pad = 300 if k % 2 else 0  # (every other locus: the read under test is "too short to span the locus" -- 300 bases and more shorter than
                                   #  the longest -- which is the list the planner sends through the pre-filter and the banded back-trace)
        loci.append(dict(left_flank=c.piece, right_flank=other, tr=tr, motifs=[b"CAG"], ploidy=2,
                         reads=[head + c.damaged + tr + other + rand_dna(rng, 60), rand_dna(rng, 50 + pad) + c.piece + tr + other + rand_dna(rng, 50 + pad)]))
        jobs.append((len(loci) - 1, "left", k))
        loci.append(dict(left_flank=other, right_flank=c.piece, tr=tr, motifs=[b"CAG"], ploidy=2,
                         reads=[rand_dna(rng, 60) + other + tr + c.damaged + tail, rand_dna(rng, 50 + pad) + other + tr + c.piece + rand_dna(rng, 50 + pad)]))
        jobs.append((len(loci) - 1, "right", k))
    return tuple(loci), tuple(jobs)


@functools.lru_cache(maxsize=None)
def flank_answers(flank_len):
    """per job of flank_loci: (optimum, fewest, most matches of a minimum-cost alignment, first exact occurrence or -1) of the piece
    against the first read of its locus"""
    loci, jobs = flank_loci(flank_len)
    out = []
    for l, side, k in jobs:
        L = loci[l]
        piece = L["left_flank"] if side == "left" else L["right_flank"]
        read = L["reads"][0]
        out.append(pywfa.match_bracket(piece, read) + (read.find(piece),))
    return tuple(out)


def flank_verdict(flank_len, frac, bracket):
    """'found' / 'missed' / 'undecided' by the bracket of match counts against the threshold flank_len * frac (span_locater.rs:19)"""
    _, lo, hi, _ = bracket
    thr = flank_len * frac
    return "found" if lo >= thr else "missed" if hi < thr else "undecided"


def verify_flank(flank_len, frac, span_start, span_end, lf_hit, rf_hit, who):
    """Hold the per-read outputs of find_tr_spans over flank_loci(flank_len) -- two reads per locus, in order -- to pywfa.  Returns the
    numbers of (found, missed, undecided) jobs."""
    loci, jobs = flank_loci(flank_len)
    ans = flank_answers(flank_len)
    counts = dict(found=0, missed=0, undecided=0)
    for (l, side, k), a in zip(jobs, ans):
        L = loci[l]
        read, r = L["reads"][0], 2 * l
        piece, other = (L["left_flank"], L["right_flank"]) if side == "left" else (L["right_flank"], L["left_flank"])
        hit, other_hit = (lf_hit[r], rf_hit[r]) if side == "left" else (rf_hit[r], lf_hit[r])
        where = (who, flank_len, frac, l, side, a)
        # the second read of the locus: both pieces exact, at their first occurrences
        r2, read2 = r + 1, L["reads"][1]
        assert int(lf_hit[r2]) == 1 and int(rf_hit[r2]) == 1, where
        assert int(span_start[r2]) == read2.find(L["left_flank"]) + flank_len and int(span_end[r2]) == read2.find(L["right_flank"]), where
        assert int(other_hit) == 1, where                       # the exact sibling of the damaged piece
        verdict = flank_verdict(flank_len, frac, a)
        counts[verdict] += 1
        assert a[3] < 0 and int(hit) != 1, where                # hit 1 only where the piece occurs exactly (no damaged piece does)
        if verdict == "missed":
            assert int(hit) == 0, where
        if verdict == "found":
            assert int(hit) == 2, where
        if int(hit) == 0:
            assert int(span_start[r]) == -1 and int(span_end[r]) == -1, where
            continue
        o = read.find(other)
        if side == "left":   # the span begins where the damaged piece's alignment ends and ends where the exact piece begins
            te = int(span_start[r])
            assert te >= 0 and int(span_end[r]) == o, where
            assert pywfa.placement_is_optimal(piece, read, None, te), ("no optimal alignment ends here", te) + where
        else:
            ts = int(span_end[r])
            assert ts >= 0 and int(span_start[r]) == o + flank_len, where
            assert pywfa.placement_is_optimal(piece, read, ts, None), ("no optimal alignment begins here", ts) + where
    return counts["found"], counts["missed"], counts["undecided"]
