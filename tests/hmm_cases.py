"""The shape lists of the independent HMM checks (tests/test_hmm_independent.py holds the CPU oracle to tests/pyhmm.py on them,
tests/test_hmm_independent_gpu.py the kernels), their pyhmm answers -- computed once per process and shared, never changed -- and the
one comparison both files use.  Seeded; reads no file."""
import functools
import math

import numpy as np

import pyhmm
from helpers import rand_dna, repeat_allele

RFC1 = [b"AAAAG", b"AAAGG", b"AAGGG", b"AAGAG", b"AGAGG", b"AACGG", b"GGGAC", b"AAAGGG", b"AAAAGG", b"AAGAC"]
EXACT_BUDGET = 50_000  # states x columns up to which a job's path is held to the exact optimum
TIE_GROUPS = ("ties_duplicates", "ties_rotations", "ties_homopolymer", "ties_random", "ties_short")
GROUPS = ("ppl", "window", "multiwave", "large", "traceback") + TIE_GROUPS


def _exactly(rng, motifs, n, err):
    """an allele of motif runs with errors, of exactly n bases"""
    a = repeat_allele(rng, motifs, n + 24, err=err)[:n]
    assert len(a) == n
    return a


def _ppl(rng):
    """position-per-lane fill: positions + 1 = 4, 8, 9, 17, 32, 33, 64 and 65 (the last does not fit: state fill), a one-base set,
    twenty one-base blocks, three motifs, N in a motif; alleles of 0, 1, 2, 3, 20, 90 bases without and with errors, side by side"""
    sets = [[b"CAG"], [b"ACGTTGC"], [b"ACGTTGCA"], [b"ACGTACGTACGTTGCA"], [rand_dna(rng, 31)], [rand_dna(rng, 32)], [rand_dna(rng, 63)],
            [rand_dna(rng, 64)], [b"A"], [b"A", b"C", b"G", b"T"] * 5, [b"ACGTA", b"CCGGA", b"TTGAC"], [b"GCN"]]
    jobs = []
    for s, m in enumerate(sets):
        for err in (0.0, 0.05):
            for n in (0, 1, 2, 3, 20, 90):
                jobs.append((s, _exactly(rng, m, n, err)))
        jobs.append((s, rand_dna(rng, 120)))
    return sets, jobs


def _window(rng):  # [CAG] across the 256-column window of the position-per-lane fill
    return [[b"CAG"]], [(0, (b"CAG" * 100)[:n]) for n in (254, 255, 256, 257, 258)]


def _multiwave(rng):  # the ten-motif RFC1 set, 173 states: more than one wave
    return [RFC1], [(0, _exactly(rng, RFC1, n, 0.02)) for n in (5, 60, 333)]


def _large(rng):
    """458 states (past the locus path's 448 lanes), 1 025 (past the 1 024 states of the one-thread-per-state kernel), 4 094 (the
    longest single motif under the 4 096-state ceiling), ten 50-base motifs (1 517); states x columns <= 1.3 M per job"""
    sets = [[rand_dna(rng, 150)], [rand_dna(rng, 339)], [rand_dna(rng, 1362)], [rand_dna(rng, 50) for _ in range(10)]]
    jobs = []
    for s, m in enumerate(sets):
        for n in (60 + 17 * s, 300 - 13 * s):
            jobs.append((s, _exactly(rng, m, n, 0.03)))
    return sets, jobs


def _traceback(rng):  # around the staged trace-back (512 columns) and the chunk-map one (1 536)
    sets = [[b"CAG"], [b"A"], [b"GGCCTG", b"CCG"]]
    jobs = [(0, _exactly(rng, sets[0], n, 0.02)) for n in (511, 512, 513, 1535, 1536, 1600)]
    jobs += [(1, b"A" * 1536), (2, _exactly(rng, sets[2], 1540, 0.03)), (0, rand_dna(rng, 1600))]
    return sets, jobs


# -- lists made for exact ties: two predecessors of one cell with equal f64 sums
def _ties_duplicates(rng):  # the same motif twice in a set: whole blocks score alike, the run end picks the first
    sets = [[b"A", b"C", b"G", b"T"] * 5, [b"CAG", b"CAG"], [b"AC", b"AC", b"GCN", b"GCN"]]
    jobs = []
    for s, m in enumerate(sets):
        jobs += [(s, repeat_allele(rng, m, n, err=e)) for n, e in ((12, 0.0), (40, 0.0), (40, 0.05), (90, 0.05))]
        jobs.append((s, rand_dna(rng, 60)))
    jobs += [(0, b"ACGT" * 10), (0, b"AAAACCCCGGGGTTTT"), (1, b"CAG" * 20), (1, b"CAGCACAGCAGGCAG")]
    return sets, jobs


def _ties_rotations(rng):  # motifs that are rotations of each other
    sets = [[b"AC", b"CA"], [b"CAG", b"AGC", b"GCA"], [b"AAG", b"AGA"]]
    jobs = []
    for s, m in enumerate(sets):
        unit = m[0]
        for n in (1, 2, 5, 9, 30, 61):
            jobs.append((s, (unit * 40)[:n]))
            jobs.append((s, (unit * 40)[1:1 + n]))
        jobs += [(s, repeat_allele(rng, m, 80, err=0.05)), (s, rand_dna(rng, 50))]
    return sets, jobs


def _ties_homopolymer(rng):  # one-base motifs: no deletion states, insertion and next copy compete on every column
    sets = [[b"A"], [b"A", b"T"], [b"N"]]
    jobs = []
    for s in range(len(sets)):
        jobs += [(s, b"A" * n) for n in (1, 2, 3, 17, 64, 130)]
        jobs += [(s, b"C" * 9), (s, b"A" * 20 + b"C" + b"A" * 20), (s, b"AT" * 15), (s, b"A" * 7 + b"TTT" + b"A" * 7)]
    return sets, jobs


def _ties_random(rng):  # random DNA: the skip state and the insertion states emit 0.25 alike
    sets = [[b"CAG"], [b"AAGGG", b"AAAAG"], [b"A"], [b"GCN"], [rand_dna(rng, 16)], RFC1]
    jobs = []
    for s in range(len(sets)):
        jobs += [(s, rand_dna(rng, n)) for n in (4, 33, 120, 121, 200)]
    return sets, jobs


def _ties_short(rng):  # alleles shorter than the motif
    sets = [[b"ACGTTGCA"], [b"ACGTACGTACGTTGCA"], [rand_dna(rng, 31)], [b"CAG", rand_dna(rng, 12)], [b"AAAAAAAC"]]
    jobs = []
    for s, m in enumerate(sets):
        long = m[-1]
        for n in sorted({1, 2, 3, len(long) // 2, len(long) - 2, len(long) - 1}):
            jobs += [(s, long[:n]), (s, long[-n:]), (s, long[1:1 + n])]
    return sets, jobs


@functools.lru_cache(maxsize=None)
def group(name):
    """-> (motif sets, jobs) of one list; a job is (set index, allele)"""
    rng = np.random.default_rng([20261017, GROUPS.index(name)])
    sets, jobs = globals()["_" + name](rng)
    return tuple(tuple(s) for s in sets), tuple(jobs)


@functools.lru_cache(maxsize=None)
def reference(name):
    """pyhmm's answer per job of a list (pyhmm.annotate, f64), plus `optimum`: the exact optimum S* over the model's f64 tables for jobs
    within EXACT_BUDGET, else None.  Computed once; callers must not change it."""
    sets, jobs = group(name)
    models = [pyhmm.build(pyhmm.clean_motifs(s)) for s in sets]
    out = []
    for s, allele in jobs:
        r = pyhmm.annotate(models[s], len(sets[s]), allele)
        r["model"] = models[s]
        r["optimum"] = None
        if r["seq"] and models[s].n * (len(r["seq"]) + 2) <= EXACT_BUDGET:
            r["optimum"] = pyhmm.label(models[s], r["seq"], "exact").score
        out.append(r)
    return tuple(out)


def path_bound(n_path, optimum):
    """S* - exact(path) may reach 8 * len(path) * 2^-53 * |S*| and no more: a path of T states costs at most 2 T f64 additions, each
    of relative error 2^-53 on partial sums no larger than |S*|; the f64 winner and the exact winner are each mis-scored by at most that
    much; the factor 8 is twice the sum of the two.  (Derived, not measured: the gap seen so far is exactly 0.)"""
    return 8 * n_path * abs(optimum) / (1 << 53)


def check_optimal(ref, path, tag):
    """`path` (someone's own: the oracle's, the GPU's) is a valid walk and within path_bound of the exact optimum; -> the gap"""
    gap = ref["optimum"] - pyhmm.exact_path_score(ref["model"], ref["seq"], path)
    assert 0 <= gap <= path_bound(len(path), ref["optimum"]), (tag, float(gap), len(path), float(ref["optimum"]))
    return gap


def check_batch(batch, out, refs, tag, optimal=True):
    """every field the reference defines, of every job of a packed batch's output (the layout of trgt_amd.hmm.hmm_batch, which
    oracle.hmm_batch shares), against pyhmm: state path, spans, n_spans, counts, edit and max distance, purity as uint64 bits; then
    the exact-optimality bound on the output's OWN path.  -> number of jobs held to the bound"""
    n_opt = 0
    for j, r in enumerate(refs):
        po, pl = int(batch["path_off"][j]), int(out["path_len"][j])
        path = out["path"][po:po + pl].tolist()
        assert path == r["path"], (tag, j, "path")
        so, ns = int(batch["span_off"][j]), int(out["n_spans"][j])
        assert ns == len(r["spans"]), (tag, j, "n_spans")
        assert out["spans"][3 * so:3 * (so + ns)].reshape(-1, 3).tolist() == [list(s) for s in r["spans"]], (tag, j, "spans")
        co = int(batch["count_off"][j])
        assert out["counts"][co:co + len(r["counts"])].tolist() == r["counts"], (tag, j, "counts")
        if r["seq"]:  # (an empty allele has no events: purity.rs:7-9 answers NaN before any distance exists)
            assert (int(out["edit"][j]), int(out["maxd"][j])) == (r["edit"], r["maxd"]), (tag, j, "edit / max distance")
        else:
            assert math.isnan(r["purity"])
        assert int(out["purity"][j:j + 1].view(np.uint64)[0]) == int(np.array([r["purity"]], np.float64).view(np.uint64)[0]), (tag, j, "purity bits")
        if optimal and r["optimum"] is not None:
            check_optimal(r, path, (tag, j))
            n_opt += 1
    return n_opt
