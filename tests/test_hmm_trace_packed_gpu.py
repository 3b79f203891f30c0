"""hmm_trace_ppl_kernel<G> (trgt_amd/csrc/hmm_trace_ppl.hpp): the trace-back of launch class 0 -- motif sets of at most 32 states, whose
alleles the position-per-lane fill wrote in packed rows of G = 8 / 16 bytes -- with 64 / G alleles per wave.

Every output array of trgt_hmm_batch (path, path_len, spans, n_spans, counts, purity as uint64 bits, edit, maxd) and of a small
trgt_locus_batch is held, for exact equality, to the CPU oracle and to hmm_viterbi_kernel<32, .> through the developer switch
TRGT_HMM_TRACE_WIDE=1 (skipped where the developer library is not built).  The shapes are the smallest at which the kernel can go
wrong: every motif length a group of 8 lanes holds and the one 32-state set of 16 lanes, alleles from no base to 40 copies with each
kind of edit, 1 / 7 / 8 / 9 / 17 jobs (a partial last wave, waves whose groups hold different sets and lengths), an allele of no bases
in a middle group of a full wave, alleles across the 64-column staging chunk and the 256-column mark, more motif visits than LDS keeps
(32) and than one read-back chunk adds (44 / 88), and a long allele that the kernel must hand to hmm_traceback_long_kernel.

Motif sets of two motifs have 33 states and more: they are launch class 1 and keep hmm_viterbi_kernel, whatever their fill width.  They
are run all the same, and the launch line of TRGT_WFA_DEBUG=1 says which kernel traced each class back."""
import functools
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# one motif of 2, 3, 6, 7 bases (fill width 8; 7 is the last that fits) and of 8 bases (32 states: the one class-0 shape of width 16)
M2, M3, M6, M7, M8 = 0, 1, 2, 3, 4
CLASS0_SETS = [[b"AC"], [b"CAG"], [b"AGGCTC"], [b"ACGTTGC"], [b"ACGTTGCA"]]
# two motifs summing to 8 (9 positions: width 16), to 15 (the last of width 16) and to 16 (width 32): 33, 54 and 57 states, class 1
TWO_MOTIF_SETS = [[b"CAG", b"TTGCA"], [b"AGGCTCA", b"CCGTTGAC"], [b"AGGCTCAT", b"CCGTTGAC"]]


def _edits(allele, foreign=b"TTTTTGGGGG"):
    """the allele pure, with one substitution, one inserted base, one deleted base, and a foreign stretch of 10 bases (skip block)"""
    a = bytes(allele)
    mid = len(a) // 2
    out = [a]
    if a:
        out.append(a[:mid] + (b"T" if a[mid:mid + 1] != b"T" else b"G") + a[mid + 1:])
        out.append(a[:mid] + (b"A" if a[mid:mid + 1] != b"A" else b"C") + a[mid:])
        out.append(a[:mid] + a[mid + 1:])
    out.append(a[:mid] + foreign + a[mid:])
    return out


def _lengths(motif):
    """alleles of 0 bases, 1 base, motif length - 1, one copy, 40 copies"""
    return [b"", motif[:1], motif[:-1], motif, motif * 40]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(motif sets, jobs) of a named batch"""
    rng = np.random.default_rng(20261021)
    if name == "shapes":  # every class-0 set x every length x every edit
        return CLASS0_SETS, [(s, a) for s, ms in enumerate(CLASS0_SETS) for base in _lengths(ms[0]) for a in _edits(base)]
    if name == "two-motif":  # class 1: hmm_viterbi_kernel, whatever the fill width
        return TWO_MOTIF_SETS, [(s, a) for s, ms in enumerate(TWO_MOTIF_SETS) for m in ms for base in _lengths(m) for a in _edits(base)]
    if name.startswith("jobs-"):  # n jobs of mixed sets and lengths in one launch
        n = int(name[5:])
        return CLASS0_SETS, [(j % 5, (CLASS0_SETS[j % 5][0] * (1 + (7 * j) % 23))[:int(rng.integers(1, 150))]) for j in range(n)]
    if name == "empty-in-the-middle":
        # lists of more than 4 096 similar alleles keep the caller's order (hmm_order_host_list): job 803 is group 3 of full wave 100
        jobs = [(M3, b"CAG" * (8 + j % 5) + b"CA"[:j % 3]) for j in range(4104)]
        jobs[803] = (M3, b"")
        return CLASS0_SETS, jobs
    if name == "windows":  # across the staging chunk (64 columns, the even start of a chunk) and the 256-column mark; columns = bases + 2
        lens = [61, 62, 63, 64, 65, 66, 67, 126, 127, 128, 129, 130, 131, 253, 254, 255, 256, 257, 258, 298, 300]
        pure = [(s, (CLASS0_SETS[s][0] * 160)[:n]) for n in lens for s in (M3, M7, M8)]
        return CLASS0_SETS, pure + [(M3, _edits((b"CAG" * 160)[:n])[1 + k % 4]) for k, n in enumerate(lens)]
    if name == "visits":  # 70 and 100 copies of a 3-base motif, 140 of a 2-base one: beyond the visits in LDS and beyond one chunk of the read-back
        return CLASS0_SETS, [(M3, b"CAG" * 70), (M3, b"CAG" * 100), (M2, b"AC" * 140), (M3, b"CAG" * 33), (M8, b"ACGTTGCA" * 50), (M3, b"CAG" * 77)]
    if name == "long":  # 512 columns and more in a class of at most 256 jobs: hmm_traceback_long_kernel's, next to short ones
        return CLASS0_SETS, [(M3, b"CAG" * 12), (M3, b"CAG" * 200), (M6, b"AGGCTC" * 5), (M8, b"ACGTTGCA" * 70), (M2, b"AC" * 255), (M7, b"ACGTTGC" * 3), (M2, b"AC" * 254)]
    raise KeyError(name)


CASES = ("shapes", "two-motif", "jobs-1", "jobs-7", "jobs-8", "jobs-9", "jobs-17", "empty-in-the-middle", "windows", "visits", "long")


@pytest.fixture(scope="module")
def hmm():
    from trgt_amd import hmm as H
    return H


_REF = {}


def _batch_and_ref(oracle, H, name):
    """the packed batch and the oracle's answer, computed once"""
    if name not in _REF:
        sets, jobs = _case(name)
        batch = H.pack_hmm_batch(sets, jobs)
        _REF[name] = (batch, oracle.hmm_batch(batch, n_threads=4, want_path=True))
    return _REF[name]


def _equal(batch, got, ref, what):
    for k in ("n_spans", "path_len", "edit", "maxd", "counts"):
        assert np.array_equal(got[k], ref[k]), (what, k)
    assert np.array_equal(got["purity"].view(np.uint64), ref["purity"].view(np.uint64)), (what, "purity")  # bit patterns: NaN of an empty allele included
    for j in range(len(batch["job_set"])):
        so, ns = int(batch["span_off"][j]), int(ref["n_spans"][j])
        assert np.array_equal(got["spans"][3 * so:3 * (so + ns)], ref["spans"][3 * so:3 * (so + ns)]), (what, "spans", j)
        po, pl = int(batch["path_off"][j]), int(ref["path_len"][j])
        assert np.array_equal(got["path"][po:po + pl], ref["path"][po:po + pl]), (what, "path", j)


def _run(H, batch, **env):
    from trgt_amd import _lib
    if not env:
        return H.hmm_batch(batch)
    ctx = _lib.context_with_env(**env)
    try:
        return H.hmm_batch(batch, ctx=ctx)
    finally:
        ctx.close()


def test_cases_are_what_they_say(hmm):
    assert [hmm.num_states(s) for s in CLASS0_SETS] == [14, 17, 26, 29, 32]  # class 0: fill widths 8, 8, 8, 8, 16
    assert [hmm.num_states(s) for s in TWO_MOTIF_SETS] == [33, 54, 57]       # class 1: fill widths 16, 16, 32
    assert [sum(map(len, s)) for s in TWO_MOTIF_SETS] == [8, 15, 16]
    sets, jobs = _case("long")
    assert max(len(a) for _, a in jobs) + 2 >= 512 and len(jobs) <= 256 and min(len(a) for _, a in jobs) < 40
    assert sorted({len(a) + 2 for _, a in _case("windows")[1]} & {255, 256, 257, 300}) == [255, 256, 257, 300]


@pytest.mark.parametrize("name", CASES)
def test_matches_the_oracle(oracle, hmm, name):
    batch, ref = _batch_and_ref(oracle, hmm, name)
    _equal(batch, _run(hmm, batch), ref, name)


@pytest.mark.parametrize("name", CASES)
def test_matches_the_two_per_wave_kernel(oracle, hmm, name):
    batch, ref = _batch_and_ref(oracle, hmm, name)
    old = _run(hmm, batch, TRGT_HMM_TRACE_WIDE=1)  # (skips where the developer library is not built)
    _equal(batch, old, ref, (name, "TRGT_HMM_TRACE_WIDE"))
    _equal(batch, _run(hmm, batch), old, (name, "against TRGT_HMM_TRACE_WIDE"))  # (what a job produced: the room behind its path and spans is nobody's)


def _trace_lines(capfd):
    return dict((int(c), k) for c, k in re.findall(r"\[hmm\] class (\d+): \d+ jobs, trace-back by (\w+)", capfd.readouterr().err))


def test_which_kernel_traces_which_class(oracle, hmm, capfd):
    """class 0 takes the packed kernel; sets of two motifs -- 16 bases in all are fill width 32 -- keep hmm_viterbi_kernel"""
    sets = CLASS0_SETS + TWO_MOTIF_SETS
    jobs = [(s, ms[0] * 9) for s, ms in enumerate(sets)]
    batch = hmm.pack_hmm_batch(sets, jobs)
    ref = oracle.hmm_batch(batch, n_threads=4, want_path=True)
    capfd.readouterr()
    _equal(batch, _run(hmm, batch, TRGT_WFA_DEBUG=1), ref, "mixed classes")
    assert _trace_lines(capfd) == {0: "hmm_trace_ppl_kernel", 1: "hmm_viterbi_kernel"}
    only16 = hmm.pack_hmm_batch([TWO_MOTIF_SETS[2]], [(0, TWO_MOTIF_SETS[2][0] * 9)])
    _run(hmm, only16, TRGT_WFA_DEBUG=1)
    assert _trace_lines(capfd) == {1: "hmm_viterbi_kernel"}
    _run(hmm, batch, TRGT_WFA_DEBUG=1, TRGT_HMM_NO_PPL=1)  # no position-per-lane fill, no packed rows
    assert _trace_lines(capfd) == {0: "hmm_viterbi_kernel", 1: "hmm_viterbi_kernel"}


def test_developer_switch_routes_class_0_back(hmm, capfd):
    batch = hmm.pack_hmm_batch(CLASS0_SETS, [(s, ms[0] * 9) for s, ms in enumerate(CLASS0_SETS)])
    capfd.readouterr()
    _run(hmm, batch, TRGT_WFA_DEBUG=1, TRGT_HMM_TRACE_WIDE=1)
    assert _trace_lines(capfd) == {0: "hmm_viterbi_kernel"}
    _run(hmm, batch, TRGT_WFA_DEBUG=1, TRGT_HMM_PPL_WIDE=1)  # rows of one byte per state are not the packed kernel's
    assert _trace_lines(capfd) == {0: "hmm_viterbi_kernel"}


def _small_loci():
    """eleven loci of every class-0 motif length (and one of two motifs), a handful of clean reads each: the device-resolved job list"""
    rng = np.random.default_rng(7)
    dna = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).tolist())
    loci = []
    for l, (motifs, copies) in enumerate([(CLASS0_SETS[M2], (9, 14)), (CLASS0_SETS[M3], (10, 30)), (CLASS0_SETS[M6], (4, 4)), (CLASS0_SETS[M7], (3, 12)),
                                          (CLASS0_SETS[M8], (5, 9)), (CLASS0_SETS[M3], (40, 41)), (TWO_MOTIF_SETS[0], (6, 8)), (CLASS0_SETS[M8], (20, 33)),
                                          (CLASS0_SETS[M2], (60, 60)), (CLASS0_SETS[M7], (1, 2)), (CLASS0_SETS[M3], (86, 22))]):
        lf, rf = dna(250), dna(250)
        alleles = [b"".join(motifs[(i + h) % len(motifs)] for i in range(c)) for h, c in enumerate(copies)]
        reads = [lf + alleles[r % 2] + rf for r in range(8)]
        loci.append(dict(left_flank=lf, right_flank=rf, tr=alleles[0], motifs=list(motifs), ploidy=2, reads=reads))
    return loci


def test_locus_batch_device_resolved_list(oracle, capfd):
    import torch
    from trgt_amd import _lib, locus
    b = locus.pack(_small_loci())
    rd, fd = torch.from_numpy(b["read_blob"]).cuda(), torch.from_numpy(b["flank_blob"]).cuda()
    capfd.readouterr()
    dctx = _lib.context_with_env(TRGT_WFA_DEBUG=1)
    try:
        new = locus.run_batch(b, flank_dev=fd, reads_dev=rd, ctx=dctx)
    finally:
        dctx.close()
    assert _trace_lines(capfd).get(0) == "hmm_trace_ppl_kernel"
    assert int(new.n_alleles.min()) >= 1
    for l in range(int(b["n_loci"])):
        a0, a1 = int(b["locus_read_begin"][l]), int(b["locus_read_begin"][l + 1])
        reads = [bytes(b["read_blob"][int(b["read_off"][r]):int(b["read_off"][r]) + int(b["read_len"][r])]) for r in range(a0, a1)]
        lf = bytes(b["flank_blob"][int(b["lf_off"][l]):int(b["lf_off"][l]) + int(b["lf_len"][l])])
        rf = bytes(b["flank_blob"][int(b["rf_off"][l]):int(b["rf_off"][l]) + int(b["rf_len"][l])])
        tr = bytes(b["tr_blob"][int(b["tr_off"][l]):int(b["tr_off"][l]) + int(b["tr_len"][l])])
        m0, m1 = int(b["set_motif_begin"][l]), int(b["set_motif_begin"][l + 1])
        motifs = [bytes(b["motif_blob"][int(b["motif_off"][m]):int(b["motif_off"][m + 1])]) for m in range(m0, m1)]
        ref = oracle.locus_analyze(lf, rf, tr, motifs, reads)
        got = locus.locus_result(b, new, l)
        assert [a.seq.decode() for a in got.genotype] == ref["alleles"], l
        f = got.vcf_fields()
        assert all(f[k] == ref[k] for k in ("AL", "ALLR", "SD", "MC", "MS", "AP")), (l, f, ref)
    octx = _lib.context_with_env(TRGT_HMM_TRACE_WIDE=1)  # (skips where the developer library is not built)
    try:
        old = locus.run_batch(b, flank_dev=fd, reads_dev=rd, ctx=octx)
    finally:
        octx.close()
    for f in ("n_alleles", "allele_len", "n_spans", "spans3", "motif_counts"):
        assert np.array_equal(getattr(new, f), getattr(old, f)), f
    assert np.array_equal(new.purity.view(np.uint64), old.purity.view(np.uint64))
