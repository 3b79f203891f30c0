"""Motif sets beyond the one-thread-per-lane kernels (more than 1 024 states in trgt_hmm_batch, more than 448 lanes in the locus
path) are labelled by hmm_viterbi_big_kernel, which tiles a model's lanes over a workgroup of 1 024 threads: models of up to 4 096
states, bit for bit like the CPU oracle (state paths, spans, counts, f64 purity bits, edit / max distances), through trgt_hmm_batch
and trgt_locus_batch; the device-built tables of such models equal the host builder's; one state past the limit the call answers
TRGT_ERR_UNSUPPORTED and writes nothing."""
import ctypes as C

import numpy as np
import pytest

from helpers import mutate, rand_dna, rand_motif, repeat_allele
from test_hmm_gpu import _same
from test_locus_gpu import _compare, _run_both
from trgt_amd.hmm import MAX_STATES as LIMIT

pytestmark = pytest.mark.gpu

assert LIMIT == 4096  # states: the envelope the library documents (include/trgt_hip.h); the set sizes below are built around it
UNSUPPORTED, NOMEM = -3, -5


@pytest.fixture(scope="module")
def hmm():
    from trgt_amd import hmm as H
    return H


def _large_sets(rng):
    """A single motif of 150 bases (458 states: the first locus-path class past 448 lanes), of 339 (1 025: the first size past the
    1 024 states of hmm_viterbi_kernel), of 700; ten motifs of 50 bases (1 517 states); three motifs at the limit exactly (4 096)."""
    return [[rand_dna(rng, 150)], [rand_dna(rng, 339)], [rand_dna(rng, 700)], [rand_dna(rng, 50) for _ in range(10)],
            [rand_dna(rng, 1000), rand_dna(rng, 361), rand_dna(rng, 1)]]


def _with_n(rng, seq, k=3):
    s = bytearray(seq)
    for p in rng.integers(0, len(s), size=k):
        s[int(p)] = ord("N")
    return bytes(s)


def _alleles(rng, motifs):
    m = motifs[0]
    clean = b"".join(motifs[int(i) % len(motifs)] for i in range(3)) if len(motifs) > 1 else m * 3
    long_total = max(1600, len(m) + 600)
    return [b"", m[: max(1, min(len(m) // 2, 40))], clean, _with_n(rng, mutate(rng, clean, 0.02, 0.01, 0.01)),
            rand_dna(rng, 400), repeat_allele(rng, motifs, long_total, err=0.02)]


def test_hmm_batch_large_sets_next_to_small_ones(oracle, hmm):
    rng = np.random.default_rng(20261017)
    sets = _large_sets(rng)
    assert [hmm.num_states(s) for s in sets] == [458, 1025, 2108, 1517, LIMIT]
    jobs = []
    for s, motifs in enumerate(sets):
        al = _alleles(rng, motifs)
        assert al[0] == b"" and len(al[1]) < len(motifs[0]) and len(al[5]) + 2 >= 1536
        jobs += [(s, a) for a in al]
    for _ in range(8):  # ordinary STR sets in the same call: the classes of hmm_viterbi_kernel launch next to the new one
        sets.append([rand_motif(rng, 3, 6, allow_n=False)])
        for n in (40, 300):
            jobs.append((len(sets) - 1, repeat_allele(rng, sets[-1], n, err=0.02)))
    order = rng.permutation(len(jobs))
    jobs = [jobs[int(i)] for i in order]
    for want_path in (True, False):
        _same(oracle, hmm, sets, jobs, want_path=want_path)


def test_hmm_batch_sizes_around_the_old_limits(oracle, hmm):
    # the last sizes hmm_viterbi_kernel takes and the first it does not (16 waves = 1 024 lanes), a deletion chain of exactly
    # 64 / 65 states (one wave / one wave and a lane), chains over several waves next to short ones in one model
    rng = np.random.default_rng(77)
    sets = [[rand_dna(rng, 337), b"A"], [rand_dna(rng, 336), b"A", b"C"], [rand_dna(rng, 339)], [rand_dna(rng, 400), b"CAG", b"AT"],
            [rand_dna(rng, 64), rand_dna(rng, 65), rand_dna(rng, 300)], [rand_dna(rng, 129), rand_dna(rng, 128), rand_dna(rng, 200), b"N"]]
    assert [hmm.num_states(s) for s in sets][:3] == [1023, 1024, 1025]
    jobs = []
    for s, motifs in enumerate(sets):
        jobs.append((s, repeat_allele(rng, motifs, 900, err=0.03)))
        jobs.append((s, _with_n(rng, repeat_allele(rng, motifs, 1700, err=0.01))))
        jobs.append((s, rand_dna(rng, 64)))
    _same(oracle, hmm, sets, jobs)


def test_large_model_visit_records_and_dropped_copies(oracle, hmm):
    # the branches of the shared step decoder behind hmm_viterbi_big_kernel: 200 visits of a 3-base motif are more than the
    # HMM_VIS_LDS = 64 records kept in LDS plus one staged chunk of 85 read back from the workspace (records in LDS, in the
    # workspace, and a second chunk of the read-back); the mutated allele has copies that remove_imperfect_motifs drops
    rng = np.random.default_rng(340)
    sets = [[rand_dna(rng, 340), b"CAG", b"AT"]]
    assert hmm.num_states(sets[0]) == 1045  # past the 1 024 states of hmm_viterbi_kernel
    clean = b"CAG" * 200
    jobs = [(0, clean), (0, mutate(rng, clean, 0.01, 0.005, 0.005))]
    batch = hmm.pack_hmm_batch(sets, jobs)
    ref = oracle.hmm_batch(batch, n_threads=2)
    co = batch["count_off"]
    assert int(ref["counts"][int(co[0]):int(co[0]) + 3].sum()) >= 150 and int(ref["n_spans"][0]) >= 1
    assert int(ref["n_spans"][1]) >= 2
    for want_path in (True, False):
        _same(oracle, hmm, sets, jobs, want_path=want_path)


def test_locus_batch_large_motif_sets(oracle):
    from trgt_amd import locus
    rng = np.random.default_rng(4096)
    dna = lambda n: rand_dna(rng, n)
    lf, rf = dna(250), dna(250)
    mk = lambda rep: dna(int(rng.integers(250, 300))) + lf + rep + rf + dna(int(rng.integers(250, 300)))
    noisy = lambda rep: mutate(rng, rep, 0.004, 0.002, 0.002)
    loci = []
    for gt in ("size", "cluster"):
        for motifs in _large_sets(rng):
            m = motifs[0]
            if len(motifs) == 1:
                a0, a1 = m * 2, m * 3
            elif len(motifs) == 10:
                a0, a1 = b"".join(motifs[:6]), b"".join(motifs[2:]) + motifs[0] * 2
            else:
                a0, a1 = motifs[0] + motifs[1], motifs[0] + motifs[1] * 2 + motifs[2]
            reads = [mk(noisy(a0 if i % 2 else a1)) for i in range(10)]
            loci.append(dict(left_flank=lf, right_flank=rf, tr=a0, motifs=motifs, genotyper=gt, reads=reads))
            # ... among STR loci
            k0, k1 = int(rng.integers(5, 20)), int(rng.integers(20, 40))
            str_m = rand_motif(rng, 3, 6, allow_n=False)
            loci.append(dict(left_flank=lf, right_flank=rf, tr=str_m * k0, motifs=[str_m], genotyper=gt,
                             reads=[mk(str_m * (k0 if i % 2 else k1)) for i in range(12)]))
    b = locus.pack(loci)
    params = locus.Params()
    for mode, out in _run_both(locus, b):
        _compare(oracle, locus, b, out, params, range(len(loci)))


def test_device_built_large_models_equal_host_builder(hmm):
    # S just below, at and above 1 024; around the locus path's 448 lanes; at the new limit
    rng = np.random.default_rng(31)
    sets = [[rand_dna(rng, 338)], [rand_dna(rng, 337), b"A"], [rand_dna(rng, 336), b"A", b"C"], [rand_dna(rng, 339)], [rand_dna(rng, 340), b"N"],
            [rand_dna(rng, 146)], [rand_dna(rng, 147)], [rand_dna(rng, 150)], [rand_dna(rng, 700)], [rand_dna(rng, 50) for _ in range(10)],
            [rand_dna(rng, 65), rand_dna(rng, 64), rand_dna(rng, 129), rand_dna(rng, 500)],
            [rand_dna(rng, 1362)], [rand_dna(rng, 1000), rand_dna(rng, 361), rand_dna(rng, 1)], [rand_dna(rng, 12) for _ in range(110)] + [rand_dna(rng, 6)]]
    S = [hmm.num_states(s) for s in sets]
    assert S[:5] == [1022, 1023, 1024, 1025, 1032] and S[-3:-1] == [4094, LIMIT] and max(S) == LIMIT
    assert hmm.models_check(sets) == 0
    for s in sets:  # ... and one set at a time (a set's tables do not depend on its place in the blob)
        assert hmm.models_check([s]) == 0


def _raw_call(_lib, ctx, H, sets, jobs, fill):
    b = H.pack_hmm_batch(sets, jobs)
    n = len(jobs)
    out = dict(path=np.full(int(b["path_off"][-1]), fill, np.uint16), path_len=np.full(n, fill, np.uint32),
               spans=np.full(3 * int(b["span_off"][-1]), fill, np.int32), n_spans=np.full(n, fill, np.uint32),
               counts=np.full(int(b["count_off"][-1]), fill, np.uint32), purity=np.full(n, float(fill), np.float64),
               edit=np.full(n, fill, np.int32), maxd=np.full(n, fill, np.int32))
    p = _lib.ptr
    rc = _lib.lib().trgt_hmm_batch(ctx.handle, len(sets), p(b["motif_blob"]), p(b["motif_off"]), p(b["set_motif_begin"]), n, p(b["job_set"]),
                                   p(b["seq_blob"]), p(b["seq_off"]), p(b["seq_len"]), p(out["path"]), p(b["path_off"]), p(out["path_len"]),
                                   p(out["spans"]), p(b["span_off"]), p(out["n_spans"]), p(out["counts"]), p(b["count_off"]), p(out["purity"]),
                                   p(out["edit"]), p(out["maxd"]))
    return rc, out, _lib.lib().trgt_hip_last_error(ctx.handle).decode()


def test_one_state_past_the_limit_is_unsupported_and_writes_nothing(oracle, hmm):
    from trgt_amd import _lib
    rng = np.random.default_rng(5)
    sets = [[b"CAG"], [rand_dna(rng, 1363)], [rand_dna(rng, 1000), rand_dna(rng, 361), rand_dna(rng, 1)]]
    assert [hmm.num_states(s) for s in sets] == [17, LIMIT + 1, LIMIT]
    jobs = [(0, b"CAG" * 20), (1, rand_dna(rng, 200)), (2, rand_dna(rng, 100))]
    ctx = _lib.Context(0)
    try:
        rc, out, msg = _raw_call(_lib, ctx, hmm, sets, jobs, 0x5A5A)
        assert rc == UNSUPPORTED
        assert "set 1" in msg and str(LIMIT + 1) in msg and "limit %d" % LIMIT in msg, msg
        for k, v in out.items():
            assert (v == (float(0x5A5A) if k == "purity" else 0x5A5A)).all(), k
        with pytest.raises(_lib.TrgtHipError):
            hmm.models_check(sets)
        # the context stays usable, and the set AT the limit runs
        keep = [sets[0], sets[2]]
        _same(oracle, hmm, keep, [(0, b"CAG" * 20), (1, rand_dna(rng, 100))])
        # back-pointer workspace above the limit: TRGT_ERR_NOMEM as for every other model
        assert _lib.lib().trgt_hip_set_workspace_limit(ctx.handle, C.c_uint64(1 << 20)) == 0
        rc, out, msg = _raw_call(_lib, ctx, hmm, keep, [(1, rand_dna(rng, 1000))], 0x5A5A)
        assert rc == NOMEM and "workspace" in msg, msg
        assert (out["n_spans"] == 0x5A5A).all() and (out["counts"] == 0x5A5A).all()
        assert _lib.lib().trgt_hip_set_workspace_limit(ctx.handle, C.c_uint64(8 << 30)) == 0
        rc, out, msg = _raw_call(_lib, ctx, hmm, keep, [(1, rand_dna(rng, 1000))], 0x5A5A)
        assert rc == 0, msg
    finally:
        ctx.close()
