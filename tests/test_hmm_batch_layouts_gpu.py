"""The host side of an HMM batch (the plan of hmm_enqueue / hmm_enqueue_slots: job order, workspace layout, result buffers, span
packing), pinned branch by branch against the CPU oracle, bit for bit: caller layouts with gaps and in another order than the jobs,
the three destinations of the spans with and without state paths, host sequences against a device blob, calls whose launch classes
interleave in job order or whose longest-first sort moves every job, empty calls and argument errors (nothing written), and the
device-resolved job list of trgt_locus_batch with every kind of slot in one call.  Every batch is tiny."""
import numpy as np
import pytest

from helpers import rand_dna, repeat_allele
from test_hmm_gpu import _same
from test_locus_gpu import _oracle_locus

pytestmark = pytest.mark.gpu

OK, INVALID = 0, -1
SENT = 0x5A5A5A5A  # what every result array holds before a call


@pytest.fixture(scope="module")
def hmm():
    from trgt_amd import hmm as H
    return H


@pytest.fixture(scope="module")
def lib_mod():
    from trgt_amd import _lib
    assert _lib.lib().trgt_hip_abi_version() == 11
    return _lib


def _bits(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _sentinel(dtype, n):
    a = np.zeros(n, dtype)
    _bits(a)[:] = SENT & ((1 << 8 * a.dtype.itemsize) - 1)
    return a


def _untouched(a):
    return bool((_bits(a) == SENT & ((1 << 8 * a.dtype.itemsize) - 1)).all())


def _outputs(n, sizes):
    """Result arrays full of the sentinel.  sizes: words of path / spans (triples) / counts."""
    return dict(path=_sentinel(np.uint16, sizes["path"]), path_len=_sentinel(np.uint32, n), spans=_sentinel(np.int32, 3 * sizes["spans"]),
                n_spans=_sentinel(np.uint32, n), counts=_sentinel(np.uint32, sizes["counts"]), purity=_sentinel(np.float64, n),
                edit=_sentinel(np.int32, n), maxd=_sentinel(np.int32, n))


def _dense_sizes(b):
    return dict(path=int(b["path_off"][-1]), spans=int(b["span_off"][-1]), counts=int(b["count_off"][-1]))


def _call(lib_mod, b, out, ctx=None, seq=None, n_jobs=None, n_sets=None, **override):
    """trgt_hmm_batch as it stands in the header; override: argument name -> array or None (a NULL pointer)."""
    ctx = ctx or lib_mod.context()
    a = dict(motif_blob=b["motif_blob"], motif_off=b["motif_off"], set_motif_begin=b["set_motif_begin"], job_set=b["job_set"],
             seq_blob=b["seq_blob"] if seq is None else seq, seq_off=b["seq_off"], seq_len=b["seq_len"], path=out["path"], path_off=b["path_off"],
             path_len=out["path_len"], spans=out["spans"], span_off=b["span_off"], n_spans=out["n_spans"], counts=out["counts"],
             count_off=b["count_off"], purity=out["purity"], edit=out["edit"], maxd=out["maxd"])
    a.update(override)
    p = lib_mod.ptr
    rc = lib_mod.lib().trgt_hmm_batch(
        ctx.handle, len(b["set_motif_begin"]) - 1 if n_sets is None else n_sets, p(a["motif_blob"]), p(a["motif_off"]), p(a["set_motif_begin"]),
        len(b["job_set"]) if n_jobs is None else n_jobs, p(a["job_set"]), p(a["seq_blob"]), p(a["seq_off"]), p(a["seq_len"]), p(a["path"]),
        p(a["path_off"]), p(a["path_len"]), p(a["spans"]), p(a["span_off"]), p(a["n_spans"]), p(a["counts"]), p(a["count_off"]), p(a["purity"]),
        p(a["edit"]), p(a["maxd"]))
    return rc, lib_mod.lib().trgt_hip_last_error(ctx.handle).decode()


def _small_batch(hmm, rng):
    """Nine jobs over four sets of three launch classes; alleles of 0 to 700 bases."""
    sets = [[b"CAG"], [b"GGCCTG", b"CCG"], [rand_dna(rng, 40), rand_dna(rng, 40)], [b"AAGGG", b"AAAAG", b"ACG"]]
    assert [hmm.num_states(s) for s in sets] == [17, 36, 249, 49]
    jobs = [(0, repeat_allele(rng, sets[0], 90)), (2, repeat_allele(rng, sets[2], 680)), (1, b""), (3, repeat_allele(rng, sets[3], 333)),
            (0, b"C"), (1, repeat_allele(rng, sets[1], 520)), (2, repeat_allele(rng, sets[2], 41)), (3, rand_dna(rng, 64)),
            (0, repeat_allele(rng, sets[0], 255, err=0.05))]
    return sets, jobs


def _job_ranges(b, ref, j):
    return (int(b["span_off"][j]), int(ref["n_spans"][j]), int(b["count_off"][j]), int(b["n_motifs"][j]), int(b["path_off"][j]), int(ref["path_len"][j]))


def _assert_jobs(b, ref, lay, got, spans=None, want_path=True):
    """Every job's results, read at the job's offsets of `lay`, against the oracle's at the dense offsets of `b`."""
    spans = got["spans"] if spans is None else spans
    for k in ("n_spans", "path_len", "edit", "maxd"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["purity"].view(np.uint64), ref["purity"].view(np.uint64))
    for j in range(len(b["job_set"])):
        so, ns, co, nm, po, pl = _job_ranges(b, ref, j)
        ls, lc, lp = int(lay["span_off"][j]), int(lay["count_off"][j]), int(lay["path_off"][j])
        assert np.array_equal(got["counts"][lc:lc + nm], ref["counts"][co:co + nm]), j
        if spans is not False:
            assert np.array_equal(spans[3 * ls:3 * (ls + ns)], ref["spans"][3 * so:3 * (so + ns)]), j
        if want_path:
            assert np.array_equal(got["path"][lp:lp + pl], ref["path"][po:po + pl]), j


def test_sparse_permuted_caller_layouts(oracle, hmm, lib_mod):
    rng = np.random.default_rng(2101)
    sets, jobs = _small_batch(hmm, rng)
    b = hmm.pack_hmm_batch(sets, jobs)
    ref = oracle.hmm_batch(b, n_threads=4)
    n = len(jobs)
    seq_len = b["seq_len"].astype(np.int64)
    path_cap = np.diff(b["path_off"].astype(np.int64))
    lay, sizes = dict(b), {}
    # every array laid out in an order of its own, a gap in front of every job's piece and behind the last
    for key, need, size_key in (("seq_off", seq_len, "seq"), ("span_off", seq_len + 1, "spans"), ("count_off", b["n_motifs"], "counts"), ("path_off", path_cap, "path")):
        off, at = np.zeros(n, np.uint64), 0
        order = rng.permutation(n)
        assert not np.array_equal(order, np.arange(n))
        for j in order:
            at += int(rng.integers(1, 8))
            off[j] = at
            at += int(need[j])
        lay[key], sizes[size_key] = off, at + 5
        assert (np.diff(off.astype(np.int64)) < 0).any()
    blob = np.frombuffer(rand_dna(rng, sizes["seq"]), np.uint8).copy()  # (bases between the alleles: a job that read past its end would show)
    for j in range(n):
        blob[int(lay["seq_off"][j]):int(lay["seq_off"][j]) + int(seq_len[j])] = b["seq_blob"][int(b["seq_off"][j]):int(b["seq_off"][j]) + int(seq_len[j])]
    lay["seq_blob"] = blob
    out = _outputs(n, sizes)
    rc, msg = _call(lib_mod, lay, out)
    assert rc == OK, msg
    _assert_jobs(b, ref, lay, out)
    # motif counts: a host array shared with other batches -- only the words of this call's jobs are written
    mine = np.zeros(sizes["counts"], bool)
    for j in range(n):
        mine[int(lay["count_off"][j]):int(lay["count_off"][j]) + int(b["n_motifs"][j])] = True
    assert _untouched(out["counts"][~mine]) and (~mine).sum() >= n
    # spans: only the triples a job produced are copied back
    rest = np.ones(sizes["spans"], bool)
    for j in range(n):
        rest[int(lay["span_off"][j]):int(lay["span_off"][j]) + int(ref["n_spans"][j])] = False
    assert _untouched(out["spans"].reshape(-1, 3)[rest]) and rest.sum() > int(seq_len.sum()) // 2


def test_three_span_destinations_with_and_without_paths(oracle, hmm, lib_mod):
    import torch
    rng = np.random.default_rng(2217)
    sets, jobs = _small_batch(hmm, rng)
    b = hmm.pack_hmm_batch(sets, jobs)
    ref = oracle.hmm_batch(b, n_threads=4)
    n, sizes = len(jobs), _dense_sizes(b)
    runs = []
    for dest in ("host", "device", "none"):
        for want_path in (True, False):
            out = _outputs(n, sizes)
            override = {}
            dev_spans = None
            if dest == "device":
                dev_spans = torch.from_numpy(out["spans"].copy()).cuda()
                override["spans"] = dev_spans
            elif dest == "none":  # purity and counts only, as the purity filter asks for them
                override.update(spans=None, span_off=None)
            if not want_path:
                override["path"] = None
                if dest == "none":  # (the filter's call: no path lengths and no distances either)
                    override.update(path_off=None, path_len=None, edit=None, maxd=None)
            rc, msg = _call(lib_mod, b, out, **override)
            assert rc == OK, (dest, want_path, msg)
            spans = out["spans"] if dest == "host" else dev_spans.cpu().numpy() if dest == "device" else False
            if not want_path:
                assert _untouched(out["path"]), dest
                if dest == "none":
                    assert all(_untouched(out[k]) for k in ("path_len", "edit", "maxd"))
                    for k in ("path_len", "edit", "maxd"):
                        out[k] = ref[k]
            _assert_jobs(b, ref, b, out, spans=spans, want_path=want_path)
            if dest != "host":
                assert _untouched(out["spans"]), dest
            runs.append(out)
    for out in runs[1:]:
        assert np.array_equal(out["counts"], runs[0]["counts"]) and np.array_equal(out["n_spans"], runs[0]["n_spans"])
        assert np.array_equal(out["purity"].view(np.uint64), runs[0]["purity"].view(np.uint64))


def test_host_sequences_against_a_device_blob(oracle, hmm, lib_mod):
    import torch
    rng = np.random.default_rng(2185)
    sets, jobs = _small_batch(hmm, rng)
    assert any(len(a) == 0 for _, a in jobs)
    for some in (jobs, jobs[3:4]):  # ... and a batch of one job
        b = hmm.pack_hmm_batch(sets, some)
        ref = oracle.hmm_batch(b, n_threads=4)
        host, dev = _outputs(len(some), _dense_sizes(b)), _outputs(len(some), _dense_sizes(b))
        rc, msg = _call(lib_mod, b, host)
        assert rc == OK, msg
        rc, msg = _call(lib_mod, b, dev, seq=torch.from_numpy(b["seq_blob"]).cuda())
        assert rc == OK, msg
        for got in (host, dev):
            _assert_jobs(b, ref, b, got)


def test_classes_interleaved_in_job_order(oracle, hmm):
    # the stable sort by class: a two-alleles-per-wave set, a one-wave set, a four-wave set and an eight-wave set, each with an allele of
    # 40 bases and one of 600, shuffled
    rng = np.random.default_rng(2169)
    sets = [[rand_dna(rng, 3)], [rand_dna(rng, 10)], [rand_dna(rng, 40), rand_dna(rng, 40)], [rand_dna(rng, 150)]]
    assert [hmm.num_states(s) for s in sets] == [17, 38, 249, 458]
    jobs = [(s, repeat_allele(rng, m, n, err=0.02)) for s, m in enumerate(sets) for n in (40, 600)]
    order = rng.permutation(len(jobs))
    jobs = [jobs[int(i)] for i in order]
    cls = [j[0] for j in jobs]
    assert cls != sorted(cls) and sum(x != y for x, y in zip(cls, cls[1:])) >= 4  # (the classes do interleave)
    for want_path in (True, False):
        _same(oracle, hmm, sets, jobs, want_path=want_path)


def test_longest_first_sort_moves_every_job(oracle, hmm):
    rng = np.random.default_rng(2180)
    sets = [[b"GGCCTG", b"CCG"]]
    jobs = [(0, repeat_allele(rng, sets[0], n, err=0.03)) for n in (0, 35, 130, 410, 680)]
    assert [len(a) for _, a in jobs] == sorted(len(a) for _, a in jobs) and len({len(a) for _, a in jobs}) == 5
    for want_path in (True, False):
        _same(oracle, hmm, sets, jobs, want_path=want_path)


def test_empty_calls_and_argument_errors_write_nothing(oracle, hmm, lib_mod):
    rng = np.random.default_rng(2110)
    sets, jobs = _small_batch(hmm, rng)
    b = hmm.pack_hmm_batch(sets, jobs)
    n, sizes = len(jobs), _dense_sizes(b)
    ctx = lib_mod.Context(0)
    try:
        def nothing_written(out):
            return all(_untouched(v) for v in out.values())
        out = _outputs(n, sizes)
        rc, msg = _call(lib_mod, b, out, ctx=ctx, n_jobs=0)
        assert rc == OK and nothing_written(out), msg
        rc, msg = _call(lib_mod, b, out, ctx=ctx, n_jobs=0, n_sets=0)
        assert rc == OK and nothing_written(out), msg
        # with no job nothing is read: every pointer may be null
        rc, msg = _call(lib_mod, b, out, ctx=ctx, n_jobs=0, n_sets=0, **{k: None for k in ("motif_blob", "motif_off", "set_motif_begin", "job_set", "seq_blob", "seq_off", "seq_len", "path", "path_off", "path_len", "spans", "span_off", "n_spans", "counts", "count_off", "purity", "edit", "maxd")})
        assert rc == OK, msg
        for null in ("motif_blob", "motif_off", "set_motif_begin", "job_set", "seq_off", "seq_len", "span_off", "n_spans", "counts", "count_off", "purity"):
            rc, msg = _call(lib_mod, b, out, ctx=ctx, **{null: None})
            assert rc == INVALID and msg == "trgt_hmm_batch: null argument", (null, msg)
            assert nothing_written(out), null
        rc, msg = _call(lib_mod, b, out, ctx=ctx, path_off=None)
        assert rc == INVALID and msg == "trgt_hmm_batch: path without path_off" and nothing_written(out), msg
        rc, msg = _call(lib_mod, b, out, ctx=ctx, n_sets=-1)
        assert rc == INVALID and msg == "trgt_hmm_batch: null argument" and nothing_written(out), msg
        bad = dict(b)
        bad["job_set"] = b["job_set"].copy()
        bad["job_set"][5] = len(sets)
        rc, msg = _call(lib_mod, bad, out, ctx=ctx)
        assert rc == INVALID and msg == "trgt_hmm_batch: job 5 bad set" and nothing_written(out), msg
        # the context stays usable
        rc, msg = _call(lib_mod, b, out, ctx=ctx)
        assert rc == OK, msg
        _assert_jobs(b, oracle.hmm_batch(b, n_threads=4), b, out)
    finally:
        ctx.close()


# ---- the device-resolved job list (hmm_enqueue_slots) through trgt_locus_batch
def _slot_loci(rng):
    dna = lambda n: rand_dna(rng, n)
    lf, rf = dna(250), dna(250)
    mk = lambda rep: dna(int(rng.integers(250, 300))) + lf + rep + rf + dna(int(rng.integers(250, 300)))
    base = dict(left_flank=lf, right_flank=rf)
    big = dna(150)   # 458 states: past the 448 lanes of the locus path's largest workgroup
    mid = dna(21)    # 71 states: a two-wave class
    return [
        dict(base, tr=b"CAG" * 10, motifs=[b"CAG"], reads=[mk(b"CAG" * (10 if i < 6 else 31)) for i in range(12)]),       # heterozygous; two alleles per wave
        dict(base, tr=b"AT" * 12, motifs=[b"AT"], reads=[mk(b"AT" * 12) for _ in range(10)]),                            # homozygous: the dedupe copy
        dict(base, tr=b"CAG" * 8, motifs=[b"CAG", b"CCG"], genotyper="cluster",                                          # beyond 256 reads: left to the host path
             reads=[mk(b"CAG" * (8 if i % 2 else 12)) for i in range(258)]),
        dict(base, tr=b"GCC" * 7, motifs=[b"GCC"], ploidy=1, reads=[mk(b"GCC" * k) for k in (7, 7, 8, 7, 6, 7)]),         # one allele
        dict(base, tr=mid * 3, motifs=[mid], reads=[mk(mid * (3 if i % 2 else 5)) for i in range(10)]),                  # a class of its own
        dict(base, tr=big * 2, motifs=[big], reads=[mk(big * (2 if i % 2 else 3)) for i in range(10)]),                  # the large-model class
    ]


def _compare_refs(locus, b, out, refs):
    for l, ref in enumerate(refs):
        a0, a1 = int(b["locus_read_begin"][l]), int(b["locus_read_begin"][l + 1])
        assert np.array_equal(out.span_start[a0:a1], ref["span_start"]) and np.array_equal(out.span_end[a0:a1], ref["span_end"]), l
        got = locus.locus_result(b, out, l)
        assert len(got.genotype) == ref["n_alleles"], l
        assert [a.seq.decode() for a in got.genotype] == ref["alleles"], l
        assert got.reads == [int(v) for v in ref["kept_read"]], l
        assert got.classification == [int(v) for v in ref["classification"]], l
        if ref["n_alleles"]:
            f = got.vcf_fields()
            for k in ("AL", "ALLR", "SD", "MC", "MS", "AP"):
                assert f[k] == ref[k], (l, k)


def test_slots_path_every_kind_of_slot(oracle, hmm, lib_mod):
    from trgt_amd import locus
    rng = np.random.default_rng(2283)
    loci = _slot_loci(rng)
    assert [hmm.num_states(L["motifs"]) for L in loci] == [17, 14, 27, 17, 71, 458]
    b = locus.pack(loci)
    params = locus.Params()
    refs = [_oracle_locus(oracle, b, l, params) for l in range(len(loci))]
    assert [r["n_alleles"] for r in refs] == [2, 2, 2, 1, 2, 2]
    assert refs[0]["alleles"][0] != refs[0]["alleles"][1] and refs[1]["alleles"][0] == refs[1]["alleles"][1]
    out = locus.run_batch(b, params)
    assert int(out.stats[22]) == 0  # (the cluster locus was not genotyped on the device)
    _compare_refs(locus, b, out, refs)
    for env in (dict(TRGT_HMM_RESOLVE_ONE_WG=1), dict(TRGT_HMM_PPL_PER_CLASS=1), dict(TRGT_HMM_NO_DEDUPE=1)):
        ctx = lib_mod.context_with_env(**env)
        try:
            got = locus.run_batch(b, params, ctx=ctx)
        finally:
            ctx.close()
        _compare_refs(locus, b, got, refs)
        assert np.array_equal(got.n_spans, out.n_spans) and np.array_equal(got.purity.view(np.uint64), out.purity.view(np.uint64)), env
    # every locus left to the host: the slots path has no candidate at all
    only = locus.pack([loci[2]])
    got = locus.run_batch(only, params)
    assert int(got.stats[22]) == 0
    _compare_refs(locus, only, got, refs[2:3])
