"""filter_impure_trs on the device (trgt_amd/csrc/locus_purity.hpp): calls with min_read_qual < 0.9 keep the device-side genotyper
chains -- selection, purity jobs, HMM batch and filter run in front of them.  Every case is compared field by field with the oracle
(test_locus_gpu._compare), reads on the host and resident in HBM, and under the planner knobs that move loci back to the host."""
import numpy as np
import pytest

import purity_cases as pc
from test_locus_gpu import _compare

pytestmark = pytest.mark.gpu

# (name, context switches, what the counters must say: stats[18] = loci repaired on the device, stats[22] = cluster loci genotyped there)
MODES = [("host reads", None), ("device", None), ("host repair", dict(TRGT_HOST_REPAIR=1)), ("host cluster", dict(TRGT_HOST_CLUSTER=1)),
         ("split hmm", dict(TRGT_SPLIT_HMM=1)), ("host purity", dict(TRGT_HOST_PURITY=1))]


class _Memo:
    """the oracle with locus_analyze remembered: one reference per locus and setting, shared by every mode"""
    def __init__(self, oracle):
        self.oracle, self.seen = oracle, {}

    def locus_analyze(self, lf, rf, tr, motifs, reads, **kw):
        rq = kw.get("read_qual")
        key = (lf, rf, tr, tuple(motifs), tuple(reads), None if rq is None else np.asarray(rq, np.float64).tobytes(),
               tuple(sorted((k, str(v)) for k, v in kw.items() if k not in ("read_qual", "meta"))), repr(kw.get("meta")))
        if key not in self.seen:
            self.seen[key] = self.oracle.locus_analyze(lf, rf, tr, motifs, reads, **kw)
        return self.seen[key]


@pytest.fixture(scope="module")
def memo(oracle):
    return _Memo(oracle)


def _loci_of(b):
    """a synthetic batch as a list of loci (to mix it with hand-made ones in one call)"""
    u = lambda blob, o, n: bytes(blob[int(o):int(o) + int(n)])
    out = []
    for l in range(int(b["n_loci"])):
        m0, m1 = int(b["set_motif_begin"][l]), int(b["set_motif_begin"][l + 1])
        a0, a1 = int(b["locus_read_begin"][l]), int(b["locus_read_begin"][l + 1])
        out.append(dict(left_flank=u(b["flank_blob"], b["lf_off"][l], b["lf_len"][l]), right_flank=u(b["flank_blob"], b["rf_off"][l], b["rf_len"][l]),
                        tr=u(b["tr_blob"], b["tr_off"][l], b["tr_len"][l]), ploidy=int(b["ploidy"][l]), genotyper=int(b["genotyper"][l]),
                        motifs=[bytes(b["motif_blob"][int(b["motif_off"][m]):int(b["motif_off"][m + 1])]) for m in range(m0, m1)],
                        reads=[u(b["read_blob"], b["read_off"][r], b["read_len"][r]) for r in range(a0, a1)]))
    return out


def _runs(locus, b, params, modes):
    import torch
    from trgt_amd import _lib
    for name, env in modes:
        if env is None:
            if name == "device":
                yield name, locus.run_batch(b, params, flank_dev=torch.from_numpy(b["flank_blob"]).cuda(), reads_dev=torch.from_numpy(b["read_blob"]).cuda())
            else:
                yield name, locus.run_batch(b, params)
            continue
        ctx = _lib.context_with_env(**env)
        try:
            out = locus.run_batch(b, params, ctx=ctx)
        finally:
            ctx.close()
        yield name, out


def _check(memo, loci, modes=MODES, max_depth=250, read_qual="own"):
    from trgt_amd import locus
    params = locus.Params(min_read_qual=0.5, max_depth=max_depth)
    b = locus.pack(loci)
    if read_qual is None:
        b["read_qual"] = None  # None for every read of the batch: trgt_locus_batch_in.read_qual == NULL
    # the oracle restates analyze_tr behind the Ploidy::Zero test of tr.rs:29-31 and knows no ploidy 0: such a locus is held to
    # LocusResult::empty directly, and its spans to the oracle's for the same reads
    zero = [l for l, L in enumerate(loci) if L.get("ploidy", 2) == 0]
    res = {}
    for name, out in _runs(locus, b, params, modes):
        n_repair = _compare(memo, locus, b, out, params, [l for l in range(len(loci)) if l not in zero])
        for l in zero:
            L, a0, a1 = loci[l], int(b["locus_read_begin"][l]), int(b["locus_read_begin"][l + 1])
            ref = memo.locus_analyze(L["left_flank"], L["right_flank"], L["tr"], L["motifs"], L["reads"])
            assert np.array_equal(out.span_start[a0:a1], ref["span_start"]) and np.array_equal(out.span_end[a0:a1], ref["span_end"]), (name, l)
            got = locus.locus_result(b, out, l)
            assert got.genotype == [] and got.reads == [] and got.classification == [] and int(out.n_alleles[l]) == 0, (name, l)
            assert (out.read_rank[a0:a1] == -1).all() and (out.classification[a0:a1] == -1).all(), (name, l)
        res[name] = (out, n_repair)
    return b, res


def test_low_read_quality_calls_keep_the_device_genotypers(memo):
    """the feature: with the filter on, consensus repair and the cluster genotyper run on the device (neither did: every locus took the
    host path, so both counters were 0)"""
    from trgt_amd import synth
    rng = np.random.default_rng(17)
    cl = _loci_of(synth.generate(4, first_locus=40, config=5, sub_rate=0.01))
    for L in cl:
        L["read_qual"] = [(0.999, 0.7, None)[int(rng.integers(0, 3))] for _ in L["reads"]]
    loci = pc.no_majority_loci() + cl
    n_cluster = sum(L.get("genotyper") in (1, "cluster") for L in loci)
    assert n_cluster == 4 and all(len(L["reads"]) <= 40 for L in loci)
    b, res = _check(memo, loci)
    for name, (out, n_repair) in res.items():
        st = [int(v) for v in out.stats[:24]]
        assert n_repair > 0, name
        if name in ("host reads", "device", "split hmm"):
            assert st[18] > 0 and st[19] == 0, (name, st[18:21])
        if name in ("host reads", "device", "host repair"):
            assert st[22] == n_cluster and st[23] == 0, (name, st[22:24])
        if name == "host repair":
            assert st[18] == 0, name
        if name in ("host cluster", "split hmm"):
            assert st[22] == 0, name
        if name == "host purity":  # the routing of the calls before the filter ran on the device
            assert st[18] == 0 and st[22] == 0, (name, st[18:24])
        assert st[3] > 0, name  # purity jobs are counted with the HMM jobs
    # (at most two HMM jobs per locus label alleles: the rest are the purity jobs of the device route)
    assert int(res["host reads"][0].stats[3]) > 2 * len(loci)


def test_budget_ordering_and_nan(memo):
    loci = pc.budget_loci() + pc.ordering_loci() + pc.nan_loci()
    b, res = _check(memo, loci)
    out = res["host reads"][0]
    lrb = b["locus_read_begin"]
    kept = [int((out.read_rank[int(lrb[l]):int(lrb[l + 1])] >= 0).sum()) for l in range(len(loci))]
    assert kept[:5] == [3, 4, 13, 22, 9] and kept[7] == 7, kept   # the budgets 1, 1, 2, 3, 1; nothing scored: nothing dropped


def test_downsample_comes_before_the_filter(memo):
    loci = pc.downsample_loci()
    b, res = _check(memo, loci, max_depth=16)
    out = res["device"][0]
    assert int((out.read_rank[:40] >= 0).sum()) == 14   # 16 selected, max(1, round(1.6)) = 2 of the impure ones among them dropped


def test_no_read_quality_in_the_whole_batch(memo):
    loci = pc.budget_loci() + pc.ordering_loci()[:2] + pc.cluster_loci()
    _check(memo, loci, modes=[MODES[0], MODES[1], MODES[5]], read_qual=None)


def test_envelope_and_large_instantiations(memo):
    # small instantiations (every locus has at most 64 reads) ...
    _check(memo, pc.envelope_loci() + pc.cluster_loci())
    # ... and, with a locus beyond GT_MAX_READS in the batch (host path, which filters it itself), the large ones
    loci = [pc.oversized_locus()] + pc.envelope_loci() + pc.cluster_loci() + pc.budget_loci()[2:4] + pc.no_majority_loci(n_loci=1)
    b, res = _check(memo, loci, modes=[MODES[0], MODES[1], MODES[5]])
    out = res["host reads"][0]
    assert int((out.read_rank[:300] >= 0).sum()) < 300 and int(out.n_alleles[0]) == 2


def test_purity_jobs_of_every_hmm_class(memo):
    _check(memo, pc.hmm_class_loci(), modes=[MODES[0], MODES[1], MODES[5]])


def test_genotype_flank_behind_the_filter(oracle):
    """alleles at most 10 apart and haplotype tags that split the reads: the flank genotype replaces the length genotype, on the reads
    the filter left (the oracle is given the reads' metadata: test_flank_gpu's comparison)"""
    from test_flank_gpu import _phased_locus
    from trgt_amd import locus
    rng = np.random.default_rng(29)
    loci = [_phased_locus(rng, b"CAG", 20, 21), _phased_locus(rng, b"CAG", 22, 24, n=20, hp_frac=0.9)]
    for L in loci:
        L["read_qual"] = [None if i % 3 else 0.7 for i in range(len(L["reads"]))]
        for i in (1, 6):   # two impure reads: the filter has something to drop
            r = bytearray(L["reads"][i])
            s = r.index(L["left_flank"]) + 250
            for k in range(0, 48, 3):
                r[s + k] = ord("T") if r[s + k] != ord("T") else ord("A")
            L["reads"][i] = bytes(r)
    params = locus.Params(min_read_qual=0.5)
    b = locus.pack(loci)
    refs, changed = [], []
    for L in loci:
        meta = dict(hp_tag=L.get("hp_tag"), start_offset=L["start_offset"], end_offset=L["end_offset"], mismatch_offsets=L["mismatch_offsets"])
        kw = dict(min_read_qual=0.5, read_qual=[np.nan if q is None else q for q in L["read_qual"]])
        refs.append(oracle.locus_analyze(L["left_flank"], L["right_flank"], L["tr"], L["motifs"], L["reads"], meta=meta, **kw))
        plain = oracle.locus_analyze(L["left_flank"], L["right_flank"], L["tr"], L["motifs"], L["reads"], **kw)
        assert len(refs[-1]["kept_read"]) < len(L["reads"])
        changed.append(refs[-1]["alleles"] != plain["alleles"] or list(refs[-1]["classification"]) != list(plain["classification"]))
    assert any(changed)  # (the metadata decides at least one of the two genotypes)
    for how, out in _runs(locus, b, params, MODES):
        for l, ref in enumerate(refs):
            got = locus.locus_result(b, out, l)
            assert [a.seq.decode() for a in got.genotype] == ref["alleles"], (how, l)
            assert got.reads == [int(v) for v in ref["kept_read"]] and got.classification == [int(v) for v in ref["classification"]], (how, l)
            f = got.vcf_fields()
            for k in ("AL", "ALLR", "SD", "MC", "MS", "AP"):
                assert f[k] == ref[k], (how, l, k)
