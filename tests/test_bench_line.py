"""bench.py's stdout contract: ONE compact JSON line below 4 KB that round-trips through json.loads and carries the
driver's keys + roofline + cpu_baseline + parity; everything else goes to the side file.  Driven here from a full record of an earlier
run (profiles/r04last_bench_default.json: the 20 KB line the driver could not keep) -- no GPU needed."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_line", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_contract_line_is_small_and_complete(tmp_path):
    bench = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r04last_bench_default.json")))
    assert len(json.dumps(full)) > 16000   # the record that went unparsed
    path = bench.write_detail(full, str(tmp_path / "bench_detail.json"))
    line = bench.compact_line(full, path)
    assert "\n" not in line and len(line.encode()) < 4096, len(line)
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline", "parity"):
        assert k in d, k
    assert d["value"] == full["value"] and d["ms_per_step"] == full["ms_per_step"] and d["vs_baseline"] is None
    assert d["config"]["baseline_config"] == 2 and d["config"]["workload"].startswith("BASELINE configs[1]")
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_ms", "launches", "algorithmic_bytes_per_launch"):
        assert k in d["roofline"], k
    assert abs(d["roofline"]["frac"] - d["roofline"]["achieved"] / d["roofline"]["peak"]) < 1e-4
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in d["cpu_baseline"], k
    assert d["parity"] == {"parity_checked_loci": 8000, "mismatches": 0}
    assert set(d["configs"]) == {"3", "4", "5"}
    for leg in d["configs"].values():
        assert leg["value"] > 0 and "kernel" in leg["roofline"] and "mismatches" in leg["parity"]
    assert d["e2e"]["pipeline_loci_per_s"] == full["e2e"]["pipeline_loci_per_s"]
    # no prose beyond the workload / sample labels
    assert not any(k in line for k in ("value_is", "launch_is", "algorithmic_bytes_model", '"note"'))
    # the side file holds the whole record
    assert json.load(open(path)) == full


def test_contract_line_says_what_binds():
    # next to the nominal SURVEY 8(d) fraction the line carries, for the headline kernel and for every leg, what actually
    # moves (frac_io_only), what the HBM counters saw as a fraction of peak (frac_traffic, where a PMC profile is committed) and the
    # measured bound; driven from this round's full record (profiles/r06f_bench_detail.json)
    bench = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r06f_bench_detail.json")))
    line = bench.compact_line(full)
    assert len(line.encode()) < 4096, len(line)
    d = json.loads(line)
    r = d["roofline"]
    for k in ("frac", "frac_io_only", "frac_traffic", "valu_issue_frac", "bound_measured", "traffic", "bound"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["bound_measured"] == "valu-issue"
    assert r["frac_io_only"] < r["frac_traffic"] < 0.05 < r["frac"]   # 0.2 % / 0.6 % of peak actually moved; the nominal pricing says 0.8
    assert abs(r["frac_traffic"] - r["traffic"] / (r["avg_launch_ms"] * 1e-3) / 1e9 / r["peak"]) < 1e-4
    for k, leg in d["configs"].items():
        assert "frac_io_only" in leg["roofline"] and "bound_measured" in leg["roofline"], k
    assert "frac_traffic" in d["configs"]["4"]["roofline"]
    e = d["e2e"]
    for k in ("ingest_loci_per_s", "ingest_loci_per_s_host", "pipeline_loci_per_s", "pipeline_loci_per_s_host_ingest", "gpu_loci_per_s", "write_loci_per_s"):
        assert e[k] > 0, k
    assert e["ingest_loci_per_s"] > 2 * e["ingest_loci_per_s_host"] and e["pipeline_loci_per_s"] > 2 * e["pipeline_loci_per_s_host_ingest"] and e["pipeline_vcf_identical"]


def test_contract_line_without_legs_or_baseline():
    bench = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r04last_bench_default.json")))
    for k in ("configs", "e2e", "cpu_baseline", "parity", "cpu_baseline_all_cores"):
        full.pop(k)
    full["multi_gpu_digest_check"] = {"ranks": 2, "shards_recomputed_on_another_gpu": 2, "digest_mismatches": 0}
    d = json.loads(bench.compact_line(full))
    assert d["multi_gpu_digest_check"]["digest_mismatches"] == 0 and "configs" not in d and d["config"]["loci_per_gpu"] == 10000


def test_dumped_outputs_are_what_locus_result_returns(tmp_path):
    # --dump-outputs: the arrays hold, locus by locus, what locus_result() gives a caller; above the size limit, a seeded sample of loci
    import numpy as np
    from trgt_amd import locus, synth
    bench = _bench()
    b = synth.generate(40, first_locus=7)
    nl, nr = int(b["n_loci"]), int(b["n_reads"])
    out = locus.BatchOutputs(b)
    rng = np.random.default_rng(1)
    for a, lo, hi in ((out.n_alleles, 0, 3), (out.allele_blob, 65, 91), (out.n_spans, 0, 4), (out.spans3, 0, 1000), (out.motif_counts, 0, 9),
                      (out.ci, 0, 300), (out.num_spanning, 0, 30), (out.read_rank, -1, 30), (out.classification, 0, 4), (out.span_start, 0, 500),
                      (out.span_end, 500, 1000)):
        a[:] = rng.integers(lo, hi, a.size)
    out.allele_len[:] = rng.integers(0, 9, 2 * nl)
    out.purity[:] = rng.random(2 * nl)
    d = bench.dump_outputs(str(tmp_path / "all"), b, out)
    for k, v in d.items():
        f = np.load(tmp_path / "all" / (k + ".npy"))
        assert f.dtype in (np.float32, np.float64) and np.array_equal(f, v), k
    assert sorted(os.listdir(tmp_path / "all")) == sorted(k + ".npy" for k in d)
    al = sp = mc = s = rd = 0
    for l in range(nl):
        got = locus.locus_result(b, out, l)
        assert d["loci"][l] == l and d["n_alleles"][l] == len(got.genotype)
        for a in got.genotype:
            n, ns, nc = len(a.seq), len(a.annotation.labels or []), len(a.annotation.motif_counts)
            assert d["allele_len"][s] == n and bytes(d["allele_seq"][al:al + n].astype(np.uint8)) == a.seq
            assert tuple(d["allele_ci"][s]) == a.ci and d["allele_num_spanning"][s] == a.num_spanning and d["allele_purity"][s] == a.annotation.purity
            assert d["allele_n_spans"][s] == ns and [tuple(x) for x in d["allele_spans"][sp:sp + ns]] == [(x.motif_index, x.start, x.end) for x in a.annotation.labels or []]
            assert list(d["allele_motif_counts"][mc:mc + nc]) == a.annotation.motif_counts
            al, sp, mc, s = al + n, sp + ns, mc + nc, s + 1
        k = int(b["locus_read_begin"][l + 1]) - int(b["locus_read_begin"][l])
        rank = d["read_rank"][rd:rd + k]
        kept = np.argsort(np.where(rank >= 0, rank, 1 << 30), kind="stable")[:int((rank >= 0).sum())]
        assert list(kept) == got.reads and list(d["read_classification"][rd:rd + k][kept]) == got.classification
        assert list(zip(d["read_span_start"][rd:rd + k][kept], d["read_span_end"][rd:rd + k][kept])) == got.tr_spans
        rd += k
    assert (al, sp, mc, s, rd) == (d["allele_seq"].size, len(d["allele_spans"]), d["allele_motif_counts"].size, d["allele_len"].size, nr)
    # the size limit: a seeded sample of loci, the same in every run
    small = sum(a.nbytes for a in d.values()) // 3
    s1 = bench.dump_outputs(str(tmp_path / "s1"), b, out, limit=small)
    s2 = bench.dump_outputs(str(tmp_path / "s2"), b, out, limit=small)
    assert sum(a.nbytes for a in s1.values()) <= small and 0 < len(s1["loci"]) < nl
    assert all(np.array_equal(s1[k], s2[k]) for k in s1)
