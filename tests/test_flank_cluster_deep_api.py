"""The haplotype-tag branch of genotype_flank behind the DEEP cluster chain is an addition to ABI 11: two new entry points, declared and
documented in the header of the cluster flank step behind the SNV pair, listed in a list of the loader's own and wrapped by the Python
layers.  No GPU needed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("trgt_hip_set_flank_cluster_deep_device", "trgt_hip_flank_cluster_deep_stats")


def _flat(comment):
    return " ".join(comment.replace("\n *", " ").split())


def test_header_declares_both_functions_behind_the_snv_pair_and_says_what_stays_on_the_host():
    """The prototypes and their comments are in trgt_hip_flank_cluster.h, not in trgt_hip.h's own text: tests/test_abi_exports.py wants
    every function of that text in _lib.EXPORTS, and tests/test_flank_deep_api.py pins the trgt_hip_*flank* names of that list to two."""
    text = open(os.path.join(ROOT, "include", "trgt_hip.h")).read()
    assert not any(n + "(" in re.sub(r"/\*.*?\*/", "", text, flags=re.S) for n in NAMES)
    protos = open(os.path.join(ROOT, "include", "trgt_hip_flank_cluster.h")).read()
    m_set = re.search(r"int\s+trgt_hip_set_flank_cluster_deep_device\(trgt_hip_ctx\*\s*ctx,\s*int\s+on\);", protos)
    m_ask = re.search(r"int\s+trgt_hip_flank_cluster_deep_stats\(const trgt_hip_ctx\*\s*ctx,\s*int64_t\s+out\[3\]\);", protos)
    assert m_set and m_ask
    assert protos.index("int trgt_hip_snv_cluster_stats") < m_set.start() < m_ask.start()  # behind the SNV pair
    # each under a comment of its own
    over_set = _flat(protos[:m_set.start()].rsplit("/*", 1)[1])
    over_ask = _flat(protos[:m_ask.start()].rsplit("/*", 1)[1])
    assert over_set.endswith("*/") and over_ask.endswith("*/") and over_set != over_ask
    assert "int trgt_hip_set_flank_cluster_deep_device" not in over_ask
    assert "genotype_flank.rs:9-76, 147-170" in over_set and "tr.rs:64-75" in over_set and "off by default" in over_set
    assert "trgt_hip_set_cluster_max_reads" in over_set and "257 to 2048" in over_set
    # what runs on the device ...
    for runs in ("hp_tag", "locus_cluster_flank_deep.hpp", "assignment by tag", "simple_consensus", "third consensus round", "reference allele first"):
        assert runs in over_ask, runs
    # ... and what stays on the host, with the same results
    assert "What stays on the host, with the same results" in over_ask
    for stays in ("get_trs_with_clustering", "cluster_max_reads setting", "ceiling", "pair budget", "TRGT_HOST_CLUSTER", "TRGT_HOST_GENOTYPER", "hand-backs",
                  "no room in the deep chain's arenas", "overflows its slot", "allele_cap"):
        assert stays in over_ask, stays
    for counts in ("out[0]", "out[1]", "out[2]", "all zero with the setting off", "without hp_tag", "without a deep cluster list", "no other count",
                   "trgt_hip_flank_cluster_stats", "trgt_hip_flank_stats", "stats[23]"):
        assert counts in over_ask, counts


def test_the_two_older_comments_point_to_the_new_setting():
    text = open(os.path.join(ROOT, "include", "trgt_hip.h")).read()
    older = _flat(text[:text.index('#include "trgt_hip_flank_cluster.h"')].rsplit("/*", 1)[1])
    assert re.search(r"deep cluster loci \(257 to 2048 reads on a context set with trgt_hip_set_cluster_max_reads\), which the host redoes as before "
                     r"unless [^;]*trgt_hip_set_flank_cluster_deep_device[^;]*\(trgt_hip_flank_cluster\.h, below\)", older)
    protos = open(os.path.join(ROOT, "include", "trgt_hip_flank_cluster.h")).read()
    snv = _flat(protos[:protos.index("int trgt_hip_set_snv_cluster_device")].rsplit("/*", 1)[1])
    assert re.search(r"deep cluster loci \(257 to 2048 reads on a context set with trgt_hip_set_cluster_max_reads\), in both branches "
                     r"unless [^;]*trgt_hip_set_flank_cluster_deep_device \(below\)", snv)


def test_a_program_that_includes_trgt_hip_h_sees_both_prototypes(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    src = tmp_path / "uses.c"
    src.write_text('#include "trgt_hip.h"\n'
                   "int (*set_it)(trgt_hip_ctx*, int) = trgt_hip_set_flank_cluster_deep_device;\n"
                   "int (*ask_it)(const trgt_hip_ctx*, int64_t*) = trgt_hip_flank_cluster_deep_stats;\n")
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_library_exports_them_at_abi_11():
    from trgt_amd import _lib
    L = _lib.lib()
    assert tuple(_lib.CLUSTER_DEEP_FLANK_EXPORTS) == NAMES
    assert not set(NAMES) & set(_lib.EXPORTS + _lib.CLUSTER_FLANK_EXPORTS + _lib.CLUSTER_SNV_EXPORTS)
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.trgt_hip_abi_version() == 11
    src = open(_lib.__file__).read()
    assert "CLUSTER_DEEP_FLANK_EXPORTS if not hasattr" in src  # checked at load time like the other lists ...
    assert "EXPORTS + CLUSTER_FLANK_EXPORTS if not hasattr" in src and "CLUSTER_SNV_EXPORTS if not hasattr" in src  # ... which are still checked


def test_setter_and_stats_refuse_a_null_context():
    from trgt_amd import _lib
    L = _lib.lib()
    assert L.trgt_hip_set_flank_cluster_deep_device(None, 1) != 0
    out = (C.c_int64 * 3)(7, 7, 7)
    assert L.trgt_hip_flank_cluster_deep_stats(None, out) != 0
    assert list(out) == [7, 7, 7]


def test_python_layers_take_the_setting():
    import inspect
    from trgt_amd import _lib, driver
    for f in (_lib.Pool.__init__, driver.ChunkDriver.__init__):
        params = inspect.signature(f).parameters
        names = list(params)
        assert names[names.index("flank_cluster_device") + 1] == "flank_cluster_deep_device"  # directly behind it
        assert params["flank_cluster_deep_device"].default is None
        assert names[-1] == "snv_cluster_device"
    assert inspect.signature(_lib.Context.set_flank_cluster_deep_device).parameters["on"].default is True
    assert callable(_lib.Context.flank_cluster_deep_stats)
    assert "TRGT_FLANK_CLUSTER_DEEP" not in open(_lib.__file__).read()  # no environment switch
    assert not any("FLANK" in k for k in _lib.RELEASE_KNOBS)


def test_chunk_driver_passes_the_setting_to_every_context_and_calls_no_other_setter():
    from trgt_amd import driver
    others = ("set_cluster_max_reads", "set_size_max_reads", "set_flank_device", "set_flank_cluster_device", "set_snv_split_device", "set_snv_cluster_device")

    class Ctx:
        def __init__(self):
            self.calls = []

        def set_flank_cluster_deep_device(self, on):
            self.calls.append(("set_flank_cluster_deep_device", on))

    for name in others:
        setattr(Ctx, name, lambda self, v, name=name: self.calls.append((name, v)))
    d = driver.ChunkDriver(devices=(0, 0), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None, flank_cluster_deep_device=True)
    assert [c.calls for c in d.contexts] == [[("set_flank_cluster_deep_device", True)]] * 2
    d = driver.ChunkDriver(devices=(0,), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None, cluster_max_reads=2048, flank_cluster_deep_device=False)
    assert [c.calls for c in d.contexts] == [[("set_cluster_max_reads", 2048), ("set_flank_cluster_deep_device", False)]]
    d = driver.ChunkDriver(devices=(0,), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None, flank_cluster_device=True, snv_cluster_device=True)
    assert [c.calls for c in d.contexts] == [[("set_flank_cluster_device", True), ("set_snv_cluster_device", True)]]  # None calls no setter
