"""The SNV branch of genotype_flank behind the DEEP cluster chain is an addition to ABI 11: two new entry points, declared and documented
in the header of the cluster flank step behind the deep tag pair, listed in a list of the loader's own, generated from a second route
table and wrapped by the Python layers.  No GPU needed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("trgt_hip_set_snv_cluster_deep_device", "trgt_hip_snv_cluster_deep_stats")


def _flat(comment):
    return " ".join(comment.replace("\n *", " ").split())


def test_header_declares_both_functions_behind_the_deep_tag_pair_and_says_what_stays_on_the_host():
    text = open(os.path.join(ROOT, "include", "trgt_hip.h")).read()
    assert not any(n + "(" in re.sub(r"/\*.*?\*/", "", text, flags=re.S) for n in NAMES)  # not in trgt_hip.h's own text (tests/test_abi_exports.py)
    protos = open(os.path.join(ROOT, "include", "trgt_hip_flank_cluster.h")).read()
    m_set = re.search(r"int\s+trgt_hip_set_snv_cluster_deep_device\(trgt_hip_ctx\*\s*ctx,\s*int\s+on\);", protos)
    m_ask = re.search(r"int\s+trgt_hip_snv_cluster_deep_stats\(const trgt_hip_ctx\*\s*ctx,\s*int64_t\s+out\[4\]\);", protos)
    assert m_set and m_ask
    assert protos.index("int trgt_hip_flank_cluster_deep_stats") < m_set.start() < m_ask.start()  # behind the deep tag pair
    over_set = _flat(protos[:m_set.start()].rsplit("/*", 1)[1])
    over_ask = _flat(protos[:m_ask.start()].rsplit("/*", 1)[1])
    assert over_set.endswith("*/") and over_ask.endswith("*/") and over_set != over_ask  # each under a comment of its own
    assert "int trgt_hip_set_snv_cluster_deep_device" not in over_ask
    for says in ("genotype_flank.rs:78-138, 171-290", "tr.rs:64-75", "off by default", "257 to 2048", "trgt_hip_set_cluster_max_reads",
                 "trgt_hip_set_flank_cluster_deep_device"):
        assert says in over_set, says
    for runs in ("mismatch_offsets", "locus_cluster_flank_deep.hpp", "tags first", "2^-30", "member of both", "third consensus round", "reference allele first"):
        assert runs in over_ask, runs
    assert "What stays on the host, with the same results" in over_ask
    for stays in ("not decided beyond the margin", "64 called SNVs", "16 distinct fully observed profiles", "16384", "cluster_max_reads setting", "ceiling",
                  "pair budget", "TRGT_HOST_CLUSTER", "TRGT_HOST_GENOTYPER", "hand-backs", "no room in the deep chain's arenas", "overflows its slot", "allele_cap"):
        assert stays in over_ask, stays
    for counts in ("out[0]", "out[1]", "out[2]", "out[3]", "all zero with the setting off", "without mismatch offsets", "without a deep cluster list",
                   "no other count", "trgt_hip_flank_cluster_deep_stats", "trgt_hip_snv_cluster_stats", "trgt_hip_flank_cluster_stats", "trgt_hip_flank_stats", "stats[23]"):
        assert counts in over_ask, counts


def test_the_older_comments_name_the_new_setting():
    """no comment says that the SNV branch of deep cluster loci is the host's without its `unless`"""
    protos = open(os.path.join(ROOT, "include", "trgt_hip_flank_cluster.h")).read()
    snv = _flat(protos[:protos.index("int trgt_hip_set_snv_cluster_device")].rsplit("/*", 1)[1])
    assert re.search(r"in both branches unless [^;]*trgt_hip_set_flank_cluster_deep_device \(below\)[^;]*trgt_hip_set_snv_cluster_deep_device \(below\)", snv)
    deep = _flat(protos[:protos.index("int trgt_hip_flank_cluster_deep_stats")].rsplit("/*", 1)[1])
    assert re.search(r"get_trs_with_clustering\) for deep cluster loci, [^;]* unless [^;]*trgt_hip_set_snv_cluster_deep_device \(below\)", deep)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "trgt_hip_set_snv_cluster_deep_device" in open(os.path.join(ROOT, doc)).read(), doc


def test_a_program_that_includes_trgt_hip_h_sees_both_prototypes(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    src = tmp_path / "uses.c"
    src.write_text('#include "trgt_hip.h"\n'
                   "int (*set_it)(trgt_hip_ctx*, int) = trgt_hip_set_snv_cluster_deep_device;\n"
                   "int (*ask_it)(const trgt_hip_ctx*, int64_t*) = trgt_hip_snv_cluster_deep_stats;\n")
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_library_exports_them_at_abi_11():
    from trgt_amd import _lib
    L = _lib.lib()
    assert tuple(_lib.CLUSTER_DEEP_SNV_EXPORTS) == NAMES
    assert not set(NAMES) & set(_lib.EXPORTS + _lib.CLUSTER_FLANK_EXPORTS + _lib.CLUSTER_SNV_EXPORTS + _lib.CLUSTER_DEEP_FLANK_EXPORTS)
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.trgt_hip_abi_version() == 11
    src = open(_lib.__file__).read()
    assert "CLUSTER_DEEP_SNV_EXPORTS if not hasattr" in src  # checked at load time like the other lists ...
    assert "EXPORTS + CLUSTER_FLANK_EXPORTS if not hasattr" in src and "CLUSTER_SNV_EXPORTS if not hasattr" in src and "CLUSTER_DEEP_FLANK_EXPORTS if not hasattr" in src


def test_the_route_has_a_table_of_its_own_with_the_row_shape_of_routes():
    from trgt_amd import _lib
    assert [r[0] for r in _lib.ROUTES] == ["flank", "snv_split", "flank_cluster", "flank_cluster_deep", "snv_cluster"]  # the five rows, in their order
    (row,) = _lib.DEEP_SNV_ROUTES
    assert len(row) == len(_lib.ROUTES[0]) and row[:4] == ("snv_cluster_deep",) + NAMES + (4,)
    assert _lib.Context.set_snv_cluster_deep_device.__doc__ == row[4] and _lib.Context.snv_cluster_deep_stats.__doc__ == row[5]
    doc = " ".join(row[4].split())
    assert "off, the default" in doc and "set_cluster_max_reads" in doc and "set_flank_cluster_deep_device" in doc


def test_setter_and_stats_refuse_null_arguments():
    from trgt_amd import _lib
    L = _lib.lib()
    assert L.trgt_hip_set_snv_cluster_deep_device(None, 1) != 0
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    assert L.trgt_hip_snv_cluster_deep_stats(None, out) != 0
    assert list(out) == [7, 7, 7, 7]


def test_python_layers_take_the_setting():
    import inspect
    from trgt_amd import _lib, driver
    for f in (_lib.Pool.__init__, driver.ChunkDriver.__init__):
        params = inspect.signature(f).parameters
        names = list(params)
        assert names[-2:] == ["snv_cluster_deep_device", "snv_cluster_device"]  # directly in front of the last parameter
        assert names[names.index("flank_cluster_device") + 1] == "flank_cluster_deep_device"
        assert params["snv_cluster_deep_device"].default is None
    assert inspect.signature(_lib.Context.set_snv_cluster_deep_device).parameters["on"].default is True
    assert callable(_lib.Context.snv_cluster_deep_stats)
    assert "TRGT_SNV_CLUSTER_DEEP" not in open(_lib.__file__).read()  # no environment switch
    assert not any("SNV" in k for k in _lib.RELEASE_KNOBS)


def test_chunk_driver_passes_the_setting_to_every_context_and_calls_no_other_setter():
    from trgt_amd import driver
    others = ("set_cluster_max_reads", "set_size_max_reads", "set_flank_device", "set_flank_cluster_device", "set_flank_cluster_deep_device", "set_snv_split_device",
              "set_snv_cluster_device")

    class Ctx:
        def __init__(self):
            self.calls = []

        def set_snv_cluster_deep_device(self, on):
            self.calls.append(("set_snv_cluster_deep_device", on))

    for name in others:
        setattr(Ctx, name, lambda self, v, name=name: self.calls.append((name, v)))
    d = driver.ChunkDriver(devices=(0, 0), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None, snv_cluster_deep_device=True)
    assert [c.calls for c in d.contexts] == [[("set_snv_cluster_deep_device", True)]] * 2
    d = driver.ChunkDriver(devices=(0,), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None, cluster_max_reads=2048, snv_cluster_deep_device=False, snv_cluster_device=True)
    assert [c.calls for c in d.contexts] == [[("set_cluster_max_reads", 2048), ("set_snv_cluster_deep_device", False), ("set_snv_cluster_device", True)]]  # applied in its place
    d = driver.ChunkDriver(devices=(0,), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None, flank_cluster_deep_device=True, snv_cluster_device=True)
    assert [c.calls for c in d.contexts] == [[("set_flank_cluster_deep_device", True), ("set_snv_cluster_device", True)]]  # None calls no setter
