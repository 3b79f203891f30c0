"""The SNV branch of genotype_flank behind the one-wave cluster chain is an addition to ABI 11: two new entry points, declared and
documented in the header of the cluster flank step, listed in a list of the loader's own and wrapped by the Python layers.  No GPU needed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("trgt_hip_set_snv_cluster_device", "trgt_hip_snv_cluster_stats")


def test_second_header_declares_both_functions_and_says_what_stays_on_the_host():
    """The prototypes and their comment are in trgt_hip_flank_cluster.h: tests/test_abi_exports.py wants every function of trgt_hip.h's own
    text in _lib.EXPORTS, and tests/test_snv_deep_api.py pins the trgt_hip_*snv* names of that list to two."""
    text = open(os.path.join(ROOT, "include", "trgt_hip.h")).read()
    assert not any(n in re.sub(r"/\*.*?\*/", "", text, flags=re.S) for n in NAMES)
    assert text.index('#include "trgt_hip_flank_cluster.h"') < text.index("int trgt_hip_set_snv_split_device")
    protos = open(os.path.join(ROOT, "include", "trgt_hip_flank_cluster.h")).read()
    assert re.search(r"int\s+trgt_hip_set_snv_cluster_device\(trgt_hip_ctx\*\s*ctx,\s*int\s+on\);", protos)
    assert re.search(r"int\s+trgt_hip_snv_cluster_stats\(const trgt_hip_ctx\*\s*ctx,\s*int64_t\s+out\[4\]\);", protos)
    comment = " ".join(protos[:protos.index("int trgt_hip_set_snv_cluster_device")].rsplit("/*", 1)[1].replace("\n *", " ").split())
    assert comment.endswith("*/") and "trgt_hip_snv_cluster_stats" in comment
    assert "genotype_flank.rs:78-138, 171-290" in comment and "tr.rs:64-75" in comment
    assert "tags first" in comment and "2^-30 * (1 + |log-likelihood|)" in comment
    for limit in ("64 called SNVs", "16 distinct fully observed profiles", "8 in-region mismatch offsets"):
        assert limit in comment, limit
    for stays in ("deep cluster loci", "trgt_hip_set_cluster_max_reads", "TRGT_HOST_CLUSTER", "TRGT_HOST_GENOTYPER", "not decided beyond the margin", "the chain's arenas",
                  "overflows its slot", "allele_cap", "trgt_hip_set_flank_cluster_device is off"):
        assert stays in comment, stays


def test_a_program_that_includes_trgt_hip_h_sees_both_prototypes(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    src = tmp_path / "uses.c"
    src.write_text('#include "trgt_hip.h"\n'
                   "int (*set_it)(trgt_hip_ctx*, int) = trgt_hip_set_snv_cluster_device;\n"
                   "int (*ask_it)(const trgt_hip_ctx*, int64_t*) = trgt_hip_snv_cluster_stats;\n")
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_library_exports_them_at_abi_11():
    from trgt_amd import _lib
    L = _lib.lib()
    assert tuple(_lib.CLUSTER_SNV_EXPORTS) == NAMES
    assert not set(NAMES) & set(_lib.EXPORTS + _lib.CLUSTER_FLANK_EXPORTS)
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.trgt_hip_abi_version() == 11
    assert "CLUSTER_SNV_EXPORTS if not hasattr" in open(_lib.__file__).read()  # checked at load time like the other two lists


def test_setter_and_stats_refuse_a_null_context():
    from trgt_amd import _lib
    L = _lib.lib()
    assert L.trgt_hip_set_snv_cluster_device(None, 1) != 0
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    assert L.trgt_hip_snv_cluster_stats(None, out) != 0
    assert list(out) == [7, 7, 7, 7]


def test_python_layers_take_the_setting():
    import inspect
    from trgt_amd import _lib, driver
    for f in (_lib.Pool.__init__, driver.ChunkDriver.__init__):
        params = inspect.signature(f).parameters
        assert list(params)[-1] == "snv_cluster_device" and params["snv_cluster_device"].default is None
    assert inspect.signature(_lib.Context.set_snv_cluster_device).parameters["on"].default is True
    assert callable(_lib.Context.snv_cluster_stats)
    assert "TRGT_SNV_CLUSTER" not in open(_lib.__file__).read()  # no environment switch


def test_chunk_driver_passes_the_setting_to_every_context_and_leaves_the_others_alone():
    from trgt_amd import driver
    others = ("set_cluster_max_reads", "set_size_max_reads", "set_flank_device", "set_flank_cluster_device", "set_snv_split_device")

    class Ctx:
        def __init__(self):
            self.calls = []

        def set_snv_cluster_device(self, on):
            self.calls.append(("set_snv_cluster_device", on))

    for name in others:
        setattr(Ctx, name, lambda self, v, name=name: self.calls.append((name, v)))
    d = driver.ChunkDriver(devices=(0, 0), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None, snv_cluster_device=True)
    assert [c.calls for c in d.contexts] == [[("set_snv_cluster_device", True)]] * 2
    d = driver.ChunkDriver(devices=(0,), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None, snv_split_device=True, flank_cluster_device=False)
    assert [c.calls for c in d.contexts] == [[("set_flank_cluster_device", False), ("set_snv_split_device", True)]]
    d = driver.ChunkDriver(devices=(0,), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None)
    assert [c.calls for c in d.contexts] == [[]]
