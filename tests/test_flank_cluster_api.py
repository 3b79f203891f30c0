"""The haplotype-tag branch of genotype_flank behind the one-wave cluster chain is an addition to ABI 11: two new entry points, declared
in the header, listed in the loader's exports and wrapped by the Python layers.  No GPU needed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("trgt_hip_set_flank_cluster_device", "trgt_hip_flank_cluster_stats")


def test_header_declares_both_functions_and_says_what_stays_on_the_host():
    """The comment is in trgt_hip.h; the two prototypes are in trgt_hip_flank_cluster.h, which trgt_hip.h includes right behind the comment
    (tests/test_abi_exports.py wants every function of trgt_hip.h's own text in _lib.EXPORTS, and tests/test_flank_deep_api.py pins the
    trgt_hip_*flank* names of that list to two)."""
    text = open(os.path.join(ROOT, "include", "trgt_hip.h")).read()
    inc = '#include "trgt_hip_flank_cluster.h"'
    assert text.count(inc) == 1
    protos = open(os.path.join(ROOT, "include", "trgt_hip_flank_cluster.h")).read()
    assert re.search(r"int\s+trgt_hip_set_flank_cluster_device\(trgt_hip_ctx\*\s*ctx,\s*int\s+on\);", protos)
    assert re.search(r"int\s+trgt_hip_flank_cluster_stats\(const trgt_hip_ctx\*\s*ctx,\s*int64_t\s+out\[3\]\);", protos)
    comment = text[:text.index(inc)].rsplit("/*", 1)[1]
    assert comment.rstrip().endswith("*/") and all(n in comment for n in NAMES)
    assert "genotype_flank.rs:9-76, 147-170" in comment and "tr.rs:64-75" in comment
    for stays in ("get_trs_with_clustering", "trgt_hip_set_cluster_max_reads", "TRGT_HOST_CLUSTER", "TRGT_HOST_GENOTYPER", "allele_cap"):
        assert stays in comment, stays
    # the setting of the size genotyper keeps its declaration and its comment
    older = text[:text.index("int trgt_hip_set_flank_device")].rsplit("/*", 1)[1]
    assert "genotype_flank.rs:43-76" in older and "tr.rs:69-75" in older and "get_trs_with_clustering" in older


def test_a_program_that_includes_trgt_hip_h_sees_both_prototypes(tmp_path):
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "no C compiler"
    src = tmp_path / "uses.c"
    src.write_text('#include "trgt_hip.h"\n'
                   "int (*set_it)(trgt_hip_ctx*, int) = trgt_hip_set_flank_cluster_device;\n"
                   "int (*ask_it)(const trgt_hip_ctx*, int64_t*) = trgt_hip_flank_cluster_stats;\n")
    r = subprocess.run([cc, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_library_exports_them_at_abi_11():
    """The loader checks them at load time like every name of EXPORTS, from a list of its own: tests/test_flank_deep_api.py pins the
    trgt_hip_*flank* names inside EXPORTS to the two of trgt_hip_set_flank_device."""
    from trgt_amd import _lib
    L = _lib.lib()
    assert tuple(_lib.CLUSTER_FLANK_EXPORTS) == NAMES
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.trgt_hip_abi_version() == 11
    src = open(_lib.__file__).read()
    assert "EXPORTS + CLUSTER_FLANK_EXPORTS if not hasattr" in src


def test_setter_and_stats_refuse_a_null_context():
    from trgt_amd import _lib
    L = _lib.lib()
    assert L.trgt_hip_set_flank_cluster_device(None, 1) != 0
    out = (C.c_int64 * 3)(7, 7, 7)
    assert L.trgt_hip_flank_cluster_stats(None, out) != 0
    assert list(out) == [7, 7, 7]


def test_python_layers_take_the_setting():
    import inspect
    from trgt_amd import _lib, driver
    assert inspect.signature(_lib.Pool.__init__).parameters["flank_cluster_device"].default is None
    assert inspect.signature(driver.ChunkDriver.__init__).parameters["flank_cluster_device"].default is None
    assert inspect.signature(_lib.Context.set_flank_cluster_device).parameters["on"].default is True
    assert callable(_lib.Context.flank_cluster_stats)


def test_chunk_driver_passes_the_setting_to_every_context_and_keeps_the_two_apart():
    from trgt_amd import driver

    class Ctx:
        def __init__(self):
            self.flank = self.flank_cluster = None

        def set_flank_device(self, on):
            self.flank = on

        def set_flank_cluster_device(self, on):
            self.flank_cluster = on

    d = driver.ChunkDriver(devices=(0, 0), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None, flank_cluster_device=True)
    assert [(c.flank, c.flank_cluster) for c in d.contexts] == [(None, True), (None, True)]
    d = driver.ChunkDriver(devices=(0,), context_factory=lambda dev: Ctx(), run_fn=lambda *a: None, flank_device=True)
    assert [(c.flank, c.flank_cluster) for c in d.contexts] == [(True, None)]
