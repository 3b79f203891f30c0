"""ingest_plan (trgt_amd/csrc/ingest_plan.hpp) is everything the device-side read ingestion decides before it touches a file or the GPU:
windows, compressed ranges, the block table off the BGZF headers, the chunks' places in the inflated bytes, the slab layout, and the lease
that owns a slab.  It compiles without HIP, so its checker (tests/tools/ingest_plan_check.cpp: literal values worked out by hand, one case
per fallback) runs here, on the host compiler.  No GPU needed."""
import ingest_plan_tool


def test_plan_header_builds_without_hip_and_the_checker_passes(tmp_path):
    status, out = ingest_plan_tool.build_and_run(tmp_path)
    assert status == 0, out[-4000:]
    assert out.rstrip().endswith("ingest_plan_check: all held")
    assert "FAILED" not in out


def test_plan_header_includes_nothing_from_hip():
    import os
    import re
    csrc = os.path.join(ingest_plan_tool.ROOT, "trgt_amd", "csrc")
    for name in ("ingest_plan.hpp", "inflate_dev.hpp"):
        includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(os.path.join(csrc, name)).read())
        assert includes and not [i for i in includes if "hip/" in i or i in ("common.hpp", "zlib.h", "fcntl.h", "unistd.h", "fstream", "cstdio")], (name, includes)
