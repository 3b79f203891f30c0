"""writer_format (trgt_amd/csrc/writer_format.hpp) is everything the writer decides about one locus: the VCF line with set_gt and the AM
field, the spanning-BAM record, the order of the kept reads.  It compiles without HIP and without zlib, so its checker
(tests/tools/writer_format_check.cpp: hand-filled batches against literal text and bytes worked out from the reference's rules) runs
here, on the host compiler.  No GPU needed."""
import os
import re

import writer_format_tool


def test_format_header_builds_without_hip_and_the_checker_passes(tmp_path):
    status, out = writer_format_tool.build_and_run(tmp_path)
    assert status == 0, out[-4000:]
    assert out.rstrip().splitlines()[-1] == "writer_format_check: all held"


def test_format_header_includes_nothing_from_hip():
    csrc = os.path.join(writer_format_tool.ROOT, "trgt_amd", "csrc")
    for name, own in (("writer_format.hpp", ["../../include/trgt_hip.h"]), ("bgzf_block.hpp", [])):  # own: the project headers it may read
        with open(os.path.join(csrc, name)) as f:
            includes = re.findall(r'#include\s+([<"][^>"]+)[>"]', f.read())
        assert includes and [i[1:] for i in includes if i[0] == '"'] == own, (name, includes)
        assert not [i for i in includes if "hip/" in i or i[1:] in ("common.hpp", "zlib.h")], (name, includes)
