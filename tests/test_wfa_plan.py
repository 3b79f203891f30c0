"""wfa_plan (trgt_amd/csrc/wfa_plan.hpp) is everything wfa_launch decides before it touches the device.  It compiles without HIP, so its
checker (tests/tools/wfa_plan_check.cpp: invariants of the workspace layout and the routes over a sweep of inputs, the routes of the
launches the project makes, every refused launch with its code and message) runs here, on the host compiler.  No GPU needed."""
import wfa_plan_tool


def test_plan_header_builds_without_hip_and_the_checker_passes(tmp_path):
    status, out = wfa_plan_tool.build_and_run(tmp_path)
    assert status == 0, out[-4000:]
    assert out.rstrip().endswith("wfa_plan_check: all held")
    rows = wfa_plan_tool.rows(out)
    # (what the GPU error test reads)
    assert rows["workspace_limit_1mib"]["rc"] == -5 and rows["workspace_limit_1mib"]["ws_per_block"] > 1 << 20
    assert rows["workspace_limit_1mib"]["ws_per_block"] == rows["workspace_limit_default"]["ws_per_block"]
    assert rows["windowed_64"]["fast_koff"] == 15 + 4 and rows["bad_metric"]["why"] == "wfa: bad metric 5"


def test_plan_header_includes_nothing_from_hip():
    import os
    import re
    csrc = os.path.join(wfa_plan_tool.ROOT, "trgt_amd", "csrc")
    for name in ("wfa_plan.hpp", "wfa_types.hpp"):
        includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(os.path.join(csrc, name)).read())
        assert includes and not [i for i in includes if "hip/" in i or i in ("common.hpp", "wfa_host.hpp", "wfa_engine.hpp")], (name, includes)
