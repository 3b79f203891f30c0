"""The launches wfa_launch refuses, through the C ABI (trgt_wfa_batch) on a developer context: both workspace-limit messages -- the
second with the bytes one workgroup needs, which is the plan's ws_per_block as tests/tools/wfa_plan_check.cpp prints it for the same
input --, a score scope beyond the descriptor ring, and the parameter errors.  The launcher returns before it takes a buffer: every
result array keeps its sentinel, and the same context then aligns the smallest list of tests/wfa_cases.py, held to tests/pywfa.py."""
import ctypes as C

import numpy as np
import pytest

import wfa_cases as cases
import wfa_plan_tool
from helpers import rand_dna
from test_wfa_independent_gpu import gpu_batch

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, NOMEM = -1, -3, -5
SENT = 0x5A  # every byte of every result array before a call
SMALLEST = min(cases.N_PAIRS, key=cases.N_PAIRS.get)


@pytest.fixture(scope="module")
def lib_mod():
    from trgt_amd import _lib
    assert _lib.lib().trgt_hip_abi_version() == 11
    return _lib


@pytest.fixture(scope="module")
def ctx(lib_mod):
    c = lib_mod.context_with_env(TRGT_WFA_DEBUG=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def W():
    from trgt_amd import wfaligner
    return wfaligner


@pytest.fixture(scope="module")
def plan_rows(tmp_path_factory):
    status, out = wfa_plan_tool.build_and_run(tmp_path_factory.mktemp("wfa_plan"))
    assert status == 0, out[-4000:]
    return wfa_plan_tool.rows(out)


def _params(lib_mod, **kw):
    p = lib_mod.WfaParams()
    lib_mod.lib().trgt_wfa_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _refused(lib_mod, ctx, p, pats, txts):
    """trgt_wfa_batch with all eight result arrays full of the sentinel: (status, message), after checking that none was written"""
    n = len(pats)
    blob = np.frombuffer(b"".join(pats) + b"".join(txts), np.uint8).copy()
    plen, tlen = np.array([len(x) for x in pats], np.uint32), np.array([len(x) for x in txts], np.uint32)
    po, to = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    po[1:] = np.cumsum(plen[:-1], dtype=np.uint64)
    to[1:] = np.cumsum(tlen[:-1], dtype=np.uint64)
    to += np.uint64(int(plen.sum()))
    coff = np.zeros(n + 1, np.uint64)
    coff[1:] = np.cumsum(plen.astype(np.uint64) + tlen.astype(np.uint64) + 1, dtype=np.uint64)
    out = dict(status=np.zeros(n, np.int32), score=np.zeros(n, np.int32), n_match=np.zeros(n, np.int32), span4=np.zeros(4 * n, np.uint32),
               cigar=np.zeros(int(coff[-1]), np.uint32), cigar_len=np.zeros(n, np.uint32), ops=np.zeros(int(coff[-1]), np.uint8), ops_len=np.zeros(n, np.uint32))
    for a in out.values():
        a.view(np.uint8)[:] = SENT
    q = lib_mod.ptr
    rc = lib_mod.lib().trgt_wfa_batch(ctx.handle, C.byref(p), n, q(blob), q(po), q(plen), q(to), q(tlen), q(out["status"]), q(out["score"]), q(out["n_match"]),
                                      q(out["span4"]), q(out["cigar"]), q(coff), q(out["cigar_len"]), q(out["ops"]), q(coff), q(out["ops_len"]))
    for k, a in out.items():
        assert (a.view(np.uint8) == SENT).all(), k
    return rc, lib_mod.lib().trgt_hip_last_error(ctx.handle).decode()


def _still_aligns(W, ctx):
    """the context after an error: the smallest list, every pair exact"""
    assert SMALLEST == "lean_deep"
    cfg = cases.DEEP_CONFIG  # (the register-resident kernels in front, the generic kernel over what they hand on)
    assert cases.verify(SMALLEST, cfg, gpu_batch(W, cfg, cases.pairs(SMALLEST), ctx), "gpu") == cases.N_PAIRS[SMALLEST]


def _two_pairs_of_2000():
    rng = np.random.default_rng(20261020)
    return [rand_dna(rng, 2000) for _ in range(2)], [rand_dna(rng, 2000) for _ in range(2)]


def _set_limit(lib_mod, ctx, n):
    assert lib_mod.lib().trgt_hip_set_workspace_limit(ctx.handle, C.c_uint64(n)) == 0  # (0: the library's default)


def test_workspace_limit_below_what_a_workgroup_needs_beside_its_arena(lib_mod, ctx, W):
    pats, txts = _two_pairs_of_2000()
    _set_limit(lib_mod, ctx, 4096)
    try:
        rc, msg = _refused(lib_mod, ctx, _params(lib_mod, metric=1, span=0, scope=1, memory_mode=0), pats, txts)
    finally:
        _set_limit(lib_mod, ctx, 0)
    assert rc == NOMEM and msg == "wfa: workspace limit 4096 B too small", (rc, msg)
    _still_aligns(W, ctx)


def test_workspace_limit_below_one_workgroup_names_the_plans_bytes(lib_mod, ctx, W, plan_rows):
    pats, txts = _two_pairs_of_2000()
    need = plan_rows["workspace_limit_1mib"]["ws_per_block"]  # the checker's row: edit distance, full history, two pairs of 2 000 + 2 000 bases
    assert plan_rows["workspace_limit_1mib"]["rc"] == NOMEM and need > 1 << 20
    _set_limit(lib_mod, ctx, 1 << 20)
    try:
        rc, msg = _refused(lib_mod, ctx, _params(lib_mod, metric=1, span=0, scope=1, memory_mode=0), pats, txts)
    finally:
        _set_limit(lib_mod, ctx, 0)
    assert rc == NOMEM and msg == "wfa: one workgroup needs %d B of workspace, limit is %d B" % (need, 1 << 20), (rc, msg)
    assert msg == plan_rows["workspace_limit_1mib"]["why"]
    _still_aligns(W, ctx)


@pytest.mark.parametrize("kw,want,message", [
    (dict(metric=3, mismatch=40, gap_open1=6, gap_ext1=2), UNSUPPORTED, "wfa: penalties need a score scope of 41 (> 32)"),
    (dict(metric=5), INVALID, "wfa: bad metric 5"),
    (dict(metric=3, mismatch=2, gap_open1=5, gap_ext1=1, heuristic=2), UNSUPPORTED, "wfa: only Heuristic::None and WFadaptive are implemented"),
    (dict(metric=3, mismatch=2, gap_open1=5, gap_ext1=1, memory_mode=3, span=1), UNSUPPORTED, "wfa: BiWFA is end-to-end only (as used by TRGT)"),
    (dict(metric=3, mismatch=0, gap_open1=5, gap_ext1=1), INVALID, "wfa: penalties must be positive"),
], ids=["score-scope", "bad-metric", "heuristic-2", "biwfa-with-a-span", "zero-mismatch"])
def test_refused_parameters(lib_mod, ctx, W, kw, want, message):
    rng = np.random.default_rng(20261021)
    pats = [rand_dna(rng, 40), rand_dna(rng, 7)]
    rc, msg = _refused(lib_mod, ctx, _params(lib_mod, **kw), pats, [p + rand_dna(rng, 5) for p in pats])
    assert rc == want and msg == message, (rc, msg)
    _still_aligns(W, ctx)
