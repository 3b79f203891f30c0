"""The HMM kernels held to tests/pyhmm.py -- the restatement written from the reference's src/hmm/*.rs alone -- and to exact
arithmetic, never to the CPU oracle and never to another context of the library.  Per job, bit for bit: state path, spans, n_spans,
motif counts, edit and max distance, the f64 purity as uint64 bits; and for every job of up to 50 000 states x columns the GPU's OWN
path must be a walk along existing edges over the whole query whose exact score is within 8 len(path) 2^-53 |S*| of the exact optimum
S* of the model's f64 tables (hmm_cases.path_bound: derived, not measured).

The lists (tests/hmm_cases.py, the same ones tests/test_hmm_independent.py holds the oracle to) are the smallest shapes at which each
path of trgt_hmm_batch can still go wrong: the position-per-lane fill at 8 / 16 / 32 / 64 lanes and one position past it, the
256-column window, several alleles per wave; the one-wave register fill, the four-round loop, the LDS fill and the one-byte rows
through developer contexts; a multi-wave model; the 1 024-thread kernel at 458, 1 025, 1 517 and 4 094 states; the staged trace-back
(512 columns) and the chunk-map one (1 536) and the latter switched off; lists made for exact ties.  pyhmm's answers are computed
once per process and shared."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_cases as HC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hmm():
    from trgt_amd import hmm as H
    return H


def _hold(H, names, env=None):
    """run the lists `names` as ONE batch (in the context made with `env`, if any) and hold every job to pyhmm"""
    from trgt_amd import _lib
    sets, jobs, refs = [], [], []
    for name in names:
        s, j = HC.group(name)
        jobs += [(len(sets) + k, a) for k, a in j]
        sets += [list(m) for m in s]
        refs += HC.reference(name)
    batch = H.pack_hmm_batch(sets, jobs)
    ctx = _lib.context_with_env(**env) if env else None
    try:
        out = H.hmm_batch(batch, ctx=ctx)
    finally:
        if ctx is not None:
            ctx.close()
    return HC.check_batch(batch, out, refs, (names, env))


def test_position_per_lane_fill(hmm):
    assert [hmm.num_states(s) for s in HC.group("ppl")[0]][:8] == [17, 29, 32, 56, 101, 104, 197, 200]
    assert _hold(hmm, ("ppl", "window")) >= 100


@pytest.mark.parametrize("env", [dict(TRGT_HMM_NO_PPL=1), dict(TRGT_HMM_NO_PPL=1, TRGT_HMM_FOUR_ROUNDS=1),
                                 dict(TRGT_HMM_NO_PPL=1, TRGT_HMM_LDS_FILL=1), dict(TRGT_HMM_PPL_WIDE=1)],
                         ids=["register-fill", "four-rounds", "lds-fill", "ppl-wide-rows"])
def test_same_batch_through_developer_contexts(hmm, env):
    assert _hold(hmm, ("ppl", "window"), env) >= 100


def test_multi_wave_model(hmm):
    assert hmm.num_states(HC.RFC1) == 173  # three waves of lanes
    assert _hold(hmm, ("multiwave",)) == 2  # (333 bases are past the budget of the exact check)


def test_large_set_kernel(hmm):
    sets, jobs = HC.group("large")
    assert [hmm.num_states(s) for s in sets] == [458, 1025, 4094, 1517]
    assert all(60 <= len(a) <= 300 and hmm.num_states(sets[s]) * (len(a) + 2) <= 1_300_000 for s, a in jobs)
    _hold(hmm, ("large",))


@pytest.mark.parametrize("env", [None, dict(TRGT_HMM_NO_LONG_TB=1)], ids=["default", "no-chunk-map"])
def test_trace_backs(hmm, env):
    assert _hold(hmm, ("traceback",), env) == 8  # (all but the two-motif set at 1 540 bases: 37 states x 1 542 columns)


@pytest.mark.parametrize("env", [None, dict(TRGT_HMM_NO_PPL=1)], ids=["default", "state-fill"])
def test_tie_lists(hmm, env):
    refs = [r for name in HC.TIE_GROUPS for r in HC.reference(name)]
    assert _hold(hmm, HC.TIE_GROUPS, env) == sum(1 for r in refs if r["seq"])
