"""The wavefront kernels (trgt_wfa_batch, trgt_flank_filter_batch, trgt_find_spans_batch) against tests/pywfa.py on the lists of
tests/wfa_cases.py -- never against the oracle, never against another context.  tests/test_wfa_independent.py holds the oracle to
the same restatement on the same lists.

Every test shows that its list ran where it was meant to run: the launcher's TRGT_WFA_DEBUG lines of a developer context, read with
capfd -- "[wfa] fast kernel ... threads=N" (the dedicated gap-affine kernel), "[wfa] lean kernels: ..." with the per-tier reasons
(the register-resident BiWFA kernels), "[wfa] LDS-arena variant: ..." and the "[spans]" lines of flank location."""
import re

import pytest

import pywfa
import wfa_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def W():
    from trgt_amd import wfaligner
    return wfaligner


@pytest.fixture(scope="module")
def contexts():
    """developer contexts by their switches, created on demand and closed with the module"""
    from trgt_amd import _lib
    made = {}

    def get(**env):
        key = tuple(sorted(env.items()))
        if key not in made:
            made[key] = _lib.context_with_env(TRGT_WFA_DEBUG=1, **env)
        return made[key]

    yield get
    for c in made.values():
        c.close()


def gpu_batch(W, cfg, pairs, ctx):
    b = W.WFAligner.builder(W.AlignmentScope.Alignment if cfg.scope == "alignment" else W.AlignmentScope.Score,
                            {"high": W.MemoryModel.MemoryHigh, "ultralow": W.MemoryModel.MemoryUltraLow}[cfg.memory])
    b = {"indel": lambda: b.indel(), "edit": lambda: b.edit(), "linear": lambda: b.linear(*cfg.pen), "affine": lambda: b.affine(*cfg.pen),
         "affine2p": lambda: b.affine2p(*cfg.pen)}[cfg.metric]()
    if cfg.heuristic == "none":
        b = b.with_heuristic(W.Heuristic.none())
    al = b.build(ctx)
    p = al._params(cfg.span, *cfg.free)
    p.bialign_min_length, p.bialign_min_score = cfg.min_length, cfg.min_score
    return al._run_batch(p, [a for a, _ in pairs], [t for _, t in pairs], want_ops=cfg.want_ops)


def run(W, name, cfg, ctx):
    return C.verify(name, cfg, gpu_batch(W, cfg, C.pairs(name), ctx), "gpu")


def fast_lines(err):
    """thread counts of the launches of the dedicated gap-affine kernel"""
    return [int(m.group(1)) for m in re.finditer(r"^\[wfa\] fast kernel .* threads=(\d+)$", err, re.M)]


def lean_lines(err):
    """per launch of the register-resident kernels: dict(second, third, generic, lost, tiers = three dicts of hand-over reasons)"""
    out = []
    for line in err.splitlines():
        m = re.match(r"\[wfa\] lean kernels: metric (\d+), (\d+) jobs at most, (\d+) went on to the second tier, (\d+) to the third, (\d+) to the generic kernel \((\d+) lost\)", line)
        if m:
            out.append(dict(metric=int(m.group(1)), second=int(m.group(3)), third=int(m.group(4)), generic=int(m.group(5)), lost=int(m.group(6)), tiers=[]))
        m = re.match(r"\[wfa\]   tier (\d) handed on: lengths (\d+), window (\d+), range (\d+), history levels (\d+), history cells (\d+), runs (\d+), stack (\d+), status (\d+)", line)
        if m:
            out[-1]["tiers"].append(dict(zip(("lengths", "window", "range", "levels", "cells", "runs", "stack", "status"), map(int, m.groups()[1:]))))
    return out


def dedicated(cfg):
    """wfa_launch's condition for the dedicated kernel, the LDS bound aside"""
    return cfg.metric == "affine" and cfg.heuristic == "none" and cfg.memory != "ultralow"


# ------------------------------------------------------------------------------------------- every metric, every span, both scopes
@pytest.mark.parametrize("metric,pen", C.PENALTY_SETS, ids=["%s%s" % (m, "-".join(map(str, p))) for m, p in C.PENALTY_SETS])
def test_every_metric_and_span(W, contexts, capfd, metric, pen):
    """indel, edit, gap-linear, eight gap-affine and two two-piece sets x end-to-end, text free, three partly free spans, on the
    shape and free-end lists; the gap-affine sets run on the dedicated kernel (one wave end to end, four ends-free; (2,5,1) with the
    text free: the flank specialisation), everything else on the generic kernel"""
    ctx = contexts()
    want = []
    capfd.readouterr()
    for name, cfg in C.METRIC_PLAN:
        if (cfg.metric, cfg.pen) == (metric, tuple(pen)):
            done = run(W, name, cfg, ctx)
            assert cfg.heuristic != "none" or done == C.N_PAIRS[name]
            if dedicated(cfg):
                want.append(64 if cfg.span == "end2end" else 256)
    assert fast_lines(capfd.readouterr().err) == want


def test_dedicated_kernel_flank_shape_ties_and_its_fallback(W, contexts, capfd):
    """(2,5,1) with the text free on 250-base pieces -- the 256-thread flank specialisation -- and on the tie lists, the same through the
    general instantiation (TRGT_WFA_NO_SPEC), with and without expanded operations; a batch whose longest pair does not fit the
    dedicated kernel's LDS runs on the generic kernel, short pairs and all"""
    flank = C.config("affine", (2, 5, 1), C.TEXT_FREE)
    for env in ({}, dict(TRGT_WFA_NO_SPEC=1)):
        capfd.readouterr()
        for name in ("flank_shape",) + C.TIE_LISTS:
            assert run(W, name, flank, contexts(**env)) == C.N_PAIRS[name]
            assert run(W, name, flank._replace(want_ops=False), contexts(**env)) == C.N_PAIRS[name]
        assert fast_lines(capfd.readouterr().err) == [256] * 6
    capfd.readouterr()
    for cfg in (C.config("affine", (2, 5, 1)), C.config("affine", (4, 6, 2)), flank):
        assert run(W, "too_long_for_lds", cfg, contexts()) == 15
    assert fast_lines(capfd.readouterr().err) == []


# ------------------------------------------------------------------------------------------------ the register-resident BiWFA kernels
def _beyond(name, limit):
    return sum(abs(len(t) - len(p)) > limit for p, t in C.pairs(name))


def _empty(name):
    return sum(len(p) == 0 or len(t) == 0 for p, t in C.pairs(name))


def test_register_resident_biwfa(W, contexts, capfd):
    """want_ops = False, edit and gap-affine (2,5,1), with and without the heuristic, bialign_min_length 100 and 0: the lean kernels.
    A tier takes no pair whose lengths differ by more than its window allows (55 / 247) and none with an empty sequence; what is past
    the last tier's window reaches the generic kernel; nothing is lost"""
    ctx = contexts()
    for cfg in C.lean_configs():
        for name in C.LEAN_LISTS:
            capfd.readouterr()
            res = gpu_batch(W, cfg, C.pairs(name), ctx)
            C.verify(name, cfg, res, "gpu")
            (line,) = lean_lines(capfd.readouterr().err)
            t1, t3 = line["tiers"][0], line["tiers"][2]
            assert line["lost"] == 0
            assert t1["window"] == _beyond(name, 55) and t1["lengths"] == _empty(name), (name, line)
            assert line["second"] == sum(t1.values()) and line["third"] == 0, (name, line)       # (no middle tier unless asked for)
            assert t3["window"] == _beyond(name, 247) and line["generic"] == sum(t3.values()) >= _beyond(name, 247) + _empty(name), (name, line)
            if name == "lean_runs" and cfg.scope == "alignment":   # more than RLE_CAP runs: no tier keeps them (the narrow one gives them up sooner, for its
                long_ = int((res["cigar_len"] > 80).sum())         # window or its history), the last one for the runs, the generic kernel finishes them
                assert long_ >= 4 and t3["runs"] == long_ == line["generic"] and line["second"] >= long_, (long_, line)
            if name == "lean_lengths":   # penalties of 11 at most, lengths within two bases: wavefronts of a dozen diagonals -- the first tier's own
                assert line["second"] == 0, (name, line)


def test_register_resident_biwfa_middle_tier(W, contexts, capfd):
    """TRGT_WFA_LEAN_MID_TIER=1: the tier of 128 diagonals between the two, limit 119"""
    ctx = contexts(TRGT_WFA_LEAN_MID_TIER=1)
    for cfg in C.lean_configs()[:4]:
        for name in ("lean_tier1", "lean_tier2", "lean_tier3"):
            capfd.readouterr()
            run(W, name, cfg, ctx)
            (line,) = lean_lines(capfd.readouterr().err)
            assert line["lost"] == 0 and line["tiers"][0]["window"] == _beyond(name, 55)
            assert line["tiers"][1]["window"] == _beyond(name, 119) and line["tiers"][2]["window"] == _beyond(name, 247)
            assert line["third"] == sum(line["tiers"][1].values())


def test_deep_split_recursion(W, contexts, capfd):
    """bialign_min_score = 2, bialign_min_length = 0: the recursion splits down to single differences, seven levels deep on 70 to 130
    differences.  The lean kernels' stack of 12 entries cannot be outrun through the public parameters -- a left spine of eleven splits
    needs a penalty beyond 4 000, and a tier gives a pair up for its window (a penalty of 250 or so) and its 80 runs long before -- so
    what this list pins is the hand-over: every pair goes on to the generic kernel (stack of 48), nothing is lost"""
    capfd.readouterr()
    assert run(W, "lean_deep", C.DEEP_CONFIG, contexts()) == 3
    run(W, "lean_deep", C.DEEP_CONFIG._replace(heuristic="default"), contexts())
    lines = lean_lines(capfd.readouterr().err)
    assert len(lines) == 2 and all(l["lost"] == 0 and l["generic"] == 3 for l in lines), lines


@pytest.mark.parametrize("env", [dict(TRGT_WFA_NO_LEAN=1), dict(TRGT_WFA_NO_LEAN=1, TRGT_WFA_LDS=1, TRGT_WFA_LDS_KB=3),
                                 dict(TRGT_WFA_NO_LEAN=1, TRGT_WFA_LDS=1, TRGT_WFA_LDS_KB=18), dict(TRGT_WFA_NO_LEAN=1, TRGT_WFA_NO_WAVE_VARIANT=1)],
                         ids=["no-lean", "lds-3k", "lds-18k", "no-wave-variant"])
def test_generic_kernels_without_operations(W, contexts, capfd, env):
    """the same lists without the lean kernels in front: the one-wave generic kernel, its LDS-arena variant with a small and a large
    arena (what does not fit goes on to the HBM variant), and the multi-wave code on one wave"""
    ctx = contexts(**env)
    capfd.readouterr()
    n = 0
    for cfg in C.lean_configs():
        for name in C.LEAN_LISTS:
            run(W, name, cfg, ctx)
            n += 1
    assert run(W, "lean_deep", C.DEEP_CONFIG, ctx) == 3
    err = capfd.readouterr().err
    assert not lean_lines(err)
    went_on = [int(m.group(1)) for m in re.finditer(r"^\[wfa\] LDS-arena variant: metric \d+, \d+ jobs at most, (\d+) went on to the HBM variant$", err, re.M)]
    if "TRGT_WFA_LDS" in env:
        assert len(went_on) == n + 1
        assert sum(went_on) > 0 if env["TRGT_WFA_LDS_KB"] == 3 else sum(went_on) < sum(C.N_PAIRS[x] for x in C.LEAN_LISTS) * len(C.lean_configs())
    else:
        assert not went_on


@pytest.mark.parametrize("env", [{}, dict(TRGT_WFA_NO_WAVE_VARIANT=1)], ids=["wave-variant", "no-wave-variant"])
def test_generic_kernels_with_operations(W, contexts, capfd, env):
    """with expanded operations no lean kernel runs: the one-wave variant of the generic kernel, and the multi-wave code through the
    developer switch that turns the variant off; BiWFA penalties above bialign_min_score = 250 among them"""
    ctx = contexts(**env)
    capfd.readouterr()
    for cfg in C.lean_configs(want_ops=True):
        for name in C.LEAN_LISTS:
            done = run(W, name, cfg, ctx)
            if name == "biwfa_high" and cfg.scope == "alignment" and cfg.heuristic == "none":
                best = C.answers(name, cfg.metric, cfg.pen, cfg.span, cfg.free)
                assert done == 6 and (cfg.metric == "edit" or sum(b > 250 for b in best) >= 3)
    assert run(W, "lean_deep", C.DEEP_CONFIG._replace(want_ops=True), ctx) == 3
    err = capfd.readouterr().err
    assert not lean_lines(err) and not fast_lines(err)


# ------------------------------------------------------------------------------------------------------------- flank location
def _filter_thresholds(ans, threshold):
    """the acceptance threshold itself, and the low end, the high end and the high end + 1 of the first brackets that hold more than one value"""
    out = [threshold]
    for _, lo, hi, _ in [a for a in ans if a[2] > a[1]][:4]:
        out += [lo, hi, hi + 1]
    return sorted(set(out))


@pytest.mark.parametrize("early_reject", [False, True])
def test_flank_pre_filter(W, contexts, early_reject):
    """trgt_flank_filter_batch (2,5,1): the score of every judged job is minus the optimum -- "the optimal alignment score, exactly" --,
    keep = 0 only where a minimum-cost alignment with fewer than min_matches matches exists (an early reject: only where every one has
    fewer), and the bound is no smaller than the fewest matches any minimum-cost alignment has"""
    judged = 0
    for flank_len in (250, 40):
        loci, jobs = C.flank_loci(flank_len)
        ans = C.flank_answers(flank_len)
        pats = [loci[l]["left_flank"] if side == "left" else loci[l]["right_flank"] for l, side, _ in jobs]
        txts = [loci[l]["reads"][0] for l, _, _ in jobs]
        for min_matches in _filter_thresholds(ans, int(flank_len * 0.7)):
            r = W.flank_filter_batch(pats, txts, min_matches, ctx=contexts(), early_reject=early_reject)
            for j, (cost, lo, hi, _) in enumerate(ans):
                score, bound, keep = int(r["score"][j]), int(r["bound"][j]), int(r["keep"][j])
                where = (flank_len, min_matches, j, (cost, lo, hi), (score, bound, keep))
                if score == pywfa.I32_MIN:               # not judged: kept, no bound
                    assert keep == 1 and bound == -1, where
                    continue
                judged += 1
                if score == pywfa.I32_MIN + 1:           # given up early: no minimum-cost alignment reaches min_matches
                    assert early_reject and keep == 0 and bound == min_matches - 1 and hi < min_matches, where
                    continue
                assert score == -cost, where
                assert bound >= lo, where
                assert keep == (1 if bound >= min_matches else 0), where
                assert keep == 1 or lo < min_matches, where
    assert judged >= 96 * 4


def _spans_counts(err):
    line = [l for l in err.splitlines() if l.startswith("[spans] fallback alignments")][-1]
    return line, [l for l in err.splitlines() if l.startswith("[spans+]")]


@pytest.mark.parametrize("flank_len,env", [(250, {}), (250, dict(TRGT_WIN_LDS=1)), (250, dict(TRGT_WFA_NO_WINDOW=1)), (40, {})],
                         ids=["250", "250-lds-launch", "250-no-windows", "40"])
def test_flank_location(contexts, capfd, flank_len, env):
    """trgt_find_spans_batch with hit bytes on damaged pieces, noise from 0 to 30 %: hit 1 only for an exact piece at its first
    occurrence; every minimum-cost alignment below the threshold: missed; every one at or above it: found with hit 2, and the end of
    the placement that the repeat span shows is the end of a minimum-cost alignment"""
    from trgt_amd import locus
    loci, jobs = C.flank_loci(flank_len)
    b = locus.pack(list(loci))
    capfd.readouterr()
    ss, se, lh, rh = locus.find_tr_spans_batch(b, locus.Params(min_flank_id_frac=0.7, search_flank_len=flank_len), ctx=contexts(**env))
    err = capfd.readouterr().err
    found, missed, undecided = C.verify_flank(flank_len, 0.7, ss, se, lh, rh, "gpu")
    line, more = _spans_counts(err)
    assert found >= 20 and missed >= 5 and 10 * undecided <= len(jobs)
    # the routes: seeded windows on the register kernel (or the LDS launch), reads without a seed, the banded back-trace of what the
    # pre-filter keeps (the reads too short to span their locus)
    kept = [tuple(map(int, re.findall(r"\d+", l))) for l in more if l.startswith("[spans+] kept by the pre-filter")]
    win = [l for l in more if l.startswith("[spans+] windowed launch")]
    no_seed = [int(re.search(r"(\d+) of its \d+ alignments had no seeds", l).group(1)) for l in more if "had no seeds" in l]
    if env.get("TRGT_WFA_NO_WINDOW"):
        assert not win and kept and kept[-1][1] >= 10 and kept[-1][2] == 0, (line, more)        # banded, and every band stood
    elif flank_len == 250:
        windowed = int(re.search(r"-> windowed (\d+)", line).group(1))
        assert windowed >= 40 and no_seed and no_seed[-1] >= 5, (line, more)
        assert ("LDS kernel" if env.get("TRGT_WIN_LDS") else "history in registers") in win[-1] and win[-1].endswith(" 0 alignments it did not take"), win
    else:
        assert kept and kept[-1][1] >= 10 and kept[-1][2] == 0, (line, more)
